"""The reference of the inverse-depth / alpha maps and their backward, composed
from the unchanged oracle as aux_reference.py composes the depth map's:

* forward: one oracle forward for the view-space depths ``z``, a second one
  with ``colors_precomp = (f, 1, 0)``, ``f = float32(1) / z`` (one correctly
  rounded float32 division), on a zero background -- channel 0 is the
  inverse-depth map ``sum f alpha T``, channel 1 the alpha map;
* backward: the oracle backward of that second forward with the cotangent
  ``(dL_dinvdepth, dL_dalpha, 0)``, plus ``-f^2 * dL_dcolors[:, 0] * V[:3, 2]``
  on ``dL_dmeans3D`` (f = 1 / z, z = m . V[:3, 2] + V[3, 2] in the row-vector
  convention), plus the ordinary colour backward;
* allowances: the two passes' ``oracle.grad_allowance`` add, the
  ``dL_dcolors[:, 0]`` allowance of the map pass scaled by ``f^2 |V[:3, 2]|``
  on ``dL_dmeans3D``.

``opacities`` may be the antialiased forward's effective opacities
(antialias_reference.effective_opacity): the composition is the same.
"""
from __future__ import annotations

import numpy as np

import aux_reference as AR
import gs_helpers as G
import oracle as O

SUMMED, COLOUR_ONLY, NAMES = AR.SUMMED, AR.COLOUR_ONLY, AR.NAMES
cotangents = AR.cotangents  # (dL_dcolor, dL_dinvdepth, dL_dalpha) of a case


def inverse(depths) -> np.ndarray:
    """f = float32(1) / z, elementwise, in float32 (IEEE: correctly rounded)."""
    z = np.asarray(depths, np.float32).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.float32(1.0) / z).astype(np.float32)


def invdepth_features(depths, radii) -> np.ndarray:
    """(f, 1, 0) per Gaussian; zeros in channel 0 where the Gaussian is not
    visible (its depth is not a depth, and it is never blended)."""
    f = np.where(np.asarray(radii).reshape(-1) > 0, inverse(depths), np.float32(0.0)).astype(np.float32)
    return np.ascontiguousarray(np.stack([f, np.ones_like(f), np.zeros_like(f)], 1).astype(np.float32))


def reference_forward(cam, means3D, opacities, kw: dict, bg=(0.0, 0.0, 0.0), sh_degree=3) -> dict:
    """kw: the oracle's colour / covariance keywords (shs or colors_precomp;
    scales + rotations or cov3D_precomp)."""
    s = O.settings_from_camera(cam, bg=bg, sh_degree=sh_degree)
    fwd = O.forward(s, means3D, opacities, **kw)
    s0 = O.settings_from_camera(cam, bg=(0.0, 0.0, 0.0), sh_degree=sh_degree)
    kwa = {k: v for k, v in kw.items() if k not in ("shs", "colors_precomp")}
    kwa["colors_precomp"] = invdepth_features(fwd.depths, fwd.radii)
    aux = O.forward(s0, means3D, opacities, **kwa)
    assert np.array_equal(aux.n_contrib, fwd.n_contrib)  # the same contributors
    return dict(s=s, s0=s0, fwd=fwd, aux=aux, kw=kw, kwa=kwa, cam=cam, means3D=means3D,
                f=kwa["colors_precomp"][:, 0].astype(np.float64),
                invdepth=aux.color[0:1].copy(), alpha=aux.color[1:2].copy())


def max_inverse_depth(ref) -> float:
    """max 1 / z over the visible Gaussians."""
    return float(ref["f"][ref["fwd"].radii > 0].max())


def _chain(ref) -> np.ndarray:
    """d f / d means3D per Gaussian: -f^2 V[:3, 2], [P, 3] float64."""
    return -(ref["f"] ** 2)[:, None] * AR._zaxis(ref)[None]


def reference_backward(ref, dL_dcolor=None, dL_dinvdepth=None, dL_dalpha=None) -> dict:
    """The composite reference gradients (float64 sums of the float32 oracle
    passes); any cotangent may be None."""
    total: dict = {}
    if dL_dinvdepth is not None or dL_dalpha is not None:
        ga = O.backward(ref["s0"], ref["aux"], ref["means3D"], AR._aux_cotangent(ref, dL_dinvdepth, dL_dalpha),
                        **ref["kwa"])
        AR._add(total, ga, SUMMED)
        total["dL_dmeans3D"] = total["dL_dmeans3D"] + ga["dL_dcolors"][:, 0:1].astype(np.float64) * _chain(ref)
    if dL_dcolor is not None:
        gc = O.backward(ref["s"], ref["fwd"], ref["means3D"], np.asarray(dL_dcolor, np.float32), **ref["kw"])
        AR._add(total, gc, SUMMED + COLOUR_ONLY)
    else:  # the colour took no part: its own gradients are zero
        P = ref["fwd"].radii.shape[0]
        total["dL_dcolors"] = np.zeros((P, 3))
        if "shs" in ref["kw"]:
            total["dL_dsh"] = np.zeros(np.asarray(ref["kw"]["shs"]).shape)
    return total


def reference_allowance(ref, dL_dcolor=None, dL_dinvdepth=None, dL_dalpha=None) -> dict:
    total: dict = {}
    if dL_dinvdepth is not None or dL_dalpha is not None:
        aa, _ = O.grad_allowance(ref["s0"], ref["aux"], ref["means3D"],
                                 AR._aux_cotangent(ref, dL_dinvdepth, dL_dalpha), **ref["kwa"])
        AR._add(total, aa, SUMMED)
        total["dL_dmeans3D"] = total["dL_dmeans3D"] + aa["dL_dcolors"][:, 0:1] * np.abs(_chain(ref))
    if dL_dcolor is not None:
        ac, _ = O.grad_allowance(ref["s"], ref["fwd"], ref["means3D"], np.asarray(dL_dcolor, np.float32),
                                 **ref["kw"])
        AR._add(total, ac, SUMMED + COLOUR_ONLY)
    return total


def check_against_reference(case, grads, ref, sc, cam, dpix, di, da):
    """The eight gradients of an inverse-depth backward against the
    reference's: the L2 bar and the element-wise bar with the summed
    allowances."""
    rg = reference_backward(ref, dpix, di, da)
    al = reference_allowance(ref, dpix, di, da)
    for n, g in zip(NAMES, grads):
        gg = g.cpu().numpy()
        assert np.all(np.isfinite(gg)), n
        if n not in rg:  # (no SH input: an empty gradient)
            assert n == "dL_dsh" and gg.size == 0, n
            continue
        assert gg.shape == rg[n].shape, n
        err = G.rel_err(gg, rg[n])
        print(f"{case} {n}: rel err {err:.3e}")
        assert err < G.GRAD_REL_TOL, (n, err)
    G.assert_grads_elementwise(case, NAMES, grads, rg, sc, cam, ref["fwd"], allow=al)
