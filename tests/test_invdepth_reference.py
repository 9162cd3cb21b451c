"""CPU checks of the inverse-depth feature: the composite oracle reference
(invdepth_reference.py) against float64 autograd, and the public surface (the
two C entry points and the depth loss at an unchanged ABI version, the
optimisation defaults and the weight schedule, the data-parallel refusal, the
rasterizer's ``return_invdepth`` argument)."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import invdepth_reference as IR
import oracle as O  # noqa: F401
from gaussian_splatting_with_eye_tracking_amd import synthetic as S
from test_oracle_autograd import _rel, torch_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def map_allowance(W, H, fmax):
    """How far one pixel of a float32 map sum f alpha T may lie from its
    float64 restatement, to first order.  d map / d alpha_i = T_i (f_i - the
    alpha-weighted mean of the later f) lies within f_max T_i, so |d map| <=
    f_max sum_i T_i alpha_i e <= f_max e, with e the relative error of one
    float32 alpha = o exp(p):
    * the pixel-space mean carries the roundings of its chain (matrix-vector
      product, perspective division, ndc -> pixel: 4 roundings) at a
      magnitude of up to max(W, H), i.e. 4 max(W, H) 2^-24 px, and the
      exponent's slope |a dx + b dy| is at most sqrt(2 |p| max(a, c)) <=
      sqrt(2 ln 255 / 0.3) = 6.1 per px for a pair that contributes at all
      (alpha >= 1 / 255 with o <= 1; conic <= 1 / 0.3 by the 0.3 px dilation);
    * the conic's own chain (16 operations) scales the three terms of p, each
      at most ln 255: 16 * 3 * ln 255 * 2^-24;
    * exp, the product with o and the two blend operations: 4 * 2^-24.
    4e-4 at 250 px, 6e-5 at 32 px: at 250 px the mean's rounding alone is
    past 1e-5, so no fixed 1e-5 can hold per pixel there."""
    u = 2.0 ** -24
    slope = math.sqrt(2.0 * math.log(255.0) / 0.3)
    return fmax * (4.0 * max(W, H) * u * slope + 16.0 * 3.0 * math.log(255.0) * u + 4.0 * u)


# the two smallest of the GPU tests' cases (test_gpu_invdepth.CASES)
@pytest.mark.parametrize("P,W,H,seed", [(64, 32, 32, 3), (3000, 250, 130, 7)])
def test_composite_reference_matches_autograd(P, W, H, seed):
    """Colour + inverse-depth + alpha cotangents together: the composite
    reference against autodiff of test_oracle_autograd.torch_forward, the maps
    rendered there as colours (1 / (m . V[:3, 2] + V[3, 2]), 1, 0) on a zero
    background: every gradient within 1e-5.  Scene parameters as in
    test_aux_reference.py (opacities <= 0.97)."""
    cam = S.make_camera(W, H)
    sc = S.make_scene(P, cam, seed=seed, spread=0.9, opacity_std=1.0, log_scale_mean=np.log(0.02))
    sc.opacities = np.minimum(sc.opacities, 0.97).astype(np.float32)
    bg = (0.3, 0.2, 0.1)
    kw = dict(shs=sc.shs, scales=sc.scales, rotations=sc.rotations)
    ref = IR.reference_forward(cam, sc.means3D, sc.opacities, kw, bg=bg)
    fwd = ref["fwd"]
    vis = fwd.radii > 0
    # the feature is the float32 quotient of the oracle's own depths
    assert np.array_equal(ref["kwa"]["colors_precomp"][vis, 0], (np.float32(1.0) / fwd.depths[vis]).astype(np.float32))
    assert 0.0 < IR.max_inverse_depth(ref) < 5.0
    dpix = S.make_cotangent(H, W, seed + 1)
    di = S.make_cotangent(H, W, seed + 2)[0:1]
    da = S.make_cotangent(H, W, seed + 3)[0:1]
    g = IR.reference_backward(ref, dpix, di, da)

    t64 = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)  # noqa: E731
    m, sca, rot, op, shs = t64(sc.means3D), t64(sc.scales), t64(sc.rotations), t64(sc.opacities), t64(sc.shs)
    m2d = torch.zeros(P, 3, dtype=torch.float64, requires_grad=True)
    V = torch.tensor(cam.world_view_transform, dtype=torch.float64)
    img = torch_forward(cam, fwd, m, sca, rot, op, shs=shs, m2d=m2d, bg=bg)
    z = m @ V[:3, 2] + V[3, 2]
    # (a Gaussian that is not visible is never blended: any finite feature will do)
    f = torch.where(torch.from_numpy(vis), 1.0 / z, torch.zeros_like(z))
    feats = torch.stack([f, torch.ones_like(z), torch.zeros_like(z)], 1)
    maps = torch_forward(cam, fwd, m, sca, rot, op, colors=feats, m2d=m2d, bg=(0, 0, 0))
    # the maps themselves: the float32 oracle against float64, per pixel (map_allowance)
    fmax = IR.max_inverse_depth(ref)
    d_inv = float((maps[0:1].detach() - torch.from_numpy(ref["invdepth"]).double()).abs().max())
    d_alpha = float((maps[1:2].detach() - torch.from_numpy(ref["alpha"]).double()).abs().max())
    print(f"{P} {W}x{H}: invdepth max diff {d_inv:.3e} (bar {map_allowance(W, H, fmax):.3e}), "
          f"alpha max diff {d_alpha:.3e} (bar {map_allowance(W, H, 1.0):.3e})")
    assert d_inv < map_allowance(W, H, fmax)
    assert d_alpha < map_allowance(W, H, 1.0)
    loss = ((img * torch.from_numpy(dpix).double()).sum() + (maps[0:1] * torch.from_numpy(di).double()).sum() +
            (maps[1:2] * torch.from_numpy(da).double()).sum())
    loss.backward()
    tol = 1e-5  # the maps' bar of test_aux_reference.py, on the gradients too (float32 oracle vs float64 autodiff)
    errs = {"dL_dopacity": _rel(g["dL_dopacity"][vis], op.grad.numpy()[vis]),
            "dL_dmeans3D": _rel(g["dL_dmeans3D"][vis], m.grad.numpy()[vis]),
            "dL_dmeans2D": _rel(g["dL_dmeans2D"][vis, :2], m2d.grad.numpy()[vis, :2]),
            "dL_dsh": _rel(g["dL_dsh"][vis], shs.grad.numpy()[vis]),
            "dL_dscales": _rel(g["dL_dscales"][vis], sca.grad.numpy()[vis]),
            "dL_drotations": _rel(g["dL_drotations"][vis], rot.grad.numpy()[vis])}
    print(errs)
    for n, e in errs.items():
        assert e < tol, (n, e)
    # the chain -f^2 dL/df V[:3, 2] is part of the gradient: without it, or with the depth map's sign, the bar is missed
    ga = O.backward(ref["s0"], ref["aux"], sc.means3D, IR.AR._aux_cotangent(ref, di, da), **ref["kwa"])
    chain = ga["dL_dcolors"][:, 0:1].astype(np.float64) * IR._chain(ref)
    assert _rel((g["dL_dmeans3D"] - chain)[vis], m.grad.numpy()[vis]) > 1e-3
    assert _rel((g["dL_dmeans3D"] - 2.0 * chain)[vis], m.grad.numpy()[vis]) > 1e-3


def test_header_declares_invdepth_entries_at_abi_7():
    from gaussian_splatting_with_eye_tracking_amd import _C
    text = open(os.path.join(ROOT, "include", "gsplat_amd.h")).read()

    def declared(name):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", text, re.M)
        assert m, f"{name} is not declared"
        return " ".join(m.group(1).split())

    fwd, fwd_ex = declared("gs_rasterizer_forward_invdepth"), declared("gs_rasterizer_forward_ex")
    bwd, bwd_ex = declared("gs_rasterizer_backward_invdepth"), declared("gs_rasterizer_backward_ex")
    # the _ex argument lists with the inverse-depth map / cotangent in the depth's place
    assert fwd == fwd_ex.replace("float* out_depth", "float* out_invdepth") != fwd_ex
    assert bwd == bwd_ex.replace("const float* dL_ddepth", "const float* dL_dinvdepth") != bwd_ex
    assert "float* out_alpha" in fwd and "const float* dL_dalpha" in bwd
    loss = declared("gs_depth_l1_loss")
    assert loss == ("const float* invdepth, const float* target, const float* mask, int H, int W, float weight, "
                    "float* grad, float* out1, gs_buffer workspace, void* stream")
    assert re.search(r"#define GSPLAT_AMD_ABI_VERSION 7\b", text)
    assert _C.abi_version() == 7
    for fn in ("rasterize_gaussians_invdepth", "rasterize_gaussians_backward_invdepth",
               "rasterize_gaussians_backward_invdepth_lean", "depth_l1_loss"):
        assert hasattr(_C, fn), fn


def test_optimization_params_defaults_and_weight_schedule():
    from gaussian_splatting_with_eye_tracking_amd.training import OptimizationParams, get_expon_lr_func
    o = OptimizationParams()
    assert o.depth_l1_weight_init == 1.0 and o.depth_l1_weight_final == 0.01 and o.iterations == 30_000
    w = get_expon_lr_func(o.depth_l1_weight_init, o.depth_l1_weight_final, max_steps=o.iterations)
    # log-linear: exp of the mean of the logs half way
    half = math.exp(0.5 * (math.log(1.0) + math.log(0.01)))
    assert abs(half - 0.1) < 1e-15
    assert w(0) == pytest.approx(1.0, rel=1e-12)
    assert w(15_000) == pytest.approx(half, rel=1e-12)
    assert w(30_000) == pytest.approx(0.01, rel=1e-12)
    assert w(45_000) == pytest.approx(0.01, rel=1e-12)  # (clipped past the end)


def test_training_signatures_take_the_depth_target():
    from gaussian_splatting_with_eye_tracking_amd import training as T
    for fn in (T.training_iteration, T.forward_backward, T.FlatGaussianModel.render_and_backward):
        p = inspect.signature(fn).parameters
        assert p["invdepth_target"].default is None and p["depth_mask"].default is None, fn


def test_refuse_depth_target_raises_only_with_a_target_and_ranks():
    from gaussian_splatting_with_eye_tracking_amd import data_parallel as DP
    target = torch.zeros(1, 4, 4)
    DP.refuse_depth_target(None, "t")            # no process group: one rank
    DP.refuse_depth_target(target, "t")
    DP.refuse_depth_target(None, "t", world=2)
    DP.refuse_depth_target(target, "t", world=1)
    with pytest.raises(NotImplementedError, match="depth"):
        DP.refuse_depth_target(target, "t", world=2)


def test_return_invdepth_signature_and_exclusion():
    from gaussian_splatting_with_eye_tracking_amd.rasterization import (GaussianRasterizer, _RasterizeBase,
                                                                        _RasterizeGaussiansInvDepth,
                                                                        rasterize_gaussians_invdepth)
    from gaussian_splatting_with_eye_tracking_amd.renderer import render
    p = inspect.signature(GaussianRasterizer.forward).parameters
    assert p["return_invdepth"].default is False and p["return_aux"].default is False
    assert list(p)[:10] == ["self", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations",
                            "cov3D_precomp", "return_aux"]
    assert list(inspect.signature(rasterize_gaussians_invdepth).parameters) == [
        "means3D", "means2D", "sh", "colors_precomp", "opacities", "scales", "rotations", "cov3Ds_precomp",
        "raster_settings"]
    assert issubclass(_RasterizeGaussiansInvDepth, _RasterizeBase)
    r = inspect.signature(render).parameters
    assert r["return_invdepth"].default is False
    # both maps at once: refused before anything reaches the device
    e = torch.zeros(0, 3)
    with pytest.raises(ValueError, match="return_aux"):
        GaussianRasterizer(None)(means3D=e, means2D=e, opacities=e, shs=e, scales=e, rotations=e, return_aux=True,
                                 return_invdepth=True)
