"""The antialiasing reference (tests/antialias_reference.py) checked on the CPU:

* the float32 restatement of the coefficient is pinned to the oracle: its
  dilated (a, b, c) give the oracle's conic bit for bit;
* the scenes are what the GPU tests assume (every Gaussian visible, none
  outside the 1.3 tan(fov) clamp, the stated shares at the 0.000025 floor);
* the composite backward (oracle at o_eff + the coefficient's chain) equals
  full float64 autograd of the antialiased forward at the 5e-5 bar of
  test_oracle_autograd.test_backward_matches_autograd -- and the plain
  gradients do not (0.3 .. 1.0 relative on dL_dopacity / dL_dscales), so a
  rasterizer without the feature cannot pass the GPU tests.
"""
import numpy as np
import pytest
import torch

import antialias_reference as AR
import oracle as O
import test_oracle_autograd as TA

TOL = 5e-5  # test_backward_matches_autograd's bar (float32 oracle vs float64 autodiff)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cases():
    """scene -> (sc, cam, dpix, settings, plain oracle forward, coef32), built once."""
    out = {}
    for k in AR.SCENES:
        sc, cam, dpix = AR.make_case(k)
        s = O.settings_from_camera(cam, bg=AR.BG)
        fwd0 = O.forward(s, sc.means3D, sc.opacities, shs=sc.shs, scales=sc.scales, rotations=sc.rotations)
        out[k] = (sc, cam, dpix, s, fwd0, AR.coef32(s, sc.means3D, scales=sc.scales, rotations=sc.rotations))
    return out


@pytest.mark.parametrize("scene", sorted(AR.SCENES))
def test_restatement_reproduces_the_oracle_conic(cases, scene):
    sc, cam, _, s, fwd0, r32 = cases[scene]
    vis = fwd0.radii > 0
    assert vis.all()  # every Gaussian is visible
    assert np.array_equal(_bits(AR.cov3d32(sc.scales, sc.rotations))[vis], _bits(fwd0.cov3D)[vis])
    assert np.array_equal(_bits(AR.conic32(r32))[vis], _bits(fwd0.conic_opacity[:, :3])[vis])
    # and from a precomputed covariance
    r32c = AR.coef32(s, sc.means3D, cov3D_precomp=fwd0.cov3D)
    assert np.array_equal(_bits(r32c["coef"]), _bits(r32["coef"]))


def test_scene_statistics(cases):
    """The table of the scenes: coef ranges, the floor counts, no clamp."""
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    stats = {}
    for k, (sc, cam, _, s, fwd0, r32) in cases.items():
        coef, ratio, inside, _ = AR.coef64(cam, t64(sc.means3D), t64(sc.scales), t64(sc.rotations))
        vis = fwd0.radii > 0
        assert (~inside[vis]).sum() <= 0.01 * vis.sum()
        assert (~inside[vis]).sum() == 0
        c = r32["coef"][vis]
        # float32 restatement against float64 (the ratio loses digits only near 0, where the floor takes over)
        assert np.max(np.abs(c - coef.numpy()[vis]) / coef.numpy()[vis]) < 1e-3
        stats[k] = (float(c.min()), float(np.median(c)), float(c.max()),
                    int((r32["ratio"][vis] <= AR.RATIO_FLOOR).sum()))
    for k, (lo, med, hi) in {1: (0.08, 0.36, 0.95), 2: (0.09, 0.50, 0.98), 3: (0.07, 0.46, 0.98)}.items():
        assert abs(stats[k][0] - lo) < 0.01 and abs(stats[k][1] - med) < 0.01 and abs(stats[k][2] - hi) < 0.01, stats[k]
        assert stats[k][3] == 0
    assert stats[4][3] == 266
    assert stats[5][3] == 400 and stats[5][0] == stats[5][2] == np.sqrt(AR.RATIO_FLOOR)


def _kw(sc, fwd0, variant, seed):
    if variant == "colors":
        colors = np.random.default_rng(seed + 9).uniform(0, 1, (sc.means3D.shape[0], 3)).astype(np.float32)
        return dict(colors_precomp=colors, scales=sc.scales, rotations=sc.rotations)
    if variant == "cov":
        return dict(shs=sc.shs, cov3D_precomp=fwd0.cov3D.copy())
    return dict(shs=sc.shs, scales=sc.scales, rotations=sc.rotations)


@pytest.mark.parametrize("scene,variant", [(k, v) for k in (1, 2, 3) for v in ("sh", "colors", "cov")] + [(4, "sh")])
def test_composite_matches_full_autograd(cases, scene, variant):
    sc, cam, dpix, s, fwd0, _ = cases[scene]
    kw = _kw(sc, fwd0, variant, AR.SCENES[scene][3])
    ref = AR.reference_forward(cam, sc.means3D, sc.opacities, kw)
    fwd = ref["fwd"]
    # the flag changes the opacities alone: the same binning
    assert np.array_equal(fwd.radii, fwd0.radii) and np.array_equal(fwd.point_list, fwd0.point_list)
    assert np.array_equal(fwd.ranges, fwd0.ranges) and fwd.num_rendered == fwd0.num_rendered
    comp = AR.reference_backward(ref, dpix)

    t64 = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)  # noqa: E731
    m, sca, rot, op, shs = t64(sc.means3D), t64(sc.scales), t64(sc.rotations), t64(sc.opacities), t64(sc.shs)
    col = t64(kw["colors_precomp"]) if variant == "colors" else None
    c6 = t64(kw["cov3D_precomp"]) if variant == "cov" else None
    coef, _, _, _ = AR.coef64(cam, m, sca, rot, cov6=c6)
    m2d = torch.zeros(sc.means3D.shape[0], 3, dtype=torch.float64, requires_grad=True)
    img = TA.torch_forward(cam, fwd, m, sca, rot, op * coef[:, None], shs=None if variant == "colors" else shs,
                           colors=col, cov6=c6, m2d=m2d, bg=AR.BG)
    assert float((img.detach() - torch.from_numpy(fwd.color).double()).abs().max()) < 1e-4
    (img * torch.from_numpy(dpix).double()).sum().backward()
    vis = fwd.radii > 0
    full = {"dL_dopacity": op, "dL_dmeans3D": m, "dL_dmeans2D": m2d}
    if variant == "colors":
        full["dL_dcolors"] = col
    else:
        full["dL_dsh"] = shs
    if variant == "cov":
        full["dL_dcov3D"] = c6
    else:
        full["dL_dscales"], full["dL_drotations"] = sca, rot
    for n, t in full.items():
        a, b = comp[n][vis], t.grad.numpy()[vis]
        if n == "dL_dmeans2D":
            a, b = a[:, :2], b[:, :2]
        assert TA._rel(a, b) < TOL, (n, TA._rel(a, b))

    # the plain gradients (no feature) are far from the antialiased ones
    g0 = O.backward(s, fwd0, sc.means3D, dpix, **kw)
    assert TA._rel(g0["dL_dopacity"][vis], op.grad.numpy()[vis]) > 0.1
    if variant != "cov":
        assert TA._rel(g0["dL_dscales"][vis], sca.grad.numpy()[vis]) > 0.1


def test_floor_scene_has_no_coefficient_gradient(cases):
    """Scene 5: every ratio is at the floor, so coef = 0.005 is a constant."""
    sc, cam, dpix, s, fwd0, r32 = cases[5]
    kw = _kw(sc, fwd0, "sh", 7)
    ref = AR.reference_forward(cam, sc.means3D, sc.opacities, kw)
    comp = AR.reference_backward(ref, dpix)
    for e in comp["_coef_term"].values():
        assert not e.any()
    plain = O.backward(s, ref["fwd"], sc.means3D, dpix, **kw)
    assert np.array_equal(comp["dL_dopacity"],
                          plain["dL_dopacity"].astype(np.float64) * np.float64(np.sqrt(AR.RATIO_FLOOR)))


def test_allowance_maps_the_opacity_allowance(cases):
    sc, cam, dpix, s, fwd0, _ = cases[1]
    kw = _kw(sc, fwd0, "sh", 3)
    ref = AR.reference_forward(cam, sc.means3D, sc.opacities, kw)
    plain, _ = O.grad_allowance(s, ref["fwd"], sc.means3D, dpix, **kw)
    al = AR.reference_allowance(ref, dpix)
    assert np.allclose(al["dL_dopacity"][:, 0], plain["dL_dopacity"][:, 0] * ref["coef"])
    for n in ("dL_dmeans3D", "dL_dscales", "dL_drotations"):
        assert (al[n] >= plain[n]).all() and (al[n] > plain[n]).any()
    for n in ("dL_dmeans2D", "dL_dsh", "dL_dcolors"):
        assert np.array_equal(al[n], plain[n])
