"""The training iteration with upstream's depth regularisation on the GPU
(training.py `invdepth_target` / `depth_mask`): the fused native sequence
(`_C.rasterize_gaussians_invdepth` -> `_C.l1_ssim_loss` + `_C.depth_l1_loss` ->
one `_C.rasterize_gaussians_backward_invdepth_lean`) against the autograd one
(`GaussianRasterizer(return_invdepth=True)` + `losses`), at
test_gpu_training.py's bars (radii equal, |loss diff| < 1e-6, every group's
gradient within 1e-5 relative); no target is the plain iteration bit for bit;
the term pulls a shifted scene towards its target; sparse Adam leaves the
invisible rows alone.
"""
import math

import numpy as np
import pytest
import torch

import gs_helpers as G

pytestmark = pytest.mark.gpu


def _T():
    from gaussian_splatting_with_eye_tracking_amd import training
    return training


def _case(P, W, H, seed):
    sc, cam = G.scene_and_camera(P, W, H, seed=seed)
    return sc, cam, G.torch_settings(cam)


def _rendered_invdepth(sc, s, shift=0.0):
    """The inverse-depth and alpha maps of the scene, its means moved by
    `shift` (a fraction of their view-space depth) along the view axis."""
    from gaussian_splatting_with_eye_tracking_amd import GaussianRasterizer
    t = G.scene_tensors(sc)
    means = t["means3D"]
    if shift:
        V = s.viewmatrix  # row-vector convention: z = m . V[:3, 2] + V[3, 2]
        axis = V[:3, 2] / V[:3, 2].norm()
        z = means @ V[:3, 2] + V[3, 2]
        means = means + shift * z[:, None] * axis[None]
    with torch.no_grad():
        _, _, invdepth, alpha = GaussianRasterizer(s)(
            means3D=means, means2D=torch.zeros_like(means), opacities=t["opacities"], shs=t["shs"],
            scales=t["scales"], rotations=t["rotations"], return_invdepth=True)
    return invdepth, alpha


def _target_and_mask(sc, s, H, W, seed):
    """A target some way off the render, and a float mask with zeros in it."""
    invdepth, alpha = _rendered_invdepth(sc, s)
    gen = torch.Generator("cuda").manual_seed(seed)
    target = invdepth * (0.8 + 0.4 * torch.rand(1, H, W, device="cuda", generator=gen))
    mask = (alpha > 0.3).float() * (0.5 + torch.rand(1, H, W, device="cuda", generator=gen))
    assert 0.1 < float((mask > 0).float().mean()) < 1.0
    return target, mask


def test_fused_iteration_matches_autograd_iteration_with_a_target():
    T = _T()
    P, W, H = 2000, 96, 64
    sc, cam, s = _case(P, W, H, seed=9)
    raw = G.raw_from_scene(sc)
    gt = torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    target, mask = _target_and_mask(sc, s, H, W, seed=2)
    iteration = 7001  # a weight well inside the schedule
    out = []
    for fused in (True, False):
        m = T.FlatGaussianModel(raw, 3, spatial_lr_scale=5.0)
        m.active_sh_degree = 3
        pkg, terms = T.forward_backward(m, iteration, s, gt, fused=fused, invdepth_target=target, depth_mask=mask)
        out.append((m, pkg, terms))
    (mf, pf, tf), (ma, pa, ta) = out
    w = float(mf.depth_l1_weight(iteration))
    assert w == pytest.approx(math.exp(math.log(1.0) + (math.log(0.01) - math.log(1.0)) * iteration / 30_000),
                              rel=1e-12)
    assert int((pf["radii"] > 0).sum()) > 100
    assert torch.equal(pf["radii"], pa["radii"])
    torch.testing.assert_close(pf["render"], pa["render"].detach(), rtol=0, atol=1e-6)
    assert set(tf) == set(ta) == {"loss", "l1", "ssim", "depth_l1"}
    print(f"loss fused {float(tf['loss'])!r} autograd {float(ta['loss'])!r}, depth_l1 {float(tf['depth_l1'])!r}, w {w}")
    assert abs(float(tf["loss"]) - float(ta["loss"])) < 1e-6
    assert abs(float(tf["depth_l1"]) - float(ta["depth_l1"])) < 1e-6
    # the depth term is in the loss, weighted
    image_loss = (1 - mf.opt.lambda_dssim) * float(tf["l1"]) + mf.opt.lambda_dssim * (1 - float(tf["ssim"]))
    assert float(tf["depth_l1"]) > 1e-3
    assert float(tf["loss"]) == pytest.approx(image_loss + w * float(tf["depth_l1"]), abs=1e-6)
    torch.testing.assert_close(pf["viewspace_grad"], pa["viewspace_grad"], rtol=1e-5, atol=1e-9)
    for g in T.GROUPS:
        a, b = mf.group_view(mf.grads, g), ma.group_view(ma.grads, g)
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), g
        rel = float((a - b).norm() / b.norm().clamp_min(1e-30))
        print(f"{g}: rel {rel:.3e}")
        assert rel < 1e-5, (g, rel)
    # ... and it moved the gradient: the same iteration without a target differs
    m0 = T.FlatGaussianModel(raw, 3, spatial_lr_scale=5.0)
    m0.active_sh_degree = 3
    T.forward_backward(m0, iteration, s, gt, fused=True)
    a, b = mf.group_view(mf.grads, "xyz"), m0.group_view(m0.grads, "xyz")
    assert float((a - b).norm() / b.norm()) > 1e-3


@pytest.mark.parametrize("fused", [True, False])
def test_no_target_is_the_plain_iteration(fused):
    """invdepth_target=None (with or without a mask), and a target at weight
    0: the calls made are the plain iteration's, so the image, the radii, the
    loss terms and -- under the deterministic backward, where two runs of the
    same calls give the same bits at all -- every gradient are its bits."""
    T = _T()
    from gaussian_splatting_with_eye_tracking_amd import rasterization as R
    P, W, H = 2000, 96, 64
    sc, cam, s = _case(P, W, H, seed=9)
    raw = G.raw_from_scene(sc)
    gt = torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    target, mask = _target_and_mask(sc, s, H, W, seed=2)

    def run(opt=None, **kw):
        m = T.FlatGaussianModel(raw, 3, spatial_lr_scale=5.0, opt=opt)
        m.active_sh_degree = 3
        pkg, terms = T.forward_backward(m, 5, s, gt, fused=fused, **kw)
        torch.cuda.synchronize()
        return m, pkg, terms

    zero = T.OptimizationParams(depth_l1_weight_init=0.0, depth_l1_weight_final=0.0)
    try:
        R.set_deterministic(True)
        m0, p0, t0 = run()
        others = (run(invdepth_target=None, depth_mask=None), run(invdepth_target=None, depth_mask=mask),
                  run(opt=zero, invdepth_target=target, depth_mask=mask))
    finally:
        R.set_deterministic(None)
    assert float(m0.grads.abs().max()) > 0
    for m1, p1, t1 in others:
        assert set(t1) == set(t0) == {"loss", "l1", "ssim"}
        assert set(p1) == set(p0)
        assert torch.equal(p1["render"], p0["render"]) and torch.equal(p1["radii"], p0["radii"])
        for k in t0:
            assert torch.equal(t1[k], t0[k]), k
        assert torch.equal(m1.grads, m0.grads)
        assert torch.equal(p1["viewspace_grad"], p0["viewspace_grad"])


def test_depth_term_pulls_the_scene_towards_its_target():
    """60 iterations on the image of the scene itself (so the image loss is
    at rest) with the inverse depth of the scene shifted 5 % along the view
    axis as the target: the unweighted depth term falls.  A direction test,
    as test_training_run_fits_a_target, not a rate."""
    T = _T()
    P, W, H = 2000, 64, 64
    sc, cam, s = _case(P, W, H, seed=3)
    from gaussian_splatting_with_eye_tracking_amd import GaussianRasterizer
    t = G.scene_tensors(sc)
    with torch.no_grad():
        gt, _ = GaussianRasterizer(s)(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]),
                                      opacities=t["opacities"], shs=t["shs"], scales=t["scales"],
                                      rotations=t["rotations"])
    target, _ = _rendered_invdepth(sc, s, shift=0.05)
    here, _ = _rendered_invdepth(sc, s)
    assert float((here - target).abs().mean()) > 1e-3
    opt = T.OptimizationParams(densify_from_iter=10_000, densify_until_iter=0, iterations=10_000)
    m = T.FlatGaussianModel(G.raw_from_scene(sc), 3, spatial_lr_scale=5.0, opt=opt)
    m.active_sh_degree = 3
    depth_l1, losses = [], []
    for it in range(1, 61):
        terms = T.training_iteration(m, it, s, gt, scene_extent=5.0, invdepth_target=target)
        depth_l1.append(float(terms["depth_l1"]))
        losses.append(float(terms["loss"]))
    assert all(math.isfinite(x) for x in depth_l1 + losses)
    assert depth_l1[0] == pytest.approx(float((here - target).abs().mean()), abs=1e-4)
    print(f"depth_l1 first 10 {np.mean(depth_l1[:10]):.5f} last 10 {np.mean(depth_l1[-10:]):.5f}")
    assert np.mean(depth_l1[-10:]) < np.mean(depth_l1[:10]), (depth_l1[:10], depth_l1[-10:])
    assert torch.isfinite(m.params).all()


def test_sparse_adam_with_a_target_leaves_invisible_rows_untouched():
    T = _T()
    P, W, H = 2000, 96, 64
    sc, cam, s = _case(P, W, H, seed=9)
    gt = torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    target, mask = _target_and_mask(sc, s, H, W, seed=2)
    opt = T.OptimizationParams(optimizer_type="sparse_adam", densify_from_iter=10_000, densify_until_iter=0)
    m = T.FlatGaussianModel(G.raw_from_scene(sc), 3, spatial_lr_scale=5.0, opt=opt)
    m.active_sh_degree = 3
    before = {g: m.param[g].detach().clone() for g in T.GROUPS}
    pkg, terms = T.forward_backward(m, 1, s, gt, fused=True, invdepth_target=target, depth_mask=mask)
    radii = pkg["radii"].clone()
    T.post_backward(m, 1, pkg, scene_extent=5.0, fused=True)
    torch.cuda.synchronize()
    assert "depth_l1" in terms
    hidden, seen = radii == 0, radii > 0
    assert int(hidden.sum()) > 0 and int(seen.sum()) > 100
    for g in T.GROUPS:
        now = m.param[g].detach()
        assert torch.equal(now[hidden], before[g][hidden]), g
        assert bool((m.group_view(m.exp_avg, g)[hidden] == 0).all()), g
        assert bool((m.group_view(m.exp_avg_sq, g)[hidden] == 0).all()), g
    assert not torch.equal(m.param["xyz"].detach()[seen], before["xyz"][seen])
