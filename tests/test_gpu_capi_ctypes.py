"""The C ABI on the GPU without the torch binding (include/gsplat_amd.h,
INTEGRATION.md §2.2): the reference's Rasterizer::forward / ::backward
(base/cr/rasterizer.h:24-84) and the AMR Rasterizer::forward
(amr/cr/rasterizer.h:24-98) replacements driven through ctypes, as a host
without the pybind module would bind them -- torch-allocated device tensors
as plain pointers, gs_buffer resize callbacks that allocate the byte buffers,
and an explicit (non-default) HIP stream.

On config 1's inputs (10k Gaussians, 256 x 256, seed 0) the results equal the
`_C` path's: K, radii, point_list, ranges and the image bit for bit; the AMR
steps' images and render_once bit for bit; the gradients bit for bit except
for the order of the blend backward's float atomics (their last bits are
run-dependent for any two runs, _C against _C included; bounded here at
1e-6 of each tensor's norm).
"""
import ctypes

import numpy as np
import pytest

import gs_helpers as G
from capi_helpers import F, I, VP, Buffers, GsBuffer, check as _check, lib as _lib, ptr as _p

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

def _inputs(P=10_000, W=256, H=256, seed=0):
    sc, cam = G.scene_and_camera(P, W, H, seed)
    s = G.torch_settings(cam)
    t = G.scene_tensors(sc)
    return sc, cam, s, t


def test_forward_backward_through_ctypes_match_the_binding():
    import gaussian_splatting_with_eye_tracking_amd._C as C
    from gaussian_splatting_with_eye_tracking_amd import synthetic as S
    lib = _lib()
    P, W, H = 10_000, 256, 256
    sc, cam, s, t = _inputs(P, W, H)
    e = torch.Tensor([])
    dpix = torch.from_numpy(S.make_cotangent(H, W, 1)).cuda()
    # the binding (torch's current stream)
    K0, col0, rad0, gb0, bb0, ib0 = C.rasterize_gaussians(
        s.bg, t["means3D"], e, t["opacities"], t["scales"], t["rotations"], 1.0, e, s.viewmatrix, s.projmatrix,
        s.tanfovx, s.tanfovy, H, W, t["shs"], 3, s.campos, False, False)
    g0 = C.rasterize_gaussians_backward(s.bg, t["means3D"], rad0, e, t["scales"], t["rotations"], 1.0, e,
                                        s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, dpix, t["shs"], 3, s.campos,
                                        gb0, K0, bb0, ib0, False)
    torch.cuda.synchronize()
    # the C ABI through ctypes, on an explicit stream
    stream = torch.cuda.Stream()
    bufs = Buffers(t["means3D"].device)
    with torch.cuda.stream(stream):
        col = torch.empty((3, H, W), device="cuda")
        radii = torch.empty(P, dtype=torch.int32, device="cuda")
        K = _check(lib, lib.gs_rasterizer_forward(
            bufs.buf("geom"), bufs.buf("binning"), bufs.buf("image"), P, 3, 16, _p(s.bg), W, H, _p(t["means3D"]),
            _p(t["shs"]), VP(0), _p(t["opacities"]), _p(t["scales"]), F(1.0), _p(t["rotations"]), VP(0),
            _p(s.viewmatrix), _p(s.projmatrix), _p(s.campos), F(s.tanfovx), F(s.tanfovy), 0, _p(col), _p(radii), 0,
            VP(stream.cuda_stream)), "gs_rasterizer_forward")
        outs = [torch.empty(shape, device="cuda") for shape in ((P, 3), (P, 1), (P, 3), (P, 3), (P, 6), (P, 16, 3),
                                                                (P, 3), (P, 4))]
        m2, op, cl, m3, cv, sh, scl, rot = outs
        _check(lib, lib.gs_rasterizer_backward(
            P, 3, 16, K, _p(s.bg), W, H, _p(t["means3D"]), _p(t["shs"]), VP(0), _p(t["scales"]), F(1.0),
            _p(t["rotations"]), VP(0), _p(s.viewmatrix), _p(s.projmatrix), _p(s.campos), F(s.tanfovx), F(s.tanfovy),
            _p(radii), _p(bufs.t["geom"]), _p(bufs.t["binning"]), _p(bufs.t["image"]), _p(dpix), _p(m2), VP(0),
            _p(op), _p(cl), _p(m3), _p(cv), _p(sh), _p(scl), _p(rot), 0, VP(stream.cuda_stream)),
            "gs_rasterizer_backward")
    stream.synchronize()
    assert K == K0 > 0
    assert torch.equal(radii, rad0)
    assert torch.equal(col, col0)
    d = C.parse_buffers(bufs.t["geom"], bufs.t["binning"], bufs.t["image"], P, K, W, H, 16)
    d0 = C.parse_buffers(gb0, bb0, ib0, P, K0, W, H, 16)
    for k in ("point_list", "ranges", "n_contrib", "accum_alpha"):
        assert torch.equal(d[k], d0[k]), k
    vis = rad0 > 0  # (culled Gaussians' geometry records are never written)
    for k in ("means2D", "conic_opacity", "depths"):
        assert torch.equal(d[k][vis], d0[k][vis]), k
    names = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
             "dL_drotations"]
    mine = dict(zip(names, [m2, cl, op, m3, cv, sh, scl, rot]))
    for n, ref in zip(names, g0):
        assert mine[n].shape == ref.shape, n
        assert G.rel_err(mine[n].cpu().numpy(), ref.cpu().numpy()) < 1e-6, n


def test_amr_forward_through_ctypes_matches_the_binding():
    import gaussian_splatting_with_eye_tracking_amd._C as C
    from diff_gaussian_rasterization_amr import _RasterizeGaussians
    lib = _lib()
    P, W, H = 10_000, 256, 256
    sc, cam, s, t = _inputs(P, W, H)
    s = G.torch_settings(cam, amr=True)
    e = torch.Tensor([])
    u8 = torch.Tensor([]).to(torch.uint8)
    m2 = torch.zeros_like(t["means3D"])
    args = (t["means3D"], m2, t["shs"], e, t["opacities"], t["scales"], t["rotations"], e)
    with torch.no_grad():
        ref_steps = []
        c, rradii, gb, bb, ib = _RasterizeGaussians.apply(*args, 0, e, u8, u8, u8, False, s)
        ref_steps.append(c.clone())
        acc = c
        for k in range(1, 5):
            c, _, gb, bb, ib = _RasterizeGaussians.apply(*args, k, acc, gb, bb, ib, False, s)
            ref_steps.append(c.clone())
            acc = acc + c
        ref_once = _RasterizeGaussians.apply(*args, -2, e, u8, u8, u8, True, s)[0]
    torch.cuda.synchronize()

    def amr_call(bufs, step, pre, out, radii, interp, stream, precomp=None):
        g = bufs.t.get("geom") if step >= 1 else None
        b = bufs.t.get("binning") if step >= 1 else None
        im = bufs.t.get("image") if step >= 1 else None
        return _check(lib, lib.gs_amr_rasterizer_forward(
            bufs.buf("geom") if step < 1 else bufs.buf("unused_g"),
            bufs.buf("binning") if step < 1 else bufs.buf("unused_b"),
            bufs.buf("image") if step < 1 else bufs.buf("unused_i"), P, 3, 16, _p(s.bg), W, H, _p(t["means3D"]),
            _p(t["shs"]), VP(0), _p(t["opacities"]), _p(t["scales"]), F(1.0), _p(t["rotations"]), VP(0),
            _p(s.viewmatrix), _p(s.projmatrix), _p(s.campos), F(s.tanfovx), F(s.tanfovy), 0, step, _p(precomp),
            _p(g), _p(b), _p(im), _p(out), _p(radii), 1 if interp else 0, 0, VP(stream.cuda_stream)),
            f"gs_amr_rasterizer_forward step {step}")

    stream = torch.cuda.Stream()
    bufs = Buffers(t["means3D"].device)
    steps = []
    with torch.cuda.stream(stream):
        radii = torch.empty(P, dtype=torch.int32, device="cuda")
        acc = None
        for k in range(5):
            out = torch.empty((3, H, W), device="cuda")
            rk = torch.empty(P, dtype=torch.int32, device="cuda")
            amr_call(bufs, k, None, out, radii if k == 0 else rk, False, stream, precomp=acc)
            steps.append(out)
            acc = out if acc is None else acc + out
        once = torch.empty((3, H, W), device="cuda")
        once_bufs = Buffers(t["means3D"].device)
        amr_call(once_bufs, -2, None, once, torch.empty(P, dtype=torch.int32, device="cuda"), True, stream)
    stream.synchronize()
    assert torch.equal(radii, rradii)
    for k in range(5):
        assert torch.equal(steps[k], ref_steps[k]), k
    assert torch.equal(once, ref_once)


SZ = ctypes.c_size_t
AMR_STEPS_1_TO_4_SPLIT = 16  # GSPLAT_AMD_AMR_STEPS_1_TO_4_SPLIT (include/gsplat_amd.h)


def _amr_forward(lib, bufs, s, t, P, W, H, step, out, radii, stream, precomp=None):
    """gs_amr_rasterizer_forward at foveaStep `step` on (step 0: into) bufs' geom / binning / image."""
    pre = [bufs.t.get(k) if step >= 1 else None for k in ("geom", "binning", "image")]
    own = [bufs.buf(k if step < 1 else "unused_" + k) for k in ("geom", "binning", "image")]
    return _check(lib, lib.gs_amr_rasterizer_forward(
        *own, P, 3, 16, _p(s.bg), W, H, _p(t["means3D"]), _p(t["shs"]), VP(0), _p(t["opacities"]), _p(t["scales"]),
        F(1.0), _p(t["rotations"]), VP(0), _p(s.viewmatrix), _p(s.projmatrix), _p(s.campos), F(s.tanfovx),
        F(s.tanfovy), 0, step, _p(precomp), _p(pre[0]), _p(pre[1]), _p(pre[2]), _p(out), _p(radii), 0, 0,
        VP(stream.cuda_stream)), f"gs_amr_rasterizer_forward step {step}")


def test_split_amr_steps_through_ctypes_match_the_per_step_calls():
    """gs_amr_accumulate_step with GSPLAT_AMD_AMR_STEPS_1_TO_4_SPLIT and
    gs_amr_set_step_state through the C ABI (so far covered only through the
    torch binding's speculation), on 7 x 5 AMR tiles with ragged right and
    bottom edges, K read back from the header (no hint): the one launch writes
    every element of the four images and radii rows, image k is the per-step
    call's image k bit for bit, and set_step_state(j) leaves the level state
    the per-step call j leaves (the ordinary step j + 1 behind it then renders
    the per-step image j + 1)."""
    import gaussian_splatting_with_eye_tracking_amd._C as C
    lib = _lib()
    lib.gs_amr_accumulate_step.argtypes = [I, VP, I, I, VP, I, VP, VP, VP, VP, VP, I, I, VP]
    lib.gs_amr_set_step_state.argtypes = [VP, SZ, I, I, I, VP]
    P, W, H = 3000, 200, 136
    sc, cam, s, t = _inputs(P, W, H)
    s = G.torch_settings(cam, amr=True)
    stream = torch.cuda.Stream()

    def state(bufs, K):
        d = C.parse_buffers(bufs.t["geom"], bufs.t["binning"], bufs.t["image"], P, K, W, H, 32)
        return d["levels_last"].clone(), d["levels_current"].clone()

    with torch.cuda.stream(stream):
        new = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device="cuda")
        # per-step calls
        per = Buffers(t["means3D"].device)
        img0, rad0 = new(3, H, W), new(P, dt=torch.int32)
        K = _amr_forward(lib, per, s, t, P, W, H, 0, img0, rad0, stream)
        assert K > 0
        want, want_state, acc = [], [], img0
        for k in range(1, 5):
            out = new(3, H, W)
            _amr_forward(lib, per, s, t, P, W, H, k, out, new(P, dt=torch.int32), stream, precomp=acc)
            want.append(out)
            want_state.append(state(per, K))
            acc = acc + out
        # the one split launch on a second frame's buffers
        one = Buffers(t["means3D"].device)
        assert _amr_forward(lib, one, s, t, P, W, H, 0, new(3, H, W), new(P, dt=torch.int32), stream) == K
        imgs = torch.full((4, 3, H, W), float("nan"), device="cuda")
        rads = torch.full((4, P), -1, dtype=torch.int32, device="cuda")
        rc = lib.gs_amr_accumulate_step(P, _p(s.bg), W, H, VP(0), AMR_STEPS_1_TO_4_SPLIT, _p(one.t["geom"]),
                                        _p(one.t["binning"]), _p(one.t["image"]), _p(imgs), _p(rads), 0, -1,
                                        VP(stream.cuda_stream))
        assert _check(lib, rc, "gs_amr_accumulate_step") == K
        assert not torch.isnan(imgs).any() and not (rads == -1).any()
        for k in range(4):
            assert torch.equal(imgs[k], want[k]), k
        for j in range(1, 4):
            _check(lib, lib.gs_amr_set_step_state(_p(one.t["image"]), one.t["image"].numel(), W, H, j,
                                                  VP(stream.cuda_stream)), "gs_amr_set_step_state")
            got = state(one, K)
            assert torch.equal(got[0], want_state[j - 1][0]) and torch.equal(got[1], want_state[j - 1][1]), j
            out = new(3, H, W)
            _amr_forward(lib, one, s, t, P, W, H, j + 1, out, new(P, dt=torch.int32), stream)
            assert torch.equal(out, want[j]), j
    stream.synchronize()


def test_deterministic_and_view_grads_entries_through_ctypes_match_the_binding():
    """gs_rasterizer_backward_deterministic and
    gs_rasterizer_backward_view_grads_deterministic through ctypes equal the
    `_C` bindings under set_deterministic_backward(True) bit for bit (the
    deterministic path is bit-reproducible); gs_rasterizer_backward_view_grads
    equals `_C.rasterize_gaussians_backward_view_grads` on the record's rows of
    non-culled Gaussians and its camera words -- word 9 (radius | clamped
    bits) and the camera bit for bit, the nine gradient words up to the order
    of the default blend backward's float atomics, which differs between any
    two runs of the same entry (the module docstring's bound: 1e-6 of the
    norm)."""
    import gaussian_splatting_with_eye_tracking_amd._C as C
    from gaussian_splatting_with_eye_tracking_amd import synthetic as S
    lib = _lib()
    bwd = [I, I, I, I, VP, I, I, VP, VP, VP, VP, F, VP, VP, VP, VP, VP, F, F, VP, VP, VP, VP, VP] + [VP] * 9
    view = [I, I, VP, I, I, VP, VP, VP, VP, F, F, VP, VP, VP, VP, VP, VP]
    lib.gs_rasterizer_backward_deterministic.argtypes = bwd + [VP, SZ, I, VP]
    lib.gs_rasterizer_backward_view_grads.argtypes = view + [I, VP]
    lib.gs_rasterizer_backward_view_grads_deterministic.argtypes = view + [VP, SZ, I, VP]
    lib.gs_backward_deterministic_scratch_bytes.argtypes = [I, I]
    lib.gs_backward_deterministic_scratch_bytes.restype = SZ
    P, W, H = 2000, 96, 80
    sc, cam, s, t = _inputs(P, W, H)
    e = torch.Tensor([])
    dpix = torch.from_numpy(S.make_cotangent(H, W, 1)).cuda()
    K, _col, radii, gb, bb, ib = C.rasterize_gaussians(
        s.bg, t["means3D"], e, t["opacities"], t["scales"], t["rotations"], 1.0, e, s.viewmatrix, s.projmatrix,
        s.tanfovx, s.tanfovy, H, W, t["shs"], 3, s.campos, False, False)
    assert K > 0
    view_args = (s.bg, radii, e, s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.campos, dpix, gb, K, bb, ib,
                 False)
    C.set_deterministic_backward(True)
    try:
        g0 = C.rasterize_gaussians_backward(s.bg, t["means3D"], radii, e, t["scales"], t["rotations"], 1.0, e,
                                            s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, dpix, t["shs"], 3,
                                            s.campos, gb, K, bb, ib, False)
        rec_det0 = C.rasterize_gaussians_backward_view_grads(*view_args)
    finally:
        C.set_deterministic_backward(False)
    rec0 = C.rasterize_gaussians_backward_view_grads(*view_args)
    torch.cuda.synchronize()

    stream = torch.cuda.Stream()
    sp = VP(stream.cuda_stream)
    with torch.cuda.stream(stream):
        scratch = torch.empty(lib.gs_backward_deterministic_scratch_bytes(P, K), dtype=torch.uint8, device="cuda")
        outs = [torch.empty(shape, device="cuda") for shape in ((P, 3), (P, 1), (P, 3), (P, 3), (P, 6), (P, 16, 3),
                                                                (P, 3), (P, 4))]
        m2, op, cl, m3, cv, sh, scl, rot = outs
        _check(lib, lib.gs_rasterizer_backward_deterministic(
            P, 3, 16, K, _p(s.bg), W, H, _p(t["means3D"]), _p(t["shs"]), VP(0), _p(t["scales"]), F(1.0),
            _p(t["rotations"]), VP(0), _p(s.viewmatrix), _p(s.projmatrix), _p(s.campos), F(s.tanfovx), F(s.tanfovy),
            _p(radii), _p(gb), _p(bb), _p(ib), _p(dpix), _p(m2), VP(0), _p(op), _p(cl), _p(m3), _p(cv), _p(sh),
            _p(scl), _p(rot), _p(scratch), scratch.numel(), 0, sp), "gs_rasterizer_backward_deterministic")
        common = (P, K, _p(s.bg), W, H, VP(0), _p(s.viewmatrix), _p(s.projmatrix), _p(s.campos), F(s.tanfovx),
                  F(s.tanfovy), _p(radii), _p(gb), _p(bb), _p(ib), _p(dpix))
        rec_det, rec = torch.empty(P * 10 + 40, device="cuda"), torch.empty(P * 10 + 40, device="cuda")
        _check(lib, lib.gs_rasterizer_backward_view_grads_deterministic(*common, _p(rec_det), _p(scratch),
                                                                        scratch.numel(), 0, sp),
               "gs_rasterizer_backward_view_grads_deterministic")
        _check(lib, lib.gs_rasterizer_backward_view_grads(*common, _p(rec), 0, sp),
               "gs_rasterizer_backward_view_grads")
    stream.synchronize()
    # (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
    for n, (mine, ref) in enumerate(zip([m2, cl, op, m3, cv, sh, scl, rot], g0)):
        assert torch.equal(mine, ref), n
    assert torch.equal(rec_det, rec_det0)
    vis = radii > 0  # (the existing test's note: what belongs to culled Gaussians is never written)
    rows, rows0 = rec[:P * 10].reshape(P, 10)[vis], rec0[:P * 10].reshape(P, 10)[vis]
    assert torch.equal(rows[:, 9], rows0[:, 9])  # radius | clamped bits
    assert torch.equal(rec[P * 10:], rec0[P * 10:])
    err = G.rel_err(rows[:, :9].cpu().numpy(), rows0[:, :9].cpu().numpy())
    print(f"view-grads record, default blend backward, ctypes vs _C: rel err {err:.3e}")
    assert err < 1e-6
