"""The sparse Adam step (csrc/train.hip sparse_adam_kernel) on the GPU, held
bit for bit to tests/sparse_adam_reference.py (pinned on the CPU by
tests/test_sparse_adam_reference.py): through ``_C.sparse_adam_step``, through
the trainer (``optimizer_type="sparse_adam"``) and through the C entry
``gs_sparse_adam_step``.

Identity is the derived expectation: the library builds with
-ffp-contract=off, every operation of the formula is one float32 instruction,
and the device's float32 division and square root are correctly rounded, as
numpy's are.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import capi_helpers as CH
import gs_helpers as G
import sparse_adam_reference as SR

pytestmark = pytest.mark.gpu

BETAS = (0.9, 0.999)
EPS = 1e-15
LRS = [1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 5e-3, 1e-3]
SIZES = [1, 2, 63, 64, 65, 257, 4997]
COEFFS = [1, 4, 16]  # SH coefficient counts: f_rest rows of 0, 9 and 45 floats
MASKS = ("all", "none", "first", "last", "alternating", "runs64", "runs65", "random50", "random10", "signed")


def _C():
    from gaussian_splatting_with_eye_tracking_amd import _C as c
    return c


def _T():
    from gaussian_splatting_with_eye_tracking_amd import training
    return training


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(t, a):
    """A float32 device tensor against a float32 numpy array, on the bits."""
    return torch.equal(t.view(torch.int32).cpu(), torch.from_numpy(np.ascontiguousarray(a, np.float32).view(np.int32)))


def _assert_state(dev, ref, what):
    for name, t, a in zip("pmv", dev, ref):
        if not _same_bits(t, a):
            d = np.nonzero(t.view(torch.int32).cpu().numpy() != np.ascontiguousarray(a).view(np.int32))[0]
            i = int(d[0])
            raise AssertionError(f"{what}: {name} differs at {d.size} elements, first {i}: "
                                 f"{float(t[i])!r} vs {float(a[i])!r}")


def _nan_invisible(g, ends, radii):
    g = g.copy()
    P, lo = radii.size, 0
    for e in ends:
        g[lo:e].reshape(P, (e - lo) // P)[radii <= 0] = np.nan
        lo = e
    return g


@pytest.mark.parametrize("M", COEFFS)
@pytest.mark.parametrize("P", SIZES)
def test_three_steps_are_the_reference_bit_for_bit(P, M):
    """Every mask in turn starts a run of three consecutive steps (the masks
    after it in MASKS, cyclically), so moments frozen under one mask are
    carried into the next; fresh gradients per step; p, m, v compared on the
    bits after every step."""
    masks = SR.masks(P)
    p0, _, m0, v0, ends = SR.make_state(P, M, seed=31 * P + M)
    if P == 4997:
        rot = ends[4]  # float offset of the rotation segment
        assert rot == P * (7 + 3 * M) and (4 * rot) % 16 != 0
    grads = [SR.make_state(P, M, seed=31 * P + M + 1 + k)[1] for k in range(3)]
    d_grads = [_dev(g) for g in grads]
    for first in range(len(MASKS)):
        ref = (p0, m0, v0)
        dev = tuple(_dev(a) for a in ref)
        if P == 4997:
            assert (dev[0].data_ptr() + 4 * ends[4]) % 16 != 0
        for k in range(3):
            name = MASKS[(first + k) % len(MASKS)]
            radii = masks[name]
            steps = [k + 1] * 6
            ref = SR.step(ref[0], grads[k], ref[1], ref[2], ends, LRS, steps, radii, *BETAS, EPS)
            _C().sparse_adam_step(dev[0], d_grads[k], dev[1], dev[2], ends, LRS, steps, _dev(radii), *BETAS, EPS)
            _assert_state(dev, ref, f"P={P} M={M} run from {MASKS[first]} step {k} ({name})")
    assert not _same_bits(dev[0], p0)


@pytest.mark.parametrize("name", ["random50", "signed", "none", "last"])
def test_invisible_rows_are_neither_written_nor_read(name):
    """NaN in the gradient of every invisible row: those rows keep p, m, v
    and the visible ones are still the reference's."""
    P, M = 4997, 16
    p, g, m, v, ends = SR.make_state(P, M, seed=5)
    radii = SR.masks(P)[name]
    steps = [3] * 6
    ref = SR.step(p, g, m, v, ends, LRS, steps, radii, *BETAS, EPS)
    dev = (_dev(p), _dev(m), _dev(v))
    _C().sparse_adam_step(dev[0], _dev(_nan_invisible(g, ends, radii)), dev[1], dev[2], ends, LRS, steps, _dev(radii),
                          *BETAS, EPS)
    _assert_state(dev, ref, name)
    inv = np.zeros(ends[-1], bool)
    lo = 0
    for e in ends:
        inv[lo:e].reshape(P, (e - lo) // P)[radii <= 0] = True
        lo = e
    assert inv.any()
    for t, a in zip(dev, (p, m, v)):
        assert np.array_equal(t.cpu().numpy().view(np.int32)[inv], a.view(np.int32)[inv])
        assert not torch.isnan(t).any()


def test_inactive_segments_keep_their_bits():
    P, M = 257, 16
    p, g, m, v, ends = SR.make_state(P, M, seed=9)
    radii = SR.masks(P)["random50"]
    steps = [1, 0, 3, 0, 1, 1]
    g_dev = g.copy()
    g_dev[ends[0]:ends[1]] = np.nan  # an inactive segment's gradient is not read either
    g_dev[ends[2]:ends[3]] = np.nan
    ref = SR.step(p, g, m, v, ends, LRS, steps, radii, *BETAS, EPS)
    dev = (_dev(p), _dev(m), _dev(v))
    _C().sparse_adam_step(dev[0], _dev(g_dev), dev[1], dev[2], ends, LRS, steps, _dev(radii), *BETAS, EPS)
    _assert_state(dev, ref, "inactive segments")
    for lo, hi in ((ends[0], ends[1]), (ends[2], ends[3])):
        for t, a in zip(dev, (p, m, v)):
            assert _same_bits(t[lo:hi], a[lo:hi])
    assert not _same_bits(dev[0][:ends[0]], p[:ends[0]])  # while the others moved


def test_step_with_no_active_group_ignores_a_stale_radii():
    """Right after densify_and_prune every group is inactive and the render
    package's radii have the old length: optimizer_step is a silent no-op."""
    T = _T()
    sc, _cam = G.scene_and_camera(300, 64, 48)
    m = T.FlatGaussianModel(G.raw_from_scene(sc), 3, 1.0, opt=T.OptimizationParams(optimizer_type="sparse_adam"))
    before = (m.params.clone(), m.exp_avg.clone(), m.exp_avg_sq.clone())
    m.optimizer_step(torch.ones(299, dtype=torch.int32, device="cuda"))
    m.optimizer_step(None)
    torch.cuda.synchronize()
    for a, b in zip(before, (m.params, m.exp_avg, m.exp_avg_sq)):
        assert torch.equal(a, b)
    assert all(s == 0 for s in m.steps.values())


def test_one_size_above_the_launch_cap():
    """More rows than one grid pass covers, so the kernel's grid-stride loop
    runs, under a random mask."""
    cap = int(_C().sparse_adam_rows_per_pass())  # rows one launch covers without striding
    P, M = cap + 4997, 4
    assert 59 * P > cap and P > cap
    rng = np.random.default_rng(3)
    ends = SR.flat_layout(P, M)
    n = ends[-1]
    p = rng.standard_normal(n, dtype=np.float32)
    g = rng.standard_normal(n, dtype=np.float32) * np.float32(1e-3)
    m = rng.standard_normal(n, dtype=np.float32) * np.float32(1e-3)
    v = rng.random(n, dtype=np.float32) * np.float32(1e-6)
    radii = np.where(rng.random(P) < 0.5, 5, 0).astype(np.int32)
    radii[-1] = 9
    steps = [2] * 6
    ref = SR.step(p, g, m, v, ends, LRS, steps, radii, *BETAS, EPS)
    dev = (_dev(p), _dev(m), _dev(v))
    _C().sparse_adam_step(dev[0], _dev(g), dev[1], dev[2], ends, LRS, steps, _dev(radii), *BETAS, EPS)
    _assert_state(dev, ref, f"P={P}")
    assert not _same_bits(dev[0][-4:], p[-4:])  # the last row, past the first pass, was updated


def _refusal_cases():
    P, M = 65, 4
    ends = SR.flat_layout(P, M)
    ok = lambda: torch.full((P,), 3, dtype=torch.int32, device="cuda")  # noqa: E731
    shifted = list(ends)
    shifted[0] += 1
    nine = [ends[-1] // 9 * (k + 1) for k in range(8)] + [ends[-1]]
    return P, M, ends, {
        "int64 radii": (ends, lambda: ok().long()),
        "non-contiguous radii": (ends, lambda: torch.full((2 * P,), 3, dtype=torch.int32, device="cuda")[::2]),
        "radii on the CPU": (ends, lambda: ok().cpu()),
        "two-dimensional radii": (ends, lambda: ok().view(P, 1)),
        "radii of the wrong length": (ends, lambda: torch.full((P + 1,), 3, dtype=torch.int32, device="cuda")),
        "a segment that is not whole rows": (shifted, ok),
        "nine segments": (nine, lambda: torch.full((1,), 3, dtype=torch.int32, device="cuda")),
    }


@pytest.mark.parametrize("why", list(_refusal_cases()[3]))
def test_refusals_come_before_any_launch(why):
    P, M, ends, cases = _refusal_cases()
    seg_end, radii = cases[why]
    p, g, m, v, _ = SR.make_state(P, M, seed=1)
    dev = [_dev(a) for a in (p, g, m, v)]
    if why == "nine segments":
        assert len(seg_end) == 9 and seg_end[-1] == dev[0].numel()
    with pytest.raises(RuntimeError):
        _C().sparse_adam_step(dev[0], dev[1], dev[2], dev[3], seg_end, [1e-3] * len(seg_end), [1] * len(seg_end),
                              radii(), *BETAS, EPS)
    torch.cuda.synchronize()
    for t, a in zip(dev, (p, g, m, v)):
        assert _same_bits(t, a), why
    # and the same call with good arguments does update
    _C().sparse_adam_step(dev[0], dev[1], dev[2], dev[3], ends, LRS, [1] * 6,
                          torch.full((P,), 3, dtype=torch.int32, device="cuda"), *BETAS, EPS)
    assert not _same_bits(dev[0], p)


# ------------------------------------------------------- through the trainer ---
@functools.lru_cache(maxsize=None)
def _partly_visible_case():
    """A synthetic scene laid out for the default camera, seen through a
    rotated and shifted one, so part of it is outside the frustum."""
    P, W, H = 3000, 128, 96
    sc, _cam = G.scene_and_camera(P, W, H, seed=2)
    cam = G.general_camera(W, H, "a")
    gt = torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    return sc, G.torch_settings(cam), gt


def _snapshot(m, radii):
    T = _T()
    return {"p": m.params.cpu().numpy().copy(), "g": m.grads.cpu().numpy().copy(),
            "m": m.exp_avg.cpu().numpy().copy(), "v": m.exp_avg_sq.cpu().numpy().copy(),
            "radii": radii.cpu().numpy().copy(), "lr": [float(m.lr[g]) for g in T.GROUPS],
            "active": [int(m.has_grad[g]) for g in T.GROUPS], "ends": list(m.seg_end)}


def _reference_of(snap):
    T = _T()
    return SR.step(snap["p"], snap["g"], snap["m"], snap["v"], snap["ends"], snap["lr"], snap["active"],
                   snap["radii"], T.BETAS[0], T.BETAS[1], T.EPS)


def test_trainer_steps_are_the_reference_applied_to_the_snapshot():
    T = _T()
    sc, s, gt = _partly_visible_case()
    opt = T.OptimizationParams(optimizer_type="sparse_adam", densify_from_iter=10**6, densify_until_iter=0)
    m = T.FlatGaussianModel(G.raw_from_scene(sc), 3, spatial_lr_scale=5.0, opt=opt)
    m.active_sh_degree = 3
    start = m.params.clone()
    for it in range(1, 4):
        pkg, terms = T.forward_backward(m, it, s, gt, fused=True)
        n_vis = int((pkg["radii"] > 0).sum())
        assert 0 < n_vis < m.P, n_vis
        snap = _snapshot(m, pkg["radii"])
        assert all(snap["active"]) and np.isfinite(snap["g"]).all()
        T.post_backward(m, it, pkg, scene_extent=5.0, fused=True)
        _assert_state((m.params, m.exp_avg, m.exp_avg_sq), _reference_of(snap), f"iteration {it}")
        assert all(m.steps[g] == it for g in T.GROUPS)
        invisible = (pkg["radii"] <= 0)
        assert torch.equal(m.group_view(m.params, "f_rest")[invisible],
                           torch.from_numpy(snap["p"]).cuda()[m.seg_end[1]:m.seg_end[2]].view(m.P, 15, 3)[invisible])
    assert not torch.equal(m.params, start)


def test_trainer_crosses_densification_and_opacity_reset():
    """Iterations 1..7 with densification at 3 and 6 and the opacity reset at
    5.  The step of a densification iteration is the no-op (no group has a
    gradient; the package's radii have the old length), the step after the
    reset leaves the opacity group alone and is the reference on the others,
    and training goes on."""
    T = _T()
    sc, s, gt = _partly_visible_case()
    opt = T.OptimizationParams(optimizer_type="sparse_adam", densify_from_iter=2, densification_interval=3,
                               opacity_reset_interval=5, densify_until_iter=100, densify_grad_threshold=1e-7)
    m = T.FlatGaussianModel(G.raw_from_scene(sc), 3, spatial_lr_scale=5.0, opt=opt)
    m.active_sh_degree = 3
    log = []
    inner = m.optimizer_step

    def spy(radii=None):
        snap = _snapshot(m, radii if radii is not None else torch.zeros(0, dtype=torch.int32))
        snap["radii_given"] = radii is not None
        inner(radii)
        snap["after"] = (m.params.clone(), m.exp_avg.clone(), m.exp_avg_sq.clone())
        log.append(snap)

    m.optimizer_step = spy
    sizes, losses = [], []
    torch.manual_seed(0)
    for it in range(1, 8):
        pkg, terms = T.forward_backward(m, it, s, gt, fused=True)
        old_P, steps_before = m.P, dict(m.steps)
        T.post_backward(m, it, pkg, scene_extent=5.0, fused=True)
        snap = log[-1]
        if it in (3, 6):
            assert m.P != old_P and pkg["radii"].numel() == old_P  # the package's radii are stale
            assert not any(snap["active"]) and m.steps == steps_before
            for t, key in zip(snap["after"], "pmv"):
                assert _same_bits(t, snap[key]), (it, key)
        else:
            assert snap["radii_given"] and snap["active"] == [1, 1, 1, int(it != 5), 1, 1]
            _assert_state(snap["after"], _reference_of(snap), f"iteration {it}")
            if it == 5:
                lo, hi = m.seg_end[2], m.seg_end[3]
                assert m.steps["opacity"] == steps_before["opacity"]
                for t, key in zip(snap["after"], "pmv"):
                    assert _same_bits(t[lo:hi], snap[key][lo:hi])
                assert float(snap["after"][1][lo:hi].abs().max()) == 0.0  # the reset zeroed its moments
        sizes.append(m.P)
        losses.append(float(terms["loss"]))
    assert len(log) == 7 and len(set(sizes)) > 1
    assert all(np.isfinite(x) for x in losses) and torch.isfinite(m.params).all()
    assert m.steps["xyz"] == 5 and m.steps["opacity"] == 4


def test_sparse_training_runs_are_bit_identical_in_deterministic_mode():
    from gaussian_splatting_with_eye_tracking_amd import set_deterministic
    T = _T()
    sc, s, gt = _partly_visible_case()
    opt = T.OptimizationParams(optimizer_type="sparse_adam", densify_from_iter=10**6, densify_until_iter=0)

    def run():
        m = T.FlatGaussianModel(G.raw_from_scene(sc), 3, spatial_lr_scale=5.0, opt=opt)
        m.active_sh_degree = 3
        out = []
        for it in range(1, 4):
            T.training_iteration(m, it, s, gt, scene_extent=5.0, fused=True)
            out.append((m.params.clone(), m.exp_avg.clone(), m.exp_avg_sq.clone()))
        return out

    set_deterministic(True)
    try:
        a, b = run(), run()
    finally:
        set_deterministic(None)
    for it, (x, y) in enumerate(zip(a, b), 1):
        for what, u, w in zip("pmv", x, y):
            assert torch.isfinite(u).all() and torch.equal(u.view(torch.int32), w.view(torch.int32)), (it, what)
    assert not torch.equal(a[0][0], a[2][0])


# ------------------------------------------------------------------ C ABI ---
def _c_entry():
    lib = CH.lib()
    LL, D = ctypes.c_longlong, ctypes.c_double
    lib.gs_sparse_adam_step.argtypes = [CH.VP] * 4 + [LL, CH.I, ctypes.POINTER(LL), ctypes.POINTER(D),
                                                      ctypes.POINTER(LL), CH.I, CH.VP, D, D, D, CH.VP]
    lib.gs_sparse_adam_step.restype = CH.I
    return lib


def test_c_entry_on_a_stream_is_the_binding_and_refuses_before_launching():
    lib = _c_entry()
    LL, D = ctypes.c_longlong, ctypes.c_double
    P, M = 4997, 4
    p, g, m, v, ends = SR.make_state(P, M, seed=13)
    radii = _dev(SR.masks(P)["random50"])
    steps = [1, 2, 0, 4, 5, 6]
    a = [_dev(x) for x in (p, g, m, v)]
    b = [_dev(x) for x in (p, g, m, v)]
    _C().sparse_adam_step(a[0], a[1], a[2], a[3], ends, LRS, steps, radii, *BETAS, EPS)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call(seg_end, radii_ptr, n_rows=P):
        k = len(seg_end)
        return lib.gs_sparse_adam_step(CH.ptr(b[0]), CH.ptr(b[1]), CH.ptr(b[2]), CH.ptr(b[3]), b[0].numel(), k,
                                       (LL * k)(*seg_end), (D * k)(*LRS[:k]), (LL * k)(*steps[:k]), n_rows, radii_ptr,
                                       BETAS[0], BETAS[1], EPS, CH.VP(stream.cuda_stream))

    # errors first: nothing may have been launched on b
    assert call(ends, CH.VP(0)) < 0 and "radii" in lib.gs_last_error().decode()
    shifted = [ends[0] + 1] + ends[1:]
    assert call(shifted, CH.ptr(radii)) < 0 and "whole rows" in lib.gs_last_error().decode()
    stream.synchronize()
    for t, x in zip(b, (p, g, m, v)):
        assert _same_bits(t, x)
    CH.check(lib, call(ends, CH.ptr(radii)), "gs_sparse_adam_step")
    stream.synchronize()
    for t, u in zip(a, b):
        assert torch.equal(t.view(torch.int32), u.view(torch.int32))
    assert not _same_bits(b[0], p)
    _assert_state((b[0], b[2], b[3]), SR.step(p, g, m, v, ends, LRS, steps, SR.masks(P)["random50"], *BETAS, EPS), "C")
