"""The training-step kernels of csrc/train.hip, called through ``_C``
directly and held element by element to float64 references
(tests/train_reference.py, pinned to torch autograd by
tests/test_train_reference.py) or, for Adam, to torch.optim.Adam's bits.

What the end-to-end training tests leave open and these close:

* sizes that are no multiple of 4, so that in the trainer's flat buffer the
  rotation rows -- read and written as float4 -- start at a float offset that
  is not 16-byte aligned (asserted per case);
* sizes above the launch caps (256*32 blocks for the activations, 256*64 for
  Adam), so the grid-stride loops run;
* M = 1, 4, 9 (max_sh_degree 0, 1, 2; at M = 1 features_rest is empty);
* ``accumulate = True``;
* Adam's segment walk with empty, one-element and eight segments, boundaries
  inside a wave and at the grid cap, a zero learning rate, a first step next
  to step 1,000,000;
* the densification statistics at several P and gradient row strides.

Every test prints the worst error-to-bound ratio per output (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

import train_reference as TR

pytestmark = pytest.mark.gpu

SH_DEGREE = {1: 0, 4: 1, 9: 2, 16: 3}
ACT_CAP = 256 * 32 * 256   # elements one pass of the activation kernels covers
ADAM_CAP = 256 * 64 * 256  # ... and of adam_kernel
GUARD = 64                 # floats of sentinel on either side of a flat buffer (keeps its 16-byte alignment)
SENTINEL = 12345.0

# (P, M, flat): flat = the raw groups and their gradients are views of one
# buffer in FlatGaussianModel._layout's order.  The rotation segment then
# starts at float offset P (7 + 3 M); that is a multiple of 4 -- aligned --
# only for (4998, 9) (34 * 4998), so (4997, 9) stands beside it.
CASES = [(1, 16, False), (255, 16, True), (257, 4, True), (4999, 16, True), (4998, 9, True), (4997, 9, True),
         (4997, 1, True), (43_703, 16, True), (2_097_157, 1, False)]
ALIGNED_FLAT = {(4998, 9)}
CASE_IDS = [f"P{p}-M{m}" for p, m, _ in CASES]


def _C():
    from gaussian_splatting_with_eye_tracking_amd import _C as c
    return c


def _T():
    from gaussian_splatting_with_eye_tracking_amd import training
    return training


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, fill):
    """A flat [n] f32 device buffer with GUARD sentinel floats on either side."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    flat = whole[GUARD:GUARD + n]
    assert flat.data_ptr() % 16 == 0
    if isinstance(fill, torch.Tensor):
        flat.copy_(fill)
    else:
        flat.fill_(fill)
    return whole, flat


def _guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _case(P, M, flat):
    """Inputs on the device and the float64 reference, computed once per case
    and shared by the forward, backward and accumulate tests (read-only)."""
    T = _T()
    case = TR.raw_inputs(P, M, seed=1000 * M + P % 997)
    raw, cot = case["raw"], case["cot"]
    sizes = [P * int(np.prod(T.group_row_shape(g, SH_DEGREE[M]))) for g in T.GROUPS]
    ends = np.cumsum(sizes).tolist()
    los = [0] + ends[:-1]
    n = ends[-1]
    rot_offset = los[T.GROUPS.index("rotation")]
    assert rot_offset == P * (7 + 3 * M)
    if flat:
        m = T.FlatGaussianModel({g: _dev(raw[g]) for g in T.GROUPS}, SH_DEGREE[M], 1.0)
        assert m.seg_end == ends  # the trainer's own layout
        whole, params = _guarded(n, m.params)
        views = {g: params[lo:hi].view(raw[g].shape) for g, lo, hi in zip(T.GROUPS, los, ends)}
    else:
        whole, params = None, None
        views = {g: _dev(raw[g]) for g in T.GROUPS}
    ref_fwd = TR.activate(raw["f_dc"], raw["f_rest"], raw["opacity"], raw["scaling"], raw["rotation"])
    ref_bwd, mags = TR.activation_backward(cot["d_shs"], cot["d_opac"], cot["d_scales"], cot["d_rot"],
                                           cot["d_means3D"], raw["opacity"], raw["scaling"], raw["rotation"])
    cot_of = {"xyz": cot["d_means3D"], "f_dc": cot["d_shs"][:, :1], "f_rest": cot["d_shs"][:, 1:],
              "opacity": cot["d_opac"], "scaling": cot["d_scales"], "rotation": cot["d_rot"]}
    return dict(P=P, M=M, flat=flat, raw=raw, cot=cot, cot_of=cot_of, dcot={k: _dev(v) for k, v in cot.items()},
                views=views, params_whole=whole, params_bits=None if params is None else params.clone(),
                params=params, los=los, ends=ends, n=n, rot_offset=rot_offset, ref_fwd=ref_fwd, ref_bwd=ref_bwd,
                mags=mags)


def _assert_coverage(c):
    """What the cases exist for, so it cannot silently disappear: the two
    large ones take the grid-stride loops, and the flat ones have rotation
    rows that are not 16-byte aligned (one, the trainer's layout at
    (4998, 9), has aligned rows inside the flat buffer)."""
    if c["P"] == 43_703:
        assert c["P"] * c["M"] * 3 > ACT_CAP >= c["P"]  # the SH loop strides
    if c["P"] == 2_097_157:
        assert c["P"] > ACT_CAP  # the per-Gaussian loop strides too
    if not c["flat"]:
        return
    ptr = c["views"]["rotation"].data_ptr()
    if (c["P"], c["M"]) in ALIGNED_FLAT:
        assert c["rot_offset"] % 4 == 0 and ptr % 16 == 0
    else:
        assert c["rot_offset"] % 4 != 0 and ptr % 16 != 0, (c["rot_offset"], ptr % 16)


def _grad_buffers(c, fill):
    """Gradient outputs: views of one guarded flat buffer (flat cases) or
    separate tensors, pre-filled with `fill` (a value, or per-group arrays)."""
    T = _T()
    if c["flat"]:
        init = fill if not isinstance(fill, dict) else torch.cat([_dev(fill[g]).reshape(-1) for g in T.GROUPS])
        whole, flat = _guarded(c["n"], init)
        views = {g: flat[lo:hi].view(c["raw"][g].shape) for g, lo, hi in zip(T.GROUPS, c["los"], c["ends"])}
        if (c["P"], c["M"]) not in ALIGNED_FLAT:
            assert views["rotation"].data_ptr() % 16 != 0
        return whole, views
    if isinstance(fill, dict):
        return None, {g: _dev(fill[g]) for g in T.GROUPS}
    return None, {g: torch.full(c["raw"][g].shape, fill, dtype=torch.float32, device="cuda") for g in T.GROUPS}


def _backward(c, gv, accumulate):
    v, d = c["views"], c["dcot"]
    _C().activation_backward(d["d_shs"], d["d_opac"], d["d_scales"], d["d_rot"], d["d_means3D"], v["opacity"],
                             v["scaling"], v["rotation"], gv["xyz"], gv["f_dc"], gv["f_rest"], gv["opacity"],
                             gv["scaling"], gv["rotation"], accumulate)
    torch.cuda.synchronize()


def _worst(got, ref, bound, what):
    """max |got - ref| / bound over the elements; where the bound is 0 the
    element must be exact.  Fails with the first offender."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} elements not finite (not written?)"
    err = np.abs(got - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    w = float(ratio.max())
    if w > 1.0:
        i = int(np.argmax(ratio))
        raise AssertionError(f"{what}: {int((ratio > 1).sum())}/{got.size} outside the bound, worst x{w:.3g} at flat "
                             f"{i} (row {i // max(1, got[0].size)}): got {got.flat[i]!r}, ref {ref.flat[i]!r}, "
                             f"bound {bound.flat[i]:.3e}")
    return w


def _unchanged_inputs(c):
    if c["flat"]:
        assert torch.equal(c["params"], c["params_bits"]), "a kernel wrote into its inputs"
        assert _guards_intact(c["params_whole"])


# ----------------------------------------------------------- activations ---
@pytest.mark.parametrize("P,M,flat", CASES, ids=CASE_IDS)
def test_activate_matches_float64(P, M, flat):
    """shs is a copy: bit-exact.  opacities, scales and rotations within
    rtol 2e-6 + atol 1e-7 of float64 (test_gpu_ply.py's bar).  Outputs start
    as NaN, so a finite result shows every element was written."""
    c = _case(P, M, flat)
    _assert_coverage(c)
    v = c["views"]
    out = {"shs": (P, M, 3), "opacities": (P, 1), "scales": (P, 3), "rotations": (P, 4)}
    out = {k: torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for k, s in out.items()}
    _C().activate(v["f_dc"], v["f_rest"], v["opacity"], v["scaling"], v["rotation"], out["shs"], out["opacities"],
                  out["scales"], out["rotations"])
    torch.cuda.synchronize()
    _unchanged_inputs(c)
    got = {k: t.cpu().numpy() for k, t in out.items()}
    assert np.isfinite(got["shs"]).all()
    np.testing.assert_array_equal(got["shs"], c["ref_fwd"]["shs"].astype(np.float32))
    worst = {}
    for k in ("opacities", "scales", "rotations"):
        r = c["ref_fwd"][k]
        worst[k] = _worst(got[k], r, 2e-6 * np.abs(r) + 1e-7, f"activate {k} P={P} M={M}")
    print(f"activate P={P} M={M}: worst error/bound {worst}")


def _base_bound(c, g):
    """|k - r| <= 2e-6 A + 1e-7 |cotangent| (0 for the copied groups)."""
    if g in ("xyz", "f_dc", "f_rest"):
        return np.zeros(c["ref_bwd"][g].shape)
    return 2e-6 * c["mags"][g] + 1e-7 * np.abs(c["cot_of"][g].astype(np.float64))


@pytest.mark.parametrize("P,M,flat", CASES, ids=CASE_IDS)
def test_activation_backward_matches_float64(P, M, flat):
    """accumulate = False over NaN-filled outputs.  g_xyz, g_dc, g_rest are
    bit-exact copies; g_scaling, g_opacity, g_rotation obey
    |k - r| <= 2e-6 A + 1e-7 |cotangent|, A the sum of the absolute terms
    (train_reference).  Rounding count of the longest chain, the rotation's
    norm term, in units of 2^-24 relative to A: |r|^2 by 4 products and 3
    sums of positive terms (<= 4), its square root (+1, halved: <= 3 on d and
    on |r|); g.r by 4 products and 3 sums (<= 4 of sum |g_j r_j|); d*d (7),
    the division by it (1), the division by |r| (3 + 1), the product with r_i
    (1), the final sum (1): 18 roundings, so 2e-6 (34 * 2^-24) holds with
    room.  The sigmoid costs expf (1 ulp), 1 + e and the reciprocal: below
    2^-24 + 2^-25 = 8.9e-8 absolute on sigma, which the 1e-7 |cotangent| term
    carries where 1 - sigma cancels (for float32, 1 - sigma is exactly 0 from
    x = 17 up)."""
    c = _case(P, M, flat)
    _assert_coverage(c)
    whole, gv = _grad_buffers(c, float("nan"))
    _backward(c, gv, False)
    _unchanged_inputs(c)
    assert whole is None or _guards_intact(whole), "write outside the gradient buffer"
    worst = {}
    for g in _T().GROUPS:
        got = gv[g].cpu().numpy()
        if g in ("xyz", "f_dc", "f_rest"):
            assert np.isfinite(got).all(), g
            np.testing.assert_array_equal(got, c["cot_of"][g], err_msg=g)
        else:
            worst[g] = _worst(got, c["ref_bwd"][g], _base_bound(c, g), f"backward {g} P={P} M={M}")
    print(f"activation_backward P={P} M={M}: worst error/bound {worst}")


@pytest.mark.parametrize("P,M,flat", CASES, ids=CASE_IDS)
def test_activation_backward_accumulates(P, M, flat):
    """accumulate = True over random prior contents g0: g0 + r within the
    bound above plus 2^-23 |g0 + r| (the one float32 addition).  The copied
    groups are one IEEE addition of two float32 values: exactly
    fl(g0 + cotangent).  A second call adds the same amount again:
    g0 + 2 r within twice the base bound plus both additions' roundings."""
    c = _case(P, M, flat)
    _assert_coverage(c)
    rng = np.random.default_rng(7 + P)
    g0 = {g: rng.standard_normal(c["raw"][g].shape).astype(np.float32) for g in _T().GROUPS}
    whole, gv = _grad_buffers(c, g0)
    worst = {}
    first = {}
    for call in (1, 2):
        _backward(c, gv, True)
        assert whole is None or _guards_intact(whole), "write outside the gradient buffer"
        for g in _T().GROUPS:
            got = gv[g].cpu().numpy()
            if g in ("xyz", "f_dc", "f_rest"):
                prev = g0[g] if call == 1 else first[g]
                np.testing.assert_array_equal(got, prev + c["cot_of"][g], err_msg=f"{g} call {call}")
            else:
                r = c["ref_bwd"][g]
                e1 = g0[g].astype(np.float64) + r
                if call == 1:
                    want, bound = e1, _base_bound(c, g) + 2.0 ** -23 * np.abs(e1)
                else:
                    want = e1 + r
                    bound = 2 * _base_bound(c, g) + 2.0 ** -23 * (np.abs(e1) + np.abs(want))
                worst[f"{g}/{call}"] = _worst(got, want, bound, f"accumulate call {call} {g} P={P} M={M}")
            first[g] = got
    _unchanged_inputs(c)
    print(f"activation_backward accumulate P={P} M={M}: worst error/bound {worst}")


# ------------------------------------------------------------------ Adam ---
ADAM_N = ADAM_CAP + 777
ADAM_ENDS = [1, 1, 65, 4097, 1_000_003, 2_500_000, ADAM_CAP, ADAM_N]
ADAM_STEPS = [1, 5, 0, 1_000_000, 3, 0, 1, 7]
ADAM_LRS = [1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 0.0, 5e-3, 1e-3, 2.5e-3]  # segment 4 (step 3) does not move p
BETAS, EPS = (0.9, 0.999), 1e-15


def _adam_buffers(seed=0):
    gen = torch.Generator().manual_seed(seed)
    N = ADAM_N
    p = torch.randn(N, generator=gen)
    m = torch.randn(N, generator=gen) * 1e-4
    v = torch.rand(N, generator=gen) * 1e-8
    g = torch.randn(N, generator=gen)
    lo = 0
    for hi, step in zip(ADAM_ENDS, ADAM_STEPS):
        g[lo:hi] *= 10.0 ** float(torch.randint(-9, 1, (1,), generator=gen))
        if step == 1:  # a first step starts from zero moments
            m[lo:hi] = 0.0
            v[lo:hi] = 0.0
        lo = hi
    g[torch.rand(N, generator=gen) < 0.05] = 0.0
    return [t.cuda() for t in (p, g, m, v)]


def _bits(t):
    return t.view(torch.int32)


def test_adam_segments_match_torch_adam_bitwise():
    """Eight segments (one element, empty, boundaries inside a wave at 65 and
    4097, at the grid cap, 777 elements past it), steps 1 / 1,000,000 / 0, a
    zero learning rate: p, m, v bit-identical to torch.optim.Adam with one
    Parameter per non-empty segment (DESIGN §1's bar), bit-unchanged where
    the step is 0, p bit-unchanged where lr = 0 while m and v move."""
    assert ADAM_N > ADAM_CAP and ADAM_ENDS[-1] == ADAM_N
    p, g, m, v = _adam_buffers()
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    params, groups = [], []
    opt_state = {}
    lo = 0
    for hi, step, lr in zip(ADAM_ENDS, ADAM_STEPS, ADAM_LRS):
        if hi > lo:
            q = torch.nn.Parameter(p0[lo:hi].clone())
            q.grad = g[lo:hi].clone() if step > 0 else None
            if step > 1:
                opt_state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0[lo:hi].clone(),
                                "exp_avg_sq": v0[lo:hi].clone()}
            params.append((lo, hi, step, lr, q))
            groups.append({"params": [q], "lr": lr})
        lo = hi
    opt = torch.optim.Adam(groups, lr=0.0, betas=BETAS, eps=EPS)
    for q, st in opt_state.items():
        opt.state[q] = st
    opt.step()
    _C().adam_step(p, g, m, v, ADAM_ENDS, ADAM_LRS, ADAM_STEPS, BETAS[0], BETAS[1], EPS)
    torch.cuda.synchronize()
    assert len(params) == 7
    for lo, hi, step, lr, q in params:
        what = f"segment [{lo}, {hi}) step {step} lr {lr}"
        if step == 0:
            for now, was in ((p, p0), (m, m0), (v, v0)):
                assert torch.equal(_bits(now[lo:hi]), _bits(was[lo:hi])), what
            assert q not in opt.state
            continue
        st = opt.state[q]
        assert int(st["step"]) == step
        for name, now, want in (("p", p, q.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
            same = _bits(now[lo:hi]) == _bits(want)
            assert bool(same.all()), f"{what}: {name} differs from torch in {int((~same).sum())}/{hi - lo} elements"
        if lr == 0.0:
            assert torch.equal(_bits(p[lo:hi]), _bits(p0[lo:hi])), what
            assert not torch.equal(m[lo:hi], m0[lo:hi]) and not torch.equal(v[lo:hi], v0[lo:hi]), what
        else:
            assert float((p[lo:hi] != p0[lo:hi]).float().mean()) > 0.9, what


@pytest.mark.parametrize("ends,n_lr,why", [
    ([100 * (i + 1) for i in range(8)] + [1000], 9, "9 segments"),
    ([100, 200, 900], 3, "ends that do not reach numel"),
    ([100, 50, 1000], 3, "decreasing ends"),
])
def test_adam_refuses_bad_segments(ends, n_lr, why):
    gen = torch.Generator().manual_seed(1)
    bufs = [torch.randn(1000, generator=gen).cuda() for _ in range(4)]
    before = [b.clone() for b in bufs]
    with pytest.raises(RuntimeError):
        _C().adam_step(bufs[0], bufs[1], bufs[2], bufs[3], ends, [1e-3] * n_lr, [1] * n_lr, BETAS[0], BETAS[1], EPS)
    torch.cuda.synchronize()
    for b, was in zip(bufs, before):  # nothing was launched
        assert torch.equal(_bits(b), _bits(was)), why


# ----------------------------------------------- densification statistics ---
@pytest.mark.parametrize("layout", ["rows3", "rows2", "view2of4"])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 3001])
def test_densify_stats_matches_float64(P, layout):
    """Gradient rows of stride 3, 2 and 4; radii of 0, negative, 1 and 5000;
    one visible row with a NaN gradient; statistics that start non-zero with
    max_radii2D above and below the new radius.  denom and max_radii2D exact,
    xyz_gradient_accum rtol 1e-6, rows with radii <= 0 bit-unchanged in all
    three, the NaN in its own row only."""
    rng = np.random.default_rng(P)
    width = {"rows3": 3, "rows2": 2, "view2of4": 4}[layout]
    radii = rng.choice(np.array([0, -3, 1, 5000], np.int32), P)
    radii[0] = 5000
    grad = (rng.standard_normal((P, width)) * 10.0 ** rng.integers(-6, 1, (P, 1))).astype(np.float32)
    nan_row = P // 2
    radii[nan_row] = 1
    if P > 1:
        grad[nan_row, 1] = np.nan
    accum = rng.uniform(0.0, 2.0, (P, 1)).astype(np.float32)
    denom = rng.integers(0, 9, (P, 1)).astype(np.float32)
    mx = rng.choice(np.array([0.0, 3.0, 9000.0], np.float32), P)
    g_dev = _dev(grad)
    g_arg = g_dev[:, :2] if layout == "view2of4" else g_dev
    assert g_arg.stride(0) == {"rows3": 3, "rows2": 2, "view2of4": 4}[layout] and g_arg.stride(1) == 1
    d_accum, d_denom, d_mx = _dev(accum), _dev(denom), _dev(mx)
    _C().densify_stats(_dev(radii), g_arg, d_accum, d_denom, d_mx)
    torch.cuda.synchronize()
    a, d, m = d_accum.cpu().numpy(), d_denom.cpu().numpy(), d_mx.cpu().numpy()
    ra, rd, rm = TR.densify_stats(radii, grad, accum, denom, mx)
    np.testing.assert_array_equal(d, rd)
    np.testing.assert_array_equal(m, rm)
    hidden = radii <= 0
    for now, was in ((a, accum), (d, denom), (m, mx)):
        assert np.array_equal(now[hidden].view(np.int32), was[hidden].view(np.int32))
    nan = np.isnan(a).reshape(-1)
    if P > 1:
        assert nan[nan_row] and int(nan.sum()) == 1 and np.isnan(ra[nan_row, 0])
    else:
        assert not nan.any()
    ok = ~nan
    err = np.abs(a[ok] - ra[ok])
    bound = 1e-6 * np.abs(ra[ok])
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), (P, layout, worst)
    print(f"densify_stats P={P} {layout}: worst error/bound {worst:.3f}")
