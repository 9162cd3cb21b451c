"""The deterministic blend backward (gs_rasterizer_backward_deterministic,
``set_deterministic``): the blend stores its per-(tile, Gaussian) terms as
rows of a scratch array, and a reduction sums each Gaussian's rows in
ascending tile index, in float64, rounding once -- no float atomics.

What is held here:
* the same gradients as the default path, against the oracle with the same
  bars (L2 1e-4, and the element-wise allowance of the default path);
* the same BITS from any two runs -- of one forward, of two forwards, with
  another launch order (zeroed work buckets), under other tunings, through
  the C ABI with a NaN-filled scratch, through autograd, through the view
  records, and over three training iterations;
* the clean-flag logic of grad_accum for any order of deterministic and
  default calls on one forward;
* the edges (P = 0, K = 0) and the AMR backward's refusal.
"""
import ctypes
import functools
import os
import warnings

import numpy as np
import pytest

import gs_helpers as G
from capi_helpers import F, I, VP, ptr as _p

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
         "dL_drotations"]
SHAPES = {c[0]: c[1:] for c in G.PARITY_CASES}
THREE = ["g1_64_32x32", "ragged_3k_250x130", "dense_20k_128"]
BG = (0.2, 0.1, 0.05)


def _C():
    import gaussian_splatting_with_eye_tracking_amd._C as C
    return C


@functools.lru_cache(maxsize=None)
def _case(name, variant="sh"):
    """Inputs of one case (built once, never modified)."""
    from gaussian_splatting_with_eye_tracking_amd import synthetic as S
    P, W, H, seed = SHAPES[name]
    sc, cam = G.scene_and_camera(P, W, H, seed)
    colors = cov = None
    if variant == "colors_precomp":
        colors = np.random.default_rng(seed + 5).uniform(0, 1, (P, 3)).astype(np.float32)
    if variant == "cov3D_precomp":
        _, r0, _ = G.oracle_forward(sc, cam)
        cov = r0.cov3D.copy()
        cov[r0.radii <= 0] = np.array([1e-4, 0, 0, 1e-4, 0, 1e-4], np.float32)
    return dict(P=P, W=W, H=H, seed=seed, sc=sc, cam=cam, colors=colors, cov=cov,
                dpix=S.make_cotangent(H, W, seed + 1))


@functools.lru_cache(maxsize=None)
def _oracle(name, variant="sh"):
    """The oracle's gradients and allowance of one case (computed once)."""
    import oracle as O
    c = _case(name, variant)
    os_, ref, kw = G.oracle_forward(c["sc"], c["cam"], c["colors"], c["cov"], bg=BG)
    rg = O.backward(os_, ref, c["sc"].means3D, c["dpix"], **kw)
    al, ties = O.grad_allowance(os_, ref, c["sc"].means3D, c["dpix"], parts=True, **kw)
    return ref, rg, al, ties


def _forward(c):
    return G.native_forward(c["sc"], c["cam"], c["colors"], c["cov"], bg=BG)


def _backward(c, fwd, det, lean=False):
    """The raw backward binding on one forward, with the native flag at `det`."""
    return G.native_backward(fwd, c["dpix"], det=det, lean=lean)


def _assert_same_bits(a, b, what=""):
    for n, x, y in zip(NAMES, a, b):
        assert x.shape == y.shape, (what, n)
        assert torch.equal(x, y), (what, n, float((x - y).abs().max()))


# ------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("name,variant", [("g1_64_32x32", "sh"), ("ragged_3k_250x130", "sh"), ("dense_20k_128", "sh"),
                                          ("ragged_3k_250x130", "colors_precomp"),
                                          ("ragged_3k_250x130", "cov3D_precomp")])
def test_matches_oracle(name, variant):
    c = _case(name, variant)
    ref, rg, al, ties = _oracle(name, variant)
    grads = _backward(c, _forward(c), True)
    for n, g in zip(NAMES, grads):
        gg = g.cpu().numpy()
        assert gg.shape == rg[n].shape, n
        assert np.all(np.isfinite(gg)), n
        err = G.rel_err(gg, rg[n])
        print(f"{name} {variant} {n}: rel_err {err:.3e}")
        assert err < G.GRAD_REL_TOL, (n, err)
    G.assert_grads_elementwise(f"deterministic_backward_{name}_{variant}", NAMES, grads, rg, c["sc"], c["cam"], ref,
                               allow=al, ties=ties)


# ------------------------------------------------- 2. bit-reproducible
@pytest.mark.parametrize("name", THREE)
def test_bit_reproducible(name):
    c = _case(name)
    fa = _forward(c)
    d1 = _backward(c, fa, True)
    d2 = _backward(c, fa, True)
    _assert_same_bits(d1, d2, "one forward")
    assert float(d1[2].abs().sum()) > 0  # the case has gradient at all
    fb = _forward(c)
    d3 = _backward(c, fb, True)
    _assert_same_bits(d1, d3, "two forwards")
    # default -> deterministic -> default on one (fresh) forward: the first
    # default call takes the forward's clean accumulator rows, the
    # deterministic one overwrites them, the second default call must zero them
    fc = _forward(c)
    a0 = _backward(c, fc, False)
    dd = _backward(c, fc, True)
    a1 = _backward(c, fc, False)
    _assert_same_bits(d1, dd, "after a default call")
    for n, x, y in zip(NAMES, a1, a0):
        assert G.rel_err(x.cpu().numpy(), y.cpu().numpy()) < 1e-5, n
    # and deterministic first (the clean flag taken without a memset), default after
    fd = _forward(c)
    _assert_same_bits(d1, _backward(c, fd, True), "deterministic first")
    a2 = _backward(c, fd, False)
    for n, x, y in zip(NAMES, a2, a0):
        assert G.rel_err(x.cpu().numpy(), y.cpu().numpy()) < 1e-5, n


# ------------------------------------------ 3. independent of launch order
@pytest.mark.parametrize("name", THREE)
def test_independent_of_launch_order_and_tunings(name):
    import gaussian_splatting_with_eye_tracking_amd as pkg
    c = _case(name)
    base = _backward(c, _forward(c), True)
    # the work buckets zeroed: every block takes the identity tile order
    lib = ctypes.CDLL(os.path.join(os.path.dirname(pkg.__file__), "libgsplat_amd.so"))
    view = (ctypes.c_void_p * 19)()
    origin = 1 << 20
    assert lib.gs_image_view_of(ctypes.c_void_p(origin), c["W"], c["H"], 16, ctypes.byref(view)) == 0
    off = view[15] - origin  # bucket_count
    f = _forward(c)
    f[2][5][off:off + 1024].zero_()
    _assert_same_bits(base, _backward(c, f, True), "zeroed work buckets")
    with G.tuning(bwd_variant=0):
        _assert_same_bits(base, _backward(c, _forward(c), True), "bwd_variant 0")
    with G.tuning(cull=0):
        r0 = _backward(c, _forward(c), True)
    with G.tuning(cull=1):
        r1 = _backward(c, _forward(c), True)
    _assert_same_bits(r0, r1, "cull 0 / 1")


# ------------------------------------------ 4. close to the default path
@pytest.mark.parametrize("name", THREE)
def test_close_to_default_path(name):
    c = _case(name)
    f = _forward(c)
    det = _backward(c, f, True)
    dflt = _backward(c, _forward(c), False)
    for n, x, y in zip(NAMES, det, dflt):
        err = G.rel_err(x.cpu().numpy(), y.cpu().numpy())
        print(f"{name} {n}: deterministic vs default rel_err {err:.3e}")
        assert err < 1e-5, (n, err)
    # the autograd wrappers' binding: the same bits
    lean = _backward(c, f, True, lean=True)
    for n, x, y in zip(NAMES, det, lean):
        if n in ("dL_dcolors", "dL_dcov3D"):
            assert y.numel() == 0, n
        else:
            assert torch.equal(x, y), n


@pytest.mark.parametrize("variant", ["sh", "colors_precomp"])
@pytest.mark.parametrize("name", ["g1_64_32x32", "ragged_3k_250x130"])
def test_base_backward_bindings_agree(name, variant):
    """The four base backward bindings reach the library through one call: on
    one forward, under the deterministic flag (bit-reproducible), _lean, and
    _aux / _aux_lean with both map cotangents empty, return
    rasterize_gaussians_backward's bits -- the lean forms with dL_dcolors /
    dL_dcov3D empty exactly when that input was -- and a map cotangent under
    the flag is still refused."""
    c = _case(name, variant)
    fwd = _forward(c)
    plain = G.native_backward(fwd, c["dpix"], det=True)
    given = {"dL_dcolors": c["colors"] is not None, "dL_dcov3D": c["cov"] is not None}
    for kw in (dict(lean=True), dict(aux=(None, None)), dict(aux=(None, None), lean=True)):
        got = G.native_backward(fwd, c["dpix"], det=True, **kw)
        for n, x, y in zip(NAMES, plain, got):
            if kw.get("lean") and not given.get(n, True):
                assert y.numel() == 0, (kw, n)
            else:  # (the plain form's, so not empty where the input was given)
                assert x.shape == y.shape and torch.equal(x, y), (kw, n)
    dalpha = np.ones((1, c["H"], c["W"]), np.float32)
    for lean in (False, True):
        with pytest.raises(RuntimeError, match="no deterministic aux backward is built"):
            G.native_backward(fwd, c["dpix"], det=True, aux=(None, dalpha), lean=lean)


# --------------------------------------------------------- 5. autograd
def _autograd_grads(c, keys=("means3D", "opacities", "shs", "scales", "rotations")):
    from diff_gaussian_rasterization import GaussianRasterizer
    s = G.torch_settings(c["cam"], bg=BG)
    t = G.scene_tensors(c["sc"], requires_grad=True)
    means2D = torch.zeros_like(t["means3D"], requires_grad=True)
    color, radii = GaussianRasterizer(s)(means3D=t["means3D"], means2D=means2D, opacities=t["opacities"],
                                         shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    (color * torch.from_numpy(c["dpix"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    out = {k: t[k].grad.clone() for k in keys}
    out["means2D"] = means2D.grad.clone()
    return out


def _direct_as_autograd(c):
    d = dict(zip(NAMES, _backward(c, _forward(c), True)))
    return {"means3D": d["dL_dmeans3D"], "opacities": d["dL_dopacity"], "shs": d["dL_dsh"],
            "scales": d["dL_dscales"], "rotations": d["dL_drotations"], "means2D": d["dL_dmeans2D"]}


def test_autograd_follows_torch_flag_and_set_deterministic(monkeypatch):
    from gaussian_splatting_with_eye_tracking_amd import set_deterministic
    C = _C()
    c = _case("ragged_3k_250x130")
    direct = _direct_as_autograd(c)
    # the native flag as each autograd backward's native call sees it
    seen = []
    native = C.rasterize_gaussians_backward_lean

    def spy(*a):
        seen.append(C.get_deterministic_backward())
        return native(*a)

    monkeypatch.setattr(C, "rasterize_gaussians_backward_lean", spy)
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        g1 = _autograd_grads(c)
        g2 = _autograd_grads(c)
        for k in g1:
            assert torch.equal(g1[k], g2[k]), k
            assert torch.equal(g1[k], direct[k]), k
        assert seen == [True, True]
        assert C.get_deterministic_backward() is False  # restored after the native call
        # False overrides torch's flag: the default path (within its atomic-order noise)
        set_deterministic(False)
        g3 = _autograd_grads(c)
        assert seen[2:] == [False]
        for k in g3:
            assert G.rel_err(g3[k].cpu().numpy(), direct[k].cpu().numpy()) < 1e-5, k
        torch.use_deterministic_algorithms(False)
        # True works with torch's flag off
        set_deterministic(True)
        g4 = _autograd_grads(c)
        assert seen[3:] == [True]
        for k in g4:
            assert torch.equal(g4[k], direct[k]), k
        # None + torch's flag off: the default path, nothing changes
        set_deterministic(None)
        assert C.get_deterministic_backward() is False
        g5 = _autograd_grads(c)
        assert seen[4:] == [False]
        for k in g5:
            assert G.rel_err(g5[k].cpu().numpy(), direct[k].cpu().numpy()) < 1e-5, k
    finally:
        set_deterministic(None)
        torch.use_deterministic_algorithms(was)


def test_amr_autograd_backward_refuses_under_torch_flag():
    from diff_gaussian_rasterization_amr import GaussianRasterizer
    sc, cam = G.scene_and_camera(500, 64, 64, 1)
    s = G.torch_settings(cam, amr=True)
    t = G.scene_tensors(sc, requires_grad=True)

    def loss():
        color, *_ = GaussianRasterizer(s)(
            means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], shs=t["shs"],
            scales=t["scales"], rotations=t["rotations"], foveaStep=-2, interpolate_image=False)
        return (color * color).sum()

    was = torch.are_deterministic_algorithms_enabled()
    was_warn = torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        with pytest.raises(RuntimeError, match="amr_rasterize_gaussians_backward"):
            loss().backward()
        torch.use_deterministic_algorithms(True, warn_only=True)
        t["means3D"].grad = None
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            loss().backward()
        assert any("amr_rasterize_gaussians_backward" in str(x.message) for x in w)
        assert t["means3D"].grad is not None and torch.isfinite(t["means3D"].grad).all()
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)


# ---------------------------------------------------- 6. view records
def test_view_records_bit_identical():
    C = _C()
    ca, cb = _case("ragged_3k_250x130"), _case("ragged_3k_250x130", "colors_precomp")
    e = torch.Tensor([])

    def record(c, det=True):
        s, t, (K, color, radii, geom, binning, img) = _forward(c)
        col = e if c["colors"] is None else torch.from_numpy(c["colors"]).cuda()
        prev = C.get_deterministic_backward()
        C.set_deterministic_backward(det)
        try:
            r = C.rasterize_gaussians_backward_view_grads(s.bg, radii, col, s.viewmatrix, s.projmatrix, s.tanfovx,
                                                          s.tanfovy, s.campos, torch.from_numpy(c["dpix"]).cuda(),
                                                          geom, K, binning, img, False)
            torch.cuda.synchronize()
        finally:
            C.set_deterministic_backward(prev)
        return r

    for c in (ca, cb):
        r1, r2 = record(c), record(c)
        assert torch.isfinite(r1).all() and torch.equal(r1, r2)
        rd = record(c, det=False)
        assert G.rel_err(r1.cpu().numpy(), rd.cpu().numpy()) < 1e-5
    # two SH views (the same scene, two cotangents) through the multi-view backward
    from gaussian_splatting_with_eye_tracking_amd import synthetic as S
    c2 = dict(ca, dpix=S.make_cotangent(ca["H"], ca["W"], 99))
    t = G.scene_tensors(ca["sc"])

    def multiview():
        views = torch.stack([record(ca), record(c2)])
        out = C.backward_gaussians_multiview(views, t["means3D"], t["shs"], 3, t["scales"], t["rotations"], 1.0, e, e,
                                             e)
        torch.cuda.synchronize()
        return out

    m1, m2 = multiview(), multiview()
    for x, y in zip(m1, m2):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    assert float(m1[0].abs().sum()) > 0


# ---------------------------------------------------- 7. the C ABI
def _lib():
    import gaussian_splatting_with_eye_tracking_amd as pkg
    lib = ctypes.CDLL(os.path.join(os.path.dirname(pkg.__file__), "libgsplat_amd.so"))
    lib.gs_rasterizer_backward_deterministic.argtypes = (
        [I, I, I, I, VP, I, I, VP, VP, VP, VP, F, VP, VP, VP, VP, VP, F, F, VP, VP, VP, VP, VP] + [VP] * 9 +
        [VP, ctypes.c_size_t, I, VP])
    lib.gs_rasterizer_backward_deterministic.restype = I
    lib.gs_backward_deterministic_scratch_bytes.argtypes = [I, I]
    lib.gs_backward_deterministic_scratch_bytes.restype = ctypes.c_size_t
    lib.gs_last_error.restype = ctypes.c_char_p
    return lib


def test_c_abi_with_nan_filled_scratch_and_short_scratch():
    lib = _lib()
    c = _case("ragged_3k_250x130")
    P = c["P"]
    fwd = _forward(c)
    s, t, (K, color, radii, geom, binning, img) = fwd
    ref = dict(zip(NAMES, _backward(c, fwd, True)))
    need = lib.gs_backward_deterministic_scratch_bytes(P, K)
    assert need >= 36 * K
    dpix = torch.from_numpy(c["dpix"]).cuda()
    stream = torch.cuda.Stream()
    sentinel = 12345.0

    def call(nbytes, null=False):
        with torch.cuda.stream(stream):
            scratch = torch.full((max(nbytes, 1),), 0xFF, dtype=torch.uint8, device="cuda")  # NaNs
            outs = [torch.full(shape, sentinel, device="cuda")
                    for shape in ((P, 3), (P, 1), (P, 3), (P, 3), (P, 6), (P, 16, 3), (P, 3), (P, 4))]
            m2, op, cl, m3, cv, sh, scl, rot = outs
            rc = lib.gs_rasterizer_backward_deterministic(
                P, 3, 16, K, _p(s.bg), c["W"], c["H"], _p(t["means3D"]), _p(t["shs"]), VP(0), _p(t["scales"]), F(1.0),
                _p(t["rotations"]), VP(0), _p(s.viewmatrix), _p(s.projmatrix), _p(s.campos), F(s.tanfovx),
                F(s.tanfovy), _p(radii), _p(geom), _p(binning), _p(img), _p(dpix), _p(m2), VP(0), _p(op), _p(cl),
                _p(m3), _p(cv), _p(sh), _p(scl), _p(rot), VP(0) if null else VP(scratch.data_ptr()), nbytes, 0,
                VP(stream.cuda_stream))
        stream.synchronize()
        return rc, dict(zip(NAMES, [m2, cl, op, m3, cv, sh, scl, rot]))

    torch.cuda.synchronize()
    rc, mine = call(need)
    assert rc >= 0, lib.gs_last_error().decode()
    for n in NAMES:
        assert torch.isfinite(mine[n]).all(), n
        assert torch.equal(mine[n], ref[n]), n
    rc, untouched = call(need - 1)
    assert rc < 0
    assert "scratch" in lib.gs_last_error().decode()
    for n in NAMES:
        assert torch.all(untouched[n] == sentinel), n
    rc, untouched = call(need, null=True)
    assert rc < 0 and "NULL" in lib.gs_last_error().decode()
    for n in NAMES:
        assert torch.all(untouched[n] == sentinel), n


# ------------------------------------------------------------ 8. edges
def test_edges_give_zeros():
    C = _C()
    e = torch.Tensor([])
    # P = 0
    sc, cam = G.scene_and_camera(0, 64, 48)
    c0 = dict(P=0, W=64, H=48, sc=sc, cam=cam, colors=None, cov=None, dpix=np.ones((3, 48, 64), np.float32))
    g = _backward(c0, _forward(c0), True)
    for n, x in zip(NAMES, g):
        assert x.shape[0] == 0 and x.numel() == 0, n
    # every Gaussian behind the near plane: K = R = 0
    sc, cam = G.scene_and_camera(500, 64, 48)
    sc.means3D[:, 2] = -5.0
    c1 = dict(P=500, W=64, H=48, sc=sc, cam=cam, colors=None, cov=None, dpix=np.ones((3, 48, 64), np.float32))
    fwd = _forward(c1)
    assert fwd[2][0] == 0
    g = _backward(c1, fwd, True)
    for n, x, shape in zip(NAMES, g, ((500, 3), (500, 3), (500, 1), (500, 3), (500, 6), (500, 16, 3), (500, 3),
                                      (500, 4))):
        assert tuple(x.shape) == shape, n
        assert torch.all(x == 0), n
    s, t, (K, color, radii, geom, binning, img) = fwd
    C.set_deterministic_backward(True)
    try:
        rec = C.rasterize_gaussians_backward_view_grads(s.bg, radii, e, s.viewmatrix, s.projmatrix, s.tanfovx,
                                                        s.tanfovy, s.campos, torch.from_numpy(c1["dpix"]).cuda(),
                                                        geom, K, binning, img, False)
    finally:
        C.set_deterministic_backward(False)
    assert rec.numel() == 500 * 10 + 40 and torch.all(rec[:5000] == 0)


# --------------------------------------------------------- 9. training
def test_training_runs_bit_identical():
    """training.py's native sequence (activate -> forward -> fused loss ->
    backward -> activation backward -> Adam) with the mode on: two runs from
    the same state agree bit for bit in every parameter, gradient and Adam
    moment after each of three iterations."""
    from gaussian_splatting_with_eye_tracking_amd import set_deterministic, training as T
    P, W, H, seed = SHAPES["cfg1_10k_256"]
    sc, cam = G.scene_and_camera(P, W, H, seed)
    s = G.torch_settings(cam)
    gt = torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    opt = T.OptimizationParams(densify_from_iter=10**6, densify_until_iter=0)  # no densification

    def run():
        torch.manual_seed(0)
        m = T.FlatGaussianModel(G.raw_from_scene(sc), 3, spatial_lr_scale=5.0, opt=opt)
        m.active_sh_degree = 3
        snaps = []
        for it in range(1, 4):
            pkg, terms = T.forward_backward(m, it, s, gt, fused=True)
            grads = m.grads.clone()
            T.post_backward(m, it, pkg, scene_extent=5.0, fused=True)
            torch.cuda.synchronize()
            snaps.append((grads, pkg["viewspace_grad"].clone(), m.params.clone(), m.exp_avg.clone(),
                          m.exp_avg_sq.clone(), terms["loss"].clone()))
        return snaps

    set_deterministic(True)
    try:
        a, b = run(), run()
    finally:
        set_deterministic(None)
    for it, (x, y) in enumerate(zip(a, b), 1):
        for what, u, v in zip(("grads", "viewspace_grad", "params", "exp_avg", "exp_avg_sq", "loss"), x, y):
            assert torch.isfinite(u).all(), (it, what)
            assert torch.equal(u, v), (it, what, float((u - v).abs().max()))
    assert not torch.equal(a[0][2], a[2][2])  # the parameters moved
