"""The forked base forward (set_tuning "fwd_fork"): the SH colour kernel on the
library's side stream beside the tile binning, against the unforked forward
(one fused preprocess on the caller's stream).

Forward: image, radii and every buffer field bit for bit -- the per-Gaussian
colour records (rgb, clamped, drgb) on the rows with radii > 0 only: a culled
Gaussian's records are never written and carry stale words by design.
Backward: the deterministic one bit for bit; the default one inside the
element-wise bar of test_gpu_parity (against the oracle, with its allowance).

Shapes: P in {1, 64, 257, 4099} (a lone thread, exactly one wave, a partial
second workgroup of the 256-thread kernels, several workgroups with culled
Gaussians among them) at 64x48 and at 130x70 (no multiple of 16 either way);
and one P past 16 chunks per compute unit's workgroup, where the colour
kernel's grid is capped and every workgroup walks several chunks.
"""
import ctypes
import os

import numpy as np
import pytest

import gs_helpers as G

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussian_splatting_with_eye_tracking_amd", "libgsplat_amd.so")

SIZES = [(64, 48), (130, 70)]
COUNTS = [1, 64, 257, 4099]
SHAPES = [(P, W, H) for (W, H) in SIZES for P in COUNTS]
IMAGE_FIELDS = ("accum_alpha", "n_contrib", "ranges")
GEOM_FIELDS = ("depths", "means2D", "conic_opacity", "tiles_touched")
NAMES = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
         "dL_drotations"]


def _C():
    import gaussian_splatting_with_eye_tracking_amd._C as C
    return C


def _drgb_rows(geom, P):
    """The geometry buffer's d(rgb)/d(dir) rows, [P][12] floats (nine used), or
    None when the buffer has no tail (parse_buffers does not list them)."""
    class View(ctypes.Structure):
        _fields_ = [(n, ctypes.c_void_p) for n in ("hdr", "depths", "radii", "means2D", "conic_opacity", "rgb",
                                                   "cov3D", "clamped", "drgb", "tiles_touched", "grad_accum")]
    lib = ctypes.CDLL(LIB)
    v = View()
    base = 1 << 20
    assert lib.gs_geom_view_of(ctypes.c_void_p(base), P, ctypes.byref(v)) == 0
    off = v.drgb - base
    raw = geom.reshape(-1).view(torch.uint8)
    if off + 48 * P > raw.numel():
        return None
    return raw[off:off + 48 * P].clone().view(torch.float32).reshape(P, 12)


def _scene(P, W, H, seed, M=16):
    sc, cam = G.scene_and_camera(P, W, H, seed)
    t = G.scene_tensors(sc)
    if M != 16:
        t["shs"] = t["shs"][:, :M].contiguous()
    return sc, cam, t


def _forward(sc, cam, t, fork, degree=3, **kw):
    with G.tuning(fwd_fork=fork):
        out = G.native_forward(sc, cam, tensors=t, sh_degree=degree, **kw)
        assert _C().get_tuning("fwd_fork") == fork
    return out


def _assert_same_forward(a, b, P, W, H, aux=False, drgb=True):
    """Two forwards' outputs and buffers, bit for bit (the colour records on the visible rows)."""
    C = _C()
    oa, ob = a[2], b[2]
    K = oa[0]
    assert K == ob[0]
    assert torch.equal(oa[1], ob[1]), "image"
    if aux:
        assert torch.equal(oa[2], ob[2]) and torch.equal(oa[3], ob[3]), "depth / alpha maps"
    ra, rb = oa[-4], ob[-4]
    assert torch.equal(ra, rb), "radii"
    vis = ra > 0
    da = C.parse_buffers(*oa[-3:], P, K, W, H, 16)
    db = C.parse_buffers(*ob[-3:], P, K, W, H, 16)
    for k in IMAGE_FIELDS:
        assert torch.equal(da[k], db[k]), k
    for k in GEOM_FIELDS + ("rgb", "clamped_bits"):
        assert torch.equal(da[k][vis], db[k][vis]), k
    if K:
        assert torch.equal(da["point_list"], db["point_list"]), "point_list"
    for w in (0, 2, 3, 7):  # K, the tile statistics, the drgb flag
        assert int(da["hdr"][w]) == int(db["hdr"][w]), w
    xa, xb = _drgb_rows(oa[-3], P), _drgb_rows(ob[-3], P)
    assert (xa is None) == (xb is None)
    if drgb:
        assert xa is not None and int(da["hdr"][7]) == 1
        assert torch.equal(xa[vis][:, :9], xb[vis][:, :9]), "drgb"
    return int(vis.sum())


@pytest.mark.parametrize("P,W,H", SHAPES)
@pytest.mark.parametrize("degree,M", [(0, 16), (1, 16), (2, 16), (3, 16), (2, 9)])
def test_forward_matches_unforked(P, W, H, degree, M):
    sc, cam, t = _scene(P, W, H, 100 + P, M)
    for aa in (False, True):
        off = _forward(sc, cam, t, 0, degree, antialiasing=aa, bg=(0.1, 0.2, 0.3))
        on = _forward(sc, cam, t, 1, degree, antialiasing=aa, bg=(0.1, 0.2, 0.3))
        nvis = _assert_same_forward(off, on, P, W, H)
    if P == 4099:
        assert 0 < nvis < P  # culled Gaussians among the visible ones


def test_forward_matches_unforked_walking_chunks():
    """P = 70001: 274 chunks of 256 Gaussians, a ragged last one, on a grid of
    one workgroup per compute unit (at most 256 on the parts this runs on):
    workgroups walk a second chunk, and the last chunk's tail waves leave."""
    P, W, H = 70001, 130, 70
    sc, cam, t = _scene(P, W, H, 5)
    nvis = _assert_same_forward(_forward(sc, cam, t, 0), _forward(sc, cam, t, 1), P, W, H)
    assert 0 < nvis < P


@pytest.mark.parametrize("P,W,H", SHAPES)
def test_aux_forward_matches_unforked(P, W, H):
    sc, cam, t = _scene(P, W, H, 200 + P)
    off = _forward(sc, cam, t, 0, aux=True)
    on = _forward(sc, cam, t, 1, aux=True)
    _assert_same_forward(off, on, P, W, H, aux=True)


@pytest.mark.parametrize("P,W,H", SHAPES)
def test_deterministic_backward_bit_identical(P, W, H):
    from gaussian_splatting_with_eye_tracking_amd import synthetic as S
    sc, cam, t = _scene(P, W, H, 300 + P)
    dpix = S.make_cotangent(H, W, P)
    g0 = G.native_backward(_forward(sc, cam, t, 0), dpix, det=True)
    g1 = G.native_backward(_forward(sc, cam, t, 1), dpix, det=True)
    for n, a, b in zip(NAMES, g0, g1):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("P,W,H", SHAPES)
def test_default_backward_inside_the_parity_bar(P, W, H):
    """The default backward of a forked forward against the oracle, at the
    element-wise bar of test_gpu_parity.test_backward_parity."""
    import oracle as O
    from gaussian_splatting_with_eye_tracking_amd import synthetic as S
    sc, cam, t = _scene(P, W, H, 400 + P)
    bg = (0.2, 0.1, 0.05)
    fwd = _forward(sc, cam, t, 1, bg=bg)
    os_, ref, kw = G.oracle_forward(sc, cam, bg=bg)
    dpix = S.make_cotangent(H, W, P + 1)
    grads = G.native_backward(fwd, dpix)
    rg = O.backward(os_, ref, sc.means3D, dpix, **kw)
    for n, g in zip(NAMES, grads):
        gg = g.cpu().numpy()
        assert gg.shape == rg[n].shape and np.all(np.isfinite(gg)), n
        assert G.rel_err(gg, rg[n]) < G.GRAD_REL_TOL, (n, G.rel_err(gg, rg[n]))
    al, ties = O.grad_allowance(os_, ref, sc.means3D, dpix, parts=True, **kw)
    G.assert_grads_elementwise(f"forward_fork_{P}_{W}x{H}", NAMES, grads, rg, sc, cam, ref, allow=al, ties=ties)


@pytest.mark.parametrize("on_side_stream", [False, True])
def test_repeated_calls_alternating_scenes(on_side_stream):
    """50 forwards alternating two scenes of different P and colours: the
    caching allocator hands consecutive calls the same memory, so a colour
    kernel not joined into the caller's stream would write into (or read from)
    the next call's buffers.  (A missing join can fail this; its presence is
    argued in DESIGN.md, not proven here.)"""
    C = _C()
    W, H = 130, 70
    scenes = [_scene(4099, W, H, 11), _scene(2500, W, H, 12)]
    ref = []
    for sc, cam, t in scenes:
        o = _forward(sc, cam, t, 0)[2]
        d = C.parse_buffers(*o[-3:], t["means3D"].shape[0], o[0], W, H, 16)
        ref.append((o[1].clone(), o[-4] > 0, d["rgb"]))
    stream = torch.cuda.Stream() if on_side_stream else torch.cuda.current_stream()
    from gaussian_splatting_with_eye_tracking_amd import rasterization as R
    got = []
    with G.tuning(fwd_fork=1), torch.cuda.stream(stream):
        for i in range(50):
            sc, cam, t = scenes[i % 2]
            s = G.torch_settings(cam)
            o = C.rasterize_gaussians(*R.native_forward_args(s, *G._operands(t)))
            # copies on the caller's stream, then the buffers go back to the allocator for the next call
            got.append((o[1].clone(), C.parse_buffers(*o[-3:], t["means3D"].shape[0], o[0], W, H, 16)["rgb"]))
            del o
        stream.synchronize()
    torch.cuda.synchronize()
    for i, (color, rgb) in enumerate(got):
        want_color, vis, want_rgb = ref[i % 2]
        assert torch.equal(color, want_color), i
        assert torch.equal(rgb[vis], want_rgb[vis]), i


def _unforked_case(kind):
    from diff_gaussian_rasterization import GaussianRasterizer
    W, H = 64, 48
    if kind == "P0":
        sc, cam = G.scene_and_camera(0, W, H)
        s = G.torch_settings(cam)
        t = G.scene_tensors(sc)
        color, radii = GaussianRasterizer(s)(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]),
                                             opacities=t["opacities"], shs=t["shs"], scales=t["scales"],
                                             rotations=t["rotations"])
        torch.cuda.synchronize()
        return [color, radii]
    sc, cam = G.scene_and_camera(257, W, H, 21)
    kw = {}
    if kind == "colors_precomp":
        kw["colors_precomp"] = np.random.default_rng(5).uniform(0, 1, (257, 3)).astype(np.float32)
    elif kind == "debug":
        kw["debug"] = True
    elif kind == "all_culled":
        sc.means3D[:, 2] = -5.0
    elif kind in ("W0", "H0"):
        s = G.torch_settings(cam)
        kw["settings"] = s._replace(image_width=0) if kind == "W0" else s._replace(image_height=0)
    s, t, o = G.native_forward(sc, cam, bg=(0.5, 0.25, 0.125), **kw)
    Wc, Hc = int(s.image_width), int(s.image_height)
    out = [torch.tensor(o[0]), o[1], o[-4]]
    if Wc and Hc:
        d = _C().parse_buffers(*o[-3:], 257, o[0], Wc, Hc, 16)
        vis = o[-4] > 0
        out += [d[k] for k in IMAGE_FIELDS] + [d[k][vis] for k in GEOM_FIELDS]
        if kind == "debug":
            out += [d["rgb"][vis], d["clamped_bits"][vis]]
    return out


@pytest.mark.parametrize("kind", ["colors_precomp", "debug", "all_culled", "P0", "W0", "H0"])
def test_unforked_cases(kind):
    """Calls that do not fork (precomputed colours, debug mode, nothing to bin)
    or have nothing to colour: the unforked call's results, and the switch
    reads back as it was set."""
    C = _C()
    with G.tuning(fwd_fork=0):
        ref = _unforked_case(kind)
    with G.tuning(fwd_fork=1):
        got = _unforked_case(kind)
        assert C.get_tuning("fwd_fork") == 1
    assert len(ref) == len(got)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a.shape == b.shape and torch.equal(a, b), (kind, i)
    if kind == "all_culled":
        assert int(ref[0]) == 0 and not bool(ref[2].any())


def test_forward_after_a_raising_call():
    """A prefiltered violation raises behind the K read-back, between fork and
    join: the next forward of the process is the unforked one's, bit for bit."""
    P, W, H = 257, 64, 48
    sc, cam, t = _scene(P, W, H, 31)
    off = _forward(sc, cam, t, 0)
    bad = dict(t, means3D=t["means3D"].clone())
    bad["means3D"][0, 2] = -1.0
    with G.tuning(fwd_fork=1):
        with pytest.raises(RuntimeError, match="prefiltered"):
            G.native_forward(sc, cam, settings=G.torch_settings(cam)._replace(prefiltered=True), tensors=bad)
        on = G.native_forward(sc, cam, tensors=t)
    _assert_same_forward(off, on, P, W, H)
