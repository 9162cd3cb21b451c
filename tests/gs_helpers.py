"""Shared test helpers: build identical inputs for the HIP path and the oracle,
and tolerance checks with the tolerances of BASELINE.json's north_star."""
from __future__ import annotations

import contextlib
import glob
import io
import os

import numpy as np

from gaussian_splatting_with_eye_tracking_amd import synthetic as S

# north_star: image L1 < 1e-5, gradients within 1e-4 relative.
IMAGE_L1_TOL = 1e-5
GRAD_REL_TOL = 1e-4


GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_PART_BYTES = 900_000  # a committed file stays under 1 MiB


def _npz_bytes(**arrays) -> int:
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getbuffer().nbytes


def save_golden(stem: str, arrays: dict) -> list:
    """Write `arrays` as tests/golden/<stem>.npz, or, where that file would
    exceed GOLDEN_PART_BYTES, as <stem>.part0.npz, .part1.npz, ...: whole
    arrays are packed into parts in order; an array too large for one part is
    cut along axis 0 into pieces "name@0", "name@1", ... (load_golden joins
    them).  Returns the files written."""
    items = []
    for k, v in arrays.items():
        v = np.asarray(v)
        n = -(-_npz_bytes(**{k: v}) // GOLDEN_PART_BYTES)
        while n > 1 and any(_npz_bytes(p=p) > GOLDEN_PART_BYTES for p in np.array_split(v, n)):
            n += 1
        items += [(k, v)] if n == 1 else [(f"{k}@{i}", p) for i, p in enumerate(np.array_split(v, n))]
    parts, cur = [], {}
    for k, v in items:
        if cur and _npz_bytes(**cur, **{k: v}) > GOLDEN_PART_BYTES:
            parts.append(cur)
            cur = {}
        cur[k] = v
    parts.append(cur)
    names = [f"{stem}.npz"] if len(parts) == 1 else [f"{stem}.part{i}.npz" for i in range(len(parts))]
    for stale in glob.glob(os.path.join(GOLDEN_DIR, f"{stem}.npz")) + glob.glob(
            os.path.join(GOLDEN_DIR, f"{stem}.part*.npz")):
        os.remove(stale)
    for name, part in zip(names, parts):
        np.savez_compressed(os.path.join(GOLDEN_DIR, name), **part)
    return names


def load_golden(stem: str) -> dict:
    """The arrays save_golden(stem, ...) wrote, whole again."""
    one = os.path.join(GOLDEN_DIR, f"{stem}.npz")
    files = [one] if os.path.exists(one) else sorted(
        glob.glob(os.path.join(GOLDEN_DIR, f"{stem}.part*.npz")),
        key=lambda f: int(f.rsplit(".part", 1)[1][:-len(".npz")]))
    assert files, f"no golden fixture {stem}"
    raw = {}
    for f in files:
        with np.load(f) as d:
            raw.update({k: d[k] for k in d.files})
    out = {k: v for k, v in raw.items() if "@" not in k}
    for k in sorted({k.split("@")[0] for k in raw if "@" in k}):
        n = sum(1 for r in raw if r.startswith(k + "@"))
        out[k] = np.concatenate([raw[f"{k}@{i}"] for i in range(n)])
    return out


def scene_and_camera(P: int, W: int, H: int, seed: int = 0, **kw):
    cam = S.make_camera(W, H)
    sc = S.make_scene(P, cam, seed=seed, **kw)
    return sc, cam


# ------------------------------------------------------------ general views
# Cameras with a full rotation (all nine entries of R distinct and non-zero, R
# far from symmetric) and a translation, so that a wrong row, column or
# transpose of the view matrix, or a wrong camera centre, changes the numbers.
# R is the camera-to-world rotation of get_world2view2: x_view = R^T x_world + T.
def _rot(axis: str, deg: float) -> np.ndarray:
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return {"x": np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]),
            "y": np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]),
            "z": np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])}[axis]


GENERAL_VIEWS = {
    "a": (_rot("y", 25.0) @ _rot("x", -15.0) @ _rot("z", 30.0), np.array([0.7, -0.4, 1.3])),
    "b": (_rot("y", -40.0) @ _rot("x", 20.0) @ _rot("z", -75.0), np.array([-1.1, 0.6, -0.8])),
    "identity": (np.eye(3), np.zeros(3)),
}
# the coverage every test on a general case asserts on its census
GENERAL_COVERAGE = {"clamp_active": 20, "alpha_clamped": 10, "near_culled": 20, "behind": 20}
# The opacity lift to 0.999 goes to a seeded half of the Gaussians in front of
# the near plane whose centre projects into the image: about 14 % of all.  A
# uniform 15 % left 2 .. 8 Gaussians at alpha's clamp in the cases used, and no
# larger uniform share (up to all) reached 10: alpha = 0.999 G exceeds 0.99
# within 0.13 sigma of the centre only, so the centre must be on a pixel's
# doorstep, and lifted splats elsewhere merely hide the ones behind them.
ALPHA_CLAMP_SHARE = 0.5
GENERAL_LOG_SCALE = float(np.log(0.06))
# the larger cases: at ln 0.06 the near-plane splats lie some 400 deep on
# every tile of a 250 x 130 image and only the first 40 entries of a list
# blend at all -- at most 7 Gaussians reach alpha's clamp however many are lifted
GENERAL_LOG_SCALE_LARGE = float(np.log(0.03))
# The spread of the log-scales.  At 0.9 the scenes hold needles of 50:1 and
# more, whose cov2D / cov3D backward cancels (denom - a c against a c, 3000:1
# for a needle 270 px long): the float32 oracle alone then misses the
# element-wise bar against float64 autograd (test_oracle_autograd.torch_forward)
# on single Gaussians at depths 0.7 .. 3 (err / bound up to 9.8 on dL_dscales /
# dL_drotations under the views "b" and "identity"; still 1.6 at 0.8, where
# the multi-view kernel had the float64 value of the offending element to six
# digits and the oracle was 1.7 % off), and the kernels missed it on other
# Gaussians of the same kind.  At 0.7 the oracle stays inside the bar on every
# case and view used (err / bound <= 0.62) and the coverage holds.  The scenes
# without clamps take 0.4, the spread of antialias_reference's own scenes:
# their composite reference sits at err / bound 0.7 .. 0.8 there and beyond
# the bar from 0.6.
GENERAL_LOG_SCALE_STD = 0.7
GENERAL_LOG_SCALE_STD_NO_CLAMP = 0.4


def general_camera(W: int, H: int, view: str = "a"):
    R, T = GENERAL_VIEWS[view]
    return S.make_camera(W, H, R=R, T=T)


def general_case(P: int, W: int, H: int, seed: int, clamp: bool = True, view: str = "a",
                 log_scale_mean: float = GENERAL_LOG_SCALE, log_scale_std: float | None = None):
    """(scene, camera, cotangent) of a general view.  The scene is drawn in
    the camera's view space and carried to the world by x_world = R (x_view -
    T) (float64, rounded once), so the view keeps make_scene's statistics:
    with `clamp`, depths -1 .. 6 (behind the camera, inside the z <= 0.2 cull,
    just in front of it, splats larger than the image), a lateral spread of
    1.7 tan(fov) (beyond the 1.3 tan(fov) clamp of t.x/t.z, t.y/t.z) and
    lifted opacities (ALPHA_CLAMP_SHARE: alpha reaches its 0.99 clamp).
    Without, the same camera on a scene no Gaussian of which needs either
    clamp (depths 2 .. 20, spread 0.9, opacities <= 0.97).  `view`: the key
    of GENERAL_VIEWS the scene is laid out for and seen from ("identity": the
    same view-space scene under the identity camera)."""
    cam = general_camera(W, H, view)
    cam0 = S.make_camera(W, H)
    if log_scale_std is None:
        log_scale_std = GENERAL_LOG_SCALE_STD if clamp else GENERAL_LOG_SCALE_STD_NO_CLAMP
    kw = dict(spread=1.7, depth_range=(-1.0, 6.0)) if clamp else dict(spread=0.9, depth_range=(2.0, 20.0))
    sc = S.make_scene(P, cam0, seed, log_scale_mean=log_scale_mean, log_scale_std=log_scale_std, opacity_std=1.0,
                      **kw)
    if clamp:
        m = sc.means3D.astype(np.float64)
        with np.errstate(all="ignore"):
            on_screen = ((m[:, 2] > 0.2) & (np.abs(m[:, 0] / m[:, 2]) < cam0.tanfovx) &
                         (np.abs(m[:, 1] / m[:, 2]) < cam0.tanfovy))
        hot = (np.random.default_rng(seed + 77).random(P) < ALPHA_CLAMP_SHARE) & on_screen
        sc.opacities[hot] = np.float32(0.999)
    else:
        sc.opacities = np.minimum(sc.opacities, 0.97).astype(np.float32)
    R, T = GENERAL_VIEWS[view]
    sc.means3D = np.ascontiguousarray(((sc.means3D.astype(np.float64) - T[None]) @ R.T).astype(np.float32))
    return sc, cam, S.make_cotangent(H, W, seed + 1)


def view_space(means3D, cam) -> np.ndarray:
    """[P, 3] float64 view-space positions (row-vector convention)."""
    m = np.asarray(means3D, np.float64)
    V = np.asarray(cam.world_view_transform, np.float64)
    return m @ V[:3, :3] + V[3, :3][None]


def clamp_active(means3D, cam) -> np.ndarray:
    """Which Gaussians lie outside the 1.3 tan(fov) clamp of t.x/t.z or t.y/t.z."""
    t = view_space(means3D, cam)
    with np.errstate(all="ignore"):
        return (np.abs(t[:, 0] / t[:, 2]) > 1.3 * cam.tanfovx) | (np.abs(t[:, 1] / t[:, 2]) > 1.3 * cam.tanfovy)


def alpha_clamp_reached(fwd) -> np.ndarray:
    """Which Gaussians reach alpha's 0.99 clamp at a pixel they contribute to:
    opacity * exp(power) > 0.99 (float64, from the oracle's forward buffers)
    at a pixel whose n_contrib covers their position in the tile's list."""
    H, W = fwd.color.shape[1:]
    B = int(fwd.block)
    gx = (W + B - 1) // B
    nc = fwd.n_contrib.reshape(H, W).astype(np.int64)
    xy = fwd.means2D.astype(np.float64)
    co = fwd.conic_opacity.astype(np.float64)
    hit = np.zeros(fwd.radii.shape[0], bool)
    for t, (beg, end) in enumerate(fwd.ranges.astype(np.int64)):
        ty, tx = divmod(t, gx)
        ys, xs = np.arange(ty * B, min(ty * B + B, H)), np.arange(tx * B, min(tx * B + B, W))
        if end == beg or not len(ys) or not len(xs):
            continue
        ids = fwd.point_list[beg:end].astype(np.int64)
        PY, PX = [a.reshape(-1, 1) for a in np.meshgrid(ys, xs, indexing="ij")]
        dx, dy = xy[ids, 0][None] - PX, xy[ids, 1][None] - PY
        c = co[ids]
        power = -0.5 * (c[None, :, 0] * dx * dx + c[None, :, 2] * dy * dy) - c[None, :, 1] * dx * dy
        with np.errstate(over="ignore"):
            a = c[None, :, 3] * np.exp(np.minimum(power, 0.0))
        reach = (power <= 0) & (a > 0.99) & (np.arange(end - beg)[None] < nc[PY, PX])
        hit[ids[reach.any(0)]] = True
    return hit


def general_case_census(scene, camera, oracle_forward, oracle_grads) -> dict:
    """What a general case covers: the counts GENERAL_COVERAGE bounds, the
    largest radius, and the boolean masks they count (keys "*_mask")."""
    z = view_space(scene.means3D, camera)[:, 2]
    vis = oracle_forward.radii > 0
    contributing = np.any(np.asarray(oracle_grads["dL_dmeans2D"]) != 0, axis=1)
    ca = clamp_active(scene.means3D, camera) & vis & contributing
    ac = alpha_clamp_reached(oracle_forward)
    return {"visible": int(vis.sum()), "near_culled": int((z <= 0.2).sum()), "behind": int((z < 0).sum()),
            "clamp_active": int(ca.sum()), "alpha_clamped": int(ac.sum()),
            "max_radius": int(oracle_forward.radii.max()), "K": int(oracle_forward.num_rendered),
            "near_culled_mask": z <= 0.2, "behind_mask": z < 0, "clamp_active_mask": ca, "alpha_clamped_mask": ac}


def assert_general_coverage(census: dict, W: int, H: int) -> None:
    """The coverage conditions of a general case (clamp=True)."""
    for k, least in GENERAL_COVERAGE.items():
        assert census[k] >= least, (k, census[k], least)
    assert census["max_radius"] >= max(W, H), census["max_radius"]


def torch_settings(cam, device="cuda", bg=(0.0, 0.0, 0.0), sh_degree=3, scale_modifier=1.0, debug=False,
                   amr=False):
    import torch
    if amr:
        from diff_gaussian_rasterization_amr import GaussianRasterizationSettings
    else:
        from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=cam.tanfovx,
        tanfovy=cam.tanfovy, bg=torch.tensor(bg, dtype=torch.float32, device=device), scale_modifier=scale_modifier,
        viewmatrix=torch.from_numpy(cam.world_view_transform).to(device),
        projmatrix=torch.from_numpy(cam.full_proj_transform).to(device), sh_degree=sh_degree,
        campos=torch.from_numpy(cam.camera_center).to(device), prefiltered=False, debug=debug)


def scene_tensors(sc, device="cuda", requires_grad=False):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device).requires_grad_(requires_grad)  # noqa: E731
    return dict(means3D=t(sc.means3D), opacities=t(sc.opacities), shs=t(sc.shs), scales=t(sc.scales),
                rotations=t(sc.rotations))


# (name, P, W, H, seed): the shapes the parity and the deterministic tests share
PARITY_CASES = [
    ("g1_64_32x32", 64, 32, 32, 3),
    ("cfg1_10k_256", 10000, 256, 256, 0),
    ("ragged_3k_250x130", 3000, 250, 130, 7),
    ("dense_20k_128", 20000, 128, 128, 11),  # large tiles: exercises the merge-sort path
    ("grid_17k_tiles", 3000, 2112, 2080, 5),  # T = 17160 > kLdsTiles: device-atomic binning path
]


_OPERAND_KEYS = ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")


def _operands(t):
    """A tensor dict's operands in the builders' order (colours / covariance not named: absent)."""
    import torch
    return tuple(t.get(k, torch.Tensor([])) for k in _OPERAND_KEYS)


def _cuda(a):
    import torch
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def native_forward(sc, cam, colors_precomp=None, cov3D_precomp=None, bg=(0.0, 0.0, 0.0), keep_scales=False, *,
                   aux=False, antialiasing=False, settings=None, tensors=None, trailing=True, **settings_kw):
    """The raw forward binding (`aux`: rasterize_gaussians_aux) on a scene:
    `(settings, tensors, out)` after a synchronise.  SHs unless colours are
    given; scales / rotations unless a covariance is (`keep_scales`: both).
    `settings` / `tensors`: the caller's (torch_settings / scene_tensors
    otherwise, with `bg` and `settings_kw`); the tensors returned are the
    operands the call was given (_OPERAND_KEYS; an empty tensor: absent), and
    native_backward reads them.  trailing=False: the reference's argument list, without the trailing
    extension argument."""
    import torch
    from gaussian_splatting_with_eye_tracking_amd import _C, rasterization as R
    s = torch_settings(cam, bg=bg, **settings_kw) if settings is None else settings
    if antialiasing:
        s = s._replace(antialiasing=True)
    t = scene_tensors(sc) if tensors is None else dict(tensors)
    e = torch.Tensor([])
    if colors_precomp is not None:
        t.update(shs=e, colors_precomp=_cuda(colors_precomp))
    if cov3D_precomp is not None:
        t["cov3D_precomp"] = _cuda(cov3D_precomp)
        if not keep_scales:
            t.update(scales=e, rotations=e)
    args = R.native_forward_args(s, *_operands(t))
    out = (_C.rasterize_gaussians_aux if aux else _C.rasterize_gaussians)(*(args if trailing else args[:-1]))
    torch.cuda.synchronize()
    return s, t, out


def native_backward(fwd, dpix, *, lean=False, det=None, aux=None, antialiasing=None, debug=False, trailing=True):
    """The raw backward binding on one native_forward (or on any `(settings,
    tensors, out)` of a forward), with the thread's
    deterministic flag at `det` for the call (None: as it is): the eight
    gradients, after a synchronise.  aux=(dL_ddepth, dL_dalpha), either None
    for an empty tensor: the _aux binding.  antialiasing: the flag passed
    (default: the forward's).
    trailing=False: the reference's argument list, without the trailing
    opacities and flag."""
    import torch
    from gaussian_splatting_with_eye_tracking_amd import _C, rasterization as R
    s, t, out = fwd
    s = s._replace(debug=debug)
    if antialiasing is not None:
        s = s._replace(antialiasing=antialiasing)
    maps = None if aux is None else tuple(torch.Tensor([]).cuda() if a is None else _cuda(a) for a in aux)
    args = R.native_backward_args(s, *_operands(t), out[-4], *out[-3:], out[0], _cuda(dpix), maps)
    fn = getattr(_C, "rasterize_gaussians_backward" + ("" if aux is None else "_aux") + ("_lean" if lean else ""))
    prev = _C.get_deterministic_backward()
    _C.set_deterministic_backward(prev if det is None else det)
    try:
        g = fn(*(args if trailing else args[:-2]))
        torch.cuda.synchronize()
    finally:
        _C.set_deterministic_backward(prev)
    return list(g)


@contextlib.contextmanager
def tuning(**kv):
    """The library's tunings set to `kv` inside the block, and what they were put back after it."""
    from gaussian_splatting_with_eye_tracking_amd import _C
    was = {k: _C.get_tuning(k) for k in kv}
    try:
        for k, v in kv.items():
            _C.set_tuning(k, v)
        yield
    finally:
        for k, v in was.items():
            _C.set_tuning(k, v)
        assert {k: _C.get_tuning(k) for k in was} == was


def oracle_forward(sc, cam, colors_precomp=None, cov3D_precomp=None, bg=(0.0, 0.0, 0.0), keep_scales=False):
    """The oracle's forward of native_forward's scene: (settings, result, the operand keywords)."""
    import oracle as O
    s = O.settings_from_camera(cam, bg=bg)
    both = cov3D_precomp is None or keep_scales
    kw = dict(shs=sc.shs if colors_precomp is None else None, colors_precomp=colors_precomp,
              scales=sc.scales if both else None,
              rotations=sc.rotations if both else None, cov3D_precomp=cov3D_precomp)
    return s, O.forward(s, sc.means3D, sc.opacities, **kw), kw


def assert_same_buffers(C, a, b, P, K, W, H, vis):
    """Every field of the two forwards' geometry / image / binning buffers
    (per-Gaussian records of the visible Gaussians: the culled ones' are never
    written; header: the words a forward defines whatever the binning
    buffer's capacity)."""
    import torch
    da = C.parse_buffers(*a, P, K, W, H, 16)
    db = C.parse_buffers(*b, P, K, W, H, 16)
    assert set(da) == set(db)
    per_gaussian = {"depths", "means2D", "conic_opacity", "rgb", "clamped_bits", "cov3D"}
    # AMR / scratch words, and the geometry buffer's own radii slot: the
    # binding hands the forward its radii tensor (compared by the caller), so
    # the slot is never written
    skip = {"hdr", "levels", "levels_last", "levels_current", "pv", "tile_count", "radii"}
    for k in da:
        if k in skip:
            continue
        if k in per_gaussian:
            if k != "cov3D":  # (written on request only)
                assert torch.equal(da[k][vis], db[k][vis]), k
        else:
            assert torch.equal(da[k], db[k]), k
    for w in (0, 2, 3, 7):  # K, the tile statistics, the drgb flag
        assert int(da["hdr"][w]) == int(db["hdr"][w]), w
    assert (int(da["hdr"][6]) != 0) == (int(db["hdr"][6]) != 0)  # hit codes left (compared above)


def raw_from_scene(sc, device="cuda"):
    """The raw (pre-activation) parameter groups of a synthetic scene, as training.FlatGaussianModel takes them."""
    import torch
    from gaussian_splatting_with_eye_tracking_amd import ply
    g = ply.from_activated(sc.means3D, sc.opacities, sc.scales, sc.rotations, sc.shs)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)  # noqa: E731
    return {"xyz": t(g.xyz), "f_dc": t(g.features_dc), "f_rest": t(g.features_rest), "opacity": t(g.opacity),
            "scaling": t(g.scaling), "rotation": t(g.rotation)}


def image_l1(a, b) -> float:
    return float(np.mean(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def rel_err(a, b) -> float:
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    den = np.linalg.norm(b)
    if den == 0:
        return float(np.linalg.norm(a))
    return float(np.linalg.norm(a - b) / den)


# Element-wise gradient bar, beside the L2-norm bar above:
#     |g - r| <= GRAD_ELEM_RTOL * |r| + atol + allow,   atol = GRAD_ELEM_ATOL_FRAC * max|r|
# per tensor.  The absolute floor is one millionth of the tensor's largest
# element.  `allow` (oracle.grad_allowance, per element) is what float32
# cannot pin down, computed by the oracle from the same inputs: the jump of
# every blend decision taken within float32 rounding of its threshold (the
# hardware exp, v_exp_f32, and libm expf differ in the last bits there), and
# 64 ulps of the sum of the magnitudes of the per-pixel terms a gradient is
# accumulated from (the GPU's float atomics add them in another order than
# the oracle's double sums; where the terms cancel that is far more than
# 1e-4 of the result) -- both carried through the per-Gaussian backward.
GRAD_ELEM_RTOL = 1e-4
GRAD_ELEM_ATOL_FRAC = 1e-6


def elementwise_check(got, ref, rtol: float = GRAD_ELEM_RTOL, atol_frac: float = GRAD_ELEM_ATOL_FRAC,
                      allow=None) -> dict:
    """Element-wise comparison of one gradient tensor:
        |g - r| <= rtol |r| + atol + allow
    where `allow` (optional, shaped like the gradient) is the oracle's
    allowance (oracle.grad_allowance: near-tie jumps + accumulation order).  Returns the violation
    count, the stated atol, the worst element (largest err / bound) with its
    leading (per-Gaussian) index, the largest element-wise relative error over
    the elements above the absolute floor and without allowance, and how many
    elements needed the allowance."""
    g = np.asarray(got, np.float64)
    r = np.asarray(ref, np.float64)
    assert g.shape == r.shape, (g.shape, r.shape)
    out = {"n": int(r.size), "violations": 0, "atol": 0.0, "max_abs_ref": 0.0, "worst": None,
           "max_rel_above_floor": 0.0, "max_excess": 0.0, "allowance_used": 0, "allowance_elements": 0}
    if r.size == 0:
        return out
    maxr = float(np.max(np.abs(r)))
    atol = atol_frac * maxr
    err = np.abs(g - r)
    base = rtol * np.abs(r) + atol
    al = np.zeros_like(r) if allow is None else np.asarray(allow, np.float64).reshape(r.shape)
    bound = base + al
    bad = err > bound
    out.update(violations=int(bad.sum()), atol=atol, max_abs_ref=maxr,
               allowance_used=int(((err > base) & ~bad).sum()), allowance_elements=int((al > 0).sum()))
    ratio = err / np.where(bound > 0, bound, np.inf)
    ratio[(bound == 0) & (err > 0)] = np.inf
    w = int(np.argmax(ratio))
    lead = int(np.unravel_index(w, r.shape)[0]) if r.ndim else 0
    out["worst"] = {"flat": w, "gaussian": lead, "got": float(g.flat[w]), "ref": float(r.flat[w]),
                    "err": float(err.flat[w]), "bound": float(bound.flat[w]), "allow": float(al.flat[w]),
                    "ratio": float(ratio.flat[w])}
    above = (np.abs(r) > atol) & (al == 0)
    if above.any():
        out["max_rel_above_floor"] = float(np.max(err[above] / np.abs(r[above])))
    large = (np.abs(r) >= 100.0 * atol) & (al == 0) & (r != 0)  # elements >= 1e-4 of the tensor's largest
    if large.any():
        out["max_rel_large"] = float(np.max(err[large] / np.abs(r[large])))
    out["max_excess"] = float(np.max((err - rtol * np.abs(r)) / maxr)) if maxr > 0 else 0.0
    return out


def gaussian_context(idx: int, sc, cam, ref=None) -> dict:
    """What makes one Gaussian's backward ill-conditioned
    (base/cr/backward.cu:144-274): its screen radius, the 2-D covariance's
    determinant `denom` (the conic is its inverse), the view-space depth t.z
    and whether the +-1.3 tan(fov) clamp of t.x/t.z, t.y/t.z is active."""
    m = np.asarray(sc.means3D[idx], np.float64)
    V = np.asarray(cam.world_view_transform, np.float64)  # row-vector convention: p_view = [m, 1] @ V
    t = np.append(m, 1.0) @ V
    lx, ly = 1.3 * cam.tanfovx, 1.3 * cam.tanfovy
    c = {"index": int(idx), "t_z": float(t[2]),
         "clamp_x": bool(abs(t[0] / t[2]) > lx) if t[2] != 0 else None,
         "clamp_y": bool(abs(t[1] / t[2]) > ly) if t[2] != 0 else None}
    if ref is not None:
        c["radius"] = int(ref.radii[idx])
        c["tiles_touched"] = int(ref.tiles_touched[idx])
        co = np.asarray(ref.conic_opacity[idx], np.float64)
        dc = co[0] * co[2] - co[1] * co[1]
        c["denom"] = float(1.0 / dc) if dc != 0 else float("inf")
        c["opacity"] = float(co[3])
    return c


def _report(record: dict) -> None:
    """Append one element-wise record to $GS_ELEM_REPORT (JSON lines) when set."""
    import json
    import os
    path = os.environ.get("GS_ELEM_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")


# (acc_sqrt, acc_ulps) combinations whose violation counts the report records
# beside the asserted one (GS_ELEM_REPORT), for calibration
_ACC_GRID = ((0.0, 0.0), (1.0, 0.0), (1.0, 4.0), (2.0, 8.0), (4.0, 16.0))


def assert_grads_elementwise(case: str, names, grads, refs, sc=None, cam=None, ref_fwd=None,
                             atol_frac: dict | None = None, allow: dict | None = None, ties: dict | None = None) -> None:
    """The element-wise bar over every named gradient: zero violations, with
    the worst element and its Gaussian's context in the message.  `allow`:
    oracle.grad_allowance's per-tensor allowances (`ties` its counts,
    recorded with the report)."""
    import oracle as O
    parts = allow if allow is not None and "tie" in allow else None
    if parts is not None:
        allow = O.combine_allowance(parts)
    fails = []
    for n, g in zip(names, grads):
        if n not in refs:
            continue
        gg = g.detach().cpu().numpy() if hasattr(g, "detach") else np.asarray(g)
        af = (atol_frac or {}).get(n, GRAD_ELEM_ATOL_FRAC)
        rep = elementwise_check(gg, refs[n], atol_frac=af, allow=None if allow is None else allow.get(n))
        if parts is not None:  # calibration: the violations under other accumulation allowances
            rep["grid"] = {f"{a}sqrt+{b}": elementwise_check(gg, refs[n], atol_frac=af,
                                                             allow=O.combine_allowance(parts, a, b)[n])["violations"]
                           for a, b in _ACC_GRID}
            # the largest multiple of the accumulation allowance any element needed
            r = np.asarray(refs[n], np.float64)
            err = np.abs(np.asarray(gg, np.float64) - r)
            base = GRAD_ELEM_RTOL * np.abs(r) + af * float(np.max(np.abs(r)) if r.size else 0.0)
            acc = O.combine_allowance(parts, O.ACC_SQRT, O.ACC_ULPS)[n] - parts["tie"][n]
            over = err - base - parts["tie"][n]
            m = over > 0
            rep["acc_multiple_needed"] = float(np.max(over[m] / np.maximum(acc[m], 1e-300))) if m.any() else 0.0
        if rep["worst"] is not None and sc is not None and cam is not None:
            rep["context"] = gaussian_context(rep["worst"]["gaussian"], sc, cam, ref_fwd)
        _report({"case": case, "tensor": n, "ties": ties, **rep})
        if rep["violations"]:
            fails.append((n, rep))
    import os
    if os.environ.get("GS_ELEM_SOFT"):  # measurement runs: record only
        return
    assert not fails,"element-wise gradient violations: " + "; ".join(
        f"{n}: {r['violations']} of {r['n']} (atol {r['atol']:.3e}), worst {r['worst']}, "
        f"context {r.get('context')}" for n, r in fails)
