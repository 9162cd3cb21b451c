"""Shared test helpers: build identical inputs for the HIP path and the oracle,
and tolerance checks with the tolerances of BASELINE.json's north_star."""
from __future__ import annotations

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
    large = (np.abs(r) >= 100.0 * atol) & (al == 0)  # elements >= 1e-4 of the tensor's largest
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
