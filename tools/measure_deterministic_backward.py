#!/usr/bin/env python3
"""Measure the deterministic blend backward against the default one on the
same build (a tool, not a test; needs the GPU).

* --grid: BASELINE configs 2 and 4, view 0, at the sizes of the full-size
  tests (1M Gaussians 1920x1080; 6.1M Gaussians 1600x1063, seed 0).  For both
  paths every gradient tensor goes through tests/gs_helpers.py
  assert_grads_elementwise in record-only mode: one JSON line per (case,
  tensor) with the violation counts under the accumulation allowances of its
  grid -- "0.0sqrt+0.0" is the oracle's tie allowance alone,
  combine_allowance(parts, 0, 0) -- and acc_multiple_needed.  A further line
  per config gives what the two paths make of single elements (--elements,
  default config 4's dL_dscales[2944233] read as a flat index and as a
  Gaussian index) and how far the two paths are apart.
* --timing: render_bwd (the library's own stage events: the blend kernel,
  plus the reduction in deterministic mode) at config 2, warm, the two paths
  alternating, the median of --runs calls each, with the scratch bytes.

Records are appended to $GS_ELEM_REPORT (default
profiles/deterministic_elementwise.jsonl).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

NAMES = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
         "dL_drotations"]
CONFIGS = {2: (1_000_000, 1920, 1080), 4: (6_100_000, 1600, 1063)}


def _setup(cfg):
    import torch
    import gs_helpers as G
    import gaussian_splatting_with_eye_tracking_amd._C as C
    from gaussian_splatting_with_eye_tracking_amd import synthetic as S
    P, W, H = CONFIGS[cfg]
    sc, cam = G.scene_and_camera(P, W, H, 0)
    s = G.torch_settings(cam)
    t = G.scene_tensors(sc)
    e = torch.Tensor([])
    fwd = C.rasterize_gaussians(s.bg, t["means3D"], e, t["opacities"], t["scales"], t["rotations"], s.scale_modifier,
                                e, s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width,
                                t["shs"], s.sh_degree, s.campos, s.prefiltered, s.debug)
    torch.cuda.synchronize()
    dpix = S.make_cotangent(H, W, 1)
    d_dev = torch.from_numpy(dpix).cuda()

    def backward(det):
        K, color, radii, geom, binning, img = fwd
        C.set_deterministic_backward(det)
        try:
            return C.rasterize_gaussians_backward(s.bg, t["means3D"], radii, e, t["scales"], t["rotations"],
                                                  s.scale_modifier, e, s.viewmatrix, s.projmatrix, s.tanfovx,
                                                  s.tanfovy, d_dev, t["shs"], s.sh_degree, s.campos, geom, K, binning,
                                                  img, False)
        finally:
            C.set_deterministic_backward(False)

    return sc, cam, dpix, fwd, backward


def grid(cfg, elements, report):
    import torch
    import gs_helpers as G
    import oracle as O
    sc, cam, dpix, fwd, backward = _setup(cfg)
    P = CONFIGS[cfg][0]
    got = {}
    for mode in ("deterministic", "default"):
        g = backward(mode == "deterministic")
        torch.cuda.synchronize()
        got[mode] = [x.cpu().numpy() for x in g]
    det2 = [x.cpu().numpy() for x in backward(True)]
    same_bits = all(np.array_equal(a, b) for a, b in zip(got["deterministic"], det2))
    del fwd, backward
    torch.cuda.empty_cache()
    O.set_threads(O.host_threads(16))
    t0 = time.time()
    os_ = O.settings_from_camera(cam)
    kw = dict(shs=sc.shs, scales=sc.scales, rotations=sc.rotations)
    ref = O.forward(os_, sc.means3D, sc.opacities, **kw)
    rg = O.backward(os_, ref, sc.means3D, dpix, **kw)
    al, ties = O.grad_allowance(os_, ref, sc.means3D, dpix, parts=True, **kw)
    print(f"config {cfg}: oracle {time.time() - t0:.1f} s", flush=True)
    os.environ["GS_ELEM_SOFT"] = "1"  # record only
    os.environ["GS_ELEM_REPORT"] = report
    for mode in ("deterministic", "default"):
        G.assert_grads_elementwise(f"config{cfg}_{mode}", NAMES, got[mode], rg, sc, cam, ref, allow=al, ties=ties)
    extra = {"case": f"config{cfg}_paths", "deterministic_repeat_same_bits": bool(same_bits),
             "rel_err_deterministic_vs_default": {n: G.rel_err(a, b) for n, a, b in
                                                  zip(NAMES, got["deterministic"], got["default"])},
             "rel_err_vs_oracle": {m: {n: G.rel_err(a, rg[n]) for n, a in zip(NAMES, got[m])} for m in got},
             "elements": []}
    for spec in elements:
        name, idx = spec.split(":")
        idx = int(idx)
        k = NAMES.index(name)
        r = np.asarray(rg[name], np.float64)
        per = r.size // P
        readings = [("flat", idx)] + [(f"gaussian_component_{j}", idx * per + j) for j in range(per)]
        for reading, flat in readings:
            if flat >= r.size:
                continue
            rec = {"tensor": name, "index": idx, "read_as": reading, "flat": flat, "gaussian": flat // per,
                   "ref": float(r.flat[flat]), "context": G.gaussian_context(flat // per, sc, cam, ref)}
            for m in got:
                v = float(got[m][k].flat[flat])
                rec[m] = v
                rec[m + "_rel_err"] = abs(v - rec["ref"]) / abs(rec["ref"]) if rec["ref"] else None
            extra["elements"].append(rec)
    with open(report, "a") as f:
        f.write(json.dumps(extra) + "\n")
    print(json.dumps(extra)[:2000], flush=True)


def timing(cfg, runs, report):
    import torch
    import gaussian_splatting_with_eye_tracking_amd._C as C
    sc, cam, dpix, fwd, backward = _setup(cfg)
    K = fwd[0]
    P = CONFIGS[cfg][0]
    C.profile_enable(True)
    C.profile_stages([])
    for det in (True, False, True, False):  # warm both paths
        backward(det)
    torch.cuda.synchronize()
    ms = {True: [], False: []}
    zero = {True: [], False: []}
    call = {True: [], False: []}
    for _ in range(runs):
        for det in (True, False):  # alternating
            C.profile_read(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            backward(det)
            e1.record()
            torch.cuda.synchronize()
            prof = C.profile_read(True)
            ms[det].append(prof["render_bwd"][0])
            zero[det].append(prof["zero_accum"][0])
            call[det].append(e0.elapsed_time(e1))
    C.profile_enable(False)
    med = lambda x: float(np.median(x))  # noqa: E731
    rec = {"case": f"config{cfg}_timing", "P": P, "K": int(K), "runs": runs,
           "scratch_bytes": int(C.backward_deterministic_scratch_bytes(P, K)),
           "render_bwd_ms": {"deterministic": med(ms[True]), "default": med(ms[False]),
                             "deterministic_min_max": [min(ms[True]), max(ms[True])],
                             "default_min_max": [min(ms[False]), max(ms[False])]},
           "accum_zeroing_ms": {"deterministic": med(zero[True]), "default": med(zero[False])},
           "backward_call_ms": {"deterministic": med(call[True]), "default": med(call[False])},
           "note": "render_bwd: the library's stage events (deterministic: blend + reduction; default: the blend "
                   "kernel's dispatch); the default path of a repeated backward also zeroes grad_accum "
                   "(accum_zeroing_ms; after a fresh forward the forward has done it); backward_call_ms: the "
                   "whole binding, profiler on"}
    rec["render_bwd_ratio"] = rec["render_bwd_ms"]["deterministic"] / rec["render_bwd_ms"]["default"]
    with open(report, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, nargs="*", default=None, help="configs for the allowance grid (2 4)")
    ap.add_argument("--timing", type=int, nargs="*", default=None, help="configs for the timing (2)")
    ap.add_argument("--runs", type=int, default=24)
    ap.add_argument("--elements", nargs="*", default=["dL_dscales:2944233"], help="tensor:index, config 4")
    a = ap.parse_args()
    report = os.environ.get("GS_ELEM_REPORT") or os.path.join(ROOT, "profiles", "deterministic_elementwise.jsonl")
    import torch
    if not torch.cuda.is_available():
        sys.exit("measure_deterministic_backward: no GPU (nothing is measured without one)")
    for cfg in (a.timing if a.timing is not None else []):
        timing(cfg, a.runs, report)
    for cfg in (a.grid if a.grid is not None else []):
        grid(cfg, a.elements if cfg == 4 else [], report)


if __name__ == "__main__":
    main()
