#!/usr/bin/env python3
"""Measure the antialiased step against the plain step on one build (a tool,
not a test; needs the GPU): BASELINE config 2 (1M Gaussians, 1920x1080, seed
0), warm, the two variants alternating, the median and quartiles of --runs
calls each (device time between two events around the calls, which includes
the forward's K read-back):

  (a) plain:        rasterize_gaussians + rasterize_gaussians_backward;
  (b) antialiased:  the same two calls with antialiasing=True (the backward
                    with the forward's opacities).

The binning is the same either way (K is recorded for both); the blends see
smaller opacities with the flag on, so their early exits move -- which is the
scene's doing, not the kernels'.  --stages adds the per-stage profile of each
variant (preprocess and the per-Gaussian backward are the kernels that differ).

Writes profiles/antialiasing.json (--out).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

CONFIG2 = (1_000_000, 1920, 1080, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "antialiasing.json"))
    ap.add_argument("--size", type=int, nargs=3, default=None, metavar=("P", "W", "H"), help="instead of config 2")
    ap.add_argument("--stages", action="store_true", help="also the per-stage medians of --runs more steps of each variant, alternating")
    a = ap.parse_args()
    import torch
    import gs_helpers as G
    import gaussian_splatting_with_eye_tracking_amd._C as C
    from gaussian_splatting_with_eye_tracking_amd import synthetic as S
    P, W, H, seed = CONFIG2 if a.size is None else (*a.size, 0)
    sc, cam = G.scene_and_camera(P, W, H, seed)
    s = G.torch_settings(cam)
    t = G.scene_tensors(sc)
    e = torch.Tensor([])
    dpix = torch.from_numpy(S.make_cotangent(H, W, 1)).cuda()
    rendered = {}

    def step(aa: bool):
        K, color, radii, geom, binning, img = C.rasterize_gaussians(
            s.bg, t["means3D"], e, t["opacities"], t["scales"], t["rotations"], s.scale_modifier, e, s.viewmatrix,
            s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width, t["shs"], s.sh_degree, s.campos,
            s.prefiltered, s.debug, aa)
        rendered[aa] = int(K)
        return C.rasterize_gaussians_backward(
            s.bg, t["means3D"], radii, e, t["scales"], t["rotations"], s.scale_modifier, e, s.viewmatrix,
            s.projmatrix, s.tanfovx, s.tanfovy, dpix, t["shs"], s.sh_degree, s.campos, geom, K, binning, img, False,
            t["opacities"], aa)

    variants = {"a_plain": lambda: step(False), "b_antialiased": lambda: step(True)}
    times = {k: [] for k in variants}
    for i in range(a.warmup + a.runs):
        for k, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[k].append(t0.elapsed_time(t1))
    rec = {"P": P, "W": W, "H": H, "seed": seed, "K": {"plain": rendered[False], "antialiased": rendered[True]},
           "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "unit": "ms per forward + backward", "variants": {}}
    for k, v in times.items():
        q1, med, q3 = (float(x) for x in np.percentile(v, [25, 50, 75]))
        rec["variants"][k] = {"median": med, "q1": q1, "q3": q3, "min": float(min(v)), "max": float(max(v))}
        print(f"{k:14s} median {med:.4f} ms  quartiles [{q1:.4f}, {q3:.4f}]")
    v = rec["variants"]
    rec["antialiased_over_plain_ms"] = v["b_antialiased"]["median"] - v["a_plain"]["median"]
    rec["quartile_ranges_overlap"] = (v["b_antialiased"]["q1"] <= v["a_plain"]["q3"] and
                                      v["a_plain"]["q1"] <= v["b_antialiased"]["q3"])
    if a.stages:
        # the stage events serialise the launches: these sum to more than the step above
        C.profile_enable(True)
        C.profile_stages([])
        per = {k: {} for k in variants}
        for _ in range(a.runs):
            for k, fn in variants.items():  # alternating, as above
                C.profile_read(True)
                fn()
                torch.cuda.synchronize()
                for n, (ms, cnt) in C.profile_read(True).items():
                    if cnt:
                        per[k].setdefault(n, []).append(ms / cnt)
        C.profile_enable(False)
        rec["stages_median_ms"] = {k: {n: float(np.median(v)) for n, v in d.items()} for k, d in per.items()}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
