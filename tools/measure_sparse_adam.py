#!/usr/bin/env python3
"""Measure the sparse Adam step against the dense one on one build (a tool,
not a test; needs the GPU): P = 1M Gaussians, M = 16 (59 floats each), warm,
all variants alternating, the median and quartiles of --runs samples each
(device time between two events around --reps calls, divided by --reps):

  dense                 _C.adam_step over all 59 P parameters (the baseline);
  sparse <f> random     _C.sparse_adam_step, every row visible with probability f;
  sparse <f> runs       the same share in contiguous runs of --run-length rows;
  sparse config2        BASELINE config 2's own forward radii (1920x1080, seed 0).

Achieved GB/s is on the byte model 28 * 59 * visible + 4 P for the sparse
step and 28 * 59 * P for the dense one.  Then one fused training_iteration at
config 2's camera with optimizer_type "default" and "sparse_adam",
alternating (densification off; includes the forward's K read-back).

Writes profiles/sparse_adam.json (--out).
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
FRACTIONS = (1.0, 0.5, 0.1, 0.0)


def quartiles(v):
    q1, med, q3 = (float(x) for x in np.percentile(v, [25, 50, 75]))
    return {"median": med, "q1": q1, "q3": q3, "min": float(min(v)), "max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="calls per timed sample")
    ap.add_argument("--run-length", type=int, default=1024, help="rows per visible run of the 'runs' masks")
    ap.add_argument("--size", type=int, nargs=3, default=None, metavar=("P", "W", "H"), help="instead of config 2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_adam.json"))
    a = ap.parse_args()
    import torch
    import gs_helpers as G
    import gaussian_splatting_with_eye_tracking_amd._C as C
    from gaussian_splatting_with_eye_tracking_amd import training as T
    P, W, H, seed = CONFIG2 if a.size is None else (*a.size, 0)
    sc, cam = G.scene_and_camera(P, W, H, seed)
    s = G.torch_settings(cam)
    gt = torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    off = dict(densify_from_iter=10**9, densify_until_iter=0)
    models = {k: T.FlatGaussianModel(G.raw_from_scene(sc), 3, spatial_lr_scale=5.0,
                                     opt=T.OptimizationParams(optimizer_type=k, **off))
              for k in T.OPTIMIZER_TYPES}
    for m in models.values():
        m.active_sh_degree = 3
    m = models["default"]
    pkg, _ = m.render_and_backward(s, gt, m.opt.lambda_dssim)  # real gradients and config 2's radii
    radii2 = pkg["radii"].clone()
    n = m.params.numel()
    width = n // P

    rng = np.random.default_rng(0)
    masks = {}
    for f in FRACTIONS:
        patterns = ("random", "runs") if 0.0 < f < 1.0 else ("all" if f == 1.0 else "none",)
        for pat in patterns:
            if pat == "runs":
                period = int(round(a.run_length / f))
                vis = (np.arange(P) % period) < a.run_length
            else:
                vis = rng.random(P) < f
            masks[f"sparse {f:g} {pat}"] = torch.from_numpy(np.where(vis, 7, 0).astype(np.int32)).cuda()
    masks["sparse config2"] = radii2
    lrs = [float(m.lr[g]) for g in T.GROUPS]
    bufs = (m.params.clone(), m.grads.clone(), m.exp_avg.clone(), m.exp_avg_sq.clone())

    def dense():
        C.adam_step(*bufs, m.seg_end, lrs, [7] * 6, T.BETAS[0], T.BETAS[1], T.EPS)

    def sparse(r):
        return lambda: C.sparse_adam_step(*bufs, m.seg_end, lrs, [7] * 6, r, T.BETAS[0], T.BETAS[1], T.EPS)

    variants = {"dense": dense, **{k: sparse(r) for k, r in masks.items()}}
    times = {k: [] for k in variants}
    for i in range(a.warmup + a.runs):
        for k, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(a.reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[k].append(t0.elapsed_time(t1) / a.reps)
    rec = {"P": P, "floats_per_gaussian": width, "W": W, "H": H, "seed": seed, "runs": a.runs, "warmup": a.warmup,
           "reps_per_sample": a.reps, "run_length": a.run_length, "device": torch.cuda.get_device_name(0),
           "unit": "ms per optimiser step", "byte_model": "sparse: 28 * width * visible + 4 P; dense: 28 * width * P",
           "variants": {}}
    for k, v in times.items():
        q = quartiles(v)
        visible = P if k == "dense" else int((masks[k] > 0).sum())
        nbytes = 28 * width * visible + (0 if k == "dense" else 4 * P)
        q.update(visible=visible, visible_fraction=visible / P, model_bytes=nbytes,
                 achieved_GBps=nbytes / (q["median"] * 1e-3) / 1e9)
        rec["variants"][k] = q
        print(f"{k:22s} visible {visible / P:6.3f}  median {q['median']:.4f} ms  [{q['q1']:.4f}, {q['q3']:.4f}]  "
              f"{q['achieved_GBps']:.0f} GB/s")
    d = rec["variants"]["dense"]["median"]
    rec["sparse_over_dense"] = {k: v["median"] / d for k, v in rec["variants"].items() if k != "dense"}

    it_times = {k: [] for k in models}
    for i in range(a.warmup + a.runs):
        for k, model in models.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            T.training_iteration(model, 1 + i, s, gt, scene_extent=5.0, fused=True)
            t1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                it_times[k].append(t0.elapsed_time(t1))
    rec["training_iteration_ms"] = {k: quartiles(v) for k, v in it_times.items()}
    rec["training_iteration_visible_fraction"] = float((radii2 > 0).sum()) / P
    for k, v in rec["training_iteration_ms"].items():
        print(f"training_iteration {k:12s} median {v['median']:.4f} ms  [{v['q1']:.4f}, {v['q3']:.4f}]")
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
