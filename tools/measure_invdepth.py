#!/usr/bin/env python3
"""Measure the inverse-depth map's and the depth-regularised iteration's cost
on one build (a tool, not a test; needs the GPU): BASELINE config 2 (1M
Gaussians, 1920x1080, seed 0), warm, the five variants alternating, the median
and quartiles of --runs calls each (device time between two events around the
calls, which includes the forward's K read-back):

  (a) plain:     rasterize_gaussians + rasterize_gaussians_backward;
  (b) aux:       rasterize_gaussians_aux + rasterize_gaussians_backward_aux
                 with all three cotangents;
  (c) invdepth:  rasterize_gaussians_invdepth +
                 rasterize_gaussians_backward_invdepth with all three
                 cotangents -- (b)'s work but for one division per staged
                 record;
  (d) iteration: training.training_iteration, fused, without a target;
  (e) iteration with an inverse-depth target and a mask.

Writes profiles/invdepth.json (--out).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "invdepth.json"))
    ap.add_argument("--size", type=int, nargs=3, default=None, metavar=("P", "W", "H"), help="instead of config 2")
    a = ap.parse_args()
    import torch
    import gs_helpers as G
    import gaussian_splatting_with_eye_tracking_amd._C as C
    from gaussian_splatting_with_eye_tracking_amd import rasterization as R
    from gaussian_splatting_with_eye_tracking_amd import synthetic as S
    from gaussian_splatting_with_eye_tracking_amd import training as T
    P, W, H, seed = CONFIG2 if a.size is None else (*a.size, 0)
    sc, cam = G.scene_and_camera(P, W, H, seed)
    s = G.torch_settings(cam)
    t = G.scene_tensors(sc)
    e = torch.Tensor([])
    ops = (t["means3D"], t["shs"], e, t["opacities"], t["scales"], t["rotations"], e)
    dpix = torch.from_numpy(S.make_cotangent(H, W, 1)).cuda()
    dd = torch.from_numpy(np.ascontiguousarray(S.make_cotangent(H, W, 2)[0:1])).cuda()
    da = torch.from_numpy(np.ascontiguousarray(S.make_cotangent(H, W, 3)[0:1])).cuda()

    def plain():
        K, color, radii, geom, binning, img = C.rasterize_gaussians(*R.native_forward_args(s, *ops))
        return K, C.rasterize_gaussians_backward(*R.native_backward_args(s, *ops, radii, geom, binning, img, K, dpix))

    def maps(forward, backward):
        def run():
            K, color, depth, alpha, radii, geom, binning, img = forward(*R.native_forward_args(s, *ops))
            return backward(*R.native_backward_args(s, *ops, radii, geom, binning, img, K, dpix, (dd, da)))
        return run

    K0 = plain()[0]
    # the training iteration of tools/bench_train.py: no densify step, the statistics and Adam included
    m = T.FlatGaussianModel(G.raw_from_scene(sc), 3, spatial_lr_scale=5.0)
    m.active_sh_degree = 3
    gt = torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    with torch.no_grad():
        target = C.rasterize_gaussians_invdepth(*R.native_forward_args(s, *ops))[2] * 1.05
    mask = (torch.rand(1, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) < 0.8).float()
    it = [100]

    def iteration(**kw):
        def run():
            it[0] += 1
            return T.training_iteration(m, it[0], s, gt, scene_extent=5.0, **kw)
        return run

    variants = {"a_plain": plain,
                "b_aux": maps(C.rasterize_gaussians_aux, C.rasterize_gaussians_backward_aux),
                "c_invdepth": maps(C.rasterize_gaussians_invdepth, C.rasterize_gaussians_backward_invdepth),
                "d_iteration": iteration(),
                "e_iteration_depth": iteration(invdepth_target=target, depth_mask=mask)}
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
    rec = {"P": P, "W": W, "H": H, "seed": seed, "K": int(K0), "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0),
           "unit": "ms per forward + backward (a-c), per training iteration (d, e)", "variants": {}}
    for k, v in times.items():
        q1, med, q3 = (float(x) for x in np.percentile(v, [25, 50, 75]))
        rec["variants"][k] = {"median": med, "q1": q1, "q3": q3, "min": float(min(v)), "max": float(max(v))}
        print(f"{k:18s} median {med:.4f} ms  quartiles [{q1:.4f}, {q3:.4f}]")
    v = rec["variants"]
    rec["invdepth_over_aux_ms"] = v["c_invdepth"]["median"] - v["b_aux"]["median"]
    rec["invdepth_over_plain_ms"] = v["c_invdepth"]["median"] - v["a_plain"]["median"]
    rec["b_c_interquartile_ranges_overlap"] = (v["c_invdepth"]["q1"] <= v["b_aux"]["q3"] and
                                                v["b_aux"]["q1"] <= v["c_invdepth"]["q3"])
    rec["depth_target_over_iteration_ms"] = v["e_iteration_depth"]["median"] - v["d_iteration"]["median"]
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
