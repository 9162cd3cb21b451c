#!/usr/bin/env python3
"""Measure the depth / alpha maps' cost on one build (a tool, not a test;
needs the GPU): BASELINE config 2 (1M Gaussians, 1920x1080, seed 0), warm,
the three variants alternating, the median and quartiles of --runs calls each
(device time between two events around the calls, which includes the
forward's K read-back):

  (a) plain:  rasterize_gaussians + rasterize_gaussians_backward;
  (b) aux:    rasterize_gaussians_aux + rasterize_gaussians_backward_aux with
              all three cotangents;
  (c) twice:  what a caller had to do without the aux entries -- (a) plus a
              second full forward + backward with colors_precomp = (z, 1, 0)
              on a zero background (z taken from the first forward's geometry
              buffer outside the timed region, in (c)'s favour; that second
              pass still cannot carry dL/dz to means3D).

Writes profiles/aux_outputs.json (--out).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_outputs.json"))
    ap.add_argument("--size", type=int, nargs=3, default=None, metavar=("P", "W", "H"), help="instead of config 2")
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
    zero_bg = torch.zeros(3, device="cuda")
    dpix = torch.from_numpy(S.make_cotangent(H, W, 1)).cuda()
    dd = torch.from_numpy(np.ascontiguousarray(S.make_cotangent(H, W, 2)[0:1])).cuda()
    da = torch.from_numpy(np.ascontiguousarray(S.make_cotangent(H, W, 3)[0:1])).cuda()
    daux = torch.cat([dd, da, torch.zeros_like(dd)], 0).contiguous()

    def fwd(fn, bg, col, sh):
        return fn(bg, t["means3D"], col, t["opacities"], t["scales"], t["rotations"], s.scale_modifier, e,
                  s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width, sh, s.sh_degree,
                  s.campos, s.prefiltered, s.debug)

    def bwd(bg, col, sh, radii, geom, K, binning, img, dp):
        return C.rasterize_gaussians_backward(bg, t["means3D"], radii, col, t["scales"], t["rotations"],
                                              s.scale_modifier, e, s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy,
                                              dp, sh, s.sh_degree, s.campos, geom, K, binning, img, False)

    def plain():
        K, color, radii, geom, binning, img = fwd(C.rasterize_gaussians, s.bg, e, t["shs"])
        return bwd(s.bg, e, t["shs"], radii, geom, K, binning, img, dpix)

    def aux():
        K, color, depth, alpha, radii, geom, binning, img = fwd(C.rasterize_gaussians_aux, s.bg, e, t["shs"])
        return C.rasterize_gaussians_backward_aux(s.bg, t["means3D"], radii, e, t["scales"], t["rotations"],
                                                  s.scale_modifier, e, s.viewmatrix, s.projmatrix, s.tanfovx,
                                                  s.tanfovy, dpix, dd, da, t["shs"], s.sh_degree, s.campos, geom, K,
                                                  binning, img, False)

    K0, _, _, geom0, bin0, img0 = fwd(C.rasterize_gaussians, s.bg, e, t["shs"])
    z = C.parse_buffers(geom0, bin0, img0, P, K0, W, H, 16)["depths"]
    feats = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1).contiguous()

    def twice():
        plain()
        K, color, radii, geom, binning, img = fwd(C.rasterize_gaussians, zero_bg, feats, e)
        return bwd(zero_bg, feats, e, radii, geom, K, binning, img, daux)

    variants = {"a_plain": plain, "b_aux": aux, "c_twice": twice}
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
           "device": torch.cuda.get_device_name(0), "unit": "ms per forward + backward", "variants": {}}
    for k, v in times.items():
        q1, med, q3 = (float(x) for x in np.percentile(v, [25, 50, 75]))
        rec["variants"][k] = {"median": med, "q1": q1, "q3": q3, "min": float(min(v)), "max": float(max(v))}
        print(f"{k:8s} median {med:.4f} ms  quartiles [{q1:.4f}, {q3:.4f}]")
    v = rec["variants"]
    rec["aux_over_plain_ms"] = v["b_aux"]["median"] - v["a_plain"]["median"]
    rec["twice_over_plain_ms"] = v["c_twice"]["median"] - v["a_plain"]["median"]
    rec["b_faster_than_c_quartiles_disjoint"] = v["b_aux"]["q3"] < v["c_twice"]["q1"]
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
