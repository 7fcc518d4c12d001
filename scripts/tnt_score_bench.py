#!/usr/bin/env python
"""Times one ICP iteration on the GPU at a realistic size, two ways, on clouds generated on the device from a seed (a 4 M-point
surface as the target, a 4 M-point noisy copy under a small motion as the source):

  fused     registration.icp_accumulate: one pmn_icp_accumulate call (search + the seventeen sums) and the 17-double download;
  composed  the same iteration from the entry points that existed before it: torch pose, pointcloud.nn_distance(return_index=True)
            (pmn_nn_distance), a gather of the matched points and torch float64 reductions, downloaded the same way.

Prints one JSON line per measurement (median of --repeat runs after a warm-up, host clock around a device synchronise), and the
largest difference between the two sets of sums relative to the sum of the terms' magnitudes.  `--profile` runs each way once, for
`rocprofv3 --kernel-trace --stats -- python scripts/tnt_score_bench.py --profile`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def clouds(dev, n):
    import torch
    g = torch.Generator(device=dev).manual_seed(7)

    def surface(m, noise):
        xy = torch.rand(m, 2, generator=g, device=dev, dtype=torch.float64) * 10.0
        z = 2.0 + 0.8 * torch.sin(xy[:, 0] / 1.7) * torch.cos(xy[:, 1] / 2.3) + 0.05 * xy[:, 0]
        p = torch.cat([xy, z[:, None]], 1)
        return (p + noise * torch.randn(m, 3, generator=g, device=dev, dtype=torch.float64)).float()

    return surface(n, 0.003), surface(n, 0.0)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, default=4_000_000)
    ap.add_argument("--tau", type=float, default=0.01)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    import tnt_ref as R
    from patchmatchnet_amd import pointcloud as PC, registration as RG
    dev = "cuda:0"
    src, tgt = clouds(dev, args.points)
    pose = R.rigid(R.rotation((1.0, 2.0, 3.0), 0.05), (0.3 * args.tau, -0.2 * args.tau, 0.25 * args.tau))
    max_dist = 2 * args.tau
    grid = PC.build_grid(tgt, 2 * args.tau)
    centre = RG.grid_centre(grid)
    order = RG.query_order(src, grid, pose)
    c = torch.tensor(centre, dtype=torch.float64, device=dev)

    def fused():
        return RG.icp_accumulate(src, grid, pose, centre, max_dist, order).cpu().numpy()

    def composed():
        moved = RG.transform(src, pose)  # (float32 queries: pmn_nn_distance takes nothing else)
        d, idx = PC.nn_distance(moved, grid, max_dist, return_index=True)
        hit = idx >= 0
        a = moved[hit].double() - c
        b = tgt[idx[hit]].double() - c
        s = torch.cat([hit.sum().double()[None], a.sum(0), b.sum(0), (a[:, :, None] * b[:, None, :]).sum(0).reshape(-1), (d[hit] * d[hit]).sum()[None]])
        return s.cpu().numpy()

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    if args.profile:
        fused()
        composed()
        return
    a, b = fused(), composed()
    rows = {}
    for name, fn in (("fused", fused), ("composed", composed), ("fused_again", fused), ("composed_again", composed)):
        med, lo, hi = timed(fn)
        rows[name] = med
        print(json.dumps({"what": "icp_iteration", "way": name, "points": [args.points, args.points], "max_dist": max_dist,
                          "median_s": round(med, 5), "min_s": round(lo, 5), "max_s": round(hi, 5), "repeat": args.repeat}), flush=True)
    print(json.dumps({"what": "icp_iteration_summary", "matched": [int(a[0]), int(b[0])],
                      "composed_over_fused": round((rows["composed"] + rows["composed_again"]) / (rows["fused"] + rows["fused_again"]), 3),
                      "note": "the composed way rounds the posed points to float32, so its matches and sums differ slightly",
                      "max_rel_sum_difference": float(np.max(np.abs(a[1:] - b[1:]) / np.maximum(np.abs(a[1:]), 1e-300)))}), flush=True)


if __name__ == "__main__":
    main()
