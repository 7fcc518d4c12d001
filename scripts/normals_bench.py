#!/usr/bin/env python
"""Timing of the surface-normal feature.  Three steps, each its own process so that a caller can give each its
own time limit (and run the first under `rocprofv3 --kernel-trace --stats -- python scripts/normals_bench.py kernel`):

    python scripts/normals_bench.py kernel                      pmn_depth_normals at 1600x1200, r = 1, 2, 3: device events, us per
                                                                launch, achieved GB/s of the 16 B/pixel the kernel must move
    python scripts/normals_bench.py gen DATA [scans] [views]    DTU-layout scans of the photo-consistent scene (tests/synth.py)
    python scripts/normals_bench.py eval DATA TREE normals      TREE/eval.py --output_type both [--normals 1] over DATA, one warm-up
                                                                and three timed runs in ONE process: depth-maps/s per run.  TREE
                                                                may be another checkout (the parent commit) for the comparison of
                                                                the default path.
"""
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0  # MI355X data-sheet HBM3E bandwidth


def kernel():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import normals_ref as NR
    from patchmatchnet_amd import ops
    H, W = 1200, 1600
    z, K = NR.random_scene(H, W, seed=1)
    zd = torch.from_numpy(z).cuda()
    floor_bytes = 16 * H * W
    for r in (1, 2, 3):
        for _ in range(20):
            ops.depth_normals(zd, K, r)
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(100):
                ops.depth_normals(zd, K, r)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 10.0)  # us per launch (back-to-back launches, output allocation included)
        us = sorted(times)[len(times) // 2]
        print("RESULT " + json.dumps({"kernel": "pmn_depth_normals", "H": H, "W": W, "radius": r, "us_median_of_5x100": round(us, 2),
                                      "us_runs": [round(t, 2) for t in times], "GBps_of_16B_per_pixel": round(floor_bytes / us / 1e3, 1),
                                      "fraction_of_hbm_peak": round(floor_bytes / us / 1e3 / HBM_PEAK_GBS, 3)}), flush=True)


def gen(data, n_scans=2, n_views=49):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    shutil.rmtree(data, ignore_errors=True)
    t0 = time.time()
    for s in range(n_scans):
        synth.write_scene_scan(data, "scan%d" % (s + 1), n_views, 1200, 1600, n_src=10, seed=s, device="cuda")
    with open(os.path.join(data, "list.txt"), "w") as f:
        f.write("".join("scan%d\n" % (s + 1) for s in range(n_scans)))
    print("generated %d scans x %d views in %.1f s" % (n_scans, n_views, time.time() - t0), flush=True)


def eval_runs(data, tree, normals):
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import eval as pm_eval
    assert os.path.dirname(os.path.abspath(pm_eval.__file__)) == tree
    ckpt = os.path.join(ROOT, "tests", "golden", "params_000007.npz")
    scans = [ln.strip() for ln in open(os.path.join(data, "list.txt")) if ln.strip()]
    n = sum(len(os.listdir(os.path.join(data, s, "cams"))) for s in scans)
    out = data.rstrip("/") + "_out"
    rates = []
    for run in range(4):
        shutil.rmtree(out, ignore_errors=True)
        argv = ["--input_folder", data, "--output_folder", out, "--checkpoint_path", ckpt, "--scan_list", os.path.join(data, "list.txt"),
                "--num_views", "5", "--output_type", "both", "--geo_mask_thres", "3"] + (["--normals", "1"] if normals else [])
        t = time.time()
        pm_eval.main(argv)
        dt = time.time() - t
        if run:  # run 0: library load, weight packing, plan recording, page cache
            rates.append(round(n / dt, 1))
    ply = sum(os.path.getsize(os.path.join(out, s, "fused.ply")) for s in scans)
    shutil.rmtree(out, ignore_errors=True)
    print("RESULT " + json.dumps({"tree": tree, "normals": int(normals), "samples": n, "depth_maps_per_s": rates,
                                  "median": sorted(rates)[1], "fused_ply_MB": round(ply / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "kernel":
        kernel()
    elif mode == "gen":
        gen(sys.argv[2], *[int(a) for a in sys.argv[3:5]])
    elif mode == "eval":
        eval_runs(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        sys.exit(__doc__)
