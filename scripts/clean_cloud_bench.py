"""Timings behind DESIGN.md section 23 (profiles/clean_cloud_measure.log): the k-nearest walk beside the one-best walk, the cell sweep
behind pointcloud.CLEAN_CELL_POINTS, the max_dist multiples behind CLEAN_MAX_DIST_CELLS, and clean_cloud.py end to end.

    python scripts/clean_cloud_bench.py [--points 5000000] [--reps 5] [--log profiles/clean_cloud_measure.log]

The cloud is generated: a noisy sheet of --points points with 2 % planted outliers up to 200 units off.  Every figure is the median of
--reps timed runs after one warm-up, measured with events on the stream; the end-to-end figure is the wall time of the subprocess."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sheet(n, seed, side):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, side, (n, 2))
    z = 40.0 * np.sin(xy[:, 0] / 90.0) * np.cos(xy[:, 1] / 70.0) + rng.normal(0.0, 0.05, n)
    out = rng.random(n) < 0.02
    z[out] += rng.uniform(-200.0, 200.0, int(out.sum()))
    return np.stack([xy[:, 0], xy[:, 1], z], 1).astype(np.float32)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "clean_cloud_measure.log"))
    ap.add_argument("--skip_cli", action="store_true")
    args = ap.parse_args()
    from patchmatchnet_amd import fusion, pointcloud as PC
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "w")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    n = args.points
    side = 1000.0 * (n / 5e6) ** 0.5  # 5 points per square unit
    host = sheet(n, 0, side)
    pts = torch.from_numpy(host).cuda()
    qry = torch.from_numpy(sheet(n, 1, side)).cuda()
    say(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {n} points over {side:.0f} x {side:.0f} units, 2 % outliers; "
        f"median [min, max] of {args.reps} runs after one warm-up, milliseconds")

    say("\n# cell sweep: same-cloud k = 20, mean only, max_dist 8 units; points per occupied cell; search alone (grid built before)")
    for cell in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0):
        g = PC.build_grid(pts, cell)
        occ = n / int(torch.unique(g.keys).numel())
        t = timed(lambda: PC.knn_distance(None, g, 20, 8.0, same_cloud=True), args.reps)
        say(f"cell {cell:5.2f}  points/cell {occ:7.2f}  knn k=20 {t[0]:9.2f} [{t[1]:.2f}, {t[2]:.2f}]")

    t = timed(lambda: PC.default_cell(pts), 3)
    cell = PC.default_cell(pts)
    g = PC.build_grid(pts, cell)
    say(f"\ndefault_cell (target {PC.CLEAN_CELL_POINTS:g} points per occupied cell): {cell:.4f}, {t[0]:.2f} ms; build_grid "
        f"{timed(lambda: PC.build_grid(pts, cell), 3)[0]:.2f} ms")

    say("\n# max_dist in cells at the default cell: same-cloud k = 20; points whose list has a capped slot")
    for mult in (4.0, 8.0, 16.0, 32.0, 64.0):
        t = timed(lambda: PC.knn_distance(None, g, 20, mult * cell, same_cloud=True), args.reps)
        _, d2 = PC.knn_distance(None, g, 20, mult * cell, same_cloud=True, return_d2=True)
        capped = int((d2[:, -1] == (mult * cell) ** 2).sum())
        del d2
        say(f"max_dist {mult:4.0f} cells = {mult * cell:7.2f}  knn k=20 {t[0]:9.2f} [{t[1]:.2f}, {t[2]:.2f}]  capped {capped} "
            f"({100.0 * capped / n:.2f} %)")

    md = PC.CLEAN_MAX_DIST_CELLS * cell
    say(f"\n# one-best walk beside the k-best walk: {n} separate queries (a second sample of the sheet), same grid, max_dist {md:.2f}")
    t1 = timed(lambda: PC.nn_distance(qry, g, md), args.reps)
    say(f"nn_distance          {t1[0]:9.2f} [{t1[1]:.2f}, {t1[2]:.2f}]")
    for k in (1, 8, 16, 20, 32):
        t = timed(lambda: PC.knn_distance(qry, g, k, md), args.reps)
        say(f"knn_distance k={k:2d}    {t[0]:9.2f} [{t[1]:.2f}, {t[2]:.2f}]  x{t[0] / t1[0]:.2f}")
    t = timed(lambda: PC.radius_count(qry, g, 2.0 * cell), args.reps)
    say(f"radius_count r={2.0 * cell:.2f}  {t[0]:9.2f} [{t[1]:.2f}, {t[2]:.2f}]")
    t = timed(lambda: PC.statistical_outliers(pts, 20), 3)
    say(f"statistical_outliers k=20, defaults (cell search, grid, walk, threshold) {t[0]:9.2f} [{t[1]:.2f}, {t[2]:.2f}]")

    if not args.skip_cli:
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "fused.ply")
            fusion.write_ply(src, host, np.full((n, 3), 200, np.uint8))
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, os.path.join(ROOT, "clean_cloud.py"), "--input", src, "--output",
                                os.path.join(d, "fused_clean.ply"), "--method", "statistical"], capture_output=True, text=True)
            wall = time.perf_counter() - t0
            say(f"\nclean_cloud.py --method statistical, {n} points, end to end (start of python to exit, {os.path.getsize(src) >> 20} MiB read): "
                f"{wall:.2f} s, exit {r.returncode}")
            say(r.stdout.strip().replace(d, "TMP") or r.stderr.strip()[-400:])
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
