"""Timings behind DESIGN.md section 31 (profiles/cloud_normals_measure.log): the fused normals kernel (pmn_knn_normals) beside the search
alone (pmn_knn_distance, mean only) and beside the unfused route built from what the library had before -- knn_distance with the index
lists, a torch gather, the covariance in torch and torch.linalg.eigh.

    python scripts/cloud_normals_bench.py [--points 5000000] [--reps 5] [--log profiles/cloud_normals_measure.log]

The cloud is scripts/clean_cloud_bench.py's: a noisy sheet of --points points with 2 % planted outliers up to 200 units off, searched
in its own default grid with the default max_dist (16 cells), same_cloud.  Every figure is the median of --reps timed runs after one
warm-up, measured with events on the stream."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clean_cloud_bench import sheet, timed  # noqa: E402


def unfused(PC, pts, grid, k, max_dist):
    """Normals by the route the library offered before the fused kernel: the lists, a gather, moments and eigh in torch (float64).
    Capped slots are masked out; no orientation, no degenerate test."""
    _, idx = PC.knn_distance(None, grid, k, max_dist, same_cloud=True, return_index=True)
    live = idx >= 0
    d = (pts[idx.clamp_min(0)].double() - pts.double()[:, None, :]) * live[:, :, None]
    m = live.sum(1).double() + 1.0
    s = d.sum(1)
    C = torch.einsum("nka,nkb->nab", d, d) - s[:, :, None] * s[:, None, :] / m[:, None, None]
    return torch.linalg.eigh(C)[1][:, :, 0].float()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "cloud_normals_measure.log"))
    ap.add_argument("--unfused_reps", type=int, default=3, help="timed runs of the unfused route (torch.linalg.eigh on every point)")
    ap.add_argument("--skip_unfused", action="store_true")
    args = ap.parse_args()
    from patchmatchnet_amd import pointcloud as PC
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "w")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    n = args.points
    side = 1000.0 * (n / 5e6) ** 0.5  # 5 points per square unit
    pts = torch.from_numpy(sheet(n, 0, side)).cuda()
    cell = PC.default_cell(pts)
    grid = PC.build_grid(pts, cell)
    md = PC.CLEAN_MAX_DIST_CELLS * cell
    views = np.stack([np.array([side * (i % 7) / 6.0, side * (i // 7) / 6.0, 800.0]) for i in range(49)])
    say(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {n} points over {side:.0f} x {side:.0f} units, 2 % outliers; "
        f"same-cloud, cell {cell:.4f}, max_dist {md:.2f}; median [min, max] of {args.reps} runs after one warm-up, milliseconds")
    say("\n# k | knn_distance (mean only) | knn_normals | knn_normals, variation and count | knn_normals, 49 viewpoints given as host "
        "numbers (the figure includes the wrapper's upload and its finiteness check, one host read); then the unfused route (lists, "
        "gather, covariance and eigh in torch)")
    for k in (8, 16, 20, 32):
        t_d = timed(lambda: PC.knn_distance(None, grid, k, md, same_cloud=True), args.reps)
        t_n = timed(lambda: PC.knn_normals(None, grid, k, md, same_cloud=True), args.reps)
        t_a = timed(lambda: PC.knn_normals(None, grid, k, md, same_cloud=True, return_variation=True, return_count=True), args.reps)
        t_v = timed(lambda: PC.knn_normals(None, grid, k, md, same_cloud=True, viewpoints=views), args.reps)
        say(f"k={k:2d}  distance {t_d[0]:8.2f} [{t_d[1]:.2f}, {t_d[2]:.2f}]  normals {t_n[0]:8.2f} [{t_n[1]:.2f}, {t_n[2]:.2f}] "
            f"x{t_n[0] / t_d[0]:.2f}  +outputs {t_a[0]:8.2f} [{t_a[1]:.2f}, {t_a[2]:.2f}]  +views {t_v[0]:8.2f} [{t_v[1]:.2f}, {t_v[2]:.2f}]")
        if not args.skip_unfused:
            try:
                t_u = timed(lambda: unfused(PC, pts, grid, k, md), args.unfused_reps)
                say(f"k={k:2d}  unfused ({args.unfused_reps} runs) {t_u[0]:8.2f} [{t_u[1]:.2f}, {t_u[2]:.2f}]  x{t_u[0] / t_n[0]:.2f} of fused")
            except torch.cuda.OutOfMemoryError:
                torch.cuda.empty_cache()
                say(f"k={k:2d}  unfused: out of memory")
    t = timed(lambda: PC.estimate_normals(pts, 16), args.reps)
    say(f"\nestimate_normals k=16, defaults (cell search, grid, walk, un-sort) {t[0]:9.2f} [{t[1]:.2f}, {t[2]:.2f}]")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
