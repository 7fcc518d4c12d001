"""Timings behind DESIGN.md section 36 (profiles/cloud_mls_measure.log): the moving-least-squares kernel (pmn_knn_mls) at both degrees
beside pmn_knn_normals at the same k on the same grid -- the same search with a cheaper epilogue -- and beside the plain route built
from what the library had before: knn_distance with the index lists, a torch gather, the weighted covariance with torch.linalg.eigh
and the quadric by batched torch.linalg.lstsq.

    python scripts/cloud_mls_bench.py [--points 5000000] [--reps 5] [--log profiles/cloud_mls_measure.log]

The cloud is scripts/clean_cloud_bench.py's: a noisy sheet of --points points with 2 % planted outliers up to 200 units off, searched
in its own default grid, same_cloud; the radius is the default max_dist of the other cloud benches (16 cells), so that knn_mls and
knn_normals walk exactly the same cells.  Every figure is the median [min, max] of --reps timed runs after one warm-up, measured with
events on the stream.  The plain route runs in chunks of --chunk queries (its [chunk, k, 6] float64 design matrices would not fit
otherwise), timed on the host around a synchronisation, one run after a warm-up.  At degree 2 it is timed on the first
--lstsq_queries queries only and the log says EXTRAPOLATED: batched torch.linalg.lstsq on this stack (torch 2.10, ROCm 7) needs about 18 ms
per 6-column system, so the whole cloud would take a day."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clean_cloud_bench import sheet, timed  # noqa: E402


def plain_chunk(pts, idx, radius, degree):
    """MLS for the queries of ``idx`` [c,k] (their own cloud: row i of idx belongs to pts_q) by library solvers in float64: the
    positions [c,3].  Capped slots get weight 0; no validity rule and no fallback."""
    q, nb = pts[0].double(), pts[1]
    live = idx >= 0
    d = (nb[idx.clamp_min(0)].double() - q[:, None, :]) * live[:, :, None]
    w = (1.0 - (d * d).sum(2) / (radius * radius)).clamp_min(0.0) ** 4 * live
    d = torch.cat([torch.zeros_like(d[:, :1]), d], 1)            # the query itself, weight 1
    w = torch.cat([torch.ones_like(w[:, :1]), w], 1)
    W = w.sum(1)
    c = (w[:, :, None] * d).sum(1) / W[:, None]
    e = d - c[:, None, :]
    vec = torch.linalg.eigh(torch.einsum("nk,nka,nkb->nab", w, e, e))[1]
    n, e1, e2 = vec[:, :, 0], vec[:, :, 1], vec[:, :, 2]
    x0 = (n * c).sum(1, keepdim=True) * n
    if degree == 2:
        r = d - x0[:, None, :]
        a, b, h = (r * e1[:, None, :]).sum(2) / radius, (r * e2[:, None, :]).sum(2) / radius, (r * n[:, None, :]).sum(2)
        sw = w.sqrt()
        phi = torch.stack([torch.ones_like(a), a, b, a * a, a * b, b * b], 2) * sw[:, :, None]
        coef = torch.linalg.lstsq(phi, (sw * h)[:, :, None]).solution[:, 0, 0]
        x0 = x0 + coef[:, None] * n
    return (q + x0).float()


def plain(PC, pts, grid, k, radius, degree, chunk, queries):
    """(milliseconds for the whole cloud, note): the plain route once, lists included; only the first ``queries`` queries go through
    the solvers, and the figure is scaled to the cloud when that is not all of them."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, idx = PC.knn_distance(None, grid, k, radius, same_cloud=True, return_index=True)
    torch.cuda.synchronize()
    t_lists = time.perf_counter() - t0
    n = int(pts.shape[0])
    queries = min(queries, n)
    t1 = time.perf_counter()
    for lo in range(0, queries, chunk):
        hi = min(lo + chunk, queries)
        plain_chunk((pts[lo:hi], pts), idx[lo:hi], radius, degree)
    torch.cuda.synchronize()
    solve = time.perf_counter() - t1
    note = f"lists {t_lists * 1e3:.1f}"
    if queries < n:
        note += f"; solvers EXTRAPOLATED from the first {queries} queries, {solve * 1e3:.1f} ms"
    return (t_lists + solve * n / queries) * 1e3, note


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "cloud_mls_measure.log"))
    ap.add_argument("--chunk", type=int, default=500_000)
    ap.add_argument("--lstsq_queries", type=int, default=1_000, help="queries of the plain route at degree 2")
    ap.add_argument("--skip_plain", action="store_true")
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
    radius = PC.CLEAN_MAX_DIST_CELLS * cell
    say(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {n} points over {side:.0f} x {side:.0f} units, 2 % outliers; "
        f"same-cloud, cell {cell:.4f}, radius = max_dist {radius:.2f}; median [min, max] of {args.reps} runs after one warm-up, milliseconds")
    say("\n# k | knn_distance (mean only) | knn_normals | knn_mls degree 1 | knn_mls degree 2 | knn_mls degree 2 with every output; the "
        "ratios are to knn_normals; then the points per status at degree 2 and the plain route (lists, gather, eigh, lstsq in torch), "
        "one run after a warm-up")
    for k in (16, 32):
        t_d = timed(lambda: PC.knn_distance(None, grid, k, radius, same_cloud=True), args.reps)
        t_n = timed(lambda: PC.knn_normals(None, grid, k, radius, same_cloud=True), args.reps)
        t_1 = timed(lambda: PC.knn_mls(None, grid, k, radius, same_cloud=True, degree=1), args.reps)
        t_2 = timed(lambda: PC.knn_mls(None, grid, k, radius, same_cloud=True, degree=2), args.reps)
        t_a = timed(lambda: PC.knn_mls(None, grid, k, radius, same_cloud=True, degree=2, return_normal=True, return_displacement=True,
                                       return_status=True, return_count=True), args.reps)
        say(f"k={k:2d}  distance {t_d[0]:8.2f} [{t_d[1]:.2f}, {t_d[2]:.2f}]  normals {t_n[0]:8.2f} [{t_n[1]:.2f}, {t_n[2]:.2f}]  "
            f"mls-1 {t_1[0]:8.2f} [{t_1[1]:.2f}, {t_1[2]:.2f}] x{t_1[0] / t_n[0]:.2f}  mls-2 {t_2[0]:8.2f} [{t_2[1]:.2f}, {t_2[2]:.2f}] "
            f"x{t_2[0] / t_n[0]:.2f}  +outputs {t_a[0]:8.2f} [{t_a[1]:.2f}, {t_a[2]:.2f}]")
        status = PC.knn_mls(None, grid, k, radius, same_cloud=True, degree=2, return_status=True)[1]
        say(f"k={k:2d}  status at degree 2 [not fitted, plane, quadric] {torch.bincount(status.long(), minlength=3).cpu().tolist()}")
        if not args.skip_plain:
            for degree in (1, 2):
                try:
                    queries = n if degree == 1 else args.lstsq_queries
                    say(f"k={k:2d}  plain route degree {degree}: warm-up and one run over {min(queries, n)} queries ...")
                    plain(PC, pts, grid, k, radius, degree, args.chunk, min(queries, args.chunk))  # warm-up
                    ms, note = plain(PC, pts, grid, k, radius, degree, args.chunk, queries)
                    fused = (t_1 if degree == 1 else t_2)[0]
                    say(f"k={k:2d}  plain route degree {degree} {ms:10.2f}  x{ms / fused:.2f} of knn_mls  ({note})")
                except (torch.cuda.OutOfMemoryError, torch.linalg.LinAlgError, NotImplementedError) as e:
                    torch.cuda.empty_cache()
                    say(f"k={k:2d}  plain route degree {degree}: {type(e).__name__}: {' '.join(str(e).split())[:200]}")
    t = timed(lambda: PC.smooth_mls(pts), args.reps)
    say(f"\nsmooth_mls, defaults (spacing, cell search, grid, k=32 degree 2, statistics) {t[0]:9.2f} [{t[1]:.2f}, {t[2]:.2f}]")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
