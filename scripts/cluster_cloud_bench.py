"""Timings behind DESIGN.md section 33 (profiles/cluster_cloud_measure.log): the stages of the order-free DBSCAN beside pmn_radius_count
alone on the same grid and eps -- the walk that the link pass repeats, so the ratio says what the unions cost --, cluster_dbscan as a
whole, and, where scipy imports, cKDTree.query_pairs + csgraph.connected_components on the host at a subsample that finishes.

    python scripts/cluster_cloud_bench.py [--points 5000000] [--reps 5] [--log profiles/cluster_cloud_measure.log]

The cloud is the one the other cloud benches generate: a noisy sheet of --points points with 2 % planted outliers up to 200 units off.
Every GPU figure is the median of --reps timed runs after one warm-up, measured with events on the stream, in one process."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clean_cloud_bench import sheet, timed  # noqa: E402  (the same cloud, the same clock)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host_points", type=int, default=500_000, help="subsample for the scipy leg")
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "cluster_cloud_measure.log"))
    args = ap.parse_args()
    from patchmatchnet_amd import _lib, pointcloud as PC
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
    say(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {n} points over {side:.0f} x {side:.0f} units, 2 % outliers; "
        f"median [min, max] of {args.reps} runs after one warm-up, milliseconds")
    spacing = PC.cloud_spacing(pts)
    cell0 = PC.default_cell(pts)
    say(f"cloud_spacing {spacing:.4f}, default_cell {cell0:.4f}")
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def row(name, t, base=None):
        say(f"{name:44s} {t[0]:9.2f} [{t[1]:.2f}, {t[2]:.2f}]" + (f"  x{t[0] / base:.2f} of radius_count" if base else ""))

    for spacings, mp in ((2.0, 10), (4.0, 10)):
        eps = spacings * spacing
        cell = max(cell0, eps / 8.0)
        g = PC.build_grid(pts, cell)
        a = PC._grid_args(g)
        core = torch.empty(n, dtype=torch.uint8, device="cuda")
        parent = torch.empty(n, dtype=torch.int32, device="cuda")
        label = torch.empty(n, dtype=torch.int32, device="cuda")
        orig = g.perm.int()
        labels, is_core, sizes = PC.cluster_dbscan(pts, eps, mp)
        noise = int((labels < 0).sum())
        pairs = int(PC.radius_count(None, g, eps, same_cloud=True).long().sum()) // 2
        say(f"\n# eps = {spacings:g} spacings = {eps:.4f}, min_points {mp}, cell {cell:.4f}: {int(is_core.sum())} core, "
            f"{n - noise - int(is_core.sum())} border, {noise} noise, {int(sizes.numel())} clusters, largest {sizes[:3].tolist()}; "
            f"{pairs} pairs within eps")
        del labels, is_core, sizes

        def core_stage():
            PC.check(L.pmn_cloud_core(*a, eps, mp, core.data_ptr(), stream), "pmn_cloud_core")

        def link_stage():
            PC.check(L.pmn_cloud_dbscan(*a, eps, core.data_ptr(), None, parent.data_ptr(), None, stream), "pmn_cloud_dbscan")

        def link_border_stage():
            PC.check(L.pmn_cloud_dbscan(*a, eps, core.data_ptr(), orig.data_ptr(), parent.data_ptr(), label.data_ptr(), stream),
                     "pmn_cloud_dbscan")

        base = timed(lambda: PC.radius_count(None, g, eps, same_cloud=True), args.reps)
        row("pmn_radius_count (same cloud, + unsort)", base)
        row("pmn_cloud_core", timed(core_stage, args.reps), base[0])
        t_link = timed(link_stage, args.reps)
        row("pmn_cloud_dbscan, label NULL (init, link, flatten)", t_link, base[0])
        t_all = timed(link_border_stage, args.reps)
        row("pmn_cloud_dbscan (init, link, flatten, border)", t_all, base[0])
        say(f"{'  border launch, by difference of the medians':44s} {t_all[0] - t_link[0]:9.2f}")
        row("build_grid", timed(lambda: PC.build_grid(pts, cell), args.reps))
        row("cluster_dbscan, cell given", timed(lambda: PC.cluster_dbscan(pts, eps, mp, cell=cell), args.reps), base[0])
        row("cluster_dbscan, defaults (+ default_cell)", timed(lambda: PC.cluster_dbscan(pts, eps, mp), args.reps), base[0])

    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
    except ImportError:
        say("\nscipy does not import: no host leg")
    else:
        m = min(args.host_points, n)
        sub = sheet(m, 0, 1000.0 * (m / 5e6) ** 0.5).astype(np.float64)  # the same density, a smaller sheet
        eps, mp = 4.0 * spacing, 10
        t0 = time.perf_counter()
        tree = cKDTree(sub)
        t1 = time.perf_counter()
        pairs = tree.query_pairs(eps, output_type="ndarray")
        t2 = time.perf_counter()
        deg = np.bincount(pairs.ravel(), minlength=m) + 1
        is_core = deg >= mp
        cp = pairs[is_core[pairs[:, 0]] & is_core[pairs[:, 1]]]
        ncomp, _ = connected_components(coo_matrix((np.ones(len(cp), np.int8), (cp[:, 0], cp[:, 1])), shape=(m, m)), directed=False)
        t3 = time.perf_counter()
        say(f"\n# host, one thread, scipy: {m} points of the same density, eps = 4 spacings, min_points 10 (core clusters only, no border "
            f"rule): cKDTree {1e3 * (t1 - t0):.0f} ms, query_pairs {1e3 * (t2 - t1):.0f} ms ({len(pairs)} pairs), core flags + "
            f"connected_components {1e3 * (t3 - t2):.0f} ms ({ncomp - int((~is_core).sum())} clusters); total {1e3 * (t3 - t0):.0f} ms")
        sub_dev = torch.from_numpy(sub.astype(np.float32)).cuda()
        row(f"cluster_dbscan, defaults, the same {m} points", timed(lambda: PC.cluster_dbscan(sub_dev, eps, mp), args.reps))
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
