#!/usr/bin/env python
"""Times meshops.smooth_taubin on the sphere meshes of scripts/simplify_bench.py and measures what it does.

    python scripts/smooth_bench.py [--grids 256,512] [--repeats 3] [--log FILE]

Per grid: the vertices, faces and adjacency entries; the time of one umbrella step and of the whole 10-iteration filter (20 steps in
one library call), each the median over --repeats runs after one warm-up, between device synchronisations; the bytes a step must move
(every vertex's position read and written once, the row indices, starts) and the share of the 8 TB/s peak the step reaches on them;
the same step written with torch.index_add_ in this script (the yardstick: the product is never its own) and the ratio; vertex
adjacency and vertex normals, timed the same way; and the RMS distance of the vertices from the analytic sphere before and after the
filter.  No time is a gate."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from meshops_bench import field  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E


def timed(fn, repeats, dev):
    out = None
    times = []
    for k in range(repeats + 1):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        if k:
            times.append(time.perf_counter() - t)
    return float(np.median(times)), out


def torch_step(v, rows, cols, degree, factor):
    """The umbrella step with torch.index_add_: float64 sums of (p_j - p_i) in whatever order the atomics land."""
    p = v.double()
    s = torch.zeros_like(p).index_add_(0, rows, p[cols] - p[rows])
    moved = p + factor * (s / degree.clamp(min=1)[:, None])
    return torch.where((degree > 0)[:, None], moved, p).float()


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--grids", default="256,512")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--log", default="")
    args = p.parse_args(argv)
    from patchmatchnet_amd import meshops, ops
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device %s" % torch.cuda.get_device_name(dev))
    for n in (int(g) for g in args.grids.split(",")):
        s = n / 256.0
        t, _ = field(n, 0, dev)
        v, f, _, _ = ops.mt_extract(t, torch.ones_like(t), (0.0, 0.0, 0.0), 1.0, normals=True)
        del t
        torch.cuda.empty_cache()
        centre = torch.tensor([127.3 * s, 128.1 * s, 126.7 * s], dtype=torch.float64, device=dev)
        rms = lambda x: float(((x.double() - centre).norm(dim=1) - 101.4 * s).pow(2).mean().sqrt())
        t_adj, adj = timed(lambda: meshops.vertex_adjacency(f, v.shape[0]), args.repeats, dev)
        nv, ne = v.shape[0], adj.neighbours.shape[0]
        say("grid %d^3: sphere -> %d vertices, %d faces, %d adjacency entries (%.2f a row), %d boundary vertices; vertex_adjacency "
            "%.2f ms" % (n, nv, f.shape[0], ne, ne / nv, int(adj.boundary.sum()), 1e3 * t_adj))
        t_step, one = timed(lambda: meshops.smooth_steps(v, f, [0.5], adjacency=adj), args.repeats, dev)
        t_all, out = timed(lambda: meshops.smooth_taubin(v, f, iterations=10, adjacency=adj), args.repeats, dev)
        must = 24 * nv + 4 * ne + 8 * (nv + 1)
        rows = torch.repeat_interleave(torch.arange(nv, device=dev), adj.starts[1:] - adj.starts[:-1])
        cols = adj.neighbours.long()
        degree = (adj.starts[1:] - adj.starts[:-1]).double()
        t_torch, ref = timed(lambda: torch_step(v, rows, cols, degree, 0.5), args.repeats, dev)
        gap = float((ref.double() - one.double()).abs().max())
        say("  one step (a call with one factor: the launch, the finiteness check and two allocations) %.3f ms; 10 Taubin iterations "
            "(20 steps, one call) %.3f ms = %.3f ms a step" % (1e3 * t_step, 1e3 * t_all, 1e3 * t_all / 20))
        say("  a step must move %.1f MB: %.1f %% of %.0f TB/s at %.3f ms a step" % (
            must / 1e6, 100.0 * must / (t_all / 20) / PEAK_BYTES_PER_S, PEAK_BYTES_PER_S / 1e12, 1e3 * t_all / 20))
        say("  the same step with torch.index_add_ (float64, atomics) %.3f ms: %.2f x the kernel's step; largest difference of the two "
            "results %.3e" % (1e3 * t_torch, t_torch / (t_all / 20), gap))
        t_nrm, _ = timed(lambda: meshops.vertex_normals(out, f), args.repeats, dev)
        say("  vertex_normals (two sorts and the kernel) %.2f ms" % (1e3 * t_nrm))
        moved = (out.double() - v.double()).norm(dim=1)
        say("  RMS distance from the analytic sphere: %.5f voxels before, %.5f after; displacement mean %.5f, max %.5f voxels" % (
            rms(v), rms(out), float(moved.mean()), float(moved.max())))
        del v, f, adj, one, out, rows, cols, degree, ref, moved
        torch.cuda.empty_cache()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
