#!/usr/bin/env python
"""Times the point-to-mesh distance on the 512^3 sphere mesh of scripts/meshops_bench.py: --queries points (5 M)
scattered about the analytic sphere with a standard deviation of --noise voxels -- a ground-truth cloud near the surface -- against
the marching-tetrahedra mesh of that sphere.

    python scripts/mesh_distance_bench.py [--grid 512] [--queries 5000000] [--tau 1.0] [--repeats 3] [--log FILE]

Device-event time (median, min, max over --repeats after one warm-up) of build_face_grid and of point_mesh_distance (cap 5 tau) at
the defaults, then over a sweep of cell (in median longest edges) and cover (in cells) from which meshops.FACE_CELL_EDGES and
FACE_COVER_CELLS are fixed; every setting must give the default's bits.  Beside it the route the search replaces on the ground-truth ->
reconstruction leg: sample_surface at spacing tau / 2 (the voxel eval_tnt.py thins both clouds to), build_grid over the samples at
cell tau, nn_distance with the same cap -- code this feature does not touch.  No time is a gate."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from meshops_bench import field  # noqa: E402
from tsdf_bench import timed  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--grid", type=int, default=512)
    p.add_argument("--queries", type=int, default=5000000)
    p.add_argument("--noise", type=float, default=0.5, help="standard deviation of the queries about the sphere, in voxels")
    p.add_argument("--tau", type=float, default=1.0, help="the scorer's threshold in voxels: cap 5 tau, sampling route at tau / 2")
    p.add_argument("--cells", default="0.5,1,2,4", help="cells of the sweep, in median longest edges")
    p.add_argument("--covers", default="1,2,4", help="covers of the sweep, in cells")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--log", default="")
    args = p.parse_args(argv)
    from patchmatchnet_amd import meshops, ops, pointcloud as PC
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device %s" % torch.cuda.get_device_name(dev))
    n = args.grid
    t, _ = field(n, 0, dev)
    v, f, _, _ = ops.mt_extract(t, torch.ones_like(t), (0.0, 0.0, 0.0), 1.0, normals=False)
    del t
    torch.cuda.empty_cache()
    s = n / 256.0
    g = torch.Generator(device=dev).manual_seed(1)
    u = torch.randn((args.queries, 3), device=dev, generator=g)
    u = u / u.norm(dim=1, keepdim=True)
    r = 101.4 * s + args.noise * torch.randn((args.queries, 1), device=dev, generator=g)
    q = (u * r + torch.tensor([127.3 * s, 128.1 * s, 126.7 * s], device=dev)).float().contiguous()
    cap = 5.0 * args.tau
    e = torch.stack([(v[f[:, a].long()] - v[f[:, b].long()]).norm(dim=1) for a, b in ((0, 1), (1, 2), (2, 0))]).max(0).values
    edge = float(e.median())
    say("grid %d^3: %d vertices, %d faces, median longest edge %.4f voxel; %d queries, sigma %.3g voxel, cap %.3g" % (
        n, v.shape[0], f.shape[0], edge, args.queries, args.noise, cap))

    def run(cell, cover, label):
        med_b, lo_b, hi_b, fg = timed(lambda: meshops.build_face_grid(v, f, cell=cell, cover=cover), args.repeats)
        med_s, lo_s, hi_s, d = timed(lambda: meshops.point_mesh_distance(q, fg, cap), args.repeats)
        say("  %s: cell %.4f, cover %.4f, R %.4f, %d entries: build median %.3f ms (min %.3f, max %.3f); search median %.3f ms "
            "(min %.3f, max %.3f) = %.2f ns per query; build + search %.3f ms" % (
                label, fg.grid.cell, fg.cover, fg.radius, fg.grid.xyz.shape[0], med_b, lo_b, hi_b, med_s, lo_s, hi_s,
                1e6 * med_s / args.queries, med_b + med_s))
        return d

    base = run(None, None, "defaults (cell %.3g edge, cover %.3g cell)" % (meshops.FACE_CELL_EDGES, meshops.FACE_COVER_CELLS))
    say("  distances: mean %.6f, median %.6f, at the cap %d" % (float(base.mean()), float(base.median()), int((base >= cap).sum())))
    for ce in (float(x) for x in args.cells.split(",")):
        for co in (float(x) for x in args.covers.split(",")):
            d = run(ce * edge, co * ce * edge, "sweep cell %.3g edge, cover %.3g cell" % (ce, co))
            say("    same bits as the defaults: %s" % bool(torch.equal(d, base)))
            del d
    # the route it replaces: the surface as samples
    spacing = args.tau / 2.0
    med_a, lo_a, hi_a, pts = timed(lambda: meshops.sample_surface(v, f, spacing=spacing, seed=1)[0], args.repeats)
    med_g, lo_g, hi_g, grid = timed(lambda: PC.build_grid(pts, args.tau), args.repeats)
    med_n, lo_n, hi_n, dn = timed(lambda: PC.nn_distance(q, grid, cap), args.repeats)
    say("  sampling route, spacing %.3g voxel: sample_surface median %.3f ms (%d samples), build_grid(cell %.3g) %.3f ms, nn_distance "
        "%.3f ms (min %.3f, max %.3f) = %.2f ns per query; all three %.3f ms" % (
            spacing, med_a, pts.shape[0], args.tau, med_g, med_n, lo_n, hi_n, 1e6 * med_n / args.queries, med_a + med_g + med_n))
    say("  sampling route distances: mean %.6f, median %.6f; mean excess over the exact distance %.6f" % (
        float(dn.mean()), float(dn.median()), float((dn - base).mean())))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
