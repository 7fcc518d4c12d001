#!/usr/bin/env python
"""Smooth an existing triangle mesh on a ROCm GPU, or give it normals, without its depth maps.

    python smooth_mesh.py --input mesh.ply --output smooth.ply [--method taubin|laplacian] [--iterations N] [--lambda L] [--mu M]
           [--boundary fixed|free] [--normals recompute|keep|drop] [--report FILE.json] [--device cuda:0]

The mesh is read with ply.read_ply_mesh (what mesh.py writes) and written with ply.write_ply_mesh.  --method taubin (the default) runs
N times an umbrella step with --lambda and one with --mu (meshops.smooth_taubin: removes ripple, keeps the volume); --method laplacian
N steps with --lambda (meshops.smooth_laplacian: smooths and shrinks).  Faces, colours and the number of vertices do not change.
--boundary fixed (the default) leaves the vertices on an open edge where they are.  --normals recompute (the default) writes the
area-weighted normals of the new geometry by the right-hand rule of the faces' winding (meshops.vertex_normals), keep writes the input's
normals unchanged, drop writes none.  --iterations 0 --normals recompute only gives a file normals.  The output is a function of the
input file and the flags alone.  One process on one ROCm GPU; torchrun is not supported."""
import argparse
import math
import os
import sys
import time

import cloud_tool

TOOL = "smooth_mesh.py"


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Taubin / Laplacian smoothing and vertex normals of a PLY mesh on a ROCm GPU. Single process "
                                            "on one GPU; torchrun is not supported.")
    p.add_argument("--input", type=str, required=True, help="a PLY mesh as mesh.py writes it")
    p.add_argument("--output", type=str, required=True, help="the smoothed PLY mesh")
    p.add_argument("--method", type=str, default="taubin", choices=("taubin", "laplacian"))
    p.add_argument("--iterations", type=int, default=10, help="taubin: pairs of steps; laplacian: steps (0 = leave the positions)")
    p.add_argument("--lambda", dest="lam", type=float, default=0.5, help="the shrinking step's factor, in (0, 1]")
    p.add_argument("--mu", type=float, default=-0.53, help="taubin: the inflating step's factor, < -lambda")
    p.add_argument("--boundary", type=str, default="fixed", choices=("fixed", "free"), help="fixed: boundary vertices stay where they are")
    p.add_argument("--normals", type=str, default="recompute", choices=("recompute", "keep", "drop"))
    p.add_argument("--report", type=str, default="", help="write the counts, settings and displacements as JSON")
    p.add_argument("--device", type=str, default="cuda:0")
    return p


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if cloud_tool.refuse_torchrun(TOOL):
        return 2
    if args.iterations < 0:
        return cloud_tool.fail(TOOL, f"--iterations must be >= 0, got {args.iterations}")
    if not (args.lam > 0.0 and args.lam <= 1.0):
        return cloud_tool.fail(TOOL, f"--lambda must be in (0, 1], got {args.lam}")
    if args.method == "taubin" and not (math.isfinite(args.mu) and args.mu < -args.lam):
        return cloud_tool.fail(TOOL, f"--mu must be finite and < -lambda = {-args.lam}, got {args.mu}")
    if not os.path.isfile(args.input):
        return cloud_tool.fail(TOOL, f"no such file: {args.input}")
    import torch
    from patchmatchnet_amd import _lib, meshops, ply
    try:
        try:
            v, f, c, n = ply.read_ply_mesh(args.input)
        except ValueError as e:
            raise _lib.PmnError(str(e)) from e
        device = torch.device(args.device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.PmnError(f"--device {args.device}: smooth_mesh.py runs on a ROCm GPU (no CPU fallback)")
        up = lambda a: None if a is None else torch.from_numpy(a).to(device).contiguous()
        t0 = time.perf_counter()
        dv, df = up(v), up(f)
        adj = meshops.vertex_adjacency(df, len(v))
        if args.method == "taubin":
            out = meshops.smooth_taubin(dv, df, args.iterations, args.lam, args.mu, boundary=args.boundary, adjacency=adj)
        else:
            out = meshops.smooth_laplacian(dv, df, args.iterations, args.lam, boundary=args.boundary, adjacency=adj)
        normals = {"recompute": lambda: meshops.vertex_normals(out, df), "keep": lambda: up(n), "drop": lambda: None}[args.normals]()
        moved = (out.double() - dv.double()).norm(dim=1)
        report = {"abi": _lib.ABI_VERSION, "input": args.input, "output": args.output, "method": args.method,
                  "iterations": args.iterations, "lambda": args.lam, "mu": args.mu if args.method == "taubin" else None,
                  "boundary": args.boundary, "normals": args.normals, "vertices": int(len(v)), "faces": int(len(f)),
                  "boundary_vertices": int(adj.boundary.sum()), "adjacency_entries": int(adj.neighbours.shape[0]),
                  "displacement_mean": float(moved.mean()) if len(v) else 0.0,
                  "displacement_max": float(moved.max()) if len(v) else 0.0}
        torch.cuda.synchronize(device)
        report["seconds"] = time.perf_counter() - t0
        ply.write_ply_mesh(args.output, out, df, up(c), normals)
        print(f"{args.input}: {len(v)} vertices ({report['boundary_vertices']} on the boundary, {args.boundary}), {len(f)} faces; "
              f"{args.method}, {args.iterations} iterations: displacement mean {report['displacement_mean']:.6g}, max "
              f"{report['displacement_max']:.6g}; normals {args.normals} -> {args.output}")
    except _lib.PmnError as e:
        return cloud_tool.fail(TOOL, e)
    if args.report:
        cloud_tool.write_report(args.report, report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
