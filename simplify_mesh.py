#!/usr/bin/env python
"""Simplify or clean an existing triangle mesh on a ROCm GPU, without its depth maps.

    python simplify_mesh.py --input mesh.ply --output small.ply --cell C | --target_faces N
           [--placement quadric|mean] [--stiffness S] [--min_component_faces N --keep_components K] [--report FILE.json] [--device cuda:0]

The mesh is read with ply.read_ply_mesh (what mesh.py writes) and written with ply.write_ply_mesh.  First the connected components with
fewer than --min_component_faces faces, or outside the --keep_components largest, are dropped (meshops.remove_components); given only
these flags the tool cleans a mesh and changes nothing else.  Then the vertices are clustered into cubic cells of side --cell, in
scene units, and every cluster becomes one vertex (meshops.simplify_clustering): placed by the clusters' plane quadrics (the default;
keeps edges and corners) or at their mean, never further than sqrt(3) * cell from any vertex it replaces.  --target_faces N looks for
the cell by bisection between 2^-10 of the bounding box's diagonal and the diagonal itself, at most 12 calls, and keeps the result with
the most faces that does not exceed N (else the one with the fewest): it reports the cell it chose and the faces it reached and
promises no more.  The output is a function of the input file and the flags alone.  One process on one ROCm GPU; torchrun is not
supported."""
import argparse
import math
import os
import sys
import time

import cloud_tool

TOOL = "simplify_mesh.py"

TARGET_CALLS = 12


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Quadric vertex clustering and component removal on a PLY mesh on a ROCm GPU. Single "
                                            "process on one GPU; torchrun is not supported.")
    p.add_argument("--input", type=str, required=True, help="a PLY mesh as mesh.py writes it")
    p.add_argument("--output", type=str, required=True, help="the simplified PLY mesh")
    p.add_argument("--cell", type=float, default=None, help="side of the clustering cells, in scene units")
    p.add_argument("--target_faces", type=int, default=None, help="bisect on the cell towards this many faces (at most 12 calls)")
    p.add_argument("--placement", type=str, default="quadric", choices=("quadric", "mean"))
    p.add_argument("--stiffness", type=float, default=1e-3, help="weight of the pull towards the cluster's mean, relative to the planes'")
    p.add_argument("--min_component_faces", type=int, default=0, help="drop connected components with fewer faces than this (0 = off)")
    p.add_argument("--keep_components", type=int, default=0, help="keep only this many components, the largest by face count (0 = off)")
    p.add_argument("--report", type=str, default="", help="write the counts and settings as JSON")
    p.add_argument("--device", type=str, default="cuda:0")
    return p


def choose_cell(simplify, n_faces_in: int, target: int, diagonal: float):
    """(cell, result, calls) of the bisection: ``simplify(cell)`` returns the tuple of simplify_clustering.  The face count falls as
    the cell grows (not strictly: it is a lattice effect), so the search halves [lo, hi] in the logarithm of the cell."""
    lo, hi = diagonal * 2.0 ** -10, diagonal
    best = None  # (over the target?, distance to it, cell, result)
    calls = []
    for _ in range(TARGET_CALLS):
        cell = math.sqrt(lo * hi)
        out = simplify(cell)
        n = int(out[1].shape[0])
        calls.append({"cell": cell, "faces": n})
        rank = (n > target, n - target if n > target else target - n)
        if best is None or rank < best[0]:
            best = (rank, cell, out)
        if n == target:
            break
        if n > target:
            lo = cell
        else:
            hi = cell
    return best[1], best[2], calls


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if cloud_tool.refuse_torchrun(TOOL):
        return 2
    if args.cell is not None and args.target_faces is not None:
        return cloud_tool.fail(TOOL, "give --cell or --target_faces, not both")
    if args.cell is not None and not (args.cell > 0.0 and math.isfinite(args.cell)):
        return cloud_tool.fail(TOOL, f"--cell must be positive and finite, got {args.cell}")
    if args.target_faces is not None and args.target_faces < 1:
        return cloud_tool.fail(TOOL, f"--target_faces must be at least 1, got {args.target_faces}")
    if not (args.stiffness > 0.0 and math.isfinite(args.stiffness)):
        return cloud_tool.fail(TOOL, f"--stiffness must be positive and finite, got {args.stiffness}")
    if args.min_component_faces < 0 or args.keep_components < 0:
        return cloud_tool.fail(TOOL, "--min_component_faces and --keep_components must be >= 0")
    cleaning = args.min_component_faces > 0 or args.keep_components > 0
    if args.cell is None and args.target_faces is None and not cleaning:
        return cloud_tool.fail(TOOL, "nothing to do: give --cell, --target_faces, --min_component_faces or --keep_components")
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
            raise _lib.PmnError(f"--device {args.device}: simplify_mesh.py runs on a ROCm GPU (no CPU fallback)")
        up = lambda a: None if a is None else torch.from_numpy(a).to(device).contiguous()
        t0 = time.perf_counter()
        mesh = (up(v), up(f), up(c), up(n))
        report = {"abi": _lib.ABI_VERSION, "input": args.input, "output": args.output, "vertices_in": int(len(v)),
                  "faces_in": int(len(f)), "placement": args.placement, "stiffness": args.stiffness}
        if cleaning:
            *mesh, (found, kept) = meshops.remove_components(*mesh, min_faces=args.min_component_faces,
                                                             keep_largest=args.keep_components, return_counts=True)
            report.update(components=found, components_kept=kept, vertices_cleaned=int(mesh[0].shape[0]),
                          faces_cleaned=int(mesh[1].shape[0]))
            print(f"{args.input}: {found} components, {kept} kept; {len(v) - mesh[0].shape[0]} vertices and "
                  f"{len(f) - mesh[1].shape[0]} faces dropped")
        if (args.cell is not None or args.target_faces is not None) and mesh[0].shape[0]:
            mv, mf, mc, mn = mesh
            simplify = lambda cell: meshops.simplify_clustering(mv, mf, cell, colors=mc, normals=mn, placement=args.placement,
                                                                stiffness=args.stiffness)
            if args.cell is not None:
                cell, mesh = args.cell, simplify(args.cell)
            else:
                extent = mesh[0].max(0).values.double() - mesh[0].min(0).values.double()
                diagonal = float(extent.norm())
                if not diagonal > 0.0:
                    raise _lib.PmnError(f"{args.input}: the mesh has no extent; --target_faces cannot choose a cell")
                cell, mesh, calls = choose_cell(simplify, int(mesh[1].shape[0]), args.target_faces, diagonal)
                report.update(target_faces=args.target_faces, calls=calls)
                print(f"{args.input}: --target_faces {args.target_faces}: cell {cell:.9g} after {len(calls)} calls reaches "
                      f"{mesh[1].shape[0]} faces")
            report["cell"] = cell
        torch.cuda.synchronize(device)
        report["seconds"] = time.perf_counter() - t0
        ply.write_ply_mesh(args.output, *mesh)
        report.update(vertices_out=int(mesh[0].shape[0]), faces_out=int(mesh[1].shape[0]))
        print(f"{args.input}: {len(v)} vertices, {len(f)} faces -> {mesh[0].shape[0]} vertices, {mesh[1].shape[0]} faces"
              + (f" at cell {report['cell']:.9g} ({args.placement})" if "cell" in report else "") + f" -> {args.output}")
    except _lib.PmnError as e:
        return cloud_tool.fail(TOOL, e)
    if args.report:
        cloud_tool.write_report(args.report, report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
