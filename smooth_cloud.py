"""Moving-least-squares smoothing of a fused point cloud, on a ROCm GPU (the reference has no counterpart).

    python smooth_cloud.py --input OUT/scan1/fused.ply --output OUT/scan1/fused_smooth.ply
           [--radius R | --radius_spacings S] [--k 32] [--degree 1|2] [--iterations N] [--normals keep|refit|drop]
           [--cell C] [--device cuda:0] [--report FILE.json]
    python smooth_cloud.py --input OUT --scan_list list.txt [--ply_name fused.ply] ...
                                                              (every OUT/<scan>/<ply_name> -> OUT/<scan>/fused_smooth.ply)

Every point is moved onto a surface fitted to the point and its k nearest neighbours within the radius, weighted by
(1 - d^2 / R^2)^4: a plane (--degree 1) or a quadric over that plane (--degree 2, the default; PCL's MovingLeastSquares with
polynomial_order 2 and no upsampling).  That takes out the noise along the viewing rays, the largest error left in an MVS cloud,
before cloud_normals.py and mesh_cloud.py read it as signal.  One HIP kernel (pmn_knn_mls) over the grid of
patchmatchnet_amd/pointcloud.py finds the neighbours, fits and projects in float64.  The radius is --radius in scene units or
--radius_spacings times the cloud's own spacing (pointcloud.cloud_spacing; default 3); --iterations repeats the filter on its own
result with the same radius; --cell changes the time only.
The number of points, their order and their colours never change (white where the input had none): a point with fewer than two
neighbours in range, or whose neighbourhood lies on a line, is written where it was and counted.  --normals keep (the default) writes
the file's normals as they are, `refit` the normals of the fitted surfaces turned to the side of the file's own -- the file must have
normals: cloud_normals.py writes and orients them -- and `drop` writes none.  The cloud is read with ply.read_ply_model and written
with ply.write_ply; other properties are not carried over.  One process on one ROCm GPU; torchrun is not supported."""
import argparse
import sys
import time

import cloud_tool

TOOL = "smooth_cloud.py"
NORMALS = ("keep", "refit", "drop")
RADIUS_SPACINGS = 3.0  # pointcloud.MLS_RADIUS_SPACINGS, restated so that the parser needs no import of the package


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Moving-least-squares smoothing of a fused point cloud on a ROCm GPU. Single process on "
                                            "one GPU; torchrun is not supported.")
    p.add_argument("--input", type=str, required=True, help="a PLY cloud, or with --scan_list the folder that holds <scan>/<ply_name>")
    p.add_argument("--output", type=str, default="", help="the smoothed PLY (with --scan_list: the folder for <scan>/fused_smooth.ply, "
                                                          "default --input)")
    p.add_argument("--scan_list", type=str, default="", help="text file with one scan per line")
    p.add_argument("--ply_name", type=str, default="fused.ply", help="with --scan_list: the file read in every scan's folder")
    p.add_argument("--radius", type=float, default=None, help="support of the fit, in scene units")
    p.add_argument("--radius_spacings", type=float, default=None,
                   help=f"support of the fit in units of the cloud's spacing (default {RADIUS_SPACINGS:g}; a setting, not a measured optimum)")
    p.add_argument("--k", type=int, default=32, help="neighbours per point (1..32); the point itself is added to them")
    p.add_argument("--degree", type=int, default=2, help="1: project onto the fitted plane, 2: onto the quadric over it")
    p.add_argument("--iterations", type=int, default=1, help="passes of the filter, each over the result of the one before")
    p.add_argument("--normals", type=str, default="keep", choices=NORMALS,
                   help="keep the file's normals, refit them from the fitted surfaces (the file's own decide the side), or drop them")
    p.add_argument("--cell", type=float, default=None, help="cell of the search grid (default: about 8 points per occupied cell)")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--report", type=str, default="", help="write the counts and settings as JSON")
    return p


def smooth_file(src: str, dst: str, args, device):
    """Smooths one file; returns (its report entry, the device in use)."""
    import numpy as np
    from patchmatchnet_amd import pointcloud as PC
    from patchmatchnet_amd._lib import PmnError

    model = cloud_tool.load_cloud(src, mesh_hint="mesh.py --smooth filters a mesh's vertices")
    n = len(model["vertices"])
    if args.normals == "refit" and model["normals"] is None:
        raise PmnError(f"{src}: --normals refit needs normals (nx ny nz) in the input file to decide the side; cloud_normals.py "
                       f"writes and orients them")
    device = cloud_tool.device_of(args, device)
    t0 = time.perf_counter()
    pts = cloud_tool.upload(model["vertices"], np.float32, device)
    moved, normal, rep = PC.smooth_mls(pts, radius=args.radius, k=args.k, degree=args.degree, iterations=args.iterations, cell=args.cell,
                                       return_normals=True,
                                       radius_spacings=RADIUS_SPACINGS if args.radius_spacings is None else args.radius_spacings)
    moved = moved.cpu().numpy()
    seconds = time.perf_counter() - t0  # the upload, the spacing, the grids, the kernels, the statistics and the copy back
    normals = None
    if args.normals == "refit":
        normals = normal.cpu().numpy()
        against = (normals.astype(np.float64) * model["normals"].astype(np.float64)).sum(1) < 0.0
        normals = np.where(against[:, None], -normals, normals)
    keep = np.ones(n, bool)
    cloud_tool.write_kept(dst, dict(model, normals=None) if args.normals == "drop" else model, keep, normals=normals, vertices=moved)
    out = {"input": src, "output": dst, "points": n, **rep, "normals": args.normals, "seconds_device": seconds}
    s0, s1, s2 = rep["status"]

    def spacings(v):
        return "n/a" if v is None else f"{v:.4g}"
    print(f"{src}: {n} points read, {s0} not fitted, {s1} on a plane, {s2} on a quadric (radius {rep['radius']:.6g}, k {args.k}); moved "
          f"{spacings(rep['mean_displacement_spacings'])} spacings on average, {spacings(rep['max_displacement_spacings'])} at most "
          f"-> {dst}")
    return out, device


def check_args(args) -> None:
    """ValueError for what can be refused before any file is read."""
    if not 1 <= args.k <= 32:
        raise ValueError(f"--k must be in 1..32, got {args.k}")
    if args.degree not in (1, 2):
        raise ValueError(f"--degree must be 1 or 2, got {args.degree}")
    if args.iterations < 1:
        raise ValueError(f"--iterations must be at least 1, got {args.iterations}")
    if args.radius is not None and args.radius_spacings is not None:
        raise ValueError("give --radius or --radius_spacings, not both")
    for name in ("radius", "radius_spacings", "cell"):
        v = getattr(args, name)
        if v is not None and not (v > 0.0 and v < float("inf")):
            raise ValueError(f"--{name} must be positive and finite, got {v}")


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if cloud_tool.refuse_torchrun(TOOL):
        return 2
    try:
        check_args(args)
        jobs = cloud_tool.jobs(args, args.ply_name, "fused_smooth.ply")
    except ValueError as e:
        return cloud_tool.fail(TOOL, e)
    settings = {k: getattr(args, k) for k in ("radius", "radius_spacings", "k", "degree", "iterations", "normals", "cell")}
    return cloud_tool.run(TOOL, jobs, lambda src, dst, scan, device: smooth_file(src, dst, args, device), settings, args.report)


if __name__ == "__main__":
    sys.exit(main())
