"""Outlier removal on a fused point cloud, on a ROCm GPU (the reference has no counterpart).

    python clean_cloud.py --input OUT/scan1/fused.ply --output OUT/scan1/fused_clean.ply
           --method statistical [--k 20 --std_ratio 2.0] | --method radius --radius R --min_neighbors N
           [--cell C] [--max_dist D] [--device cuda:0] [--report FILE.json]
    python clean_cloud.py --input OUT --scan_list list.txt ...     (every OUT/<scan>/fused.ply -> OUT/<scan>/fused_clean.ply)

statistical: a point stays when the mean distance to its k nearest neighbours is at most mu + std_ratio * sigma of that mean over the
cloud (PCL's StatisticalOutlierRemoval; Open3D's remove_statistical_outlier keeps "<").  radius: a point stays when at least
min_neighbors other points lie within R of it.  Both searches are HIP kernels (pmn_knn_distance, pmn_radius_count) over the grid of
patchmatchnet_amd/pointcloud.py; --cell changes the time only, --max_dist caps the k-nearest search (pointcloud.statistical_outliers).
The cloud is read with ply.read_ply_model (either kind of fused.ply, or any cloud with further scalar properties) and the kept
points are written in their original order with ply.write_ply: x y z [nx ny nz] red green blue, normals when the input had them,
white where it had no colours; other properties are not carried over.  `eval_dtu.py --ply_name fused_clean.ply` and `eval_tnt.py
--ply_path .../fused_clean.ply` read the result.  One process on one ROCm GPU; torchrun is not supported."""
import argparse
import sys
import time

import cloud_tool

TOOL = "clean_cloud.py"


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Statistical or radius outlier removal on a fused point cloud on a ROCm GPU. Single "
                                            "process on one GPU; torchrun is not supported.")
    p.add_argument("--input", type=str, required=True, help="a PLY cloud, or with --scan_list the folder that holds <scan>/fused.ply")
    p.add_argument("--output", type=str, default="", help="the cleaned PLY (with --scan_list: the folder for <scan>/fused_clean.ply, "
                                                          "default --input)")
    p.add_argument("--scan_list", type=str, default="", help="text file with one scan per line")
    p.add_argument("--method", type=str, default="statistical", choices=["statistical", "radius"])
    p.add_argument("--k", type=int, default=20, help="statistical: neighbours per point (1..32)")
    p.add_argument("--std_ratio", type=float, default=2.0, help="statistical: threshold = mean + std_ratio * standard deviation")
    p.add_argument("--radius", type=float, default=None, help="radius: the neighbourhood, in scene units")
    p.add_argument("--min_neighbors", type=int, default=None, help="radius: other points within --radius a point needs to stay")
    p.add_argument("--cell", type=float, default=None, help="cell of the search grid (default: about 8 points per occupied cell)")
    p.add_argument("--max_dist", type=float, default=None, help="statistical: cap of the neighbour search (default: 16 cells)")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--report", type=str, default="", help="write the counts and settings as JSON")
    return p


def clean_file(src: str, dst: str, args, device):
    """Cleans one file; returns (its report entry, the device in use)."""
    import numpy as np
    from patchmatchnet_amd import pointcloud as PC

    model = cloud_tool.load_cloud(src, mesh_hint="drop a mesh's floaters with mesh.py --keep_components / --min_component_faces")
    n = len(model["vertices"])
    device = cloud_tool.device_of(args, device)
    t0 = time.perf_counter()
    pts = cloud_tool.upload(model["vertices"], np.float32, device)
    out = {"input": src, "output": dst, "points": n}
    if args.method == "statistical":
        keep, _, threshold = PC.statistical_outliers(pts, k=args.k, std_ratio=args.std_ratio, max_dist=args.max_dist, cell=args.cell)
        out["threshold"] = threshold
        what = f"mean distance to {args.k} neighbours <= {threshold:.6g}"
    else:
        keep, _ = PC.radius_outliers(pts, args.radius, args.min_neighbors, cell=args.cell)
        what = f">= {args.min_neighbors} neighbours within {args.radius:g}"
    keep = keep.cpu().numpy()
    out["seconds_search"] = time.perf_counter() - t0
    cloud_tool.write_kept(dst, model, keep)
    out.update(kept=int(keep.sum()), removed=int(n - keep.sum()))
    print(f"{src}: {n} points read, {out['kept']} kept, {out['removed']} removed ({what}) -> {dst}")
    return out, device


def check_args(args) -> None:
    """ValueError for what can be refused before any file is read."""
    if args.method == "radius":
        if args.radius is None or args.min_neighbors is None:
            raise ValueError("--method radius needs --radius and --min_neighbors")
        if not (args.radius >= 0.0 and args.radius < float("inf")) or args.min_neighbors < 0:
            raise ValueError(f"--radius must be finite and >= 0 and --min_neighbors >= 0, got {args.radius} and {args.min_neighbors}")
    elif not 1 <= args.k <= 32:
        raise ValueError(f"--k must be in 1..32, got {args.k}")


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if cloud_tool.refuse_torchrun(TOOL):
        return 2
    try:
        check_args(args)
        jobs = cloud_tool.jobs(args, "fused.ply", "fused_clean.ply")
    except ValueError as e:
        return cloud_tool.fail(TOOL, e)
    settings = {k: getattr(args, k) for k in ("method", "k", "std_ratio", "radius", "min_neighbors", "cell", "max_dist")}
    return cloud_tool.run(TOOL, jobs, lambda src, dst, scan, device: clean_file(src, dst, args, device), settings, args.report)


if __name__ == "__main__":
    sys.exit(main())
