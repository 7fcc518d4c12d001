"""Dominant planes of a fused point cloud, on a ROCm GPU (Open3D calls it segment_plane, PCL SACSegmentation; the
reference has no counterpart): finds the table a scan stands on, the ground, the walls and the floor of a room, and takes them out of
the cloud or keeps only them.  clean_cloud.py and cluster_cloud.py keep such a plane by construction: it is neither an outlier nor a
small cluster.

    python segment_cloud.py --input OUT/scan1/fused.ply --output OUT/scan1/fused_noplane.ply
           [--threshold T | --threshold_spacings 2] [--hypotheses 1024] [--seed 0] [--refine 3] [--max_planes 1]
           [--min_inliers N | --min_inlier_share F] [--normal_angle DEG] [--keep rest|planes] [--drop_beyond --mvs_folder DATA/scan1]
           [--color_by_plane] [--labels FILE.npy] [--planes FILE.npz] [--device cuda:0] [--report FILE.json]
    python segment_cloud.py --input OUT --scan_list list.txt ...   (every OUT/<scan>/fused.ply -> OUT/<scan>/fused_noplane.ply;
                                                                    --mvs_folder then holds <scan>/cams)

Seeded RANSAC (pointcloud.segment_planes; HIP kernels pmn_plane_score and pmn_plane_inliers): --hypotheses triplets of points are drawn
by numpy's PCG64 from --seed, every plane through a triplet is scored by the number of points within the threshold of it (and, with
--normal_angle, whose normal lies within that angle of the plane's), the best one is refitted by least squares over its inliers at most
--refine times, its inliers leave the cloud and the search goes on for --max_planes planes or until the best plane holds fewer than
--min_inliers points (or --min_inlier_share of the file).  The result is a function of the file, the settings and the seed alone, bit
for bit; the ORDER of the points in the file matters, through the draw.  The threshold defaults to --threshold_spacings times
pointcloud.cloud_spacing.  The defaults (2 spacings, 1024 hypotheses, 3 refits) are SETTINGS chosen by reasoning, not measured optima.
--keep rest (the default) writes the cloud without the planes, --keep planes the planes alone; the kept records are written unchanged and
in their order with ply.write_ply: x y z [nx ny nz] red green blue, white where the input had no colours.  --drop_beyond also drops every
point beyond the FIRST plane on the side that holds the minority of the camera centres of --mvs_folder/cams (a side is the sign of the
residual outside the threshold band): a table and what lies under it.  --color_by_plane writes one colour per plane and grey for the
rest, for render.py; --labels the int32 label of EVERY input point (-1, or the plane's index in order of extraction); --planes an .npz
with field P, [k][4] float64 -- [4] with one plane, which pointcloud.load_plane and so eval_dtu.py read.
One process on one ROCm GPU; torchrun is not supported."""
import argparse
import os
import sys
import time

import cloud_tool

TOOL = "segment_cloud.py"


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Dominant planes of a fused point cloud on a ROCm GPU by seeded RANSAC, the result a function "
                                            "of file, settings and seed. Single process on one GPU; torchrun is not supported.")
    p.add_argument("--input", type=str, required=True, help="a PLY cloud, or with --scan_list the folder that holds <scan>/<ply_name>")
    p.add_argument("--output", type=str, default="", help="the PLY of the kept points (with --scan_list: the folder for "
                                                          "<scan>/fused_noplane.ply, default --input)")
    p.add_argument("--scan_list", type=str, default="", help="text file with one scan per line")
    p.add_argument("--ply_name", type=str, default="fused.ply", help="with --scan_list: the file read in every scan's folder")
    p.add_argument("--threshold", type=float, default=None, help="the largest distance of an inlier from its plane, in scene units "
                                                                 "(default: --threshold_spacings times the cloud's spacing)")
    p.add_argument("--threshold_spacings", type=float, default=None, help="the threshold in units of the cloud's spacing (default 2: a "
                                                                          "setting, not a measured optimum)")
    p.add_argument("--hypotheses", type=int, default=1024, help="triplets drawn per plane (a setting, not a measured optimum)")
    p.add_argument("--seed", type=int, default=0, help="seed of the draw")
    p.add_argument("--refine", type=int, default=3, help="least-squares refits of the best plane at most (a setting, not a measured "
                                                         "optimum)")
    p.add_argument("--max_planes", type=int, default=1, help="planes extracted at most")
    p.add_argument("--min_inliers", type=int, default=None, help="stop when the best plane holds fewer points (default 3)")
    p.add_argument("--min_inlier_share", type=float, default=None, help="the same as a share of the file's points, in (0, 1]")
    p.add_argument("--normal_angle", type=float, default=None, help="an inlier's normal lies within this many degrees of the plane's "
                                                                    "(needs normals in the file)")
    p.add_argument("--keep", choices=("rest", "planes"), default="rest", help="write the cloud without the planes, or the planes alone")
    p.add_argument("--drop_beyond", action="store_true", help="also drop the points beyond the first plane, away from the cameras")
    p.add_argument("--mvs_folder", type=str, default="", help="--drop_beyond: the scan folder with cams/*_cam.txt (with --scan_list: the "
                                                              "folder that holds <scan>/cams)")
    p.add_argument("--color_by_plane", action="store_true", help="write a colour per plane, grey for the rest, instead of the input's")
    p.add_argument("--labels", type=str, default="", help="write the int32 labels of all input points as .npy (single file only)")
    p.add_argument("--planes", type=str, default="", help="write the planes as .npz, field P (single file only)")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--report", type=str, default="", help="write the planes, counts and settings as JSON")
    return p


def camera_side(plane, threshold: float, centres):
    """+1 or -1: the side of ``plane`` that holds the MAJORITY of the camera ``centres`` ([V,3] float64); a side is the sign of
    r = a x + b y + c z + d where |r| > threshold, centres inside the band count for neither.  ValueError on an even split."""
    import numpy as np
    c = np.asarray(centres, np.float64)
    r = plane[0] * c[:, 0] + plane[1] * c[:, 1] + plane[2] * c[:, 2] + plane[3]
    pos, neg = int((r > threshold).sum()), int((r < -threshold).sum())
    if pos == neg:
        raise ValueError(f"--drop_beyond: the cameras split evenly over the plane ({pos} on either side): no side to drop")
    return 1 if pos > neg else -1


def segment_file(src: str, dst: str, cams: str, args, device):
    """Segments one file; returns (its report entry, the device in use)."""
    import numpy as np
    from patchmatchnet_amd import pointcloud as PC
    from patchmatchnet_amd._lib import PmnError
    from cluster_cloud import cluster_colors

    model = cloud_tool.load_cloud(src, min_points=3, few_points_msg="a plane needs 3")
    n = len(model["vertices"])
    if args.normal_angle is not None and model["normals"] is None:
        raise PmnError(f"{src}: --normal_angle needs normals in the file (cloud_normals.py writes them)")
    centres = None
    if args.drop_beyond:
        from cloud_normals import camera_centres
        try:
            centres = camera_centres(cams)
        except FileNotFoundError as e:
            raise PmnError(f"--drop_beyond: no cameras: {e}") from e
    device = cloud_tool.device_of(args, device)
    t0 = time.perf_counter()
    pts = cloud_tool.upload(model["vertices"], np.float32, device)
    nrm = cloud_tool.upload(model["normals"], np.float32, device) if args.normal_angle is not None else None
    out = {"input": src, "output": dst, "points": n}
    threshold = args.threshold
    if threshold is None:
        out["spacing"] = PC.cloud_spacing(pts)
        threshold = (2.0 if args.threshold_spacings is None else args.threshold_spacings) * out["spacing"]
        if not (threshold >= 0.0 and np.isfinite(threshold)):
            raise PmnError(f"{src}: the cloud's spacing is {out['spacing']}; give --threshold")
    min_inliers = 3 if args.min_inliers is None else args.min_inliers
    if args.min_inlier_share is not None:
        min_inliers = max(1, int(np.ceil(args.min_inlier_share * n)))
    res = PC.segment_planes(pts, threshold, max_planes=args.max_planes, min_inliers=min_inliers, hypotheses=args.hypotheses,
                            seed=args.seed, refine=args.refine, normals=nrm, normal_angle=args.normal_angle)
    labels = res["labels"].cpu().numpy().astype(np.int32)
    on_plane = labels >= 0
    dropped = np.zeros(n, bool)
    if args.drop_beyond and len(res["counts"]):
        P = [float(v) for v in res["planes"][0]]
        try:
            side = camera_side(P, threshold, centres)
        except ValueError as e:
            raise PmnError(str(e)) from e
        p = pts.double()
        r = (P[0] * p[:, 0] + P[1] * p[:, 1] + P[2] * p[:, 2] + P[3]).cpu().numpy()
        dropped = (r < -threshold) if side > 0 else (r > threshold)
        out["camera_side"] = side
    keep = (on_plane if args.keep == "planes" else ~on_plane) & ~dropped
    out["seconds_search"] = time.perf_counter() - t0
    cloud_tool.write_kept(dst, model, keep, colors=cluster_colors(labels) if args.color_by_plane else None)
    if args.labels:
        cloud_tool.save_side_file(args.labels, lambda path: np.save(path, labels))
    if args.planes:
        planes = res["planes"][0] if len(res["counts"]) == 1 else res["planes"]
        cloud_tool.save_side_file(args.planes, lambda path: np.savez(path, P=planes))
    out.update(threshold=float(threshold), min_inliers=int(min_inliers), dropped_beyond=int(dropped.sum()), kept=int(keep.sum()),
               planes=[{"plane": [float(v) for v in r["plane"]], "inliers": r["count"], "rmse": r["rmse"], "hypothesis": r["hypothesis"],
                        "refits": r["refits"]} for r in res["results"]])
    print(f"{src}: {n} points read, threshold {out['threshold']:.6g}, {len(out['planes'])} planes found")
    for k, r in enumerate(out["planes"]):
        a, b, c, d = r["plane"]
        print(f"  plane {k}: {a:.9g} {b:.9g} {c:.9g} {d:.9g}, {r['inliers']} inliers, rmse {r['rmse']:.6g}, hypothesis "
              f"{r['hypothesis']}, {r['refits']} refits")
    print(f"  {out['dropped_beyond']} points dropped beyond the first plane; {out['kept']} points written -> {dst}")
    return out, device


def check_args(args) -> None:
    """ValueError for what can be refused before any file is read."""
    inf = float("inf")
    if args.threshold is not None and args.threshold_spacings is not None:
        raise ValueError("--threshold and --threshold_spacings exclude each other")
    if args.threshold is not None and not (args.threshold >= 0.0 and args.threshold < inf):
        raise ValueError(f"--threshold must be finite and >= 0, got {args.threshold}")
    if args.threshold_spacings is not None and not (args.threshold_spacings >= 0.0 and args.threshold_spacings < inf):
        raise ValueError(f"--threshold_spacings must be finite and >= 0, got {args.threshold_spacings}")
    if args.hypotheses < 1 or args.max_planes < 1:
        raise ValueError(f"--hypotheses and --max_planes must be >= 1, got {args.hypotheses} and {args.max_planes}")
    if args.seed < 0 or args.refine < 0:
        raise ValueError(f"--seed and --refine must be >= 0, got {args.seed} and {args.refine}")
    if args.min_inliers is not None and args.min_inlier_share is not None:
        raise ValueError("--min_inliers and --min_inlier_share exclude each other")
    if args.min_inliers is not None and args.min_inliers < 1:
        raise ValueError(f"--min_inliers must be >= 1, got {args.min_inliers}")
    if args.min_inlier_share is not None and not (0.0 < args.min_inlier_share <= 1.0):
        raise ValueError(f"--min_inlier_share must lie in (0, 1], got {args.min_inlier_share}")
    if args.normal_angle is not None and not (0.0 <= args.normal_angle <= 90.0):
        raise ValueError(f"--normal_angle must lie in [0, 90] degrees, got {args.normal_angle}")
    if args.drop_beyond and not args.mvs_folder:
        raise ValueError("--drop_beyond needs --mvs_folder, the scan folder with cams/*_cam.txt")
    if args.mvs_folder and not args.drop_beyond:
        raise ValueError("--mvs_folder is read by --drop_beyond only")


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if cloud_tool.refuse_torchrun(TOOL):
        return 2
    one_file = "--labels and --planes name one file each; they cannot be combined with --scan_list" if args.labels or args.planes else ""
    try:
        check_args(args)
        jobs = cloud_tool.jobs(args, args.ply_name, "fused_noplane.ply", single_only=one_file)
    except ValueError as e:
        return cloud_tool.fail(TOOL, e)
    settings = {k: getattr(args, k) for k in ("threshold", "threshold_spacings", "hypotheses", "seed", "refine", "max_planes",
                                              "min_inliers", "min_inlier_share", "normal_angle", "keep", "drop_beyond",
                                              "color_by_plane")}

    def per_file(src, dst, scan, device):
        return segment_file(src, dst, os.path.join(args.mvs_folder, scan) if scan else args.mvs_folder, args, device)

    return cloud_tool.run(TOOL, jobs, per_file, settings, args.report)


if __name__ == "__main__":
    sys.exit(main())
