"""Density clustering of a fused point cloud, on a ROCm GPU (the reference has no counterpart): takes a cloud
apart into its connected dense pieces and drops the pieces that are too small -- a patch of sky, a reflection, the turntable: clumps of
consistently wrong points that clean_cloud.py's filters keep because they are as dense inside as the surface is.

    python cluster_cloud.py --input OUT/scan1/fused.ply --output OUT/scan1/fused_clusters.ply
           [--eps E | --eps_spacings 4] [--min_points 10] [--min_cluster_points N] [--keep_clusters K] [--keep_noise]
           [--color_by_cluster] [--labels FILE.npy] [--cell C] [--device cuda:0] [--report FILE.json]
    python cluster_cloud.py --input OUT --scan_list list.txt ...   (every OUT/<scan>/fused.ply -> OUT/<scan>/fused_clusters.ply)

DBSCAN with an order-free border rule (pointcloud.cluster_dbscan; HIP kernels pmn_cloud_core and pmn_cloud_dbscan): a point is core
when at least --min_points points, itself included, lie within eps of it; clusters are the connected components of the core points; a
point that is not core joins the cluster of its nearest core point within eps (ties: the lower index in the file) or is noise.  The
labels are a function of the file and the two settings alone.  eps defaults to --eps_spacings times pointcloud.cloud_spacing (the
median over the cloud of the mean distance to the 8 nearest other points).  The defaults (4 spacings, 10 points) are SETTINGS chosen
by reasoning -- a few rings of neighbours, a count a stray pair or triple cannot reach -- not measured optima.
Kept are the points of the clusters with at least --min_cluster_points points and, with --keep_clusters K, of the K largest of them;
noise only with --keep_noise.  With neither selection every cluster stays and only noise goes.  The kept points are written unchanged
and in their order with ply.write_ply: x y z [nx ny nz] red green blue, normals when the input had them, white where it had no colours.
--color_by_cluster replaces the colours by a fixed hash of the label (noise grey), so that render.py shows the segmentation;
--labels writes the int32 label of EVERY input point (-1 noise; clusters numbered by descending size).  --cell changes the time only.
One process on one ROCm GPU; torchrun is not supported."""
import argparse
import sys
import time

import cloud_tool

TOOL = "cluster_cloud.py"
NOISE_GREY = 128


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="DBSCAN clustering of a fused point cloud on a ROCm GPU, labels independent of any visiting "
                                            "order. Single process on one GPU; torchrun is not supported.")
    p.add_argument("--input", type=str, required=True, help="a PLY cloud, or with --scan_list the folder that holds <scan>/<ply_name>")
    p.add_argument("--output", type=str, default="", help="the PLY of the kept points (with --scan_list: the folder for "
                                                          "<scan>/fused_clusters.ply, default --input)")
    p.add_argument("--scan_list", type=str, default="", help="text file with one scan per line")
    p.add_argument("--ply_name", type=str, default="fused.ply", help="with --scan_list: the file read in every scan's folder")
    p.add_argument("--eps", type=float, default=None, help="the neighbourhood radius, in scene units (default: --eps_spacings times the "
                                                           "cloud's spacing)")
    p.add_argument("--eps_spacings", type=float, default=4.0, help="eps in units of the cloud's spacing when --eps is not given (a "
                                                                   "setting, not a measured optimum)")
    p.add_argument("--min_points", type=int, default=10, help="points within eps, the point itself included, that make a point core (a "
                                                              "setting, not a measured optimum)")
    p.add_argument("--min_cluster_points", type=int, default=0, help="drop clusters with fewer points")
    p.add_argument("--keep_clusters", type=int, default=0, help="keep only this many of the largest clusters (0: all)")
    p.add_argument("--keep_noise", action="store_true", help="also keep the points that belong to no cluster")
    p.add_argument("--color_by_cluster", action="store_true", help="write a colour per cluster instead of the input's colours")
    p.add_argument("--labels", type=str, default="", help="write the int32 labels of all input points as .npy (single file only)")
    p.add_argument("--cell", type=float, default=None, help="cell of the search grid (default: about 8 points per occupied cell, at least "
                                                            "eps / 8)")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--report", type=str, default="", help="write the counts and settings as JSON")
    return p


def cluster_colors(labels):
    """uint8 [n,3]: a fixed colour per label, the low three bytes of the splitmix64 finaliser (csrc/meshops.hip's mesh_mix) of
    (label + 1) * 0x9E3779B97F4A7C15, each byte lifted into 64..255 so that no cluster is dark; noise (-1) is grey."""
    import numpy as np
    lab = np.asarray(labels, np.int64)
    with np.errstate(over="ignore"):
        z = (lab + 1).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    rgb = np.stack([(z >> np.uint64(s)) & np.uint64(0xFF) for s in (0, 8, 16)], 1)
    rgb = (64 + rgb * 3 // 4).astype(np.uint8)
    rgb[lab < 0] = NOISE_GREY
    return rgb


def cluster_file(src: str, dst: str, args, device):
    """Clusters one file; returns (its report entry, the device in use)."""
    import numpy as np
    import torch
    from patchmatchnet_amd import pointcloud as PC
    from patchmatchnet_amd._lib import PmnError

    model = cloud_tool.load_cloud(src, mesh_hint="drop a mesh's floaters with mesh.py --keep_components / --min_component_faces")
    n = len(model["vertices"])
    device = cloud_tool.device_of(args, device)
    t0 = time.perf_counter()
    pts = cloud_tool.upload(model["vertices"], np.float32, device)
    out = {"input": src, "output": dst, "points": n}
    eps = args.eps
    if eps is None:
        out["spacing"] = PC.cloud_spacing(pts)
        eps = args.eps_spacings * out["spacing"]
        if not (eps >= 0.0 and np.isfinite(eps)):
            raise PmnError(f"{src}: the cloud's spacing is {out['spacing']}; give --eps")
    labels, core, sizes = PC.cluster_dbscan(pts, eps, args.min_points, cell=args.cell)
    keep = PC.select_clusters(labels, sizes, args.min_cluster_points, args.keep_clusters)
    kept_clusters = int(torch.unique(labels[keep]).numel())
    if args.keep_noise:
        keep = keep | (labels < 0)
    keep, labels, core = keep.cpu().numpy(), labels.cpu().numpy().astype(np.int32), core.cpu().numpy()
    out["seconds_search"] = time.perf_counter() - t0
    cloud_tool.write_kept(dst, model, keep, colors=cluster_colors(labels) if args.color_by_cluster else None)
    if args.labels:
        cloud_tool.save_side_file(args.labels, lambda path: np.save(path, labels))
    noise = int((labels < 0).sum())
    out.update(eps=float(eps), core=int(core.sum()), border=int(n - noise - core.sum()), noise=noise, clusters=int(sizes.numel()),
               clusters_kept=kept_clusters, kept=int(keep.sum()), largest=[int(v) for v in sizes[:8].cpu().tolist()])
    print(f"{src}: {n} points read, eps {out['eps']:.6g}, min_points {args.min_points}: {out['core']} core, {out['border']} border, "
          f"{noise} noise; {out['clusters']} clusters found, {kept_clusters} kept; {out['kept']} points kept -> {dst}")
    return out, device


def check_args(args) -> None:
    """ValueError for what can be refused before any file is read."""
    if args.eps is not None and not (args.eps >= 0.0 and args.eps < float("inf")):
        raise ValueError(f"--eps must be finite and >= 0, got {args.eps}")
    if not (args.eps_spacings >= 0.0 and args.eps_spacings < float("inf")):
        raise ValueError(f"--eps_spacings must be finite and >= 0, got {args.eps_spacings}")
    if args.min_points < 1:
        raise ValueError(f"--min_points must be >= 1, got {args.min_points}")
    if args.min_cluster_points < 0 or args.keep_clusters < 0:
        raise ValueError(f"--min_cluster_points and --keep_clusters must be >= 0, got {args.min_cluster_points} and {args.keep_clusters}")
    if args.cell is not None and not (args.cell > 0.0 and args.cell < float("inf")):
        raise ValueError(f"--cell must be positive and finite, got {args.cell}")


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if cloud_tool.refuse_torchrun(TOOL):
        return 2
    try:
        check_args(args)
        jobs = cloud_tool.jobs(args, args.ply_name, "fused_clusters.ply",
                               single_only="--labels names one file; it cannot be combined with --scan_list" if args.labels else "")
    except ValueError as e:
        return cloud_tool.fail(TOOL, e)
    settings = {k: getattr(args, k) for k in ("eps", "eps_spacings", "min_points", "min_cluster_points", "keep_clusters", "keep_noise",
                                              "color_by_cluster", "cell")}
    return cloud_tool.run(TOOL, jobs, lambda src, dst, scan, device: cluster_file(src, dst, args, device), settings, args.report)


if __name__ == "__main__":
    sys.exit(main())
