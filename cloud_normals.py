"""Normals for a point cloud from its own neighbourhoods, on a ROCm GPU (the reference has no counterpart).

    python cloud_normals.py --input A.ply --output B.ply [--k 16] [--max_dist D] [--cell C] [--line_ratio R]
           [--orient cameras --mvs_folder SCAN | --orient viewpoint --viewpoint X Y Z | --orient existing | --orient none]
           [--drop_degenerate] [--device cuda:0] [--report FILE.json]
    python cloud_normals.py --input OUT --scan_list list.txt ...   (every OUT/<scan>/fused.ply -> OUT/<scan>/fused_normals.ply;
                                                                    --mvs_folder then holds <scan>/cams)

A point's normal is the direction of least variance of the point and its k nearest neighbours (PCA, Open3D's estimate_normals with
knn = k + 1), found by one HIP kernel (pmn_knn_normals) over the grid of patchmatchnet_amd/pointcloud.py: the k-nearest search of
clean_cloud.py with the covariance and its eigenvector computed by the lane that found the neighbours.  --cell changes the time only,
--max_dist caps the search (default 16 cells); a point with fewer than two neighbours in range, or whose neighbourhood lies on a line
(second eigenvalue <= --line_ratio times the largest), gets the normal 0 0 0.
--orient: `cameras` turns every normal towards the nearest camera centre -R^T t of SCAN/cams/*_cam.txt, `viewpoint` towards --viewpoint;
both are heuristics, the cloud does not say which camera saw a point.  `existing` keeps the side of the normals the input file
already has (for example the depth-map normals of `eval.py --normals 1`), `none` makes the largest component positive.  Without
--orient: cameras when --mvs_folder is given, viewpoint when --viewpoint is, else none.
The cloud is read with ply.read_ply_model and written with ply.write_ply: x y z nx ny nz red green blue, positions and colours
unchanged and in order (white where the input had no colours), normals added or replaced; other properties are not carried over.
--drop_degenerate removes the points whose normal is zero; by default they stay and the report counts them.  `render.py --model B.ply`
shades the result and Poisson meshers read it.  One process on one ROCm GPU; torchrun is not supported."""
import argparse
import glob
import os
import sys
import time

import cloud_tool

TOOL = "cloud_normals.py"
ORIENT = ("cameras", "viewpoint", "existing", "none")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Normals of a point cloud from k-nearest-neighbour PCA on a ROCm GPU, oriented to cameras. "
                                            "Single process on one GPU; torchrun is not supported.")
    p.add_argument("--input", type=str, required=True, help="a PLY cloud, or with --scan_list the folder that holds <scan>/fused.ply")
    p.add_argument("--output", type=str, default="", help="the PLY with normals (with --scan_list: the folder for "
                                                          "<scan>/fused_normals.ply, default --input)")
    p.add_argument("--scan_list", type=str, default="", help="text file with one scan per line")
    p.add_argument("--k", type=int, default=16, help="neighbours per point (1..32); the point itself is added to them")
    p.add_argument("--max_dist", type=float, default=None, help="cap of the neighbour search (default: 16 cells)")
    p.add_argument("--cell", type=float, default=None, help="cell of the search grid (default: about 8 points per occupied cell)")
    p.add_argument("--orient", type=str, default=None, choices=ORIENT,
                   help="which side the normals face (default: cameras with --mvs_folder, viewpoint with --viewpoint, else none)")
    p.add_argument("--mvs_folder", type=str, default="", help="cameras: the scan folder with cams/*_cam.txt (with --scan_list: the "
                                                              "folder that holds <scan>/cams)")
    p.add_argument("--viewpoint", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="viewpoint: the point to face")
    p.add_argument("--line_ratio", type=float, default=1e-6, help="no normal where the second eigenvalue <= this times the largest")
    p.add_argument("--drop_degenerate", action="store_true", help="remove the points whose normal is zero")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--report", type=str, default="", help="write the counts and settings as JSON")
    return p


def resolve_orient(args) -> str:
    """The orientation mode the arguments ask for; ValueError where they contradict each other."""
    mode = args.orient
    if mode is None:
        if args.mvs_folder and args.viewpoint is not None:
            raise ValueError("--mvs_folder and --viewpoint together need --orient cameras or --orient viewpoint")
        mode = "cameras" if args.mvs_folder else ("viewpoint" if args.viewpoint is not None else "none")
    if mode == "cameras" and not args.mvs_folder:
        raise ValueError("--orient cameras needs --mvs_folder")
    if mode == "viewpoint" and args.viewpoint is None:
        raise ValueError("--orient viewpoint needs --viewpoint X Y Z")
    if mode != "cameras" and args.mvs_folder:
        raise ValueError(f"--mvs_folder is read by --orient cameras only, not by --orient {mode}")
    if mode != "viewpoint" and args.viewpoint is not None:
        raise ValueError(f"--viewpoint is read by --orient viewpoint only, not by --orient {mode}")
    return mode


def camera_centres(folder: str):
    """float64 [V,3]: the camera centres -R^T t of <folder>/cams/*_cam.txt, in file-name order."""
    import numpy as np

    from patchmatchnet_amd.data_io import read_cam_file
    files = sorted(glob.glob(os.path.join(folder, "cams", "*_cam.txt")))
    if not files:
        raise FileNotFoundError(os.path.join(folder, "cams", "*_cam.txt"))
    out = []
    for f in files:
        E = np.asarray(read_cam_file(f)[1], np.float64)
        out.append(-E[:3, :3].T @ E[:3, 3])
    return np.stack(out)


def normals_file(src: str, dst: str, args, mode: str, views, device):
    """Normals for one file; returns (its report entry, the device in use)."""
    import numpy as np
    from patchmatchnet_amd import _lib, pointcloud as PC
    from patchmatchnet_amd._lib import PmnError

    model = cloud_tool.load_cloud(src, mesh_hint="mesh.py writes vertex normals from the faces")
    n = len(model["vertices"])
    if mode == "existing" and model["normals"] is None:
        raise PmnError(f"{src}: --orient existing needs normals (nx ny nz) in the input file")
    if views is not None and len(views) > _lib.NORMAL_MAX_VIEWPOINTS:
        raise PmnError(f"{len(views)} cameras: at most {_lib.NORMAL_MAX_VIEWPOINTS} viewpoints")
    device = cloud_tool.device_of(args, device)
    t0 = time.perf_counter()
    pts = cloud_tool.upload(model["vertices"], np.float32, device)
    cell = PC.default_cell(pts) if args.cell is None else float(args.cell)
    max_dist = PC.CLEAN_MAX_DIST_CELLS * cell if args.max_dist is None else float(args.max_dist)
    like = cloud_tool.upload(model["normals"], np.float32, device) if mode == "existing" else None
    normal, variation, count = PC.estimate_normals(pts, k=args.k, max_dist=max_dist, cell=cell, viewpoints=views, orient_like=like,
                                                   line_ratio=args.line_ratio, return_variation=True, return_count=True)
    has = (normal != 0).any(1)
    zero = int(n - has.sum())
    capped = int((count < args.k).sum())
    mean_variation = float(variation[has].mean()) if zero < n else 0.0
    normal, has = normal.cpu().numpy(), has.cpu().numpy()
    seconds = time.perf_counter() - t0  # the upload, the cell search, the grid, the kernel, the counts and the copy back
    keep = has if args.drop_degenerate else np.ones(n, bool)
    cloud_tool.write_kept(dst, model, keep, normals=normal)
    out = {"input": src, "output": dst, "n": n, "k": args.k, "cell": cell, "max_dist": max_dist, "orient": mode,
           "viewpoints": 0 if views is None else len(views), "zero_normals": zero, "capped": capped, "written": int(keep.sum()),
           "mean_variation": mean_variation, "seconds_device": seconds}
    print(f"{src}: {n} points read, {zero} without a normal, {capped} with fewer than {args.k} neighbours within {max_dist:.6g}, "
          f"{out['written']} written (orient {mode}) -> {dst}")
    return out, device


def check_args(args) -> str:
    """The orientation mode; ValueError for what can be refused before any file is read."""
    if not 1 <= args.k <= 32:
        raise ValueError(f"--k must be in 1..32, got {args.k}")
    if not (args.line_ratio >= 0.0 and args.line_ratio < float("inf")):
        raise ValueError(f"--line_ratio must be finite and >= 0, got {args.line_ratio}")
    for name in ("max_dist", "cell"):
        v = getattr(args, name)
        if v is not None and not (v > 0.0 and v < float("inf")):
            raise ValueError(f"--{name} must be positive and finite, got {v}")
    return resolve_orient(args)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if cloud_tool.refuse_torchrun(TOOL):
        return 2
    try:
        mode = check_args(args)
        jobs = cloud_tool.jobs(args, "fused.ply", "fused_normals.ply")
    except ValueError as e:
        return cloud_tool.fail(TOOL, e)

    def per_file(src, dst, scan, device):  # the scan's cameras are read before the file is opened
        import numpy as np
        from patchmatchnet_amd._lib import PmnError
        views = None
        if mode == "cameras":
            try:
                views = camera_centres(os.path.join(args.mvs_folder, scan) if scan else args.mvs_folder)
            except FileNotFoundError as e:
                raise PmnError(f"no camera files: {e}") from e
        elif mode == "viewpoint":
            views = np.asarray([args.viewpoint], np.float64)
        return normals_file(src, dst, args, mode, views, device)

    settings = {"k": args.k, "line_ratio": args.line_ratio, "orient": mode, "drop_degenerate": bool(args.drop_degenerate)}
    return cloud_tool.run(TOOL, jobs, per_file, settings, args.report)


if __name__ == "__main__":
    sys.exit(main())
