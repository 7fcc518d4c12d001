"""A surface mesh from an oriented point cloud, on a ROCm GPU (the reference has no counterpart).

    python mesh_cloud.py --input A.ply --output mesh.ply [--voxel V] [--radius R] [--trunc T] [--k 16] [--boundary B]
           [--min_neighbors 3] [--max_blocks N] [--no_color] [--no_normals] [--min_component_faces N] [--keep_components K]
           [--device cuda:0] [--report FILE.json]
    python mesh_cloud.py --input OUT --scan_list list.txt [--ply_name fused_normals.ply] ...
                                                    (every OUT/<scan>/<ply_name> -> OUT/<scan>/mesh_cloud.ply)

mesh.py needs a scan's depth maps; this needs only points with normals: a cleaned cloud (clean_cloud.py, then cloud_normals.py), a
fused.ply whose depth maps are gone, a merged cloud, a laser scan, a cloud from another tool.  One HIP kernel (pmn_cloud_sdf_blocks)
writes, for every lattice sample near the cloud, the signed distance to the tangent planes of its k nearest points within --radius,
blended with a polynomial weight and summed in a fixed order (an implicit moving-least-squares surface; bit-reproducible), into the
block-sparse volume of mesh.py --volume sparse, whose marching tetrahedra (pmn_mt_count_blocks / pmn_mt_emit_blocks) give the mesh:
watertight wherever the cloud is, open where it ends (a sample is unobserved when the nearest point's tangent plane is met further
than --boundary from that point), with vertex colours blended from the points' and normals from the field's gradient.
Defaults, all of them settings rather than measurements: s = the median distance of a point to its 8 nearest, --voxel s,
--radius 3 voxels, --trunc = radius, --boundary radius / 2; a vertex needs --min_neighbors points within radius of both ends of its
edge.  Points whose normal is 0 0 0 or not finite (cloud_normals.py's degenerate points) are dropped and counted.  The file must have
normals (nx ny nz): cloud_normals.py adds them.  --min_component_faces / --keep_components drop floaters as in mesh.py.  The result is
written with ply.write_ply_mesh; render.py, eval_dtu.py --mesh_distance 1, eval_tnt.py --mesh_distance 1, compare_mesh.py,
simplify_mesh.py and smooth_mesh.py read it.  One process on one ROCm GPU; torchrun is not supported."""
import argparse
import sys
import time

import cloud_tool

TOOL = "mesh_cloud.py"


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Surface mesh from an oriented point cloud on a ROCm GPU: signed distance from the k "
                                            "nearest points, marching tetrahedra.  Single process on one GPU; torchrun is not supported.")
    p.add_argument("--input", type=str, required=True, help="a PLY cloud with normals, or with --scan_list the folder that holds "
                                                            "<scan>/<ply_name>")
    p.add_argument("--output", type=str, default="", help="the mesh PLY (with --scan_list: the folder for <scan>/mesh_cloud.ply, "
                                                          "default --input)")
    p.add_argument("--scan_list", type=str, default="", help="text file with one scan per line")
    p.add_argument("--ply_name", type=str, default="fused_normals.ply", help="with --scan_list: the cloud's file name in a scan's folder")
    p.add_argument("--voxel", type=float, default=None, help="lattice spacing (default: the cloud's median 8-neighbour distance)")
    p.add_argument("--radius", type=float, default=None, help="support of the neighbour search and of the weight (default: 3 voxels)")
    p.add_argument("--trunc", type=float, default=None, help="the distance that maps to +-1 in the volume (default: radius)")
    p.add_argument("--k", type=int, default=16, help="neighbours per sample (1..32)")
    p.add_argument("--boundary", type=float, default=None, help="a sample further than this along the nearest point's tangent plane "
                                                                "is unobserved (default: radius / 2)")
    p.add_argument("--min_neighbors", type=int, default=3, help="neighbours a sample needs to take part in the mesh (1..k)")
    p.add_argument("--max_blocks", type=int, default=None, help="pool size in 8 x 8 x 8-sample blocks (default: 2^20)")
    p.add_argument("--no_color", action="store_true", help="no colour planes, no vertex colours")
    p.add_argument("--no_normals", action="store_true", help="no vertex normals")
    p.add_argument("--min_component_faces", type=int, default=0, help="drop connected components with fewer faces than this (0 = off)")
    p.add_argument("--keep_components", type=int, default=0, help="keep only this many connected components, the largest by face "
                                                                  "count (0 = off)")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--report", type=str, default="", help="write the counts and settings as JSON")
    return p


def check_args(args) -> None:
    """ValueError for what can be refused before any file is read."""
    if not 1 <= args.k <= 32:
        raise ValueError(f"--k must be in 1..32, got {args.k}")
    if not 1 <= args.min_neighbors <= args.k:
        raise ValueError(f"--min_neighbors must be in 1..k, got {args.min_neighbors}")
    for name in ("voxel", "radius", "trunc", "boundary"):
        v = getattr(args, name)
        if v is not None and not (v > 0.0 and v < float("inf")):
            raise ValueError(f"--{name} must be positive and finite, got {v}")
    if args.max_blocks is not None and args.max_blocks < 1:
        raise ValueError("--max_blocks must be at least 1")
    if args.min_component_faces < 0 or args.keep_components < 0:
        raise ValueError("--min_component_faces and --keep_components must be >= 0")


def jobs_of(args):
    """[(source, destination)] of the arguments; ValueError where they do not name existing files."""
    return [(src, dst) for src, dst, _ in cloud_tool.jobs(args, args.ply_name, "mesh_cloud.ply")]


def mesh_file(src: str, dst: str, args, device):
    """The mesh of one file; returns (its report entry, the device in use)."""
    import numpy as np
    from patchmatchnet_amd import meshops, ply, pointcloud as PC
    from patchmatchnet_amd._lib import PmnError

    model = cloud_tool.load_cloud(src)
    if model["normals"] is None:
        raise PmnError(f"{src}: the cloud has no normals (nx ny nz); cloud_normals.py --input {src} --output B.ply estimates them")
    device = cloud_tool.device_of(args, device)
    t0 = time.perf_counter()
    pts = cloud_tool.upload(model["vertices"], np.float32, device)
    nrm = cloud_tool.upload(model["normals"], np.float32, device)
    col = None
    if model["colors"] is not None and not args.no_color:
        col = cloud_tool.upload(model["colors"], np.uint8, device)
    kw = {} if args.max_blocks is None else {"max_blocks": args.max_blocks}
    vertices, faces, colors, normals, info = PC.mesh_from_cloud(pts, nrm, col, voxel=args.voxel, radius=args.radius, trunc=args.trunc,
                                                                k=args.k, boundary=args.boundary, min_neighbors=args.min_neighbors,
                                                                normals_out=not args.no_normals, **kw)
    cleaned = None
    if args.min_component_faces > 0 or args.keep_components > 0:
        vertices, faces, colors, normals, (found, kept) = meshops.remove_components(
            vertices, faces, colors, normals, min_faces=args.min_component_faces, keep_largest=args.keep_components, return_counts=True)
        cleaned = {"components": int(found), "kept": int(kept)}
    ply.write_ply_mesh(dst, vertices, faces, colors, normals)
    seconds = time.perf_counter() - t0  # the upload, the spacing, the grids, the kernels, the cleaning and the file
    out = {"input": src, "output": dst, "points": info["points"], "dropped": info["dropped"], "s": info["s"], "voxel": info["voxel"],
           "radius": info["radius"], "trunc": info["trunc"], "boundary": info["boundary"], "k": info["k"],
           "min_neighbors": info["min_neighbors"], "dims": list(info["dims"]), "blocks": info["blocks"],
           "block_share": info["block_share"], "observed": info["observed"], "vertices": int(vertices.shape[0]),
           "faces": int(faces.shape[0]), "components": cleaned, "note": info["note"], "seconds_device": seconds}
    if info["note"]:
        print(f"{src}: {info['note']}")
    s = "given voxel" if info["s"] is None else "s {:.6g}".format(info["s"])
    print(f"{src}: {out['points']} points read, {out['dropped']} dropped (no normal); {s}, voxel {out['voxel']:.6g}, radius "
          f"{out['radius']:.6g}, trunc {out['trunc']:.6g}, k {out['k']}; {out['blocks']} blocks ({100 * out['block_share']:.3g} % of the "
          f"virtual lattice {out['dims'][0]} x {out['dims'][1]} x {out['dims'][2]}), {out['observed']} samples observed; "
          + (f"{cleaned['components']} components, {cleaned['kept']} kept; " if cleaned else "")
          + f"{out['vertices']} vertices, {out['faces']} faces -> {dst}")
    return out, device


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if cloud_tool.refuse_torchrun(TOOL):
        return 2
    try:
        check_args(args)
        jobs = jobs_of(args)
    except ValueError as e:
        return cloud_tool.fail(TOOL, e)
    return cloud_tool.run(TOOL, jobs, lambda src, dst, device: mesh_file(src, dst, args, device), {}, args.report,
                          also_catch=(ValueError,))


if __name__ == "__main__":
    sys.exit(main())
