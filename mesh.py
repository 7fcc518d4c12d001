#!/usr/bin/env python
"""PatchmatchNet results -> a triangle mesh per scan (the reference stops at fused.ply).

    python mesh.py --input_folder MVS --results_folder OUT [--output_folder OUT] [--scan_list list.txt] [--device cuda:0]

<input> is the MVSNet-layout folder (per scan pair.txt, cams/, images/), <results> holds what `eval.py --output_type both` wrote
(depth_est/<id>.pfm|.bin and mask/<id>_final.png).  The masked depth maps of every reference view are integrated into a dense
truncated-signed-distance volume on the device (pmn_tsdf_integrate) and the iso-surface is extracted by marching tetrahedra
(pmn_mt_count / pmn_mt_emit): <output>/<scan>/mesh.ply, binary PLY with vertex colours and normals, closed wherever the volume was
observed.  --volume sparse keeps only the 8 x 8 x 8-sample blocks near the surface: a scene whose dense lattice
would exceed --max_voxels keeps its natural voxel, and where both fit the mesh is the dense one.  --min_component_faces N and
--keep_components K drop the floaters before the file is written: connected components with fewer than N faces, or outside the K
largest.  --smooth N then runs N iterations of Taubin's filter over the vertices (DESIGN.md section 30;
--smooth_lambda, --smooth_mu, --smooth_boundary) and, unless --no_normals, replaces the normals by those of the smoothed faces;
smooth_mesh.py does the same to a file.  --simplify K then clusters the vertices into cells of K voxels and
writes one vertex per cluster, placed by the clusters' plane quadrics; simplify_mesh.py does the same to a file.
One process on one ROCm GPU; torchrun is not supported."""
import argparse
import os
import sys
import time

import cloud_tool

# pmn_mt_emit winds its triangles so that (B - A) x (C - A) points WITH the TSDF gradient it writes as the normal, from inside to outside
# (measured on a meshed sphere: DESIGN.md section 30, tests/test_smooth_gpu.py), so normals recomputed from the faces are not flipped.
MESHER_WINDING_FLIP = False


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="TSDF integration of eval.py's depth maps and marching-tetrahedra mesh extraction on a ROCm "
                                            "GPU. Single process on one GPU; torchrun is not supported.")
    p.add_argument("--input_folder", type=str, help="PatchmatchNet input folder (per scan: cams/, images/, pair.txt)")
    p.add_argument("--results_folder", type=str, default="", help="eval.py --output_type both output folder (default: the input folder)")
    p.add_argument("--output_folder", type=str, default="", help="where <scan>/mesh.ply goes (default: the results folder)")
    p.add_argument("--scan_list", type=str, default="", help="text file with one scan per line (default: the input folder is the scan)")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--image_max_dim", type=int, default=-1, help="the value eval.py ran with (the maps' size follows from it)")
    p.add_argument("--voxel", type=float, default=None,
                   help="sample spacing in world units (default: 2 x the median over the masked pixels of depth / fx)")
    p.add_argument("--trunc", type=float, default=None, help="truncation distance in world units (default: 4 x voxel)")
    p.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("XMIN", "YMIN", "ZMIN", "XMAX", "YMAX", "ZMAX"),
                   help="the volume (default: the 1st-99th percentile box of the back-projected masked pixels grown by trunc)")
    p.add_argument("--max_voxels", type=int, default=2 ** 29, help="largest lattice; a finer grid gets a larger voxel (and says so)")
    p.add_argument("--volume", type=str, default="dense", choices=("dense", "sparse"),
                   help="dense: the whole lattice (bounded by --max_voxels); sparse: only the blocks near the surface (--max_blocks)")
    p.add_argument("--max_blocks", type=int, default=2 ** 20,
                   help="--volume sparse: largest pool in blocks of 512 samples; a scene that needs more gets a larger voxel (and says so)")
    p.add_argument("--mask", type=str, default="final", choices=("final", "none"), help="which pixels of a depth map count")
    p.add_argument("--min_weight", type=float, default=1.0, help="observations a sample needs for its cells to be meshed")
    p.add_argument("--no_color", action="store_true", help="no colour planes: 8 instead of 24 bytes per sample, no vertex colours")
    p.add_argument("--no_normals", action="store_true", help="no vertex normals")
    p.add_argument("--min_component_faces", type=int, default=0,
                   help="drop connected components with fewer faces than this (0 = off)")
    p.add_argument("--keep_components", type=int, default=0,
                   help="keep only this many connected components, the largest by face count (0 = off)")
    p.add_argument("--smooth", type=int, default=0,
                   help="iterations of Taubin's filter over the mesh, before --simplify (0 = off)")
    p.add_argument("--smooth_lambda", type=float, default=0.5, help="--smooth: the shrinking step's factor, in (0, 1]")
    p.add_argument("--smooth_mu", type=float, default=-0.53, help="--smooth: the inflating step's factor, < -smooth_lambda")
    p.add_argument("--smooth_boundary", type=str, default="fixed", choices=("fixed", "free"),
                   help="--smooth: fixed leaves the vertices on an open edge where they are")
    p.add_argument("--simplify", type=float, default=0.0,
                   help="cluster the vertices into cells of this many voxels, one vertex per cluster (> 1; 0 = off)")
    p.add_argument("--views_per_launch", type=int, default=8, help="views integrated per kernel launch (1..16)")
    return p


def _load_scan(args, scan, device):
    """(maps [V,h*w] device, sizes, cams [V,21], masks | None, images | None, K, E lists) of one scan's reference views."""
    import numpy as np
    import torch
    import eval as ev  # the intrinsics are scaled to the maps' size by eval.py's own fusion-stage code
    from patchmatchnet_amd import PmnError, tsdf
    from patchmatchnet_amd.data_io import read_image, read_image_u8, read_map, read_pair_file
    from PIL import Image
    src = os.path.join(args.input_folder, scan)
    res = os.path.join(args.results_folder, scan)
    ids = [r for r, _ in read_pair_file(os.path.join(src, "pair.txt"))]
    if not ids:
        raise PmnError("{}: pair.txt lists no reference view".format(src))
    cams, sizes = ev._scan_cameras(args, scan, ids)
    if args.mask == "final":
        missing = [os.path.join(res, "mask/{:0>8}_final.png".format(v)) for v in ids
                   if not os.path.isfile(os.path.join(res, "mask/{:0>8}_final.png".format(v)))]
        if missing:
            raise PmnError("{} of {} reference views have no final mask ({}{}); run eval.py --output_type both first, or pass "
                           "--mask none".format(len(missing), len(ids), ", ".join(missing[:5]), ", ..." if len(missing) > 5 else ""))
    stride = max(h * w for h, w in sizes.values())
    maps = torch.zeros((len(ids), stride), dtype=torch.float32)
    masks, images = [], []
    for n, v in enumerate(ids):
        path = next((os.path.join(res, "depth_est/{:0>8}{}".format(v, ext)) for ext in (".pfm", ".bin")
                     if os.path.isfile(os.path.join(res, "depth_est/{:0>8}{}".format(v, ext)))), None)
        if path is None:
            raise PmnError("{}: no depth map depth_est/{:0>8}.pfm|.bin".format(res, v))
        d = np.ascontiguousarray(read_map(path).squeeze(2), np.float32)
        if d.shape != sizes[v]:
            raise PmnError("{}: the map of view {} is {}x{}, its image (after --image_max_dim) is {}x{}".format(res, v, *d.shape, *sizes[v]))
        maps[n, :d.size] = torch.from_numpy(d.reshape(-1))
        if args.mask == "final":
            m = np.array(Image.open(os.path.join(res, "mask/{:0>8}_final.png".format(v))))
            if m.shape[:2] != sizes[v]:
                raise PmnError("{}: the final mask of view {} is not {}x{}".format(res, v, *sizes[v]))
            masks.append(torch.from_numpy(np.ascontiguousarray((m.reshape(m.shape[0], m.shape[1], -1)[..., 0] > 0).astype(np.uint8))).to(device))
        if not args.no_color:
            ipath = os.path.join(src, "images/{:0>8}.jpg".format(v))
            u8 = read_image_u8(ipath, args.image_max_dim)
            if u8 is None:
                u8 = (read_image(ipath, args.image_max_dim)[0] * 255.0).astype(np.uint8)
            images.append(torch.from_numpy(np.ascontiguousarray(u8)).to(device))
    cam21 = np.stack([tsdf.camera21(cams[v]["intrinsics"], cams[v]["extrinsics"]) for v in ids])
    return (ids, maps.to(device), [sizes[v] for v in ids], cam21, masks if args.mask == "final" else None,
            images if not args.no_color else None, [cams[v] for v in ids])


def mesh_scan(args, scan, device):
    import torch
    from patchmatchnet_amd import PmnError, meshops, ops, tsdf
    t0 = time.perf_counter()
    ids, maps, sizes, cam21, masks, images, cams = _load_scan(args, scan, device)
    t1 = time.perf_counter()
    pts, foot = [], []
    for n in range(len(ids)):
        h, w = sizes[n]
        p, f = tsdf.backproject(maps[n, :h * w].view(h, w), None if masks is None else masks[n], cams[n]["intrinsics"],
                                cams[n]["extrinsics"])
        pts.append(p)
        foot.append(f)
    pts, foot = torch.cat(pts), torch.cat(foot)
    name = scan or args.input_folder
    sparse = args.volume == "sparse"
    if not sparse:
        origin, voxel, trunc, dims, note = tsdf.choose_grid(pts, foot, args.voxel, args.trunc, args.bounds, args.max_voxels)
        if note:
            print("{}: {}".format(name, note))
        vol = tsdf.TsdfVolume(origin, voxel, dims, trunc, device, color=not args.no_color)
    else:
        voxel = args.voxel
        while True:
            origin, voxel, trunc, dims, note = tsdf.choose_grid(pts, foot, voxel, args.trunc, args.bounds, tsdf.MAX_VIRTUAL_VOXELS,
                                                                "the virtual lattice's", ops.SPARSE_MAX_AXIS - 1)
            if note:
                print("{}: {}".format(name, note))
            vol = tsdf.SparseTsdfVolume(origin, voxel, dims, trunc, device, color=not args.no_color, max_blocks=args.max_blocks)
            try:
                vol.allocate(maps, list(range(len(ids))), sizes, cam21, masks)
                break
            except PmnError:
                if vol.needed <= args.max_blocks:
                    raise
            # the blocks follow the surface, whose area in voxels falls with the square of the voxel
            voxel *= max((vol.needed / float(args.max_blocks)) ** 0.5, 1.01)
            print("{}: {} blocks would exceed --max_blocks {}: voxel enlarged to {:.6g}{}".format(
                name, vol.needed, args.max_blocks, voxel, "" if args.trunc is not None else " (trunc {:.6g})".format(4.0 * voxel)))
            del vol
    del pts, foot
    torch.cuda.synchronize(device)
    t2 = time.perf_counter()
    vol.integrate(maps, list(range(len(ids))), sizes, cam21, masks, images, batch=args.views_per_launch)
    torch.cuda.synchronize(device)
    t3 = time.perf_counter()
    vertices, faces, colors, normals = vol.extract(args.min_weight, normals=not args.no_normals)
    cleaned = None
    if args.min_component_faces > 0 or args.keep_components > 0:
        nv0, nf0 = vertices.shape[0], faces.shape[0]
        vertices, faces, colors, normals, (found, kept) = meshops.remove_components(
            vertices, faces, colors, normals, min_faces=args.min_component_faces, keep_largest=args.keep_components, return_counts=True)
        cleaned = "{}: {} components, {} kept; {} vertices and {} faces dropped".format(
            name, found, kept, nv0 - vertices.shape[0], nf0 - faces.shape[0])
    smoothed = None
    if args.smooth > 0:
        nb, mean_d, max_d = 0, 0.0, 0.0
        if vertices.shape[0]:
            adjacency = meshops.vertex_adjacency(faces, vertices.shape[0])
            before = vertices
            vertices = meshops.smooth_taubin(before, faces, args.smooth, args.smooth_lambda, args.smooth_mu,
                                             boundary=args.smooth_boundary, adjacency=adjacency)
            if normals is not None:  # of the geometry that is written, on the side the mesher's own normals point to
                normals = meshops.vertex_normals(vertices, faces, flip=MESHER_WINDING_FLIP)
            moved = (vertices.double() - before.double()).norm(dim=1) / voxel
            nb, mean_d, max_d = int(adjacency.boundary.sum()), float(moved.mean()), float(moved.max())
        smoothed = "{}: smoothed by {} Taubin iterations (lambda {:g}, mu {:g}, boundary {}): {} vertices, {} on the boundary; " \
                   "displacement mean {:.4f}, max {:.4f} voxels".format(name, args.smooth, args.smooth_lambda, args.smooth_mu,
                                                                         args.smooth_boundary, vertices.shape[0], nb, mean_d, max_d)
    simplified = None
    if args.simplify > 0:
        nv0, nf0 = vertices.shape[0], faces.shape[0]
        if nv0:
            vertices, faces, colors, normals = meshops.simplify_clustering(vertices, faces, args.simplify * voxel, colors=colors,
                                                                           normals=normals)
        simplified = "{}: simplified at cell {:.6g} ({:g} voxels): {} vertices, {} faces -> {} vertices, {} faces".format(
            name, args.simplify * voxel, args.simplify, nv0, nf0, vertices.shape[0], faces.shape[0])
    torch.cuda.synchronize(device)
    t4 = time.perf_counter()
    out = os.path.join(args.output_folder, scan, "mesh.ply")
    tsdf.write_ply_mesh(out, vertices, faces, colors, normals)
    t5 = time.perf_counter()
    blocks = ""
    if sparse:
        nb = vol.nblocks[0] * vol.nblocks[1] * vol.nblocks[2]
        blocks = ", {} of {} blocks allocated ({:.3g} % of the virtual lattice)".format(vol.needed, nb, 100.0 * vol.needed / nb)
    print("{}: grid {} x {} x {} at origin ({:.6g}, {:.6g}, {:.6g}), voxel {:.6g}, trunc {:.6g}{}, {} views -> {} vertices, {} faces; "
          "load {:.3f} s, grid {:.3f} s, integrate {:.3f} s, extract {:.3f} s, write {:.3f} s -> {}".format(
              name, dims[0], dims[1], dims[2], origin[0], origin[1], origin[2], voxel, trunc, blocks, len(ids), vertices.shape[0],
              faces.shape[0], t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, out))
    if cleaned:
        print(cleaned)
    if smoothed:
        print(smoothed)
    if simplified:
        print(simplified)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if cloud_tool.refuse_torchrun("mesh.py"):
        return 2
    if not args.input_folder or not os.path.isdir(args.input_folder):
        raise Exception("Invalid input folder: {}".format(args.input_folder))
    args.results_folder = args.results_folder or args.input_folder
    args.output_folder = args.output_folder or args.results_folder
    import torch
    from patchmatchnet_amd import PmnError
    if not 1 <= args.views_per_launch <= 16:
        raise PmnError("--views_per_launch must be 1..16")
    if args.max_blocks < 1:
        raise PmnError("--max_blocks must be at least 1")
    if args.min_component_faces < 0 or args.keep_components < 0:
        raise PmnError("--min_component_faces and --keep_components must be >= 0")
    if args.simplify != 0 and not (args.simplify > 1 and args.simplify < float("inf")):
        raise PmnError("--simplify must be 0 (off) or a finite number of voxels greater than 1, got {}".format(args.simplify))
    if args.smooth < 0:
        raise PmnError("--smooth must be >= 0 iterations, got {}".format(args.smooth))
    if not (args.smooth_lambda > 0 and args.smooth_lambda <= 1):
        raise PmnError("--smooth_lambda must be in (0, 1], got {}".format(args.smooth_lambda))
    if not (args.smooth_mu < -args.smooth_lambda and args.smooth_mu > float("-inf")):
        raise PmnError("--smooth_mu must be finite and < -smooth_lambda = {}, got {}".format(-args.smooth_lambda, args.smooth_mu))
    device = torch.device(args.device)
    if device.type != "cuda":
        raise PmnError("--device {}: mesh.py runs on a ROCm GPU (no CPU fallback)".format(args.device))
    if not torch.cuda.is_available():
        raise PmnError("mesh.py runs on a ROCm GPU; none is visible")
    if args.scan_list:
        if not os.path.isfile(args.scan_list):
            raise PmnError("Invalid scan list file: {}".format(args.scan_list))
        scans = cloud_tool.read_scan_list(args.scan_list)
    else:
        scans = [""]
    with torch.no_grad():
        for scan in scans:
            mesh_scan(args, scan, device)
    return 0


if __name__ == "__main__":
    from patchmatchnet_amd import PmnError
    try:
        sys.exit(main(sys.argv[1:]))
    except PmnError as e:
        sys.exit("mesh.py: " + str(e))
