#!/usr/bin/env python
"""A mesh or a point cloud drawn back into a scan's cameras (the reference only has an interactive viewer).

    python render.py --input_folder MVS --model OUT/{scan}/mesh.ply --output_folder DST [--scan_list list.txt]
                     [--write depth_gt,masks,images,normals] [--radius_px R | --radius_world R] [--orbit N --size H W --fov DEG]

<input> is the MVSNet-layout folder (per scan pair.txt, cams/, images/); --model is a PLY mesh (mesh.py's, or a ground-truth mesh) or a
PLY cloud (either kind of fused.ply, a laser scan) and may contain {scan}.  Per reference view of pair.txt, with the cameras scaled to
the images' size as eval.py scales them: <output>/<scan>/depth_gt/<id>.pfm (0 = nothing seen: what train.py --mode test reads as ground
truth), masks/<id>.png (depth > 0), render/<id>.png and normal_maps/<id>.geometric.bin.  --orbit N draws N views on a circle around
the model instead of (without --input_folder) or besides the scan's cameras: <output>/<scan>/orbit/%04d.png.  One process on one ROCm
GPU; torchrun is not supported."""
import argparse
import os
import sys
import time

import cloud_tool

WRITES = ("depth_gt", "masks", "images", "normals")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Z-buffered rendering of a PLY mesh or point cloud into a scan's cameras on a ROCm GPU: "
                                            "ground-truth depth maps, masks, pictures, normal maps. Single process on one GPU; torchrun "
                                            "is not supported.")
    p.add_argument("--input_folder", type=str, default="", help="PatchmatchNet input folder (per scan: cams/, images/, pair.txt)")
    p.add_argument("--model", type=str, help="PLY mesh or cloud; may contain {scan}")
    p.add_argument("--output_folder", type=str, help="where <scan>/depth_gt, masks, render, normal_maps, orbit go")
    p.add_argument("--scan_list", type=str, default="", help="text file with one scan per line (default: the input folder is the scan)")
    p.add_argument("--write", type=str, default="depth_gt,masks,images", help="comma-separated subset of " + ",".join(WRITES))
    p.add_argument("--image_max_dim", type=int, default=-1, help="render at the size eval.py --image_max_dim would run at")
    p.add_argument("--radius_px", type=float, default=0.0, help="cloud footprint radius in pixels (0: the nearest pixel only)")
    p.add_argument("--radius_world", type=float, default=0.0, help="cloud footprint radius in world units (a disc of R * fx / z pixels)")
    p.add_argument("--shade", type=int, default=1, choices=(0, 1), help="1: multiply the colour by a head-light Lambert term")
    p.add_argument("--orbit", type=int, default=0, metavar="N", help="draw N views on a circle around the model")
    p.add_argument("--size", type=int, nargs=2, default=(600, 800), metavar=("H", "W"), help="size of the orbit views")
    p.add_argument("--fov", type=float, default=50.0, help="vertical field of view of the orbit views, degrees")
    p.add_argument("--device", type=str, default="cuda:0")
    return p


def _draw(renderer, model, K, E, h, w, args, want_normal):
    if model["faces"] is not None:
        return renderer.render_mesh(model["vertices"], model["faces"], K, E, h, w, model["colors"], model["normals"],
                                    shade=bool(args.shade), rgb=True, normal=want_normal)
    return renderer.render_points(model["vertices"], K, E, h, w, model["colors"], model["normals"], radius_px=args.radius_px,
                                  radius_world=args.radius_world, shade=bool(args.shade), rgb=True, normal=want_normal)


def render_scan(args, scan, device, renderer, cache):
    import numpy as np
    import torch
    import eval as ev  # the intrinsics are scaled to the images' size by eval.py's own fusion-stage code, as in mesh.py
    from patchmatchnet_amd import PmnError, render
    from patchmatchnet_amd.data_io import read_pair_file, save_bin, save_image, save_pfm
    t0 = time.perf_counter()
    path = args.model.replace("{scan}", scan)
    if path not in cache:
        cache.clear()
        host = render.read_ply_model(path)
        if len(host["vertices"]) == 0:
            raise PmnError("{}: the model has no vertices".format(path))
        cache[path] = (render.upload_model(host, device), np.concatenate((host["vertices"].min(0), host["vertices"].max(0))))
    model, bounds = cache[path]
    kind = "mesh" if model["faces"] is not None else "cloud"
    prims = (model["faces"] if model["faces"] is not None else model["vertices"]).shape[0]
    out = os.path.join(args.output_folder, scan)
    writes = set(args.write.split(",")) if args.write else set()
    t1 = time.perf_counter()
    t_render = t_write = 0.0
    counters, n_views = [], 0
    if args.input_folder:
        src = os.path.join(args.input_folder, scan)
        ids = [r for r, _ in read_pair_file(os.path.join(src, "pair.txt"))]
        if not ids:
            raise PmnError("{}: pair.txt lists no reference view".format(src))
        cams, sizes = ev._scan_cameras(args, scan, ids)
        for sub, key in (("depth_gt", "depth_gt"), ("masks", "masks"), ("render", "images"), ("normal_maps", "normals")):
            if key in writes:
                os.makedirs(os.path.join(out, sub), exist_ok=True)
        for v in ids:
            a = time.perf_counter()
            h, w = sizes[v]
            depth, _, rgb, normal, cnt = _draw(renderer, model, cams[v]["intrinsics"], cams[v]["extrinsics"], h, w, args,
                                               "normals" in writes)
            counters.append(cnt)
            d = depth.cpu().numpy()  # (the copies wait for the view's kernels; the planes are reused by the next view)
            img = rgb.cpu().numpy() if "images" in writes else None
            nrm = normal.cpu().numpy() if "normals" in writes else None
            b = time.perf_counter()
            if "depth_gt" in writes:
                save_pfm(os.path.join(out, "depth_gt/{:0>8}.pfm".format(v)), d)
            if "masks" in writes:
                save_image(os.path.join(out, "masks/{:0>8}.png".format(v)), d > 0)
            if img is not None:
                save_image(os.path.join(out, "render/{:0>8}.png".format(v)), img)
            if nrm is not None:
                save_bin(os.path.join(out, "normal_maps/{:0>8}.geometric.bin".format(v)), nrm)
            t_render += b - a
            t_write += time.perf_counter() - b
        n_views += len(ids)
    if args.orbit > 0:
        os.makedirs(os.path.join(out, "orbit"), exist_ok=True)
        h, w = args.size
        Ks, Es = render.orbit_cameras(bounds, args.orbit, h, w, args.fov)
        for n in range(args.orbit):
            a = time.perf_counter()
            _, _, rgb, _, cnt = _draw(renderer, model, Ks[n], Es[n], h, w, args, False)
            counters.append(cnt)
            img = rgb.cpu().numpy()
            b = time.perf_counter()
            save_image(os.path.join(out, "orbit/{:04d}.png".format(n)), img)
            t_render += b - a
            t_write += time.perf_counter() - b
        n_views += args.orbit
    c = torch.stack(counters).sum(0).tolist()  # the counters' one host read, after the loops
    skipped = c[0] + c[1] + c[2]
    print("{}: {} of {} {}, {} views -> kept {} (passed the projection; they may still cover no pixel), skipped {} (behind the camera or not finite {}, outside the guard band {}, zero area "
          "{}; summed over the views), {} large triangles; load {:.3f} s, render {:.3f} s, write {:.3f} s -> {}".format(
              scan or args.input_folder or path, kind, prims, "triangles" if kind == "mesh" else "points", n_views,
              prims * n_views - skipped, skipped, c[0], c[1], c[2], c[3], t1 - t0, t_render, t_write, out))


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if cloud_tool.refuse_torchrun("render.py"):
        return 2
    from patchmatchnet_amd import PmnError
    if args.input_folder and not os.path.isdir(args.input_folder):
        raise Exception("Invalid input folder: {}".format(args.input_folder))
    if not args.input_folder and args.orbit <= 0:
        raise PmnError("nothing to draw: give --input_folder (the scan's cameras) or --orbit N")
    if not args.model:
        raise PmnError("--model is required (a PLY mesh or cloud; may contain {scan})")
    if not args.output_folder:
        raise PmnError("--output_folder is required")
    if "{scan}" not in args.model:
        head = b""
        if os.path.isfile(args.model):
            with open(args.model, "rb") as f:
                head = f.read(4)
        if head[:3] != b"ply":
            raise PmnError("--model {}: neither a PLY mesh nor a PLY cloud".format(args.model))
    bad = [x for x in args.write.split(",") if x and x not in WRITES]
    if bad:
        raise PmnError("--write {}: choose from {}".format(",".join(bad), ",".join(WRITES)))
    if args.radius_px < 0 or args.radius_world < 0 or (args.radius_px > 0 and args.radius_world > 0):
        raise PmnError("--radius_px and --radius_world must be >= 0 and only one of them may be given")
    if args.orbit < 0 or min(args.size) < 1:
        raise PmnError("--orbit must be >= 0 and --size positive")
    import torch
    device = torch.device(args.device)
    if device.type != "cuda":
        raise PmnError("--device {}: render.py runs on a ROCm GPU (no CPU fallback)".format(args.device))
    if not torch.cuda.is_available():
        raise PmnError("render.py runs on a ROCm GPU; none is visible")
    if args.scan_list:
        if not os.path.isfile(args.scan_list):
            raise PmnError("Invalid scan list file: {}".format(args.scan_list))
        scans = cloud_tool.read_scan_list(args.scan_list)
    else:
        scans = [""]
    from patchmatchnet_amd import render
    renderer = render.Renderer(device)
    cache = {}
    with torch.no_grad():
        for scan in scans:
            render_scan(args, scan, device, renderer, cache)
    return 0


if __name__ == "__main__":
    from patchmatchnet_amd import PmnError
    try:
        sys.exit(main(sys.argv[1:]))
    except PmnError as e:
        sys.exit("render.py: " + str(e))
