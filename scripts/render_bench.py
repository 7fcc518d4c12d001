#!/usr/bin/env python
"""Times the renderer: the 600 x 600 x 500 mesh of scripts/tsdf_bench.py and a 30 M-point cloud drawn into 49
views of 1600 x 1200, the coarse icosphere with and without the worklist kernel, and a sweep of max_box over finer icospheres.

    python scripts/render_bench.py [--views 49] [--repeats 5] [--points 30000000] [--grid 600,600,500] [--log FILE]

Per model: device-event time of all views (keys cleared, drawn, resolved), median of --repeats after one warm-up with min..max, and per
view the bytes that must move (vertices + faces or points once, the key plane written by the clear and read-modify-written by the draw
and read by the resolve, the output planes once) over the 6.3 TB/s achievable HBM figure of the MI355X as the floor."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_ACHIEVABLE = 6.3e12


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=49)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--points", type=int, default=30000000)
    p.add_argument("--grid", default="600,600,500")
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--log", default="")
    args = p.parse_args(argv)
    import render_ref as RR
    import synth
    from patchmatchnet_amd import render, tsdf
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    V, H, W = args.views, args.height, args.width
    cams = synth.arc_cameras(V, H, W)
    images, intr, extr, depths = synth.render_scene(V, H, W, device=dev, cameras=cams, all_depths=True)
    maps = torch.stack([d.to(dev).reshape(-1) for d in depths]).contiguous()
    imgs = [(im[0].permute(1, 2, 0) * 255.0).round().to(torch.uint8).contiguous() for im in images]
    cam21 = np.stack([tsdf.camera21(intr[0, v], extr[0, v]) for v in range(V)])
    dims = tuple(int(x) for x in args.grid.split(","))
    extent, centre = np.array([330.0, 250.0, 140.0]), np.array([0.0, 0.0, 650.0])
    voxel = float((extent / (np.array(dims) - 1)).max())
    vol = tsdf.TsdfVolume(centre - voxel * (np.array(dims) - 1) / 2, voxel, dims, 4 * voxel, dev, color=True)
    vol.integrate(maps, list(range(V)), [(H, W)] * V, cam21, None, imgs, batch=8)
    vert, faces, col, nrm = vol.extract(1.0, normals=True)
    del vol, maps, imgs, images
    torch.cuda.empty_cache()
    say("device %s; %d views of %d x %d; mesh of the %d x %d x %d grid: %d vertices, %d faces" % (
        torch.cuda.get_device_name(dev), V, W, H, dims[0], dims[1], dims[2], vert.shape[0], faces.shape[0]))
    r = render.Renderer(dev)
    planes = H * W * (8 + 8 + 8 + 8 + 4 + 4 + 3)  # keys: cleared, read-modify-written, read; depth, index, rgb

    def report(name, ms, must, extra=""):
        floor = must / HBM_ACHIEVABLE * 1e3
        say("  %s: median %.3f ms per view (min %.3f, max %.3f over %d repeats of %d views); must move %.1f MB per view -> floor %.3f ms, "
            "%.0f %% of it reached%s" % (name, ms[0] / V, ms[1] / V, ms[2] / V, args.repeats, V, must / 1e6, floor, 100 * floor / (ms[0] / V),
                                         extra))

    def mesh_views(max_box=0):
        for v in range(V):
            out = r.render_mesh(vert, faces, intr[0, v], extr[0, v], H, W, col, nrm, max_box=max_box)
        return out
    for cap in (16, 64, 256, 1024):
        ms = timed(lambda: mesh_views(cap), args.repeats)
        large = int(mesh_views(cap)[4][3])
        report("mesh, max_box %4d" % cap, ms, vert.shape[0] * (12 + 3 + 12) + faces.shape[0] * 12 + planes, "; %d large triangles in the last view" % large)
    g = torch.Generator(device=dev).manual_seed(0)
    pick = torch.randint(0, faces.shape[0], (args.points,), generator=g, device=dev)
    bary = torch.rand((args.points, 3), generator=g, device=dev)
    bary = bary / bary.sum(1, keepdim=True)
    pts = (vert[faces[pick].long()] * bary[:, :, None]).sum(1).contiguous()
    pcol = col[faces[pick, 0].long()].contiguous()
    del pick, bary
    for kw in ({}, {"radius_px": 1.0}, {"radius_world": 0.3}):
        def cloud_views():
            for v in range(V):
                r.render_points(pts, intr[0, v], extr[0, v], H, W, pcol, None, **kw)
        report("cloud of %d points, %s" % (args.points, kw or "nearest pixel"), timed(cloud_views, args.repeats), args.points * 15 + planes)
    # the coarse icosphere close to the camera: with the worklist kernel and in the one-kernel form (no triangle is 'large')
    iv, ifc = RR.icosphere(1, RR.TARGET, 1.2)
    K, E, _ = RR.case_camera(H, W, 2.4)
    iv, ifc = torch.from_numpy(iv).to(dev), torch.from_numpy(ifc).to(dev)
    for name, cap in (("two kernels (max_box 64)", 64), ("one kernel (max_box 2^40)", 1 << 40)):
        def ico():
            for _ in range(V):
                r.render_mesh(iv, ifc, K, E, H, W, max_box=cap)
        ms = timed(ico, args.repeats)
        say("  icosphere of %d faces filling the frame, %s: median %.3f ms per view (min %.3f, max %.3f)" % (
            ifc.shape[0], name, ms[0] / V, ms[1] / V, ms[2] / V))
    # the cap: icospheres whose triangles have bounding boxes of tens to thousands of pixels, one thread per triangle up to max_box
    for level in (6, 5, 4, 3):
        sv, sf = RR.icosphere(level, RR.TARGET, 1.0)
        K, E, _ = RR.case_camera(H, W, 4.0)
        sv, sf = torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(dev)
        row = []
        for cap in (16, 64, 256, 1024, 4096):
            def sphere():
                for _ in range(V):
                    out = r.render_mesh(sv, sf, K, E, H, W, max_box=cap)
                return out
            ms = timed(sphere, args.repeats)
            row.append("max_box %d: %.3f ms (%d large)" % (cap, ms[0] / V, int(sphere()[4][3])))
        say("  icosphere level %d (%d faces, radius 1 at distance 4), median per view: %s" % (level, sf.shape[0], "; ".join(row)))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
