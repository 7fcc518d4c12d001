#!/usr/bin/env python
"""Times the mesher's phases on a generated scene: 49 views of 1600 x 1200 (the rendered height field of
tests/synth.py seen from an arc), grids of 256^3, 512^3 and a DTU-like 600 x 600 x 500 box, with colour.

    python scripts/tsdf_bench.py [--grids 256,512,dtu] [--views 49] [--views_per_launch 1,4,8,16] [--repeats 5] [--log FILE]
                                 [--volume dense|sparse|both]

Per grid and batch size: device-event time of the integration of all views (median and spread over --repeats after one warm-up), the
bytes the phase must move computed from the shapes (24 B per sample read and written once per launch; the depth maps, masks and
images once per launch set) and the resulting GB/s against the 8.0 TB/s peak / 6.3 TB/s achievable HBM figures of the MI355X; then the
extraction (count, scan, emit) the same way, with the share of the torch scan.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python scripts/tsdf_bench.py --grids 512 --views_per_launch 8 --repeats 2` run.

--volume sparse times the block-sparse volume on the same scene and grids -- marking + dilation + list / table /
pool (allocate), the integration of the allocated blocks and the extraction over the pool -- and reports the blocks allocated, their
share of the virtual lattice and the pool's bytes; a grid may then be one the dense volume cannot hold (--grids 2048).  ``both`` runs
the dense figures first, in the same process, for the comparison."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12


def timed(fn, repeats):
    fn()  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms)), out


def time_integrate(say, args, vol, label, plane_bytes, share_of_peak, maps, sizes, cam21, masks, imgs):
    """Times vol.integrate of all views per batch size of --views_per_launch, from cleared planes.  ``plane_bytes`` = the bytes of the
    volume's planes (read and written once per launch); the maps, masks and images move once per launch set."""
    V = len(sizes)
    for b in (int(x) for x in args.views_per_launch.split(",")):
        def run():
            vol.tsdf.fill_(1)
            vol.weight.zero_()
            vol.rgb.zero_()
            vol.cweight.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            vol.integrate(maps, list(range(V)), sizes, cam21, masks, imgs, batch=b)
            e1.record()
            return e0, e1
        ms = []
        for r in range(args.repeats + 1):
            e0, e1 = run()
            torch.cuda.synchronize()
            if r:
                ms.append(e0.elapsed_time(e1))
        launches = -(-V // b)
        must = launches * 2 * plane_bytes + V * sizes[0][0] * sizes[0][1] * (4 + 1 + 3)
        med = float(np.median(ms))
        line = "  %s %2d views/launch (%2d launches): median %.2f ms (min %.2f, max %.2f, n=%d); must move %.1f GB -> %.0f GB/s" % (
            label, b, launches, med, min(ms), max(ms), len(ms), must / 1e9, must / med / 1e6)
        if share_of_peak:
            line += " = %.0f %% of the 6.3 TB/s achievable, %.0f %% of the 8.0 TB/s peak" % (
                100 * must / med / 1e-3 / HBM_ACHIEVABLE, 100 * must / med / 1e-3 / HBM_PEAK)
        say(line)


def sparse_grid(say, args, tsdf, dev, dims, origin, voxel, trunc, maps, sizes, cam21, masks, imgs):
    V = len(sizes)
    slots = list(range(V))
    vol = tsdf.SparseTsdfVolume(origin, voxel, dims, trunc, dev, color=True, max_blocks=2 ** 21)
    med, lo, hi, B = timed(lambda: vol.allocate(maps, slots, sizes, cam21, masks), args.repeats)
    nb = vol.nblocks[0] * vol.nblocks[1] * vol.nblocks[2]
    say("  sparse allocate (mark %d views, dilate, list, table, pool): median %.2f ms (min %.2f, max %.2f); %d blocks marked, %d "
        "allocated = %.3f %% of %d, pool %.3f GB with colour" % (V, med, lo, hi, vol.marked, B, 100.0 * B / nb, nb, 24 * 512 * B / 1e9))
    time_integrate(say, args, vol, "sparse integrate", 24 * 512 * B, False, maps, sizes, cam21, masks, imgs)
    med, lo, hi, out = timed(lambda: vol.extract(1.0, normals=True), args.repeats)
    say("  sparse extract: %d vertices, %d faces; median %.2f ms (min %.2f, max %.2f)" % (out[0].shape[0], out[1].shape[0], med, lo, hi))
    del out, vol
    torch.cuda.empty_cache()


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--grids", default="256,512,dtu")
    p.add_argument("--views", type=int, default=49)
    p.add_argument("--views_per_launch", default="1,4,8,16")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--log", default="")
    p.add_argument("--volume", default="dense", choices=("dense", "sparse", "both"))
    args = p.parse_args(argv)
    import synth
    from patchmatchnet_amd import ops, tsdf
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    V, H, W = args.views, args.height, args.width
    t0 = time.perf_counter()
    cams = synth.arc_cameras(V, H, W)
    images, intr, extr, depths = synth.render_scene(V, H, W, device=dev, cameras=cams, all_depths=True)
    maps = torch.stack([d.to(dev).reshape(-1) for d in depths]).contiguous()
    imgs = [(im[0].permute(1, 2, 0) * 255.0).round().to(torch.uint8).contiguous() for im in images]
    masks = [torch.ones((H, W), dtype=torch.uint8, device=dev) for _ in range(V)]
    cam21 = np.stack([tsdf.camera21(intr[0, v], extr[0, v]) for v in range(V)])
    say("scene: %d views of %d x %d rendered in %.1f s; device %s" % (V, W, H, time.perf_counter() - t0, torch.cuda.get_device_name(dev)))
    extent = np.array([330.0, 250.0, 140.0])  # the part of the height field every view sees, with the band around it
    centre = np.array([0.0, 0.0, 650.0])
    for g in args.grids.split(","):
        dims = (600, 600, 500) if g == "dtu" else (int(g),) * 3
        torch.cuda.empty_cache()
        voxel = float((extent / (np.array(dims) - 1)).max())
        origin = centre - voxel * (np.array(dims) - 1) / 2
        trunc = 4 * voxel
        n = dims[0] * dims[1] * dims[2]
        say("grid %d x %d x %d (%.2f GB with colour), voxel %.4f, trunc %.4f" % (dims + (24 * n / 1e9, voxel, trunc)))
        if args.volume != "dense":
            sparse_grid(say, args, tsdf, dev, dims, origin, voxel, trunc, maps, [(H, W)] * V, cam21, masks, imgs)
            if args.volume == "sparse":
                continue
        if n > 2 ** 31 - 1:
            say("  dense: the lattice does not fit a dense volume")
            continue
        vol = tsdf.TsdfVolume(origin, voxel, dims, trunc, dev, color=True)
        time_integrate(say, args, vol, "integrate", 24 * n, True, maps, [(H, W)] * V, cam21, masks, imgs)
        med, lo, hi, out = timed(lambda: vol.extract(1.0, normals=True), args.repeats)
        nv, nt = out[0].shape[0], out[1].shape[0]
        del out
        must = 2 * 8 * n + 2 * n + 2 * (2 + 8) * n + nv * (12 + 3 + 12) + nt * 12  # count reads tsdf+weight; emit again; scans
        say("  extract: %d vertices, %d faces; median %.2f ms (min %.2f, max %.2f); must move about %.1f GB -> %.0f GB/s" % (
            nv, nt, med, lo, hi, must / 1e9, must / med / 1e6))
        vm = torch.empty(vol.tsdf.shape, dtype=torch.uint8, device=dev)
        nt8 = torch.empty(vol.tsdf.shape, dtype=torch.uint8, device=dev)

        def scan():
            vc = ops._popcount_u8(vm)
            tot = torch.stack((vc.sum(dtype=torch.int64), nt8.sum(dtype=torch.int64))).tolist()
            return torch.cumsum(vc.reshape(-1), 0, dtype=torch.int32), torch.cumsum(nt8.reshape(-1), 0, dtype=torch.int32), tot
        vm.zero_()
        nt8.zero_()
        smed, slo, shi, _ = timed(scan, args.repeats)
        say("  of which the torch scan (popcount, two sums + one host read, two cumsums): median %.2f ms (min %.2f, max %.2f) = %.0f %% of "
            "the extraction" % (smed, slo, shi, 100 * smed / med))
        del vol, vm, nt8
        torch.cuda.empty_cache()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
