#!/usr/bin/env python
"""Times the mesh operations on the sphere meshes of section 15: the marching-tetrahedra surface of a sphere in
a 256^3 and a 512^3 volume (radius 101.4 / 256 of the side), with --floaters small blobs in the free space around it.

    python scripts/meshops_bench.py [--grids 256,512] [--floaters 48] [--spacing 0.5] [--repeats 5] [--log FILE]

Per grid: device-event time (median, min, max over --repeats after one warm-up) of the components pass alone (pmn_mesh_components:
three launches), of meshops.components (with the counting and its host read), of remove_components(keep_largest=1), and of
sample_surface at --spacing voxels with colours; the same labels on the host by scipy.sparse.csgraph.connected_components (wall
time, the device-to-host copy of the faces not included) if scipy is installed.  No time is a gate."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tsdf_bench import timed  # noqa: E402


def field(n, floaters, dev):
    s = n / 256.0
    ax = torch.arange(n, dtype=torch.float32, device=dev)
    k, j, i = torch.meshgrid(ax, ax, ax, indexing="ij")
    c = (127.3 * s, 128.1 * s, 126.7 * s)
    d = torch.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - 101.4 * s
    placed = 0
    for g in np.ndindex(6, 6, 6):  # blobs of radius 3 voxels on a 6 x 6 x 6 grid, where the sphere leaves room
        p = [(0.09 + 0.164 * q) * n for q in g]
        if placed < floaters and np.sqrt(sum((p[a] - c[a]) ** 2 for a in range(3))) > 101.4 * s + 12:
            d = torch.minimum(d, torch.sqrt((i - p[0]) ** 2 + (j - p[1]) ** 2 + (k - p[2]) ** 2) - 3.0)
            placed += 1
    return torch.clamp(d / 3.0, -1, 1).contiguous(), placed


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--grids", default="256,512")
    p.add_argument("--floaters", type=int, default=48)
    p.add_argument("--spacing", type=float, default=0.5, help="sample spacing in voxels")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--log", default="")
    args = p.parse_args(argv)
    from patchmatchnet_amd import meshops, ops
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device %s" % torch.cuda.get_device_name(dev))
    for n in (int(g) for g in args.grids.split(",")):
        t, placed = field(n, args.floaters, dev)
        v, f, _, _ = ops.mt_extract(t, torch.ones_like(t), (0.0, 0.0, 0.0), 1.0, normals=False)
        del t
        torch.cuda.empty_cache()
        nv, nt = v.shape[0], f.shape[0]
        col = torch.randint(0, 256, (nv, 3), dtype=torch.uint8, device=dev)
        say("grid %d^3: sphere + %d blobs -> %d vertices, %d faces" % (n, placed, nv, nt))
        med, lo, hi, (label, invalid) = timed(lambda: meshops._enqueue_components(f, nv), args.repeats)
        say("  pmn_mesh_components (init, hook, flatten): median %.3f ms (min %.3f, max %.3f) = %.2f ns per face" % (
            med, lo, hi, 1e6 * med / nt))
        med, lo, hi, (label, roots, count) = timed(lambda: meshops.components(f, nv), args.repeats)
        say("  components (+ roots, face counts, one host read): median %.3f ms (min %.3f, max %.3f); %d components, largest %d faces, "
            "smallest %d" % (med, lo, hi, roots.numel(), int(count.max()), int(count.min())))
        med, lo, hi, out = timed(lambda: meshops.remove_components(v, f, col, None, keep_largest=1), args.repeats)
        say("  remove_components(keep_largest=1): median %.3f ms (min %.3f, max %.3f); kept %d vertices, %d faces" % (
            med, lo, hi, out[0].shape[0], out[1].shape[0]))
        med, lo, hi, (pts, face, pc) = timed(lambda: meshops.sample_surface(out[0], out[1], spacing=args.spacing, seed=1, colors=out[2]),
                                             args.repeats)
        say("  sample_surface(spacing %.3g voxel, colours): median %.3f ms (min %.3f, max %.3f); %d samples = %.2f ns per sample" % (
            args.spacing, med, lo, hi, pts.shape[0], 1e6 * med / max(pts.shape[0], 1)))
        try:
            import scipy.sparse as sp
            from scipy.sparse.csgraph import connected_components
        except ImportError:
            say("  host components: scipy is not installed, not measured")
        else:
            fh = f.cpu().numpy().astype(np.int64)
            ms = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                e = np.concatenate((fh[:, [0, 1]], fh[:, [1, 2]]))
                g = sp.coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(nv, nv)).tocsr()
                ncomp, lab = connected_components(g, directed=False)
                ms.append(1e3 * (time.perf_counter() - t0))
            first = np.full(ncomp, nv, np.int64)
            np.minimum.at(first, lab, np.arange(nv))
            same = bool(np.array_equal(first[lab], label.cpu().numpy()))
            say("  host scipy.sparse.csgraph.connected_components (graph build + labels): median %.1f ms (min %.1f, max %.1f); "
                "%d components, partition equal to the device's: %s" % (float(np.median(ms)), min(ms), max(ms),
                                                                       ncomp, same))
        del v, f, col, out, pts, face, pc, label
        torch.cuda.empty_cache()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
