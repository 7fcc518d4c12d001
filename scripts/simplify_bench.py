#!/usr/bin/env python
"""Times meshops.simplify_clustering on the sphere meshes of scripts/meshops_bench.py and measures what it costs.

    python scripts/simplify_bench.py [--grids 256,512] [--cells 2,4,8] [--repeats 3] [--log FILE]

Per grid and cell (in voxels): faces in and out, the wall time of each stage between device synchronisations (sort, means, remap,
placement, compaction; the median over --repeats after one warm-up), and the mean and the largest exact distance
(meshops.point_mesh_distance) from the input's vertices to the output surface and from the output's vertices to the input surface,
for both placements.  No time is a gate."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from meshops_bench import field  # noqa: E402

STAGES = ("sort", "means", "remap", "placement", "compaction")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--grids", default="256,512")
    p.add_argument("--cells", default="2,4,8", help="cell sizes in voxels")
    p.add_argument("--repeats", type=int, default=3)
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
        t, _ = field(n, 0, dev)
        v, f, _, nrm = ops.mt_extract(t, torch.ones_like(t), (0.0, 0.0, 0.0), 1.0, normals=True)
        del t
        torch.cuda.empty_cache()
        col = torch.randint(0, 256, (v.shape[0], 3), dtype=torch.uint8, device=dev)
        say("grid %d^3: sphere -> %d vertices, %d faces" % (n, v.shape[0], f.shape[0]))
        grid_in = meshops.build_face_grid(v, f)
        for cell in (float(c) for c in args.cells.split(",")):
            for placement in ("quadric", "mean"):
                runs = []
                for k in range(args.repeats + 1):
                    tm = {}
                    out = meshops.simplify_clustering(v, f, cell, colors=col, normals=nrm, placement=placement, timings=tm)
                    if k:
                        runs.append(tm)
                med = {s: 1e3 * float(np.median([r.get(s, 0.0) for r in runs])) for s in STAGES}
                ov, of = out[0], out[1]
                a = meshops.point_mesh_distance(v, meshops.build_face_grid(ov, of), float(n))
                b = meshops.point_mesh_distance(ov, grid_in, float(n))
                say("  cell %g voxels, %s: %d -> %d faces, %d -> %d vertices; %s; total %.2f ms; input vertices -> output: mean %.4f, "
                    "max %.4f; output vertices -> input: mean %.4f, max %.4f (bound %.4f)" % (
                        cell, placement, f.shape[0], of.shape[0], v.shape[0], ov.shape[0],
                        ", ".join("%s %.2f ms" % (s, med[s]) for s in STAGES), sum(med.values()), float(a.mean()), float(a.max()),
                        float(b.mean()), float(b.max()), 3 ** 0.5 * cell))
                del out, ov, of, a, b
        del v, f, col, nrm, grid_in
        torch.cuda.empty_cache()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
