#!/usr/bin/env python
"""Cost of validation against ground truth (train.py --mode test): depth-maps/s of the launch-plan forward alone against the same
forward plus pmn_depth_metrics and the rows' download (patchmatchnet_amd/validate.py, Validator hip_graph=1), at 640x512, batch 12,
5 source views.  The batches are read once into pinned host memory, so the decode is out of both numbers; each leg replays all of
them ``reps`` times and is timed from the first upload to a final synchronisation.  Prints one JSON line.

    python scripts/validate_bench.py [reps=5] [n_views=24]

Under ``rocprofv3 --kernel-trace --stats -- python scripts/validate_bench.py 2`` the kernel table gives depth_metrics_kernel's time.
"""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402
import train  # noqa: E402
from patchmatchnet_amd import data_io  # noqa: E402
from patchmatchnet_amd import validate as V  # noqa: E402
from patchmatchnet_amd.graph import PlannedForward  # noqa: E402
from patchmatchnet_amd.mvs import MVSDataset  # noqa: E402

pos = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(pos[0]) if len(pos) > 0 else 5
n_views = int(pos[1]) if len(pos) > 1 else 24
H, W, B, SRC = 512, 640, 12, 5

base = tempfile.mkdtemp(prefix="pmn_validate_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    synth.write_scene_scan(base, "scan1", n_views, H, W, n_src=SRC, seed=1, device="cuda")
    _, _, _, depths = synth.render_scene(n_views, H, W, seed=1, device="cuda", cameras=synth.arc_cameras(n_views, H, W), all_depths=True)
    os.makedirs(os.path.join(base, "scan1", "depth_gt"))
    for v, d in enumerate(depths):
        data_io.save_pfm(os.path.join(base, "scan1", "depth_gt", "{:0>8}.pfm".format(v)), d.cpu().numpy().astype(np.float32))
    with open(os.path.join(base, "list.txt"), "w") as f:
        f.write("scan1\n")
    ds = MVSDataset(base, num_views=SRC, max_dim=640, scan_list=os.path.join(base, "list.txt"), load_depth_gt=True)
    batches = list(DataLoader(ds, B, shuffle=False, num_workers=4, pin_memory=True))
finally:
    shutil.rmtree(base, ignore_errors=True)

dev = torch.device("cuda")
model = train.load_model(train.build_parser().parse_args(["--mode", "test", "--checkpoint_path",
                                                         os.path.join(ROOT, "tests", "golden", "params_000007.npz")]), dev)
planned = PlannedForward(model)
val = V.Validator(model, V.stage_iterations(model), hip_graph=1, depth=4)


def up(t):
    return t.to(dev, non_blocking=True)


def forward_leg():
    with torch.no_grad():
        for b in batches:
            planned([up(im) for im in b["images"]], up(b["intrinsics"]), up(b["extrinsics"]), up(b["depth_min"]), up(b["depth_max"]))


def validation_leg():
    for b in batches:
        val.submit(b)
    val.drain()


out = {"H": H, "W": W, "batch": B, "source_views": SRC, "samples": len(ds), "reps": reps}
for name, leg in (("forward", forward_leg), ("validation", validation_leg)):
    leg()  # plan recording, allocator warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        leg()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    out[name + "_maps_per_s"] = round(len(ds) / float(np.median(times)), 1)
out["validation_over_forward"] = round(out["validation_maps_per_s"] / out["forward_maps_per_s"], 4)
print(json.dumps(out))
