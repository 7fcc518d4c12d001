#!/usr/bin/env python
"""pmn_undistort_image on one 6000 x 4000 x 3 picture (24 Mpixel, a full-frame camera), for an OPENCV and an OPENCV_FISHEYE camera.

    python scripts/undistort_bench.py [--launches 20] [--rounds 5]

Per camera: the undistorted camera (host, timed once), a warm-up, then ``rounds`` windows of ``launches`` back-to-back launches
between device events.  Prints per-launch milliseconds (median and minimum window) and GB/s counted as (source bytes + destination
bytes) / time -- the bytes the algorithm has to move; it is also given as a share of the 6.29 TB/s a float4 copy reaches on MI355X
(VERDICT "what's weak" 3).  One RESULT line of JSON per camera.  No gate hangs on these numbers (profiles/undistort_bench.log)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_TBS = 6.29
W, H = 6000, 4000
CAMERAS = {
    "OPENCV": (4300.0, 4310.0, 3011.0, 1989.0, -0.11, 0.035, 0.0008, -0.0005),
    "OPENCV_FISHEYE": (2900.0, 2905.0, 3004.0, 2007.0, -0.03, 0.004, -0.0006, 0.00005),
}


def main(argv=None) -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--device", type=str, default="cuda:0")
    a = p.parse_args(argv)
    if a.launches < 20:
        p.error("--launches must be at least 20")
    from patchmatchnet_amd import colmap, ops, undistort
    assert torch.cuda.is_available(), "this benchmark needs a ROCm device (nothing is measured without one)"
    dev = torch.device(a.device)
    g = torch.Generator(device="cpu").manual_seed(0)
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    for model, params in CAMERAS.items():
        cam = colmap.Camera(1, model, W, H, params)
        t = time.perf_counter()
        dst = undistort.undistorted_camera(cam)
        host_ms = (time.perf_counter() - t) * 1e3
        out = torch.empty((dst.height, dst.width, 3), dtype=torch.uint8, device=dev)
        for _ in range(3):
            ops.undistort_image(img, cam, dst, out=out)
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(a.rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(a.launches):
                ops.undistort_image(img, cam, dst, out=out)
            stop.record()
            stop.synchronize()
            ms.append(start.elapsed_time(stop) / a.launches)
        nbytes = img.numel() + out.numel()
        med, best = float(np.median(ms)), float(min(ms))
        res = {"kernel": "pmn_undistort_image", "model": model, "src": [H, W, 3], "dst": [dst.height, dst.width, 3],
               "launches_per_window": a.launches, "windows": a.rounds, "ms_median": round(med, 4), "ms_min": round(best, 4),
               "bytes_src_plus_dst": nbytes, "GBps_median": round(nbytes / med / 1e6, 1),
               "share_of_6.29TBps_copy": round(nbytes / med / 1e6 / (HBM_COPY_TBS * 1e3), 4),
               "byte_floor_ms_at_6.29TBps": round(nbytes / (HBM_COPY_TBS * 1e9), 4), "undistorted_camera_host_ms": round(host_ms, 1),
               "valid_fraction": round(float(ops.undistort_image(img, cam, dst, want_valid=True)[1].float().mean()), 4)}
        print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
