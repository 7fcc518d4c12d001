"""Timings behind DESIGN.md section 34 (profiles/segment_plane_measure.log): pmn_plane_score at 1024 hypotheses, pmn_plane_inliers and
segment_plane as a whole, beside the plain torch route for the scores -- chunked float64 planes @ points^T, compare, sum -- which is the
yardstick: what one would write without the kernel.

    python scripts/segment_plane_bench.py [--points 5000000] [--hypotheses 1024] [--reps 5] [--log profiles/segment_plane_measure.log]

The cloud is the one the other cloud benches generate: a noisy sheet of --points points with 2 % planted outliers up to 200 units off.
Every GPU figure is the median of --reps timed runs after one warm-up, measured with events on the stream, in one process.  The torch
route's counts may differ from the kernel's for points within rounding of the threshold (a matrix product does not keep the written
order of the sums); the log says in how many hypotheses."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clean_cloud_bench import sheet, timed  # noqa: E402  (the same cloud, the same clock)

TORCH_CHUNK = 1 << 18  # points per product: 1024 x 2^18 float64 = 2 GiB of residuals at a time


def torch_scores(p64, planes, threshold):
    counts = torch.zeros(planes.shape[0], dtype=torch.int64, device=planes.device)
    A, d = planes[:, :3].contiguous(), planes[:, 3:]
    for s in range(0, p64.shape[0], TORCH_CHUNK):
        r = A @ p64[s:s + TORCH_CHUNK].T + d
        counts += (r.abs_() <= threshold).sum(1)
    return counts


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=5_000_000)
    ap.add_argument("--hypotheses", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "segment_plane_measure.log"))
    args = ap.parse_args()
    from patchmatchnet_amd import pointcloud as PC
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "w")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    n, H = args.points, args.hypotheses
    side = 1000.0 * (n / 5e6) ** 0.5  # 5 points per square unit
    host = sheet(n, 0, side)
    pts = torch.from_numpy(host).cuda()
    say(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {n} points over {side:.0f} x {side:.0f} units, 2 % outliers; "
        f"{H} hypotheses; median [min, max] of {args.reps} runs after one warm-up, milliseconds")
    spacing = PC.cloud_spacing(pts)
    thr = PC.PLANE_THRESHOLD_SPACINGS * spacing
    say(f"cloud_spacing {spacing:.4f}, threshold {thr:.4f}")
    rng = np.random.Generator(np.random.PCG64(0))
    trip = rng.integers(0, n, size=(H, 3))
    planes_host = PC.plane_hypotheses(host[trip], trip)
    planes = torch.from_numpy(planes_host).cuda()
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, device="cuda"), dim=1).contiguous()
    counts = PC.plane_score(pts, planes, thr)
    best = int(counts.argmax())
    say(f"{int(np.isnan(planes_host).any(1).sum())} invalid hypotheses; best count {int(counts[best])} (hypothesis {best})")

    def row(name, t, base=None):
        say(f"{name:52s} {t[0]:9.2f} [{t[1]:.2f}, {t[2]:.2f}]" + (f"  x{t[0] / base:.2f} of pmn_plane_score" if base else ""))

    base = timed(lambda: PC.plane_score(pts, planes, thr), args.reps)
    row(f"pmn_plane_score, H = {H}", base)
    say(f"{'':52s} {7.0 * n * H / (base[0] * 1e-3) / 1e12:9.2f} T float64 operations per second at 7 per (point, hypothesis)")
    row(f"pmn_plane_score, H = {H}, normals, min_cos 0.9", timed(lambda: PC.plane_score(pts, planes, thr, nrm, None, 0.9), args.reps),
        base[0])
    active = torch.rand(n, device="cuda") < 0.5
    row(f"pmn_plane_score, H = {H}, half the points active", timed(lambda: PC.plane_score(pts, planes, thr, None, active), args.reps),
        base[0])
    centre, extent = PC.plane_frame(pts)
    scratch = torch.empty(PC._lib.plane_scratch(n), dtype=torch.int64, device="cuda")
    row("pmn_plane_inliers (mask + ten exact sums)",
        timed(lambda: PC.plane_inliers(pts, planes_host[best], thr, centre=centre, extent=extent, scratch=scratch), args.reps))
    row("plane_frame (bounding box of the active points)", timed(lambda: PC.plane_frame(pts), args.reps))
    row(f"segment_plane, {H} hypotheses, 3 refits", timed(lambda: PC.segment_plane(pts, thr, hypotheses=H, seed=0), args.reps), base[0])
    res = PC.segment_plane(pts, thr, hypotheses=H, seed=0)
    say(f"{'':52s} plane {res['plane'].tolist()}, {res['count']} inliers, rmse {res['rmse']:.4f}, {res['refits']} refits")
    p64 = pts.double()
    t = timed(lambda: torch_scores(p64, planes, thr), args.reps)
    row("torch: chunked float64 planes @ points^T, <=, sum", t, base[0])
    differ = int((torch_scores(p64, planes, thr) != counts.long()).sum())
    say(f"{'':52s} {differ} of {H} counts differ from the kernel's (a matrix product does not keep the written order)")
    say(f"pmn_plane_score is x{t[0] / base[0]:.2f} the speed of the torch route" if t[0] > base[0] else
        f"pmn_plane_score is NOT faster than the torch route: x{t[0] / base[0]:.2f}")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
