#!/usr/bin/env python
"""What --fuse_merge 1 costs and saves, two measurements:

  python scripts/fuse_merge_measure.py kernel [H=1200 W=1600 sources=10]
      launch-to-launch device time (events around runs of back-to-back launches, the two entry points alternating) of
      pmn_fuse_view and pmn_fuse_view_merged for one reference view against ``sources`` source views of a consistent scene
  python scripts/fuse_merge_measure.py eval [views=10 H=480 W=640]
      eval.py --output_type both in fresh processes, --fuse_merge 0 and 1 alternating, twice each, on the generated scan of
      tests/test_eval_gpu.py's largest case: points written, bytes of fused.ply, depth-maps/s of the "both stages" line
"""
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import synth  # noqa: E402
from patchmatchnet_amd import fusion, ops  # noqa: E402


def kernel(H=1200, W=1600, n_src=10):
    V = n_src + 1
    _, intr, extr, depths = synth.render_scene(V, H, W, seed=0, device="cuda", all_depths=True)
    g = torch.Generator().manual_seed(0)
    maps = torch.stack([torch.stack((d.cuda() + 0.02 * torch.randn(H, W, generator=g).cuda(),
                                     (0.4 + 0.6 * torch.rand(H, W, generator=g)).cuda())) for d in depths]).contiguous()
    K, E = intr[0].astype(np.float32), extr[0].astype(np.float32)
    ref = V // 2
    srcs = [v for v in range(V) if v != ref]
    mats = torch.from_numpy(fusion.camera_block(K[ref], E[ref], [(K[s], E[s]) for s in srcs])).cuda()
    thr = (1.0, 0.01, 3, 0.5)
    claimed = torch.zeros((V, H * W), dtype=torch.uint8, device="cuda")
    runs = {"pmn_fuse_view": lambda: ops.fuse_view(maps, ref, srcs, mats, *thr),
            "pmn_fuse_view_merged": lambda: ops.fuse_view_merged(maps, ref, srcs, mats, *thr, claimed)}
    m0, x0, _, _ = runs["pmn_fuse_view"]()
    m1, x1, emit = runs["pmn_fuse_view_merged"]()
    torch.cuda.synchronize()
    assert torch.equal(m0, m1) and x0.cpu().numpy().tobytes() == x1.cpu().numpy().tobytes()
    print("MEASURE kernel: %dx%d, %d sources; final %.3f of the pixels, %d claims set in %d source maps"
          % (W, H, n_src, float(m1[2].float().mean()), int(claimed.sum()), n_src))
    for f in runs.values():  # warm up (the output tensors come from the caching allocator from here on)
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    reps, per = 10, 20
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for name, f in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per):
                f()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / per)
    for name, v in ms.items():
        print("MEASURE kernel: %-22s median %.4f ms per launch (min %.4f, max %.4f over %d runs of %d launches)"
              % (name, float(np.median(v)), min(v), max(v), reps, per))


def evaluate(n_views=10, H=480, W=640):
    base = "/dev/shm/pmn_fuse_merge_measure" if os.path.isdir("/dev/shm") else "/tmp/pmn_fuse_merge_measure"
    shutil.rmtree(base, ignore_errors=True)
    data = os.path.join(base, "data")
    synth.write_scene_scan(data, "scan1", n_views, H, W, n_src=6, seed=2, device="cuda")
    with open(os.path.join(data, "list.txt"), "w") as f:
        f.write("scan1\n")
    common = [sys.executable, os.path.join(ROOT, "eval.py"), "--input_folder", data, "--checkpoint_path",
              os.path.join(ROOT, "tests", "golden", "params_000007.npz"), "--scan_list", os.path.join(data, "list.txt"), "--num_views", "4",
              "--output_type", "both", "--sample_seed", "9", "--geo_mask_thres", "2", "--photo_thres", "0.3"]
    print("MEASURE eval: " + " ".join(common[1:]) + " --fuse_merge 0|1")
    for rep in range(2):
        for flag in ("0", "1"):
            out = os.path.join(base, "out%s_%d" % (flag, rep))
            log = subprocess.run(common + ["--output_folder", out, "--fuse_merge", flag], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                 text=True, timeout=600, check=True).stdout
            ply = os.path.join(out, "scan1", "fused.ply")
            head = open(ply, "rb").read(400)
            points = int(re.search(rb"element vertex (\d+)", head).group(1))
            rate = re.search(r"both stages: .*", log).group(0)
            merged = re.search(r"fusion stage: --fuse_merge 1 .*", log)
            print("MEASURE eval: rep %d --fuse_merge %s: %d points, fused.ply %d bytes; %s%s"
                  % (rep, flag, points, os.path.getsize(ply), rate, "; " + merged.group(0) if merged else ""))
    shutil.rmtree(base, ignore_errors=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    nums = [int(x) for x in sys.argv[2:]]
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: these are measurements, there is nothing to fall back to")
    kernel(*nums) if what == "kernel" else evaluate(*nums)
