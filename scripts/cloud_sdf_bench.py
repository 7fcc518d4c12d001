"""Timings behind DESIGN.md section 32 (profiles/cloud_sdf_measure.log): the fused signed-distance kernel (pmn_cloud_sdf_blocks) beside
the unfused route built from what the library had before -- knn_distance with the lists at the sample positions, a torch gather and
torch sums -- and the whole of pointcloud.mesh_from_cloud with the extraction alone.

    python scripts/cloud_sdf_bench.py [--points 5000000] [--reps 5] [--log profiles/cloud_sdf_measure.log]

The cloud is scripts/clean_cloud_bench.py's sheet of --points points; its 2 % planted outliers are removed first with
statistical_outliers (the pipeline's order: clean_cloud.py, cloud_normals.py, mesh_cloud.py; left in, every outlier allocates 27 blocks
of its own), then estimate_normals orients it upwards.  The unfused route needs 12 k bytes per sample for its lists, so it runs on the
first --unfused_blocks blocks of the volume, and the fused kernel is timed on the same blocks beside it.  Every figure is the median of
--reps timed runs after one warm-up, measured with events on the stream."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clean_cloud_bench import sheet, timed  # noqa: E402


def sub_volume(TS, vol, nb):
    """A volume that holds the first ``nb`` blocks of ``vol`` (fresh planes)."""
    sub = TS.SparseTsdfVolume(vol.origin, vol.voxel, vol.dims, vol.trunc, vol.device, color=False)
    sub.blocks = vol.blocks[:nb].contiguous()
    shape = (nb, 8, 8, 8)
    sub.tsdf = torch.ones(shape, dtype=torch.float32, device=vol.device)
    sub.weight = torch.zeros(shape, dtype=torch.float32, device=vol.device)
    return sub


def block_positions(vol):
    """float32 [B * 512, 3] positions of the samples of a volume's blocks, and bool [B * 512]: inside the lattice."""
    nbx, nby, nbz = vol.nblocks
    b = vol.blocks.long()
    o = torch.arange(8, device=vol.device)
    i = ((b % nbx) * 8)[:, None, None, None] + o[None, None, None, :]
    j = ((b // nbx % nby) * 8)[:, None, None, None] + o[None, None, :, None]
    k = ((b // (nbx * nby)) * 8)[:, None, None, None] + o[None, :, None, None]
    i, j, k = torch.broadcast_tensors(i, j, k)
    idx = torch.stack([i, j, k], -1).reshape(-1, 3)
    inside = (idx < torch.tensor(vol.dims, device=vol.device)).all(1)
    org = torch.from_numpy(vol.origin).to(vol.device)
    return (org + idx.float() * np.float32(vol.voxel)).contiguous(), inside


def unfused(PC, vol, grid, nrm_sorted_by_original, pts, k, radius, boundary):
    """The planes by the route the library offered before: the lists at the sample positions, a gather, the sums in torch (float64;
    torch.sum's order, so the bits are not the kernel's)."""
    x, inside = block_positions(vol)
    _, d2, idx = PC.knn_distance(x, grid, k, radius, return_d2=True, return_index=True)
    live = idx >= 0
    at = idx.clamp_min(0)
    u = 1.0 - d2 / (radius * radius)
    w = (u * u) ** 2 * live
    s = (nrm_sorted_by_original[at].double() * (x.double()[:, None, :] - pts[at].double())).sum(2)
    sw = w.sum(1)
    f = (w * s).sum(1) / sw
    t2 = d2[:, 0] - s[:, 0] ** 2
    ok = inside & live[:, 0] & (sw > 0) & ~(t2 > boundary * boundary)
    vol.tsdf.view(-1).copy_(torch.where(ok, (f / vol.trunc).clamp(-1.0, 1.0).float(), torch.ones_like(f, dtype=torch.float32)))
    vol.weight.view(-1).copy_(torch.where(ok, live.sum(1).float(), torch.zeros_like(f, dtype=torch.float32)))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--unfused_blocks", type=int, default=8192)
    ap.add_argument("--log", type=str, default=os.path.join(ROOT, "profiles", "cloud_sdf_measure.log"))
    args = ap.parse_args()
    from patchmatchnet_amd import pointcloud as PC, tsdf as TS
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "w")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    n = args.points
    side = 1000.0 * (n / 5e6) ** 0.5  # 5 points per square unit
    raw = torch.from_numpy(sheet(n, 0, side)).cuda()
    pts = raw[PC.statistical_outliers(raw)[0]].contiguous()
    nrm = PC.estimate_normals(pts, 16, viewpoints=[[side / 2, side / 2, 1e6]])
    s = PC.cloud_spacing(pts)
    say(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {n} points over {side:.0f} x {side:.0f} units, "
        f"{int(pts.shape[0])} after statistical_outliers, normals from estimate_normals k=16; spacing s {s:.4f}; median [min, max] of "
        f"{args.reps} runs after one warm-up, milliseconds")
    v, f, _, _, info = PC.mesh_from_cloud(pts, nrm)
    say(f"mesh_from_cloud defaults: {info}")
    t = timed(lambda: PC.mesh_from_cloud(pts, nrm), args.reps)
    say(f"mesh_from_cloud as a whole (spacing, lattice, grid, blocks, kernel, extraction) {t[0]:9.2f} [{t[1]:.2f}, {t[2]:.2f}]")
    radius, boundary = info["radius"], info["boundary"]
    vol = TS.SparseTsdfVolume(info["origin"], info["voxel"], info["dims"], info["trunc"], "cuda", color=False)
    vol.allocate_points(pts, radius)
    grid = PC.build_grid(pts, radius)
    say(f"\n# cloud_sdf on the whole volume: {int(vol.blocks.shape[0])} blocks, {int(vol.blocks.shape[0]) * 512} samples")
    for k in (8, 16, 32):
        t = timed(lambda: PC.cloud_sdf(vol, grid, nrm, None, k=k, radius=radius, boundary=boundary), args.reps)
        say(f"k={k:2d}  cloud_sdf (gather of the normals through perm included) {t[0]:9.2f} [{t[1]:.2f}, {t[2]:.2f}]  observed "
            f"{int((vol.weight > 0).sum())} samples")
    PC.cloud_sdf(vol, grid, nrm, None, k=16, radius=radius, boundary=boundary)
    t = timed(lambda: vol.extract(min_weight=3.0), args.reps)
    say(f"extraction alone (k=16 planes, min_weight 3) {t[0]:9.2f} [{t[1]:.2f}, {t[2]:.2f}]")
    nb = min(args.unfused_blocks, int(vol.blocks.shape[0]))
    sub = sub_volume(TS, vol, nb)
    say(f"\n# fused beside unfused on the first {nb} blocks ({nb * 512} samples), same volume, same session")
    for k in (8, 16, 32):
        t_f = timed(lambda: PC.cloud_sdf(sub, grid, nrm, None, k=k, radius=radius, boundary=boundary), args.reps)
        fused_w = sub.weight.clone()
        try:
            t_u = timed(lambda: unfused(PC, sub, grid, nrm, pts, k, radius, boundary), args.reps)
            same = bool(torch.equal(fused_w, sub.weight))
            say(f"k={k:2d}  fused {t_f[0]:9.2f} [{t_f[1]:.2f}, {t_f[2]:.2f}]  unfused {t_u[0]:9.2f} [{t_u[1]:.2f}, {t_u[2]:.2f}]  "
                f"x{t_u[0] / t_f[0]:.2f} of fused; weight planes equal: {same}")
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            say(f"k={k:2d}  fused {t_f[0]:9.2f} [{t_f[1]:.2f}, {t_f[2]:.2f}]  unfused: out of memory")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
