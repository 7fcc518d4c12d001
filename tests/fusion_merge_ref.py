"""CPU restatement of merged fusion (pmn_fuse_view_merged, csrc/fusion.hip) -- TEST INFRASTRUCTURE, a helper of
tests/test_fusion_merge_ref.py (CPU) and tests/test_fusion_merge_gpu.py, not a test module.

The per-view arithmetic (photo / geo / final masks, averaged depth, world points, colours) is oracle.fusion_oracle's; on top of it,
in numpy, the rule: a reference view emits its final pixels that no earlier view has claimed, and every final pixel claims, in each
source view that agreed with it, the pixel nearest to its forward projection -- if that pixel is inside the source map and the source
view's own depth there agrees with the point's depth in that camera."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

import synth
from oracle import fusion_oracle as FO

TIE_WINDOW = 1e-4  # a claim whose x or y lies this close to k + 0.5 could round to either neighbour


def consistent_scene(V: int, H: int, W: int, sizes=None, seed: int = 0) -> Dict[int, Dict]:
    """Geometrically consistent maps: every view's ground-truth depth of synth.render_scene's analytic surface in its own camera
    (+ 0.02 noise), so that most pixels pass the consistency test against most other views; ``sizes[v]`` = (h, w) renders view v at
    its own size with its intrinsics scaled.  View ids are 3, 5, 7, ..."""
    rng = np.random.default_rng(seed)
    views = {}
    for v in range(V):
        h, w = (H, W) if sizes is None else sizes[v]
        imgs, intr, extr, depths = synth.render_scene(V, h, w, seed=seed, all_depths=True)
        d = depths[v].numpy() + rng.standard_normal((h, w)).astype(np.float32) * 0.02
        c = (0.4 + 0.6 * rng.random((h, w))).astype(np.float32)
        views[v * 2 + 3] = dict(depth=d.astype(np.float32), confidence=c, intrinsics=intr[0, v].astype(np.float32),
                                extrinsics=extr[0, v].astype(np.float32), image=imgs[v][0].permute(1, 2, 0).numpy())
    return views


def forward_projection(ref: Dict, src: Dict):
    """The first half of oracle.fusion_oracle.reproject_with_depth (reference eval.py:96-127), kept apart because the claims need
    it: float32 (x_src, y_src) [H,W] -- the coordinates that feed the bilinear sample -- and the reference points' float32 depth in
    the source camera."""
    depth_ref = np.asarray(ref["depth"], np.float32)
    height, width = depth_ref.shape
    x_ref, y_ref = np.meshgrid(np.arange(0, width), np.arange(0, height))
    x_ref, y_ref = x_ref.reshape([-1]), y_ref.reshape([-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        xyz_ref = np.matmul(np.linalg.inv(ref["intrinsics"]), np.vstack((x_ref, y_ref, np.ones_like(x_ref))) * depth_ref.reshape([-1]))
        xyz_src = np.matmul(np.matmul(src["extrinsics"], np.linalg.inv(ref["extrinsics"])), np.vstack((xyz_ref, np.ones_like(x_ref))))[:3]
        k_xyz_src = np.matmul(src["intrinsics"], xyz_src)
        xy_src = k_xyz_src[:2] / k_xyz_src[2:3]
    shape = [height, width]
    return (xy_src[0].reshape(shape).astype(np.float32), xy_src[1].reshape(shape).astype(np.float32),
            xyz_src[2].reshape(shape).astype(np.float32))


def view_claims(ref: Dict, srcs: Sequence[Dict], final: np.ndarray, geo_pixel_thres: float, geo_depth_thres: float):
    """The claims one reference view lays: [(iy, ix) integer arrays per source view], and how many of them sit in the tie window."""
    out, ties = [], 0
    ref_depth = np.asarray(ref["depth"], np.float32)
    for s in srcs:
        agreed, _ = FO.check_geometric_consistency(ref_depth, ref["intrinsics"], ref["extrinsics"], np.asarray(s["depth"], np.float32),
                                                   s["intrinsics"], s["extrinsics"], geo_pixel_thres, geo_depth_thres)
        xs, ys, z = forward_projection(ref, s)
        d_s = np.asarray(s["depth"], np.float32)
        h, w = d_s.shape
        with np.errstate(invalid="ignore", divide="ignore"):
            fx, fy = np.rint(xs), np.rint(ys)  # to nearest, ties to even: rintf
            inside = (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)  # NaN and infinities fail
            ix = np.where(inside, fx, 0).astype(np.int64)
            iy = np.where(inside, fy, 0).astype(np.int64)
            guard = np.abs(d_s[iy, ix] - z) / z < np.float32(geo_depth_thres)  # float32 throughout
        claim = final & agreed & inside & guard
        out.append((iy[claim], ix[claim]))
        fr = np.stack((xs[claim], ys[claim])).astype(np.float64)
        ties += int(np.count_nonzero((np.abs(fr - np.floor(fr) - 0.5) < TIE_WINDOW).any(0)))
    return out, ties


def merge_scan(views: Dict[int, Dict], pairs: List[Tuple[int, List[int]]], geo_pixel_thres: float, geo_depth_thres: float,
               geo_mask_thres: int, photo_thres: float):
    """Merged fusion of a scan in ``pairs`` order -> dict(emit {ref: bool [h,w]}, final {ref: bool [h,w]}, vertices [M,3] float32,
    colors [M,3] uint8 (the merged cloud), full_vertices [N,3] (today's cloud), claims, ties)."""
    claimed = {v: np.zeros(np.shape(views[v]["depth"]), bool) for v in views}
    emit, finals, verts, cols, full = {}, {}, [], [], []
    n_claims = n_ties = 0
    for ref, srcs in pairs:
        assert ref not in srcs
        r = FO.fuse_view(views[ref], [views[s] for s in srcs], geo_pixel_thres, geo_depth_thres, geo_mask_thres, photo_thres)
        final = r["final"]
        emit[ref] = final & ~claimed[ref]
        finals[ref] = final
        keep = emit[ref][final]  # the oracle's vertex list is the final pixels in row-major order
        verts.append(r["vertices"][keep])
        cols.append(r["colors"][keep])
        full.append(r["vertices"])
        claims, ties = view_claims(views[ref], [views[s] for s in srcs], final, geo_pixel_thres, geo_depth_thres)
        for s, (iy, ix) in zip(srcs, claims):
            claimed[s][iy, ix] = True
            n_claims += len(iy)
        n_ties += ties
    return dict(emit=emit, final=finals, vertices=np.concatenate(verts, 0), colors=np.concatenate(cols, 0),
                full_vertices=np.concatenate(full, 0), first_view_vertices=full[0], claims=n_claims, ties=n_ties)


def nearest_distance(a: np.ndarray, b: np.ndarray, exclude_self: bool = False, device: str = "cpu") -> np.ndarray:
    """Distance from every point of ``a`` [n,3] to its nearest point of ``b`` [m,3] (brute force in float64, in row blocks);
    ``exclude_self``: a is b and a point is not its own neighbour."""
    centre = np.asarray(b, np.float64).mean(0)
    A = torch.from_numpy(np.asarray(a, np.float64) - centre).to(device)
    B = torch.from_numpy(np.asarray(b, np.float64) - centre).to(device)
    b2 = (B * B).sum(1)
    out = torch.empty(len(A), dtype=torch.float64, device=device)
    step = 2048
    for i in range(0, len(A), step):
        blk = A[i:i + step]
        d2 = torch.addmm(b2[None, :].expand(len(blk), -1), blk, B.T, alpha=-2.0)  # |b|^2 - 2 a.b; |a|^2 joins after the minimum
        if exclude_self:
            k = torch.arange(len(blk), device=device)
            d2[k, k + i] = float("inf")
        out[i:i + step] = (d2.min(1).values + (blk * blk).sum(1)).clamp_min(0.0).sqrt()
    return out.cpu().numpy()


def gap_over_spacing(full: np.ndarray, merged: np.ndarray, first_view: np.ndarray, device: str = "cpu"):
    """(largest distance from a point of the full cloud to its nearest merged point, median nearest-neighbour spacing inside the
    first view's own points)."""
    gap = float(nearest_distance(full, merged, device=device).max())
    spacing = float(np.median(nearest_distance(first_view, first_view, exclude_self=True, device=device)))
    return gap, spacing
