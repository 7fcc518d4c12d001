"""Numpy float64 statement of the Tanks and Temples score and the synthetic scene the tests score.  Test infrastructure
only: brute force everywhere, no spatial index -- nothing here is shared with patchmatchnet_amd/registration.py or
csrc/registration.hip.  This file is the written specification the GPU code is held to; the protocol's constants are restated from the
published description of the benchmark's toolbox, none of its code was available.

Every expression is evaluated as numpy evaluates it: one rounding per product and per sum, no fused multiply-add.
"""
import math

import numpy as np

CHUNK = 256
LONG_RUN = 256  # PMN_VOXEL_LONG_RUN of include/pmn_hip.h


# ---- poses --------------------------------------------------------------------------------------------------------------------------

def apply_pose(pose, pts):
    """p' = r0 * x + r1 * y + r2 * z + t per row, left to right, float64 [n,3], of float32 (or float64) points."""
    P = np.asarray(pose, np.float64)
    p = np.asarray(pts).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([P[r, 0] * x + P[r, 1] * y + P[r, 2] * z + P[r, 3] for r in range(3)], 1)


def transform(pose, pts):
    return apply_pose(pose, pts).astype(np.float32)


def rotation(axis, degrees):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = math.radians(degrees)
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def rigid(R, t, s=1.0):
    T = np.eye(4)
    T[:3, :3] = s * np.asarray(R)
    T[:3, 3] = t
    return T


# ---- nearest neighbour --------------------------------------------------------------------------------------------------------------

def nearest(query, target, second=False):
    """Per float64 query [n,3] the squared distance dx * dx + dy * dy + dz * dz (d = target - query) to the nearest float32 target
    point and its index (the lowest among equals); with ``second`` also the second-smallest squared distance."""
    q = np.asarray(query, np.float64)
    t = np.asarray(target, np.float32).astype(np.float64)
    d2 = np.empty(len(q))
    idx = np.empty(len(q), np.int64)
    d2b = np.full(len(q), np.inf)
    for s in range(0, len(q), CHUNK):
        d = t[None, :, 0] - q[s:s + CHUNK, None, 0]
        d *= d
        for axis in (1, 2):  # (dx * dx + dy * dy) + dz * dz, in place
            e = t[None, :, axis] - q[s:s + CHUNK, None, axis]
            e *= e
            d += e
        idx[s:s + CHUNK] = d.argmin(1)
        d2[s:s + CHUNK] = d.min(1)
        if second and len(t) > 1:
            d2b[s:s + CHUNK] = np.partition(d, 1, axis=1)[:, 1]
    return (d2, idx, d2b) if second else (d2, idx)


def nn_distance(query_f32, target, cap):
    """min(sqrt(d2), cap) of float32 queries: what pmn_nn_distance returns."""
    d2, _ = nearest(np.asarray(query_f32, np.float32).astype(np.float64), target)
    return np.where(d2 < cap * cap, np.sqrt(d2), cap)


# ---- the seventeen sums -------------------------------------------------------------------------------------------------------------

def icp_terms(src, target, pose, centre, max_dist):
    """[17, n_matched] float64: the terms pmn_icp_accumulate sums (count, a, b, a b^T row-major, |q - p'|^2), one column per matched
    pair; a = p' - centre, b = q - centre."""
    c = np.asarray(centre, np.float64)
    p = apply_pose(pose, src)
    d2, idx = nearest(p, target)
    hit = d2 < max_dist * max_dist
    a = p[hit] - c
    b = np.asarray(target, np.float32).astype(np.float64)[idx[hit]] - c
    rows = [np.ones(int(hit.sum()))] + [a[:, i] for i in range(3)] + [b[:, i] for i in range(3)]
    rows += [a[:, i] * b[:, j] for i in range(3) for j in range(3)] + [d2[hit]]
    return np.stack(rows)


def icp_sums(src, target, pose, centre, max_dist):
    """The exactly rounded sums (math.fsum) and the sums of the terms' magnitudes."""
    t = icp_terms(src, target, pose, centre, max_dist)
    return np.array([math.fsum(r) for r in t]), np.array([math.fsum(np.abs(r)) for r in t])


# ---- Kabsch / Umeyama ---------------------------------------------------------------------------------------------------------------

def _rotation_from(H):
    U, S, Vt = np.linalg.svd(H)
    D = np.array([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0])
    return Vt.T @ np.diag(D) @ U.T, S, D


def kabsch(a, b, with_scale=False):
    """4 x 4 least-squares similarity / rigid motion taking the points a onto b (Umeyama's closed form)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ma, mb = a.mean(0), b.mean(0)
    da, db = a - ma, b - mb
    R, S, D = _rotation_from(da.T @ db)
    s = float((S * D).sum() / (da * da).sum()) if with_scale else 1.0
    return rigid(R, mb - s * R @ ma, s)


def bbox_centre(pts):
    p = np.asarray(pts, np.float32).astype(np.float64)
    return (p.min(0) + p.max(0)) / 2


def icp(src, target, init, max_dist, max_iter=20, rel_fitness=1e-6, rel_rmse=1e-6):
    """The ICP loop of registration.icp, brute force: evaluate, stop or update, at most max_iter updates."""
    pose = np.array(init, np.float64)
    t64 = np.asarray(target, np.float32).astype(np.float64)
    history = []
    updates = 0
    while True:
        p = apply_pose(pose, src)
        d2, idx = nearest(p, target)
        hit = d2 < max_dist * max_dist
        n = int(hit.sum())
        if n < 3:
            raise ValueError("fewer than 3 pairs")
        fitness, rmse = n / len(p), float(np.sqrt(math.fsum(d2[hit]) / n))
        done = bool(history) and abs(fitness - history[-1][0]) < rel_fitness * history[-1][0] and \
            abs(rmse - history[-1][1]) < rel_rmse * history[-1][1]
        history.append((fitness, rmse))
        if done or updates >= max_iter:
            break
        pose = kabsch(p[hit], t64[idx[hit]]) @ pose
        updates += 1
    return {"pose": pose, "fitness": fitness, "rmse": rmse, "iterations": updates, "history": history}


# ---- voxel mean ---------------------------------------------------------------------------------------------------------------------

def _run_mean(v):
    """Float32 mean of one run [len, C] float32, summed as pmn_voxel_mean sums it."""
    v = v.astype(np.float64)
    if len(v) <= LONG_RUN:
        s = np.zeros(v.shape[1])
        for row in v:
            s = s + row
    else:
        lanes = np.zeros((64, v.shape[1]))
        for i, row in enumerate(v):
            lanes[i % 64] = lanes[i % 64] + row
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[np.arange(64) ^ o]
        s = lanes[0]
    return (s / float(len(v))).astype(np.float32)


def voxel_downsample(pts, voxel, attr=None):
    """Mean of the points (and attributes) of every occupied voxel; lattice corner min - voxel / 2, voxels in ascending (z, y, x)
    order, the points of a voxel in input order."""
    pts = np.asarray(pts, np.float32)
    origin = pts.min(0).astype(np.float64) - voxel / 2
    c = np.floor((pts.astype(np.float64) - origin) / voxel).astype(np.int64)
    order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))  # stable; last key is primary
    cs = c[order]
    first = np.flatnonzero(np.r_[True, (cs[1:] != cs[:-1]).any(1)])
    bounds = np.r_[first, len(pts)]
    cols = pts[order] if attr is None else np.concatenate([pts[order], np.asarray(attr, np.float32)[order]], 1)
    out = np.stack([_run_mean(cols[bounds[i]:bounds[i + 1]]) for i in range(len(first))])
    return out[:, :3] if attr is None else (out[:, :3], out[:, 3:])


# ---- crop ---------------------------------------------------------------------------------------------------------------------------

def crop_mask(pts, polygon, axis, axis_min, axis_max, pose=None):
    """Even-odd rule over the polygon's edges (i, j = i - 1) in the two axes other than ``axis`` (ascending), and the slab along it."""
    p = apply_pose(pose, pts) if pose is not None else np.asarray(pts).astype(np.float64)
    u, v = [a for a in (0, 1, 2) if a != axis]
    poly = np.asarray(polygon, np.float64)
    px, py, c = p[:, u], p[:, v], p[:, axis]
    inside = np.zeros(len(p), bool)
    k = len(poly)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(k):
            xi, yi, xj, yj = poly[i, u], poly[i, v], poly[i - 1, u], poly[i - 1, v]
            cross = ((yi > py) != (yj > py)) & (px < (xj - xi) * (py - yi) / (yj - yi) + xi)
            inside ^= cross
    return inside & (axis_min <= c) & (c <= axis_max)


# ---- score --------------------------------------------------------------------------------------------------------------------------

def f_score(d_est, d_gt, tau):
    hit_est, hit_gt = int((d_est < tau).sum()), int((d_gt < tau).sum())
    P, R = 100.0 * hit_est / len(d_est), 100.0 * hit_gt / len(d_gt)
    return {"precision": P, "recall": R, "fscore": 2 * P * R / (P + R) if P + R > 0 else 0.0, "n_est": len(d_est), "n_gt": len(d_gt),
            "n_est_within_tau": hit_est, "n_gt_within_tau": hit_gt}


def tnt_score(est, gt, volume, tau, init, register=True, max_points=4_000_000):
    """The protocol of registration.tnt_score.  ``volume``: (polygon [k,3], axis, axis_min, axis_max)."""
    crop = lambda p: p[crop_mask(p, *volume)]
    pose = np.array(init, np.float64)
    gt_c = crop(gt)
    if register:
        for voxel, dist in ((tau, 80 * tau), (tau / 2, 20 * tau), (None, 2 * tau)):
            moved = crop(transform(pose, est))
            if voxel is None:
                k = lambda p: max(1, -(-len(p) // max_points))
                source, target = moved[::k(moved)], gt_c[::k(gt_c)]
            else:
                source, target = voxel_downsample(moved, voxel), voxel_downsample(gt_c, voxel)
            pose = icp(source, target, np.eye(4), dist)["pose"] @ pose
    prepared = lambda p: crop(voxel_downsample(crop(p), tau / 2))
    est_s, gt_s = prepared(transform(pose, est)), prepared(gt)
    d_est, d_gt = nn_distance(est_s, gt_s, 5 * tau), nn_distance(gt_s, est_s, 5 * tau)
    out = f_score(d_est, d_gt, tau)
    out["pose"] = pose
    return out, d_est, d_gt


# ---- the synthetic scene ------------------------------------------------------------------------------------------------------------

TAU = 0.01
MOTION = rigid(rotation((1.0, 2.0, 3.0), 2.0), (3 * TAU, -2 * TAU, 2.5 * TAU))  # takes the reconstruction onto the ground truth
POLYGON = np.array([[-1.0, -1.1, 0.0], [0.9, -1.0, 0.0], [1.1, 0.2, 0.0], [0.3, 0.1, 0.0], [0.5, 1.0, 0.0], [-0.6, 1.1, 0.0],
                    [-1.1, 0.25, 0.0]])  # 7 vertices, not convex ((0.3, 0.1) is a notch)


def trajectory(seed, m=12):
    """m camera-to-world matrices on a ring around the scene."""
    rng = np.random.default_rng(seed)
    out = np.empty((m, 4, 4))
    for i in range(m):
        a = 2 * math.pi * i / m
        out[i] = rigid(rotation(rng.standard_normal(3), 360 * rng.random()), (2.5 * math.cos(a), 2.5 * math.sin(a), 0.8 + 0.3 * rng.random()))
    return out


def synthetic_scene(seed=0):
    """gt: a bumpy sphere cap (6000 points) over a plane (3000), extent about +-1.2, float32; est: 5001 of those points under the inverse
    of MOTION; est_noisy: the same with sigma = 0.3 tau noise and 5 % uniform outliers; volume: a 7-vertex non-convex polygon along z between two float32-representable bounds;
    traj_est / traj_gt: 12 cameras each, related by ``similarity`` (est frame -> reference-trajectory frame), and gt_trans such that
    gt_trans @ similarity == MOTION."""
    rng = np.random.default_rng(seed)
    u, v = rng.random(6000), rng.random(6000)
    polar, az = np.arccos(1 - 0.75 * u), 2 * math.pi * v
    r = 1.0 + 0.04 * np.sin(7 * az) * np.sin(5 * polar)
    cap = np.stack([r * np.sin(polar) * np.cos(az), r * np.sin(polar) * np.sin(az), r * np.cos(polar) - 0.2], 1)
    plane = np.stack([rng.uniform(-1.2, 1.2, 3000), rng.uniform(-1.2, 1.2, 3000), -0.45 + 0.01 * rng.standard_normal(3000)], 1)
    gt = np.concatenate([cap, plane]).astype(np.float32)
    pick = np.sort(rng.choice(len(gt), 5001, replace=False))
    inv = np.linalg.inv(MOTION)
    est = transform(inv, gt[pick])
    noisy = apply_pose(inv, gt[pick]) + 0.3 * TAU * rng.standard_normal((5001, 3))
    out_idx = rng.choice(5001, 250, replace=False)
    noisy[out_idx] = rng.uniform(-1.5, 1.5, (250, 3))
    similarity = rigid(rotation((0.3, -1.0, 0.5), 25.0), (0.4, -0.2, 0.1), 1.7)
    traj_est = trajectory(seed + 100)
    traj_gt = np.array([rigid(np.eye(3), similarity[:3, :3] @ T[:3, 3] + similarity[:3, 3]) for T in traj_est])
    for i, T in enumerate(traj_est):
        traj_gt[i, :3, :3] = rotation((0.3, -1.0, 0.5), 25.0) @ T[:3, :3]
    return {"tau": TAU, "gt": gt, "pick": pick, "est": est, "est_noisy": noisy.astype(np.float32), "motion": MOTION,
            "volume": (POLYGON, 2, -0.625, 0.875), "similarity": similarity, "traj_est": traj_est, "traj_gt": traj_gt,
            "gt_trans": MOTION @ np.linalg.inv(similarity)}
