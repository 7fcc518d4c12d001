"""Independent numpy float64 statement of the DTU point-cloud score (reference evaluations/dtu/*.m), and the synthetic scan the
tests score.  Test infrastructure only: brute force everywhere, no spatial index, no scipy -- nothing here is shared with
patchmatchnet_amd/pointcloud.py or csrc/pointcloud.hip.

Distances are sqrt(dx*dx + dy*dy + dz*dz) of the float32 coordinates widened to float64, summed in x, y, z order (numpy evaluates
each product and sum separately: no fused multiply-add).

    reduce_points      reducePts_haa.m:8-31        (the visiting order is an input: the MATLAB draws an unseeded randperm, :9)
    max_dist_cp        MaxDistCP.m:3-39            (60-unit blocks; the to-points of the block grown by MaxDist)
    data_in_mask       PointCompareMain.m:32-41
    stl_above_plane    PointCompareMain.m:51-53
    stats / score_scan BaseEvalMain_web.m:62-75, ComputeStat_web.m:52-68
    totals             BaseEvalMain_web.m:98-99
"""
import numpy as np

CHUNK = 1024


def pair_distances(a, b):
    """[len(a), len(b)] float64 distances between float32 point sets."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return np.sqrt(dx * dx + dy * dy + dz * dz)


def neighbour_lists(pts, dst):
    """rangesearch(NS, pts', dst) (reducePts_haa.m:22): per point the indices within distance <= dst, itself included."""
    out = []
    for s in range(0, len(pts), CHUNK):
        d = pair_distances(pts[s:s + CHUNK], pts)
        out.extend(np.flatnonzero(row <= dst) for row in d)
    return out


def reduce_points(pts, dst, order):
    """reducePts_haa.m:8-31: visit the points in ``order``; a point still kept un-marks every point within dst and stays.
    Returns the bool mask indexSet."""
    n = len(pts)
    keep = np.ones(n, bool)
    nb = neighbour_lists(pts, dst)
    for i in np.asarray(order):
        if keep[i]:
            keep[nb[i]] = False
            keep[i] = True
    return keep


def nearest_distance(q_from, q_to):
    """knnsearch (MaxDistCP.m:32): (distance to the nearest to-point, its index), brute force in chunks."""
    dist = np.empty(len(q_from), np.float64)
    idx = np.empty(len(q_from), np.int64)
    for s in range(0, len(q_from), CHUNK):
        d = pair_distances(q_from[s:s + CHUNK], q_to)
        idx[s:s + CHUNK] = d.argmin(1)
        dist[s:s + CHUNK] = d.min(1)
    return dist, idx


def block_bounds(bb, max_dist=60.0):
    """MaxDistCP.m:5-15: per axis the (Low, High) of every block, computed as the MATLAB does (Low = BB(1,:) + k * MaxDist,
    High = Low + MaxDist)."""
    bb = np.asarray(bb, np.float64)
    rng = np.floor((bb[1] - bb[0]) / max_dist).astype(int)
    return [[(bb[0, a] + k * max_dist, bb[0, a] + k * max_dist + max_dist) for k in range(rng[a] + 1)] for a in range(3)]


def max_dist_cp(q_to, q_from, bb, max_dist=60.0):
    """MaxDistCP.m, literally: a from-point of block [Low, High) gets the distance to the nearest to-point of [Low - MaxDist,
    High + MaxDist); a block without to-points, and a from-point in no block, gives MaxDist.  (No clamp: a value can exceed MaxDist.)"""
    f = np.asarray(q_from, np.float32).astype(np.float64)
    t = np.asarray(q_to, np.float32).astype(np.float64)
    dist = np.ones(len(f)) * max_dist
    bx, by, bz = block_bounds(bb, max_dist)
    for lx, hx in bx:
        for ly, hy in by:
            for lz, hz in bz:
                low, high = np.array([lx, ly, lz]), np.array([hx, hy, hz])
                idx_f = np.flatnonzero(((f >= low) & (f < high)).all(1))
                low, high = low - max_dist, high + max_dist
                idx_t = np.flatnonzero(((t >= low) & (t < high)).all(1))
                if len(idx_f) == 0:
                    continue
                if len(idx_t) == 0:
                    dist[idx_f] = max_dist
                else:
                    dist[idx_f] = nearest_distance(np.asarray(q_from, np.float32)[idx_f], np.asarray(q_to, np.float32)[idx_t])[0]
    return dist


def matlab_round(x):
    """MATLAB round: halves away from zero (numpy rounds halves to even)."""
    x = np.asarray(x, np.float64)
    t = np.trunc(x)
    return t + np.sign(x) * (np.abs(x - t) >= 0.5)


def data_in_mask(q_data, obs_mask, bb, res):
    """PointCompareMain.m:32-41: Qv = round((Qdata - BB(1,:)) / Res + 1), 1-based and inside size(ObsMask), ObsMask(Qv) set."""
    q = np.asarray(q_data, np.float32).astype(np.float64)
    qv = matlab_round((q - np.asarray(bb, np.float64)[0]) / float(res) + 1)
    inside = ((qv > 0) & (qv <= np.array(obs_mask.shape))).all(1)
    out = np.zeros(len(q), bool)
    iv = qv[inside].astype(np.int64) - 1
    out[np.flatnonzero(inside)] = np.asarray(obs_mask, bool)[iv[:, 0], iv[:, 1], iv[:, 2]]
    return out


def stl_above_plane(q_stl, plane):
    """PointCompareMain.m:53: P' * [Qstl; 1] > 0."""
    q = np.asarray(q_stl, np.float32).astype(np.float64)
    p = np.asarray(plane, np.float64).reshape(4)
    return q[:, 0] * p[0] + q[:, 1] * p[1] + q[:, 2] * p[2] + p[3] > 0


def stats(d):
    """ComputeStat_web.m:59-68: n, mean, median (mean of the two middle values for an even count), variance (n - 1)."""
    d = np.asarray(d, np.float64)
    n = len(d)
    nan = float("nan")
    return {"n": n, "mean": float(d.mean()) if n else nan, "median": float(np.median(d)) if n else nan,
            "var": float(d.var(ddof=1)) if n > 1 else nan}


def score_scan(data_xyz, stl_xyz, obs_mask, bb, res, plane, order, dst=0.2, max_dist=20.0, search_dist=60.0):
    keep = reduce_points(data_xyz, dst, order)
    qd = np.asarray(data_xyz, np.float32)[keep]
    d_data = max_dist_cp(stl_xyz, qd, bb, search_dist)
    d_stl = max_dist_cp(qd, stl_xyz, bb, search_dist)
    acc = d_data[data_in_mask(qd, obs_mask, bb, res)]
    acc = acc[acc < max_dist]
    comp = d_stl[stl_above_plane(stl_xyz, plane)]
    comp = comp[comp < max_dist]
    out = {"n_data_in": len(data_xyz), "n_data_reduced": int(keep.sum())}
    for name, d in (("acc", acc), ("comp", comp)):
        for k, v in stats(d).items():
            out[f"{name}_{k}"] = v
    return out


def totals(per_scan):
    """BaseEvalMain_web.m:98-99: the mean of the per-scan means, overall = (acc + comp) / 2."""
    acc = float(np.mean([s["acc_mean"] for s in per_scan]))
    comp = float(np.mean([s["comp_mean"] for s in per_scan]))
    return {"acc": acc, "comp": comp, "overall": (acc + comp) / 2}


# ---- synthetic scan ---------------------------------------------------------------------------------------------------------------

def height(x, y):
    return 20.0 + 8.0 * np.sin(x / 17.0) * np.cos(y / 23.0) + 0.05 * x


def synthetic_scan(seed=0, n_stl=6000, n_data=9000, res=2.0):
    """A smooth height-field "object" of side ~100 units inside BB; an ObsMask volume that covers part of it; a plane that cuts part
    of the ground truth away; a method cloud of noisy surface samples that misses one patch entirely, with exact duplicates and a
    few per cent of far outliers: beyond 20, beyond 60, outside BB on the low and the high side, within half a voxel below BB(1,:).
    Returns a dict of float32 clouds and the mask / plane fields under the .mat names."""
    rng = np.random.default_rng(seed)
    bb = np.array([[-10.0, -10.0, -10.0], [128.0, 115.0, 75.0]])
    sx = rng.uniform(0.0, 100.0, n_stl)
    sy = rng.uniform(0.0, 100.0, n_stl)
    stl = np.stack([sx, sy, height(sx, sy)], 1)
    n_surf = int(n_data * 0.9)
    dx = rng.uniform(0.0, 100.0, n_surf)
    dy = rng.uniform(0.0, 100.0, n_surf)
    hole = (dx > 60) & (dx < 80) & (dy > 20) & (dy < 45)  # the patch the method misses
    dx, dy = dx[~hole], dy[~hole]
    surf = np.stack([dx, dy, height(dx, dy)], 1) + rng.normal(0.0, 0.15, (len(dx), 3))
    n_out = n_data - n_surf
    k = n_out // 6
    centre = np.array([50.0, 50.0, 20.0])

    def shell(n, r0, r1):
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return centre + v * rng.uniform(r0, r1, (n, 1))

    near = stl[rng.integers(0, n_stl, k)] + np.array([0.0, 0.0, 1.0]) * rng.uniform(21.0, 35.0, (k, 1))  # beyond 20
    far = shell(k, 150.0, 260.0)                                                                          # beyond 60, mostly outside BB
    low = bb[0] - rng.uniform(1.0, 90.0, (k, 3))                                                          # outside BB, low side
    high = bb[1] + rng.uniform(1.0, 90.0, (k, 3))                                                         # outside BB, high side
    edge = np.stack([bb[0, 0] - rng.uniform(0.0, res / 2, k), rng.uniform(0, 100, k), rng.uniform(0, 40, k)], 1)  # half a voxel below
    mid = shell(n_out - 5 * k, 30.0, 70.0)
    data = np.concatenate([surf, near, far, low, high, edge, mid]).astype(np.float32)
    dup = rng.integers(0, len(data), max(len(data) // 50, 2))  # exact duplicates
    data = np.concatenate([data, data[dup]])
    data = data[rng.permutation(len(data))]
    # ObsMask: voxels of side res from BB(1,:), set within 12 units of the surface where x < 85
    shape = np.floor((bb[1] - bb[0]) / res).astype(int) + 1
    gx, gy, gz = np.meshgrid(*(bb[0, a] + np.arange(shape[a]) * res for a in range(3)), indexing="ij")
    obs = (np.abs(gz - height(gx, gy)) < 12.0) & (gx < 85.0) & (gx > -11.0) & (gy > -5.0) & (gy < 105.0)
    plane = np.array([0.05, 0.0, 1.0, -18.0])  # keeps z + 0.05 x > 18: cuts the low part of the surface away
    return {"data": data, "stl": stl.astype(np.float32), "ObsMask": obs, "BB": bb, "Res": float(res), "P": plane.reshape(4, 1)}
