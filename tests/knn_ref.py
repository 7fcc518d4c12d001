"""Brute-force numpy float64 statements of the k-nearest-neighbour and radius searches behind cloud cleaning (pmn_knn_distance,
pmn_radius_count, pointcloud.statistical_outliers / radius_outliers, clean_cloud.py).  No spatial index, nothing shared with the
product: the full matrix of squared distances, sorted row by row.  The test clouds of tests/test_knn_gpu.py live here too so that the
CPU suite can check them (tests/test_clean_cloud_io.py)."""
import numpy as np

from dtu_ref import pair_distances


def pair_d2(a, b):
    """[len(a), len(b)] float64 squared distances between float32 point sets: dx*dx + dy*dy + dz*dz in x, y, z order."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return dx * dx + dy * dy + dz * dz


def sorted_d2(query, points, same_cloud=False):
    """Every row of the full matrix of squared distances, sorted; the diagonal is excluded (infinite, hence last) under same_cloud."""
    m = pair_d2(points if same_cloud else query, points)
    if same_cloud:
        m[np.arange(len(m)), np.arange(len(m))] = np.inf
    return np.sort(m, axis=1)


def knn_d2(query, points, k, max_dist, same_cloud=False, rows=None):
    """float64 [n, k]: the k smallest squared distances of every row, ascending; the diagonal is excluded under same_cloud; an entry
    not below max_dist^2 (and every slot beyond the number of candidates) is the cap max_dist * max_dist.  ``rows``: sorted_d2 of the
    same arguments, where a caller asks for several k."""
    m = (sorted_d2(query, points, same_cloud) if rows is None else rows)[:, :k]
    cap = float(max_dist) * float(max_dist)
    out = np.full((len(m), k), cap, np.float64)
    out[:, :m.shape[1]] = np.where(m < cap, m, cap)
    return out


def knn_mean(d2, max_dist):
    """float64 [n]: (sum_j sqrt(d2_j)) / k, added column by column (ndarray.sum adds pairwise); a capped slot adds max_dist itself."""
    cap = float(max_dist) * float(max_dist)
    s = np.zeros(len(d2), np.float64)
    for j in range(d2.shape[1]):
        s = s + np.where(d2[:, j] == cap, float(max_dist), np.sqrt(d2[:, j]))
    return s / float(d2.shape[1])


def radius_count(query, points, radius, same_cloud=False):
    """int [n]: the number of points with sqrt(d2) <= radius, the query itself (the diagonal) not counted under same_cloud."""
    within = pair_distances(points if same_cloud else query, points) <= float(radius)
    return within.sum(1) - (1 if same_cloud else 0)


def statistical_outliers(points, k, std_ratio, max_dist):
    """(keep, mean, threshold): keep = mean <= mu + std_ratio * sigma, sigma with n - 1 in the denominator."""
    mean = knn_mean(knn_d2(None, points, k, max_dist, same_cloud=True), max_dist)
    sigma = mean.std(ddof=1) if len(mean) > 1 else 0.0
    threshold = float(mean.mean() + std_ratio * sigma)
    return mean <= threshold, mean, threshold


def radius_outliers(points, radius, min_neighbors):
    count = radius_count(None, points, radius, same_cloud=True)
    return count >= min_neighbors, count


# ---- the clouds of the tests ---------------------------------------------------------------------------------------------------

def surface_cloud(n=2900, outliers=0.02, seed=0):
    """A noisy sheet z = 4 sin(x / 9) cos(y / 7) over 60 x 60 units (noise sigma 0.05) with `outliers` of the points planted
    uniformly in the box around it, up to 40 units off.  Returns (points float32 [n,3], planted bool [n], offset float64 [n]: the
    distance of a planted point from the noise-free sheet along z, 0 for surface points)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, 60.0, (n, 2))
    sheet = 4.0 * np.sin(xy[:, 0] / 9.0) * np.cos(xy[:, 1] / 7.0)
    z = sheet + rng.normal(0.0, 0.05, n)
    planted = np.zeros(n, bool)
    planted[rng.choice(n, int(round(n * outliers)), replace=False)] = True
    z[planted] = sheet[planted] + rng.uniform(-40.0, 40.0, int(planted.sum()))
    pts = np.stack([xy[:, 0], xy[:, 1], z], 1).astype(np.float32)
    offset = np.where(planted, np.abs(pts[:, 2].astype(np.float64) - sheet), 0.0)
    return pts, planted, offset


def lattice_cloud(side=(7, 6, 5), spacing=1.0):
    """Every integer lattice point of a box, shuffled: ties at every rank, and with a cell that divides the spacing, points exactly
    on cell faces."""
    g = np.stack(np.meshgrid(*[np.arange(s) for s in side], indexing="ij"), -1).reshape(-1, 3).astype(np.float64) * spacing
    return np.random.default_rng(3).permutation(g).astype(np.float32)


def duplicate_cloud(n=301, seed=5):
    """Random points of which a third are exact copies of others (up to four copies of one point)."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-3.0, 3.0, (n - n // 3, 3)).astype(np.float32)
    return rng.permutation(np.concatenate([base, base[rng.integers(0, 25, n // 3)]]))


def axis_cloud(n=257, seed=7):
    """Points along the x axis only (y = z = 0): a grid of one row."""
    x = np.sort(np.random.default_rng(seed).uniform(0.0, 50.0, n))
    return np.stack([x, np.zeros(n), np.zeros(n)], 1).astype(np.float32)


def far_queries(points, n=131, seed=11):
    """A separate query set: points near the cloud, inside its box, and far outside it on every side (6 faces, a corner)."""
    rng = np.random.default_rng(seed)
    p = np.asarray(points, np.float64)
    lo, hi = p.min(0), p.max(0)
    ext = max(float((hi - lo).max()), 1.0)
    near = p[rng.integers(0, len(p), n // 2)] + rng.normal(0.0, 0.02 * ext, (n // 2, 3))
    inside = rng.uniform(lo, hi, (n - n // 2 - 13, 3))
    c = (lo + hi) / 2
    far = [c + s * d * np.eye(3)[a] for a in range(3) for s in (-1.0, 1.0) for d in (0.8 * ext, 30.0 * ext)]
    far.append(hi + 5.0 * ext)
    return np.concatenate([near, inside, np.array(far)]).astype(np.float32)
