"""Brute-force numpy float64 statement of normals from neighbourhoods (pmn_knn_normals, pointcloud.knn_normals / estimate_normals,
cloud_normals.py; include/pmn_hip.h states the definition).  Neighbours come from the full matrix of squared distances with a stable
sort on (d2, index), as in tests/knn_ref.py; nothing is shared with the product.  Two eigen-solvers: numpy.linalg.eigh, the independent
one that the normals are judged by, and `jacobi`, a host model of the kernel's fixed sweeps, operation for operation, that the
kernel's float64 outputs must equal bit for bit.  The test clouds live here so that the CPU suite can check them."""
import numpy as np

import knn_ref as K

SWEEPS = 6  # PMN_NORMAL_SWEEPS


def neighbours(query, points, k, max_dist, same_cloud=False, rank=None):
    """int64 [n, k]: indices into ``points`` of the k nearest of every query, ascending (d2, rank of the index); -1 in a slot whose
    candidate is not below max_dist^2 or does not exist.  ``rank`` [len(points)] is the order that breaks ties among equal squares
    (the product's is the grid's sorted position); default: the index itself."""
    d2 = K.pair_d2(points if same_cloud else query, points)
    n, npts = d2.shape
    if same_cloud:
        d2[np.arange(n), np.arange(n)] = np.inf
    rank = np.arange(npts) if rank is None else np.asarray(rank)
    by_rank = np.argsort(rank, kind="stable")
    idx = by_rank[np.argsort(d2[:, by_rank], axis=1, kind="stable")][:, :k]
    out = np.full((n, k), -1, np.int64)
    cap = float(max_dist) * float(max_dist)
    val = np.take_along_axis(d2, idx, 1)
    out[:, :idx.shape[1]] = np.where(val < cap, idx, -1)
    return out


def moments(query, points, idx):
    """(count int [n], s float64 [n,3], M float64 [n,6] as xx xy xz yy yz zz): the sums of the deltas p_j - q over the neighbours
    ``idx`` [n,k] (-1 = none), added column by column, i.e. in rank order."""
    q = np.asarray(query, np.float32).astype(np.float64)
    p = np.asarray(points, np.float32).astype(np.float64)
    n = len(q)
    s, M, count = np.zeros((n, 3)), np.zeros((n, 6)), np.zeros(n, np.int64)
    for j in range(idx.shape[1]):
        live = idx[:, j] >= 0
        d = np.where(live[:, None], p[np.maximum(idx[:, j], 0)] - q, 0.0)
        s = s + d
        M = M + np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                          d[:, 2] * d[:, 2]], 1)
        count += live
    return count, s, M


def covariance(count, s, M):
    """float64 [n,6] (xx xy xz yy yz zz): C_ab = M_ab - (s_a * s_b) / m, m = count + 1."""
    m = (count + 1).astype(np.float64)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    return np.stack([M[:, i] - (s[:, a] * s[:, b]) / m for i, (a, b) in enumerate(pairs)], 1)


def full(C):
    """[n,6] -> symmetric [n,3,3]"""
    return np.stack([np.stack([C[:, 0], C[:, 1], C[:, 2]], 1), np.stack([C[:, 1], C[:, 3], C[:, 4]], 1),
                     np.stack([C[:, 2], C[:, 4], C[:, 5]], 1)], 1)


def _rotate(app, aqq, apq, arp, arq, vp, vq):
    """One rotation of the kernel (pc_jacobi_rotate) on arrays; vp / vq are the columns p and q of V as lists of three rows."""
    on = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        root = np.abs(theta) + np.sqrt(theta * theta + 1.0)
        t = np.where(theta < 0.0, -1.0 / root, 1.0 / root)
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        h = t * apq
        new = [app - h, aqq + h, np.zeros_like(apq), c * arp - s * arq, s * arp + c * arq]
        nvp = [c * vp[i] - s * vq[i] for i in range(3)]
        nvq = [s * vp[i] + c * vq[i] for i in range(3)]
    old = [app, aqq, apq, arp, arq]
    return [np.where(on, a, b) for a, b in zip(new, old)], [np.where(on, a, b) for a, b in zip(nvp, vp)], \
        [np.where(on, a, b) for a, b in zip(nvq, vq)]


def jacobi(C, sweeps=SWEEPS):
    """The kernel's eigen-solver on [n,6] matrices: (values [n,3] ascending, equal values in column order; vectors [n,3,3],
    vectors[:, :, j] belonging to values[:, j])."""
    n = len(C)
    a00, a01, a02, a11, a12, a22 = (C[:, i].copy() for i in range(6))
    one, zero = np.ones(n), np.zeros(n)
    v = [[one, zero, zero], [zero, one, zero], [zero, zero, one]]  # v[column][row]
    for _ in range(sweeps):
        (a00, a11, a01, a02, a12), v[0], v[1] = _rotate(a00, a11, a01, a02, a12, v[0], v[1])
        (a00, a22, a02, a01, a12), v[0], v[2] = _rotate(a00, a22, a02, a01, a12, v[0], v[2])
        (a11, a22, a12, a01, a02), v[1], v[2] = _rotate(a11, a22, a12, a01, a02, v[1], v[2])
    lam = np.stack([a00, a11, a22], 1)
    vec = np.stack([np.stack(col, 1) for col in v], 2)  # [n, row, column]
    order = np.argsort(lam, axis=1, kind="stable")
    return np.take_along_axis(lam, order, 1), np.take_along_axis(vec, order[:, None, :], 2)


def eigh(C):
    """numpy.linalg.eigh of the same matrices: (values ascending [n,3], vectors [n,3,3])."""
    return np.linalg.eigh(full(C))


def canonical(n):
    """The component of largest magnitude positive, the lowest axis among equal magnitudes."""
    lead = np.take_along_axis(n, np.argmax(np.abs(n), axis=1)[:, None], 1)[:, 0]
    return np.where((lead < 0.0)[:, None], -n, n)


def nearest_viewpoint(query, viewpoints):
    """(index [n], e = c - q float64 [n,3]) of the viewpoint nearest to every query: e.x^2 + e.y^2 + e.z^2, the lowest index among
    equals (argmin returns the first)."""
    q = np.asarray(query, np.float32).astype(np.float64)
    e = np.asarray(viewpoints, np.float64)[None, :, :] - q[:, None, :]
    d = e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1] + e[:, :, 2] * e[:, :, 2]
    j = np.argmin(d, axis=1)
    return j, e[np.arange(len(q)), j]


def orient(query, n, viewpoints):
    """Negates the canonical normal where n . (c - q) < 0 for the nearest viewpoint c; exactly 0 keeps it."""
    _, e = nearest_viewpoint(query, viewpoints)
    dot = n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1] + n[:, 2] * e[:, 2]
    return np.where((dot < 0.0)[:, None], -n, n)


def normals(query, points, k, max_dist, same_cloud=False, viewpoints=None, line_ratio=1e-6, solver=jacobi, rank=None, idx=None):
    """dict: normal float64 [n,3] (unrounded), variation [n], count [n], values [n,3], valid bool [n], C [n,6], s [n,3], idx [n,k].
    ``idx``: `neighbours` of the same arguments for this or a larger k, where a caller asks for several k (the lists are nested)."""
    q = points if same_cloud else query
    idx = neighbours(query, points, k, max_dist, same_cloud, rank) if idx is None else idx[:, :k]
    count, s, M = moments(q, points, idx)
    C = covariance(count, s, M)
    lam, vec = solver(C)
    valid = (count >= 2) & (lam[:, 2] != 0.0) & (lam[:, 1] > float(line_ratio) * lam[:, 2])
    nrm = canonical(vec[:, :, 0])
    if viewpoints is not None:
        nrm = orient(q, nrm, viewpoints)
    with np.errstate(all="ignore"):
        var = lam[:, 0] / (lam[:, 0] + lam[:, 1] + lam[:, 2])
    return {"normal": np.where(valid[:, None], nrm, 0.0), "variation": np.where(valid, var, 0.0), "count": count, "values": lam,
            "valid": valid, "C": C, "s": s, "idx": idx}


def gap(values):
    """(l1 - l0) / l2, the separation that conditions the normal (0 where l2 is not positive)."""
    with np.errstate(all="ignore"):
        g = (values[:, 1] - values[:, 0]) / values[:, 2]
    return np.where(values[:, 2] > 0.0, g, 0.0)


def angle(a, b, signed=True):
    """Angle in radians between rows of a and b, computed from the cross product (accurate near 0); up to sign unless ``signed``."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    cr = np.linalg.norm(np.cross(a, b), axis=1)
    dt = (a * b).sum(1)
    return np.arctan2(cr, dt if signed else np.abs(dt))


# ---- the clouds of the tests ---------------------------------------------------------------------------------------------------

def sphere_cloud(n=1500, centre=(300.0, -200.0, 650.0), radius=10.0, noise=0.002, seed=0):
    """Points on a sphere far from the origin with relative radial noise: (points float32 [n,3], centre float64 [3])."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = radius * (1.0 + noise * rng.normal(size=n))
    c = np.asarray(centre, np.float64)
    return (c + d * r[:, None]).astype(np.float32), c


def sheet_cloud(n=1800, planted=40, seed=0):
    """tests/knn_ref.py's wavy sheet with exactly ``planted`` outliers."""
    return K.surface_cloud(n, planted / n, seed)[0]


def plane_cloud(side=9):
    """Integer lattice points of the plane z = x + 2 y (normal (1, 2, -1) / sqrt 6), shuffled: every coordinate and every moment is
    an integer, exact in float64."""
    x, y = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), (x + 2 * y).ravel()], 1).astype(np.float64)
    return np.random.default_rng(2).permutation(p).astype(np.float32)
