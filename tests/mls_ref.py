"""Brute-force numpy float64 statement of moving least squares on a point cloud (pmn_knn_mls, pointcloud.knn_mls / smooth_mls,
smooth_cloud.py; include/pmn_hip.h states the definition).  Neighbours, the Jacobi model and the test clouds are those of
tests/cloud_normals_ref.py and tests/knn_ref.py; nothing is shared with the product.  Two routes: `mls`, the host model of the kernel,
operation for operation and vectorised over the queries, that the kernel's outputs must equal bit for bit; and `mls_independent`, the
same fit written the way a textbook would (centred weighted covariance, numpy.linalg.eigh for the frame, numpy.linalg.lstsq for the
quadric in unscaled coordinates), that the model is judged by."""
import numpy as np

import cloud_normals_ref as R
import knn_ref as K

QUADRIC_MIN = 6     # PMN_MLS_QUADRIC_MIN
PIVOT_MIN = 1e-10   # PMN_MLS_PIVOT_MIN


def _at(i, j):
    return i * (i + 1) // 2 + j


def _dot3(a, b):
    """(a.x * b.x + a.y * b.y) + a.z * b.z on [n,3] arrays"""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _members(query, points, idx, same_cloud, R2):
    """The members of every fit in the kernel's order: a list of (live bool [n], delta float64 [n,3], weight float64 [n]); under
    same_cloud the query itself comes first, the zero delta with weight 1."""
    q = np.asarray(query, np.float32).astype(np.float64)
    p = np.asarray(points, np.float32).astype(np.float64)
    n = len(q)
    out = []
    if same_cloud:
        out.append((np.ones(n, bool), np.zeros((n, 3)), np.ones(n)))
    for j in range(idx.shape[1]):
        live = idx[:, j] >= 0
        d = np.where(live[:, None], p[np.maximum(idx[:, j], 0)] - q, 0.0)
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        u = 1.0 - d2 / R2
        u2 = u * u
        out.append((live, d, np.where(live, u2 * u2, 0.0)))
    return out


def _cholesky_solve(G, g, floor):
    """The kernel's Cholesky on [n,21] lower triangles and [n,6] right-hand sides: (ok bool [n], c float64 [n,6])."""
    L = [G[:, i].copy() for i in range(21)]
    ok = np.ones(len(G), bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            v = L[_at(j, j)]
            for k in range(j):
                v = v - L[_at(j, k)] * L[_at(j, k)]
            ok &= v > floor
            ljj = np.sqrt(v)
            L[_at(j, j)] = ljj
            for i in range(j + 1, 6):
                u = L[_at(i, j)]
                for k in range(j):
                    u = u - L[_at(i, k)] * L[_at(j, k)]
                L[_at(i, j)] = u / ljj
        y = [None] * 6
        for i in range(6):
            v = g[:, i]
            for k in range(i):
                v = v - L[_at(i, k)] * y[k]
            y[i] = v / L[_at(i, i)]
        c = [None] * 6
        for i in range(5, -1, -1):
            v = y[i]
            for k in range(i + 1, 6):
                v = v - L[_at(k, i)] * c[k]
            c[i] = v / L[_at(i, i)]
    return ok, np.stack(c, 1)


def mls(query, points, k, radius, same_cloud=False, degree=2, line_ratio=1e-6, rank=None, idx=None):
    """The host model of pmn_knn_mls.  dict: position float32 [n,3], normal float32 [n,3], displacement float64 [n], status int [n],
    count int [n]; and what the tests look into: moved float64 [n,3] (q + delta, unrounded), delta [n,3], values [n,3], A [n,6],
    t [n], n [n,3], W [n], idx [n,k].  ``idx``: cloud_normals_ref.neighbours of the same arguments for this or a larger k."""
    radius = float(radius)
    R2 = radius * radius
    src = points if same_cloud else query
    q32 = np.asarray(src, np.float32)
    q = q32.astype(np.float64)
    nq = len(q)
    idx = R.neighbours(query, points, k, radius, same_cloud, rank) if idx is None else idx[:, :k]
    members = _members(src, points, idx, same_cloud, R2)
    W = np.ones(nq) if same_cloud else np.zeros(nq)
    s, M = np.zeros((nq, 3)), np.zeros((nq, 6))
    count = np.zeros(nq, np.int64)
    for live, d, w in members[1 if same_cloud else 0:]:
        wd = w[:, None] * d
        W = W + w
        s = s + wd
        M = M + np.stack([wd[:, 0] * d[:, 0], wd[:, 0] * d[:, 1], wd[:, 0] * d[:, 2], wd[:, 1] * d[:, 1], wd[:, 1] * d[:, 2],
                          wd[:, 2] * d[:, 2]], 1)
        count += live
    m = count + (1 if same_cloud else 0)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    with np.errstate(all="ignore"):
        c = s / W[:, None]
        A = np.stack([M[:, i] - (s[:, a] * s[:, b]) / W for i, (a, b) in enumerate(pairs)], 1)
        lam, vec = R.jacobi(A)
        nrm, e1, e2 = R.canonical(vec[:, :, 0]), R.canonical(vec[:, :, 1]), R.canonical(vec[:, :, 2])
        valid = (m >= 3) & (W > 0.0) & (lam[:, 2] != 0.0) & (lam[:, 1] > float(line_ratio) * lam[:, 2])
        t = _dot3(nrm, c)
        x0 = t[:, None] * nrm
    delta, out_n = x0.copy(), nrm.copy()
    status = valid.astype(np.int64)
    if degree == 2:
        G, g = np.zeros((nq, 21)), np.zeros((nq, 6))
        with np.errstate(all="ignore"):
            for live, d, w in members:
                r = d - x0
                a = _dot3(e1, r) / radius
                b = _dot3(e2, r) / radius
                h = _dot3(nrm, r)
                phi = [np.ones(nq), a, b, a * a, a * b, b * b]
                for j in range(6):
                    wp = w if j == 0 else w * phi[j]
                    g[:, j] = g[:, j] + np.where(live, wp * h, 0.0)
                    for i in range(j, 6):
                        G[:, _at(i, j)] = G[:, _at(i, j)] + np.where(live, wp * phi[i], 0.0)
            ok, cf = _cholesky_solve(G, g, PIVOT_MIN * W)
            gd = x0 + cf[:, :1] * nrm
            gg = _dot3(gd, gd)
            k1, k2 = cf[:, 1] / radius, cf[:, 2] / radius
            u = (nrm - k1[:, None] * e1) - k2[:, None] * e2
            u = u / np.sqrt(_dot3(u, u))[:, None]
            take = valid & (m >= QUADRIC_MIN) & ok & (gg <= R2)
        delta = np.where(take[:, None], gd, delta)
        out_n = np.where(take[:, None], u, out_n)
        status = np.where(take, 2, status)
    on = status > 0
    with np.errstate(all="ignore"):
        moved = q + delta
        disp = np.sqrt(_dot3(delta, delta))
    return {"position": np.where(on[:, None], moved.astype(np.float32), q32), "normal": np.where(on[:, None], out_n, 0.0).astype(np.float32),
            "displacement": np.where(on, disp, 0.0), "status": status, "count": count, "moved": np.where(on[:, None], moved, q),
            "delta": np.where(on[:, None], delta, 0.0), "values": lam, "A": A, "t": t, "n": nrm, "W": W, "idx": idx}


def mls_independent(query, points, k, radius, same_cloud=False, degree=2, rank=None, idx=None):
    """The same fit by library solvers, query by query: weighted centroid, CENTRED weighted covariance, numpy.linalg.eigh, and for
    degree 2 numpy.linalg.lstsq on sqrt(w) * (1, a, b, a^2, a b, b^2) with a, b in scene units.  No validity rule and no fallback:
    (moved float64 [n,3] = q + delta, values [n,3]); rows with fewer than 3 members (6 for the quadric's step) are NaN."""
    radius = float(radius)
    src = points if same_cloud else query
    q = np.asarray(src, np.float32).astype(np.float64)
    p = np.asarray(points, np.float32).astype(np.float64)
    idx = R.neighbours(query, points, k, radius, same_cloud, rank) if idx is None else idx[:, :k]
    moved, values = np.full((len(q), 3), np.nan), np.full((len(q), 3), np.nan)
    for i in range(len(q)):
        nb = idx[i][idx[i] >= 0]
        d = p[nb] - q[i]
        w = (1.0 - (d * d).sum(1) / (radius * radius)) ** 4
        if same_cloud:
            d, w = np.concatenate([np.zeros((1, 3)), d]), np.concatenate([[1.0], w])
        if len(w) < 3 or not w.sum() > 0.0:
            continue
        c = (w[:, None] * d).sum(0) / w.sum()
        e = d - c
        lam, vec = np.linalg.eigh((w[:, None, None] * e[:, :, None] * e[:, None, :]).sum(0))
        values[i] = lam
        n, e1, e2 = vec[:, 0], vec[:, 1], vec[:, 2]
        x0 = (n @ c) * n
        if degree == 2:
            if len(w) < QUADRIC_MIN:
                continue
            r = d - x0
            a, b, h = r @ e1, r @ e2, r @ n
            sw = np.sqrt(w)
            phi = np.stack([np.ones_like(a), a, b, a * a, a * b, b * b], 1)
            coef = np.linalg.lstsq(sw[:, None] * phi, sw * h, rcond=None)[0]
            x0 = x0 + coef[0] * n
        moved[i] = q[i] + x0
    return moved, values


# ---- the clouds of the tests ---------------------------------------------------------------------------------------------------

def noisy_sphere(n=1500, noise=0.01, seed=0):
    """cloud_normals_ref.sphere_cloud with relative radial noise ``noise``: (points float32 [n,3], centre float64 [3], radius)."""
    pts, centre = R.sphere_cloud(n, noise=noise, seed=seed)
    return pts, centre, 10.0


def sphere_distance(points, centre, radius):
    """signed distance float64 [n] of points to the sphere, positive outside"""
    return np.linalg.norm(np.asarray(points, np.float64) - centre, axis=1) - radius


def planar_lattice(side=(9, 8), z=3.0):
    """An axis-aligned integer lattice in the plane z = const, shuffled."""
    x, y = np.meshgrid(np.arange(float(side[0])), np.arange(float(side[1])), indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), np.full(x.size, z)], 1)
    return np.random.default_rng(4).permutation(p).astype(np.float32)


lattice_cloud, duplicate_cloud, axis_cloud, far_queries = K.lattice_cloud, K.duplicate_cloud, K.axis_cloud, K.far_queries
sphere_cloud, sheet_cloud = R.sphere_cloud, R.sheet_cloud
