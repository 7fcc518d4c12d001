"""Numpy restatement of meshops.vertex_adjacency, smooth_steps / smooth_taubin / smooth_laplacian (pmn_mesh_smooth) and vertex_normals
(pmn_mesh_vertex_normals); DESIGN.md section 30: the yardstick of tests/test_smooth_ref.py and tests/test_smooth_gpu.py.  Test
infrastructure: nothing in the product imports it.

Every sum runs in the kernels' order (a row in row order from 0.0; a row longer than LONG_ROW over 64 lanes and pmn_voxel_mean's
butterfly), every expression in the header's order.  ``dtype`` is the arithmetic: np.float64 restates the kernel, np.longdouble is the
same text at 64 bits of mantissa, the reference the positions are held to.  The integers are the same for both."""
from __future__ import annotations

import numpy as np

import simplify_ref

LONG_ROW = 256  # PMN_MESH_SMOOTH_LONG_ROW of include/pmn_hip.h


def adjacency(faces, n_vertices):
    """(starts int64 [Nv + 1], neighbours int32 [E], boundary bool [Nv]): the six directed pairs of every face without those with equal
    ends, distinct, ascending within a row; a boundary edge is named by exactly one corner-pair of the faces with three different
    vertices.  Plain Python over the faces."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = int(n_vertices)
    rows = [set() for _ in range(nv)]
    edges = {}
    for a, b, c in f.tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            if p != q:
                rows[p].add(q)
                rows[q].add(p)
        if a != b and b != c and a != c:
            for p, q in ((a, b), (b, c), (c, a)):
                key = (min(p, q), max(p, q))
                edges[key] = edges.get(key, 0) + 1
    starts = np.zeros(nv + 1, np.int64)
    starts[1:] = np.cumsum([len(r) for r in rows])
    neighbours = np.asarray([j for r in rows for j in sorted(r)], np.int32).reshape(-1)
    boundary = np.zeros(nv, bool)
    for (p, q), n in edges.items():
        if n == 1:
            boundary[p] = boundary[q] = True
    return starts, neighbours, boundary


def _sum_row(rows, dtype):
    """The per-component sum of one row [len, 3] as both kernels add it (simplify_ref._sum_run's rule with this file's constant)."""
    if len(rows) <= LONG_ROW:
        s = np.zeros(3, dtype)
        for row in rows:
            s = s + row
        return s
    lanes = np.zeros((64, 3), dtype)
    for i, row in enumerate(rows):
        lanes[i % 64] = lanes[i % 64] + row
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(64) ^ o]
    return lanes[0]


def step(vertices, starts, neighbours, factor, pinned=None, dtype=np.float64):
    """One umbrella step: the UNROUNDED positions [Nv,3] in ``dtype`` (the kernel stores their float32 rounding).  A vertex without
    neighbours, or a pinned one, keeps its float32 value exactly."""
    T = dtype
    v = np.asarray(vertices, np.float32)
    p = v.astype(T)
    out = p.copy()
    for i in range(len(v)):
        r = neighbours[starts[i]:starts[i + 1]]
        if len(r) == 0 or (pinned is not None and pinned[i]):
            continue
        s = _sum_row(p[r] - p[i], T)
        out[i] = p[i] + T(factor) * (s / T(len(r)))
    return out


def steps(vertices, faces, factors, boundary="fixed", pinned=None, dtype=np.float64):
    """float32 [Nv,3] after one step per factor, each rounded to float32 as the kernel rounds it."""
    v = np.asarray(vertices, np.float32).copy()
    starts, neighbours, rim = adjacency(faces, len(v))
    pin = rim.copy() if boundary == "fixed" else np.zeros(len(v), bool)
    if pinned is not None:
        pin |= np.asarray(pinned, bool)
    for factor in factors:
        v = step(v, starts, neighbours, factor, pin, dtype).astype(np.float32)
    return v


def taubin(vertices, faces, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", pinned=None, dtype=np.float64):
    return steps(vertices, faces, [lam, mu] * iterations, boundary, pinned, dtype)


def laplacian(vertices, faces, iterations=1, lam=0.5, boundary="fixed", pinned=None, dtype=np.float64):
    return steps(vertices, faces, [lam] * iterations, boundary, pinned, dtype)


def normals(vertices, faces, flip=False, dtype=np.float64):
    """The UNROUNDED vertex normals [Nv,3] in ``dtype``: per vertex the sum of (B - A) x (C - A) over its corners in the order of
    meshops.vertex_normals (the faces in canonical order, the corners stably sorted by vertex), divided by its length; zero where
    the length is zero or not finite."""
    T = dtype
    v = np.asarray(vertices, np.float32).astype(T)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[simplify_ref.canonical_face_order(f)]
    corner_vertex = f.reshape(-1)
    by_vertex = np.argsort(corner_vertex, kind="stable")
    starts = np.searchsorted(corner_vertex[by_vertex], np.arange(len(v) + 1))
    face = by_vertex // 3
    with np.errstate(all="ignore"):
        a = v[f[face, 0]]
        e1, e2 = v[f[face, 1]] - a, v[f[face, 2]] - a
        cross = np.stack((e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), 1).astype(T)
        out = np.zeros((len(v), 3), T)
        for i in range(len(v)):
            n = _sum_row(cross[starts[i]:starts[i + 1]], T)
            length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            if length > 0 and np.isfinite(length):
                out[i] = n / length
    return -out if flip else out


# ---- meshes ----------------------------------------------------------------------------------------------------------------------

def plane_grid(nx, ny, step=0.125):
    """(nx + 1) * (ny + 1) vertices on z = 0, x and y multiples of ``step`` (exact in float32), every square split along the same
    diagonal: an open mesh whose boundary vertices are its rim.  Vertex (i, j) has index i * (ny + 1) + j."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.stack((i.ravel() * step, j.ravel() * step, np.zeros(i.size)), 1).astype(np.float32)
    idx = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    p, q, r, s = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return v, np.concatenate([np.stack([p, q, r], 1), np.stack([p, r, s], 1)]).astype(np.int32)


def grid_rim(nx, ny):
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    return ((i == 0) | (i == nx) | (j == 0) | (j == ny)).ravel()


def odd_mesh():
    """Three faces round the corner of a tetrahedron (open), one of them twice, a face (a, a, b), a face (a, a, a) and a vertex no
    face names: (vertices [6,3], faces)."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 2, 2], [0.5, 0.5, 3]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [0, 1, 3], [4, 4, 1], [2, 2, 2]], np.int32)
    return v, f


def noisy_sphere(vertices, sigma=0.02, seed=0):
    """The unit icosphere with radial noise: v + standard_normal((Nv, 1)) * sigma * v, drawn from default_rng(seed)."""
    v = np.asarray(vertices, np.float32)
    return (v + np.random.default_rng(seed).standard_normal((len(v), 1)) * sigma * v).astype(np.float32)


def radius_stats(vertices):
    """(the RMS deviation of |v| from its mean, the mean of |v|), float64."""
    r = np.linalg.norm(np.asarray(vertices, np.float64), axis=1)
    return float(np.sqrt(np.mean((r - r.mean()) ** 2))), float(r.mean())
