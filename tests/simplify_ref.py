"""Numpy restatement of meshops.simplify_clustering (pmn_mesh_remap_faces, pmn_mesh_cluster_place and the torch around them; DESIGN.md
section 28): the yardstick of tests/test_simplify_ref.py and tests/test_simplify_gpu.py.  Test infrastructure: nothing in the product
imports it.

Every sum runs in the kernels' order (a run in ascending (face, corner) order; a run longer than LONG_RUN over 64 lanes and
pmn_voxel_mean's butterfly), every expression in the header's order.  ``dtype`` is the arithmetic of the placement: np.float64 restates
the kernel, np.longdouble is the same text at 64 bits of mantissa, the reference the positions are held to.  The cells, the cluster
means (float32, tnt_ref._run_mean) and the integers are the same for both."""
from __future__ import annotations

import numpy as np

import tnt_ref

LONG_RUN = 256  # PMN_MESH_PLACE_LONG_RUN of include/pmn_hip.h
N_SUMS = 10     # Sxx Sxy Sxz Syy Syz Szz tx ty tz W


def clusters(vertices, cell, origin=None):
    """(cluster [Nv] int64, cells [m,3] int64 in ascending key order, order [Nv] the stable sort, starts [m+1], origin float64 [3])."""
    v = np.asarray(vertices, np.float32)
    origin = v.min(0).astype(np.float64) - cell / 2 if origin is None else np.asarray(origin, np.float64)
    c = np.floor((v.astype(np.float64) - origin) / cell).astype(np.int64)
    order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))  # stable; the last key is primary: ascending (z, y, x), the key's order
    cs = c[order]
    head = np.r_[True, (cs[1:] != cs[:-1]).any(1)]
    starts = np.r_[np.flatnonzero(head), len(v)]
    cluster = np.empty(len(v), np.int64)
    cluster[order] = np.cumsum(head) - 1
    return cluster, cs[head], order, starts, origin


def _sum_run(rows, dtype):
    """The N_SUMS sums of one run [len, N_SUMS] as pmn_mesh_cluster_place adds them."""
    if len(rows) <= LONG_RUN:
        s = np.zeros(N_SUMS, dtype)
        for row in rows:
            s = s + row
        return s
    lanes = np.zeros((64, N_SUMS), dtype)
    for i, row in enumerate(rows):
        lanes[i % 64] = lanes[i % 64] + row
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(64) ^ o]
    return lanes[0]


def canonical_face_order(faces):
    """The faces by (vertex triple rotated so that the smallest index comes first, the rotation), equal ones in input order."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    shift = np.where((b < a) & (b < c), 1, np.where((c < a) & (c < b), 2, 0))
    rot = np.stack([f[np.arange(len(f)), (shift + k) % 3] for k in range(3)], 1) if len(f) else f
    return np.lexsort((shift, rot[:, 2], rot[:, 1], rot[:, 0]))


def place(vertices, faces, cluster, cells, mean, origin, cell, stiffness, dtype=np.float64, return_condition=False):
    """Unrounded representatives [m,3] in ``dtype`` (the kernel stores their float32 rounding) and, on request, the condition number of
    every cluster's system (1 where it has no weight), from numpy's eigenvalues in float64."""
    T = dtype
    v = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    m = len(cells)
    half = T(0.5)
    ctr = np.asarray(origin, np.float64).astype(T) + (cells.astype(T) + half) * T(cell)          # [m,3]
    f = f[canonical_face_order(f)]  # simplify_clustering hands the kernel the faces in this order, not the array's
    corner_cluster = cluster[f].reshape(-1)
    by_cluster = np.argsort(corner_cluster, kind="stable")
    starts = np.searchsorted(corner_cluster[by_cluster], np.arange(m + 1))
    face = by_cluster // 3
    cc = ctr[corner_cluster[by_cluster]]                                                            # every entry's centre
    with np.errstate(all="ignore"):
        a = v[f[face, 0]].astype(T) - cc
        b = v[f[face, 1]].astype(T) - cc
        c = v[f[face, 2]].astype(T) - cc
        e1, e2 = b - a, c - a
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        w = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok = (w > 0) & np.isfinite(w)
        ws = np.where(ok, w, T(1))
        hx, hy, hz = nx / ws, ny / ws, nz / ws
        q = (hx * a[:, 0] + hy * a[:, 1]) + hz * a[:, 2]
        gx, gy, gz = w * hx, w * hy, w * hz
        rows = np.stack((gx * hx, gx * hy, gx * hz, gy * hy, gy * hz, gz * hz, q * gx, q * gy, q * gz, w), 1).astype(T)
    out = np.zeros((m, 3), T)
    cond = np.ones(m)
    h = T(cell) * half
    for r in range(m):
        sel = np.arange(starts[r], starts[r + 1])
        S = _sum_run(rows[sel[ok[sel]]] if len(sel) <= LONG_RUN else np.where(ok[sel, None], rows[sel], T(0)), T)
        mt = np.asarray(mean[r], np.float32).astype(T) - ctr[r]
        x = mt.copy()
        W = S[9]
        if W > 0 and np.isfinite(W):
            lam = T(stiffness) * W
            d0 = S[0] + lam
            l10, l20 = S[1] / d0, S[2] / d0
            d1 = (S[3] + lam) - l10 * S[1]
            u = S[4] - l10 * S[2]
            l21 = u / d1
            d2 = ((S[5] + lam) - l20 * S[2]) - l21 * u
            y0 = S[6] + lam * mt[0]
            y1 = (S[7] + lam * mt[1]) - l10 * y0
            y2 = ((S[8] + lam * mt[2]) - l20 * y0) - l21 * y1
            z = y2 / d2
            y = y1 / d1 - l21 * z
            x = np.array([(y0 / d0 - l10 * y) - l20 * z, y, z], T)
            if return_condition:
                A = np.array([[S[0] + lam, S[1], S[2]], [S[1], S[3] + lam, S[4]], [S[2], S[4], S[5] + lam]], np.float64)
                ev = np.linalg.eigvalsh(A)
                cond[r] = ev[-1] / ev[0]
        x = np.where(x > h, h, x)
        x = np.where(x < -h, -h, x)
        out[r] = ctr[r] + x
    return (out, cond) if return_condition else out


def remap_faces(faces, cluster):
    """(triples [Nt,3] rotated so that the smallest cluster comes first, dropped [Nt] bool: two corners in one cluster)."""
    t = cluster[np.asarray(faces, np.int64).reshape(-1, 3)]
    dropped = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
    shift = np.where((t[:, 1] < t[:, 0]) & (t[:, 1] < t[:, 2]), 1, np.where((t[:, 2] < t[:, 0]) & (t[:, 2] < t[:, 1]), 2, 0))
    rot = np.stack([t[np.arange(len(t)), (shift + k) % 3] for k in range(3)], 1) if len(t) else t
    return np.where(dropped[:, None], t, rot), dropped


def simplify(vertices, faces, cell, colors=None, normals=None, origin=None, placement="quadric", stiffness=1e-3, dtype=np.float64,
             return_condition=False):
    """dict(vertices float32 [n,3], exact [n,3] in ``dtype`` (before the one rounding), faces int32, colors uint8 | None, normals float32
    | None, vertex_map int32 [Nv], cluster [Nv], cells, origin, kept_clusters[, condition [n]])."""
    v = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cluster, cells, order, starts, origin = clusters(v, cell, origin)
    m = len(cells)
    cols = [np.asarray(t).astype(np.float32) for t in (colors, normals) if t is not None]
    table = np.concatenate([v] + cols, 1)[order]
    means = np.stack([tnt_ref._run_mean(table[starts[r]:starts[r + 1]]) for r in range(m)])
    mean = means[:, :3]
    out_colors = out_normals = None
    if colors is not None:
        out_colors = np.clip(np.floor(means[:, 3:6] + np.float32(0.5)), 0, 255).astype(np.uint8)
    if normals is not None:
        n64 = means[:, -3:].astype(np.float64)
        with np.errstate(all="ignore"):
            length = np.sqrt((n64[:, 0] * n64[:, 0] + n64[:, 1] * n64[:, 1]) + n64[:, 2] * n64[:, 2])
            ok = (length > 0) & np.isfinite(length)
            out_normals = np.where(ok[:, None], n64 / np.where(ok, length, 1.0)[:, None], 0.0).astype(np.float32)
    cond = None
    if placement == "quadric":
        rep = place(v, f, cluster, cells, mean, origin, cell, stiffness, dtype, return_condition)
        if return_condition:
            rep, cond = rep
    else:
        rep = mean.astype(dtype)
    tri, dropped = remap_faces(f, cluster)
    seen, fkeep = set(), np.zeros(len(f), bool)
    for i, t in enumerate(map(tuple, tri.tolist())):
        if not dropped[i] and t not in seen:
            seen.add(t)
            fkeep[i] = True
    named = np.zeros(m, bool)
    named[tri[fkeep].reshape(-1)] = True
    new = np.full(m, -1, np.int64)
    new[named] = np.arange(int(named.sum()))
    pick = lambda a: None if a is None else a[named]
    out = {"vertices": rep[named].astype(np.float32), "exact": rep[named], "faces": new[tri[fkeep]].astype(np.int32).reshape(-1, 3),
           "colors": pick(out_colors), "normals": pick(out_normals), "vertex_map": new[cluster].astype(np.int32), "cluster": cluster,
           "cells": cells, "origin": origin, "kept_clusters": np.flatnonzero(named), "mean": mean[named], "exact_all": rep,
           "mean_all": mean}
    if cond is not None:
        out["condition"] = cond[named]
        out["condition_all"] = cond
    return out


# ---- meshes ----------------------------------------------------------------------------------------------------------------------

def grid_plane(n, step=0.125, a=0.5, b=0.25, c=3.0):
    """(n + 1)^2 vertices on z = a x + b y + c, x and y multiples of ``step``: every coordinate is exact in float32."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    x, y = i.ravel() * step, j.ravel() * step
    v = np.stack((x, y, a * x + b * y + c), 1).astype(np.float32)
    idx = np.arange((n + 1) ** 2).reshape(n + 1, n + 1)
    p, q, r, s = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return v, np.concatenate([np.stack([p, q, r], 1), np.stack([p, r, s], 1)]).astype(np.int32)


def cube(n):
    """The surface of the unit cube, n x n squares a side, outward winding, vertices shared along the edges: closed, 12 n^2 faces."""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            for i in range(n):
                for j in range(n):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side * n, i + di, j + dj
                        quad.append(vid(tuple(p)))
                    if not side:
                        quad = quad[::-1]
                    faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    return (np.asarray(verts, np.float64) / n).astype(np.float32), np.asarray(faces, np.int32)


def fan(n, radius=1.0, centre=(0.0, 0.0, 0.0), lift=0.3):
    """n faces round vertex 0 (a cone of height ``lift``): vertex 0 is a corner of every face."""
    ang = 2 * np.pi * np.arange(n) / n
    rim = np.stack((radius * np.cos(ang), radius * np.sin(ang), np.zeros(n)), 1)
    v = (np.concatenate([[[0.0, 0.0, lift]], rim]) + np.asarray(centre, np.float64)).astype(np.float32)
    k = np.arange(n)
    return v, np.stack((np.zeros(n, np.int64), 1 + k, 1 + (k + 1) % n), 1).astype(np.int32)


def two_sheets():
    """The sheets z = 0 and z = 0.25 + 0.25 x over [0, 2]^2 (every coordinate exact in float32), with the lattice that puts both into
    one layer of cells for x < 0.96: (vertices, faces, cell, origin).  Their planes meet at x = -1, outside every such cell, so the
    unclamped minimiser leaves the cell."""
    a, b = grid_plane(16, a=0.0, b=0.0, c=0.0), grid_plane(16, a=0.25, b=0.0, c=0.25)
    v = np.concatenate([a[0], b[0]])
    return v, np.concatenate([a[1], b[1] + len(a[0])]).astype(np.int32), 0.5, (-0.25, -0.25, -0.01)


def face_set(faces):
    return set(map(tuple, np.asarray(faces).tolist()))
