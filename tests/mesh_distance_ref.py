"""Numpy restatement of pmn_mesh_distance (include/pmn_hip.h): the distance from points to a triangle mesh as a
brute force over all (query, face) pairs, in the formulation of the kernel and in a floating-point type of the caller's choice.  With
np.float64 every operation is the kernel's, in its order; with np.longdouble (the default) it is the yardstick the kernel is gated by.

    segment(P, Q)  e = Q - P, w = q - P, l2 = e.e, t = l2 > 0 ? (w.e) / l2 : 0 clamped to [0, 1], c = P + t e, d2 = |q - c|^2
    plane          n = (B - A) x (C - A), nn = n.n; only if nn > 0 and the projection is inside: d2 = (w.n)^2 / nn, c = q - ((w.n) / nn) n
    face           the least of segment(A, B), segment(B, C), segment(C, A), plane -- the first among equals

No helper here imports the package under test."""
import numpy as np

TWO_M52 = 2.0 ** -52


def _dot(ax, ay, az, bx, by, bz):
    return ax * bx + ay * by + az * bz


def _segment(P, Q, q, best):
    ex, ey, ez = Q[0] - P[0], Q[1] - P[1], Q[2] - P[2]
    wx, wy, wz = q[0] - P[0], q[1] - P[1], q[2] - P[2]
    l2 = _dot(ex, ey, ez, ex, ey, ez)
    ok = l2 > 0
    t = np.where(ok, _dot(wx, wy, wz, ex, ey, ez) / np.where(ok, l2, 1), 0)
    t = np.where(t < 0, 0, np.where(t > 1, 1, t)).astype(l2.dtype)
    sx, sy, sz = P[0] + t * ex, P[1] + t * ey, P[2] + t * ez
    dx, dy, dz = q[0] - sx, q[1] - sy, q[2] - sz
    s2 = _dot(dx, dy, dz, dx, dy, dz)
    if best is None:
        return [s2, sx, sy, sz]
    take = s2 < best[0]
    return [np.where(take, new, old) for new, old in zip((s2, sx, sy, sz), best)]


def point_triangle(q, A, B, C, dtype=np.longdouble):
    """(d2, closest) of the points q [..., 3] and the triangles A, B, C [..., 3] (broadcast against each other), computed in ``dtype``."""
    q, A, B, C = (np.asarray(x).astype(dtype) for x in (q, A, B, C))
    q, A, B, C = np.broadcast_arrays(q, A, B, C)
    q, A, B, C = ([x[..., k] for k in range(3)] for x in (q, A, B, C))
    best = _segment(A, B, q, None)
    best = _segment(B, C, q, best)
    best = _segment(C, A, q, best)
    e1x, e1y, e1z = B[0] - A[0], B[1] - A[1], B[2] - A[2]
    e2x, e2y, e2z = C[0] - A[0], C[1] - A[1], C[2] - A[2]
    nx, ny, nz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
    nn = _dot(nx, ny, nz, nx, ny, nz)
    area = nn > 0
    nn1 = np.where(area, nn, 1)
    wx, wy, wz = q[0] - A[0], q[1] - A[1], q[2] - A[2]
    ux, uy, uz = e1y * wz - e1z * wy, e1z * wx - e1x * wz, e1x * wy - e1y * wx
    vx, vy, vz = wy * e2z - wz * e2y, wz * e2x - wx * e2z, wx * e2y - wy * e2x
    u, v = _dot(ux, uy, uz, nx, ny, nz) / nn1, _dot(vx, vy, vz, nx, ny, nz) / nn1
    dp = _dot(wx, wy, wz, nx, ny, nz)
    p2 = (dp * dp) / nn1
    s = dp / nn1
    take = area & (u >= 0) & (v >= 0) & (u + v <= 1) & (p2 < best[0])
    best = [np.where(take, new, old) for new, old in zip((p2, q[0] - s * nx, q[1] - s * ny, q[2] - s * nz), best)]
    return best[0], np.stack(best[1:], -1)


def magnitude(vertices, faces, query):
    """The coordinate magnitude the tolerance is relative to: the largest |coordinate| of the query and of the vertices in use."""
    v = np.asarray(vertices, np.float64)[np.asarray(faces).reshape(-1)]
    return float(max(np.abs(v).max(), np.abs(np.asarray(query, np.float64)).max()))


def brute_force(vertices, faces, query, dtype=np.longdouble, screen=True, chunk=256):
    """The minimum over ALL faces, per query: (d2 [n] dtype, face [n] int64 -- the lowest index among the faces at the minimal d2 --,
    closest [n, 3] dtype, d_all [n, Nt] dtype -- the distance to every face, from which near_faces takes the set of faces that attain
    the minimum within a tolerance).  All faces must be valid.
    ``screen`` (for a dtype wider than float64): every pair is first evaluated in float64 and only the pairs within 2^-20 (relative to
    max(d_min, magnitude)) of a query's float64 minimum are evaluated again in ``dtype`` -- nine orders of magnitude above the float64
    error, so the minimum is that of the full evaluation (tests/test_mesh_distance_ref.py compares the two); d_all is then infinite
    for the pairs screened out."""
    vertices, faces, query = np.asarray(vertices), np.asarray(faces).astype(np.int64), np.asarray(query)
    n, nt = len(query), len(faces)
    mag = magnitude(vertices, faces, query)
    A, B, C = (vertices[faces[:, k]] for k in range(3))
    d2 = np.empty(n, dtype)
    face = np.empty(n, np.int64)
    closest = np.empty((n, 3), dtype)
    d_all = np.empty((n, nt), dtype)
    wide = np.dtype(dtype).itemsize > 8 and screen
    f64 = (np.empty(n), np.empty(n, np.int64), np.empty((n, 3)))  # the float64 evaluation, kept for gate()
    for i0 in range(0, n, chunk):
        q = query[i0:i0 + chunk]
        m = len(q)
        if wide:
            s2, p64 = point_triangle(q[:, None, :], A[None], B[None], C[None], np.float64)
            a64 = s2.argmin(1)
            f64[0][i0:i0 + m], f64[1][i0:i0 + m], f64[2][i0:i0 + m] = s2[np.arange(m), a64], a64, p64[np.arange(m), a64]
            s = np.sqrt(s2)
            smin = s.min(1, keepdims=True)
            qi, fi = np.nonzero(s <= smin + 2.0 ** -20 * np.maximum(smin, mag))
            c2, cc = point_triangle(q[qi], A[fi], B[fi], C[fi], dtype)
            full = np.full((m, nt), np.inf, dtype)
            full[qi, fi] = c2
            pts = np.zeros((m, nt, 3), dtype)
            pts[qi, fi] = cc
        else:
            full, pts = point_triangle(q[:, None, :], A[None], B[None], C[None], dtype)
        arg = full.argmin(1)  # numpy: the first among equals
        rows = np.arange(m)
        d2[i0:i0 + m], face[i0:i0 + m], closest[i0:i0 + m] = full[rows, arg], arg, pts[rows, arg]
        d_all[i0:i0 + m] = np.sqrt(full)
    out = Result((d2, face, closest, d_all))
    out.float64 = f64 if wide else None
    return out


class Result(tuple):
    """brute_force's four results; ``float64`` holds (d2, face, closest) of the float64 screening pass where there was one."""
    float64 = None


def near_faces(d_all, allowed):
    """bool [n, Nt]: the faces whose distance exceeds the query's minimum by at most allowed [n] -- the acceptable answers for `face`
    (ties on shared edges and vertices are the common case, so the arg-min itself is not demanded)."""
    return d_all - d_all.min(1, keepdims=True) <= np.asarray(allowed)[:, None]


def face_distance(vertices, faces, query, face, dtype=np.longdouble):
    """d [n]: the distance from query i to the one face face[i]."""
    vertices, faces = np.asarray(vertices), np.asarray(faces).astype(np.int64)
    f = faces[np.asarray(face)]
    d2, _ = point_triangle(query, vertices[f[:, 0]], vertices[f[:, 1]], vertices[f[:, 2]], dtype)
    return np.sqrt(d2)


def gate(vertices, faces, query, wide=None):
    """The tolerance of the GPU tests, from the yardstick's own error: the disagreement between the float64 and
    the longdouble evaluation of this very formulation on THESE inputs,
        figure = max over queries of |d64 - d_wide| / max(d_wide, magnitude * 2^-52),
    and the gate is 4 x the figure.  The figure is taken separately over the queries ON the surface (d_wide <= magnitude * 2^-26,
    where the error is cancellation in q - c and the denominator is the absolute unit magnitude * 2^-52) and over the others (where
    it is a relative error of d): one figure over both would let the first group's, which is of order 1 to 100, stand as a RELATIVE
    error for the second, and check nothing there.  Each group's figure is at most the common one, so this gate is never wider.  A
    figure is not taken below 2^-52: where float64 happens to be exact, the rounding of the result to float64 still is not an error.
    The nearest POINT is gated in the same way, in the absolute unit: 4 x max |c64 - c_wide| / (magnitude * 2^-52) over the queries
    whose two evaluations chose the same face.
    Returns (allowed_d [n], allowed_c, figures): |d - d_wide| <= allowed_d[i] and |c - c_wide| <= allowed_c per coordinate."""
    mag = magnitude(vertices, faces, query)
    unit = np.longdouble(mag * TWO_M52)
    wide = wide if wide is not None else brute_force(vertices, faces, query)
    d2, face64, c64 = getattr(wide, "float64", None) or brute_force(vertices, faces, query, np.float64)[:3]
    dw = np.sqrt(wide[0])
    denom = np.maximum(dw, unit)
    rel = np.abs(np.sqrt(d2).astype(np.longdouble) - dw) / denom
    on = dw <= np.longdouble(mag * 2.0 ** -26)
    fig_on = max(float(rel[on].max()) if on.any() else 0.0, TWO_M52)
    fig_off = max(float(rel[~on].max()) if (~on).any() else 0.0, TWO_M52)
    same = face64 == wide[1]
    fig_c = max(float((np.abs(c64.astype(np.longdouble) - wide[2])[same] / unit).max()) if same.any() else 0.0, 1.0)
    allowed = 4.0 * np.where(on, fig_on, fig_off) * denom
    return allowed, float(4.0 * fig_c * unit), {"on_surface": fig_on, "off_surface": fig_off, "closest_units": fig_c,
                                                "common": float(rel.max()), "magnitude": mag}


# ---- meshes --------------------------------------------------------------------------------------------------------------------------

def icosphere(level=3, radius=1.0):
    """(vertices float32 [Nv, 3], faces int32 [20 * 4^level, 3]): an icosahedron subdivided ``level`` times, every vertex pushed to the
    sphere in float64 and rounded to float32.  level 3: 642 vertices, 1 280 faces."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return (np.asarray(v) * radius).astype(np.float32), np.asarray(f, np.int32)


def plane_grid(nx, ny, step=1.0, z=0.0, origin=(0.0, 0.0)):
    """A triangulated rectangle of nx x ny squares in the plane z = const: 2 nx ny faces."""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    v = np.stack([origin[0] + xs * step, origin[1] + ys * step, np.full(xs.shape, z)], -1).reshape(-1, 3).astype(np.float32)
    i = (ys[:-1, :-1] * (nx + 1) + xs[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 1, i + nx + 2], 1), np.stack([i, i + nx + 2, i + nx + 1], 1)])
    return v, f.astype(np.int32)
