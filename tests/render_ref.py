"""Numpy restatement of csrc/render.hip: the yardstick of tests/test_render_io.py and tests/test_render_gpu.py.
Test infrastructure, like tsdf_ref.py: nothing in the product imports it.

The projection and the depth are evaluated in ``dtype`` in the order the kernel's header comment states (numpy never contracts a
multiply-add, its float32 division and square root are IEEE, np.rint rounds half to even: dtype=float32 is expected to reproduce the
kernel's bits); dtype=float64 is the same computation carried out wide, and the difference between the two sizes the gates.  Coverage is
int64 arithmetic on the snapped coordinates: exact.  The z-buffer is "smallest depth, then smallest index" taken in two order-free
passes (np.minimum.at), which for float32 is the order of the kernel's uint64 keys."""
from __future__ import annotations

import numpy as np

GUARD = 1 << 22          # units of 1/256 px
MAX_BOX = 64             # PMN_RASTER_MAX_BOX
SPLAT_MAX_RADIUS = 32    # PMN_SPLAT_MAX_RADIUS


def project(points, cam, dtype=np.float32):
    """-> pc [n,3] (dtype), X, Y int64 (1/256 px), state int8: 0 drawable, 1 behind / non-finite, 2 outside the guard band."""
    T = dtype
    cam = np.asarray(cam, np.float32).astype(T)
    K, E = cam[:9], cam[9:]
    p = np.asarray(points, np.float32).astype(T)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        pc = np.stack([((E[4 * r] * x + E[4 * r + 1] * y) + E[4 * r + 2] * z) + E[4 * r + 3] for r in range(3)], 1)
        front = np.isfinite(pc).all(1) & (pc[:, 2] > 0)
        q = [(K[3 * r] * pc[:, 0] + K[3 * r + 1] * pc[:, 1]) + K[3 * r + 2] * pc[:, 2] for r in range(3)]
        su, sv = np.rint((q[0] / q[2]) * T(256)), np.rint((q[1] / q[2]) * T(256))
        band = (np.abs(su) <= GUARD) & (np.abs(sv) <= GUARD)
    state = np.where(~front, 1, np.where(~band, 2, 0)).astype(np.int8)
    ok = state == 0
    X = np.where(ok, su, 0).astype(np.int64)
    Y = np.where(ok, sv, 0).astype(np.int64)
    return pc, X, Y, state


class ZBuffer:
    """depth (dtype, inf = untouched) and index (int64, -1) per pixel; ``put`` takes candidates in any order."""

    def __init__(self, h, w, dtype, count_hits=False):
        self.h, self.w, self.T = h, w, dtype
        self.cand = []
        self.hits = np.zeros(h * w, np.int64) if count_hits else None

    def put(self, pix, depth, index):
        with np.errstate(all="ignore"):
            ok = (depth > 0) & (depth < np.inf)
        self.cand.append((pix[ok], depth[ok].astype(self.T), index[ok].astype(np.int64)))
        if self.hits is not None:
            np.add.at(self.hits, pix[ok], 1)

    def finish(self):
        depth = np.full(self.h * self.w, np.inf, self.T)
        index = np.full(self.h * self.w, np.iinfo(np.int64).max, np.int64)
        for pix, d, _ in self.cand:
            np.minimum.at(depth, pix, d)
        for pix, d, i in self.cand:
            win = d == depth[pix]
            np.minimum.at(index, pix[win], i[win])
        hit = depth < np.inf
        return np.where(hit, depth, 0).reshape(self.h, self.w), np.where(hit, index, -1).reshape(self.h, self.w)


def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _setup(vertices, faces, cam, h, w, dtype):
    f = np.asarray(faces, np.int64)
    nv = len(vertices)
    valid = ((f >= 0) & (f < nv)).all(1)
    fs = np.where(valid[:, None], f, 0)
    pc, X, Y, state = project(vertices, cam, dtype)
    st = state[fs]
    behind = ~valid | (st == 1).any(1)
    band = ~behind & (st == 2).any(1)
    X3, Y3, z3 = X[fs], Y[fs], pc[fs, 2]
    area = _orient(X3[:, 0], Y3[:, 0], X3[:, 1], Y3[:, 1], X3[:, 2], Y3[:, 2])
    zero = ~behind & ~band & (area == 0)
    draw = ~behind & ~band & ~zero
    s = np.where(area > 0, 1, -1).astype(np.int64)
    px0 = np.maximum((X3.min(1) + 255) >> 8, 0)
    px1 = np.minimum(X3.max(1) >> 8, w - 1)
    py0 = np.maximum((Y3.min(1) + 255) >> 8, 0)
    py1 = np.minimum(Y3.max(1) >> 8, h - 1)
    return dict(fs=fs, pc=pc, X=X3, Y=Y3, z=z3, area=area, s=s, draw=draw, px0=px0, px1=px1, py0=py0, py1=py1,
                counts=(int(behind.sum()), int(band.sum()), int(zero.sum())))


def _edge_values(S, t, Px, Py):
    """s * w_i [3, ...] and coverage at the pixel centres (Px, Py) (1/256 px) for the triangles ``t`` (index array; broadcast)."""
    X, Y, s = S["X"][t], S["Y"][t], S["s"][t]
    ws, inside = [], True
    for i, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
        wi = s * _orient(X[..., a], Y[..., a], X[..., b], Y[..., b], Px, Py)
        dx, dy = s * (X[..., b] - X[..., a]), s * (Y[..., b] - Y[..., a])
        top_left = (dy < 0) | ((dy == 0) & (dx > 0))
        inside = inside & ((wi > 0) | ((wi == 0) & top_left))
        ws.append(wi)
    return ws, inside


def _inv_depth_terms(S, t, ws, T):
    with np.errstate(all="ignore"):
        fa = (S["s"][t] * S["area"][t]).astype(T)
        return [(ws[i].astype(T) / fa) / S["z"][t][..., i] for i in range(3)]


def raster_triangles(vertices, faces, cam, h, w, dtype=np.float32, max_box=MAX_BOX, count_hits=False):
    """-> dict(depth [h,w] dtype, index [h,w] int64 (-1), counters (behind, band, zero area, large), hits [h,w] | None)."""
    T = dtype
    S = _setup(vertices, faces, cam, h, w, dtype)
    zb = ZBuffer(h, w, T, count_hits)
    bw, bh = S["px1"] - S["px0"] + 1, S["py1"] - S["py0"] + 1
    live = S["draw"] & (bw > 0) & (bh > 0)
    large = int((live & (bw * bh > max_box)).sum())
    small = np.nonzero(live & (bw <= 16) & (bh <= 16))[0]
    for oy in range(int(bh[small].max()) if len(small) else 0):
        for ox in range(int(bw[small].max()) if len(small) else 0):
            t = small[(bw[small] > ox) & (bh[small] > oy)]
            if not len(t):
                continue
            px, py = S["px0"][t] + ox, S["py0"][t] + oy
            ws, inside = _edge_values(S, t, px << 8, py << 8)
            t, px, py, ws = t[inside], px[inside], py[inside], [x[inside] for x in ws]
            c = _inv_depth_terms(S, t, ws, T)
            with np.errstate(all="ignore"):
                zb.put(py * w + px, T(1) / ((c[0] + c[1]) + c[2]), t)
    for t in np.nonzero(live & ((bw > 16) | (bh > 16)))[0]:
        py, px = np.meshgrid(np.arange(S["py0"][t], S["py1"][t] + 1), np.arange(S["px0"][t], S["px1"][t] + 1), indexing="ij")
        tt = np.full(px.shape, t)
        ws, inside = _edge_values(S, tt, px << 8, py << 8)
        tt, px, py, ws = tt[inside], px[inside], py[inside], [x[inside] for x in ws]
        c = _inv_depth_terms(S, tt, ws, T)
        with np.errstate(all="ignore"):
            zb.put(py * w + px, T(1) / ((c[0] + c[1]) + c[2]), tt)
    depth, index = zb.finish()
    return dict(depth=depth, index=index, counters=S["counts"] + (large,),
                hits=None if zb.hits is None else zb.hits.reshape(h, w))


def splat_points(points, cam, h, w, dtype=np.float32, radius_px=0.0, radius_world=0.0, chunk=1 << 21):
    """-> dict(depth, index, counters (behind, band))."""
    T = dtype
    pc, X, Y, state = project(points, cam, dtype)
    zb = ZBuffer(h, w, T)
    ok = np.nonzero(state == 0)[0]
    fx = np.asarray(cam, np.float32).astype(T)[0]
    for a in range(0, len(ok), chunk):
        t = ok[a:a + chunk]
        x, y, z = X[t], Y[t], pc[t, 2]
        nx, ny = (x + 128) >> 8, (y + 128) >> 8
        if radius_world > 0:
            with np.errstate(all="ignore"):
                r = np.minimum((T(np.float32(radius_world)) * fx) / z, T(SPLAT_MAX_RADIUS))
        else:
            r = np.full(len(t), T(np.float32(radius_px)))
        Rq = np.rint(r * T(256)).astype(np.int64)
        near = Rq < 128
        s = near & (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
        zb.put(ny[s] * w + nx[s], z[s], t[s])
        t, x, y, z, nx, ny, Rq = (v[~near] for v in (t, x, y, z, nx, ny, Rq))
        if not len(t):
            continue
        px0, px1 = np.maximum((x - Rq + 255) >> 8, 0), np.minimum((x + Rq) >> 8, w - 1)
        py0, py1 = np.maximum((y - Rq + 255) >> 8, 0), np.minimum((y + Rq) >> 8, h - 1)
        for oy in range(int((py1 - py0).max()) + 1):
            for ox in range(int((px1 - px0).max()) + 1):
                px, py = px0 + ox, py0 + oy
                dx, dy = (px << 8) - x, (py << 8) - y
                s = (px <= px1) & (py <= py1) & ((dx * dx + dy * dy <= Rq * Rq) | ((px == nx) & (py == ny)))
                zb.put(py[s] * w + px[s], z[s], t[s])
    depth, index = zb.finish()
    return dict(depth=depth, index=index, counters=(int((state == 1).sum()), int((state == 2).sum())))


def _byte(c):
    with np.errstate(all="ignore"):
        return np.clip(np.floor(c + c.dtype.type(0.5)), 0, 255).astype(np.uint8)


def resolve(depth, index, cam, vertices, faces, dtype=np.float32, colors=None, normals=None, shade=False):
    """rgb [h,w,3] uint8 and camera-frame normal [h,w,3] (dtype) of the winners in (depth, index), as pmn_raster_resolve states them."""
    T = dtype
    h, w = depth.shape
    hit = index >= 0
    py, px = np.nonzero(hit)
    idx = index[hit]
    d = depth[hit].astype(T)
    E = np.asarray(cam, np.float32).astype(T)[9:]
    n_pix = len(idx)
    col = np.full((n_pix, 3), T(128))
    n = np.zeros((n_pix, 3), T)
    with np.errstate(all="ignore"):
        if faces is not None:
            S = _setup(vertices, faces, cam, h, w, dtype)
            ws, _ = _edge_values(S, idx, px << 8, py << 8)
            c = _inv_depth_terms(S, idx, ws, T)
            f = S["fs"][idx]
            interp = lambda a: ((c[0][:, None] * a[f[:, 0]] + c[1][:, None] * a[f[:, 1]]) + c[2][:, None] * a[f[:, 2]]) * d[:, None]
            p = interp(S["pc"])
            if colors is not None:
                col = interp(np.asarray(colors).astype(T))
            if normals is not None:
                nw = interp(np.asarray(normals, np.float32).astype(T))
                n = np.stack([(E[4 * r] * nw[:, 0] + E[4 * r + 1] * nw[:, 1]) + E[4 * r + 2] * nw[:, 2] for r in range(3)], 1)
            else:
                a, b = S["pc"][f[:, 1]] - S["pc"][f[:, 0]], S["pc"][f[:, 2]] - S["pc"][f[:, 0]]
                n = np.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                              a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), 1)
        else:
            p = project(np.asarray(vertices)[idx], cam, dtype)[0]
            if colors is not None:
                col = np.asarray(colors)[idx].astype(T)
            if normals is not None:
                nw = np.asarray(normals, np.float32)[idx].astype(T)
                n = np.stack([(E[4 * r] * nw[:, 0] + E[4 * r + 1] * nw[:, 1]) + E[4 * r + 2] * nw[:, 2] for r in range(3)], 1)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        good = (ln > 0) & (ln < np.inf)
        n = np.where(good[:, None], n / ln[:, None], T(0))
        dot = (n[:, 0] * p[:, 0] + n[:, 1] * p[:, 1]) + n[:, 2] * p[:, 2]
        n = np.where((dot > 0)[:, None], -n, n)
        plen = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        lambert = np.where(good & (plen > 0) & bool(shade), np.abs(dot) / plen, T(1))
        rgb = np.zeros((h, w, 3), np.uint8)
        rgb[hit] = _byte(col * lambert[:, None])
    normal = np.zeros((h, w, 3), T)
    normal[hit] = n
    return rgb, normal


# ---- generated models -----------------------------------------------------------------------------------------------------------------

def icosphere(level, centre=(0.0, 0.0, 0.0), radius=1.0):
    """(vertices [n,3] float32, faces [m,3] int32) of an icosahedron subdivided ``level`` times, outward winding, on the sphere."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(centre) + radius * np.asarray(v)).astype(np.float32), np.asarray(f, np.int32)


def chord_sag(vertices, faces, centre, radius):
    """The largest distance between the sphere and an inscribed flat triangle of the mesh, exactly: a flat triangle with its corners on
    the sphere is farthest from it at its circumcentre, at radius * (1 - cos(alpha)) with alpha the angle between the triangle's unit
    normal (through the circumcentre) and a corner.  (The circumcentre lies inside every icosphere triangle: they are acute.)  For icosphere(level) this is the bound the
    subdivision level gives: 0.2053, 0.0658, 0.01775, 0.004528, 0.001138 radii at levels 0..4, a factor 3.1 .. 3.98 per level (a step
    halves every arc; the centre triangle of a step comes out a little larger than the corner ones, hence not exactly 4)."""
    p = (np.asarray(vertices, np.float64) - np.asarray(centre, np.float64))[np.asarray(faces)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n /= np.linalg.norm(n, axis=1)[:, None]
    return float((radius - np.abs((n * p[:, 0]).sum(1))).max())


def plane_grid(nu, nv, origin, eu, ev, winding=1, jitter=0.0, seed=0):
    """(vertices, faces): a closed tessellation of the parallelogram origin + a eu + b ev, (nu + 1) x (nv + 1) vertices, two triangles
    per cell with alternating diagonals; interior vertices moved inside the plane by ``jitter`` (fraction of a cell) so that the edges
    have general directions."""
    rng = np.random.default_rng(seed)
    a, b = np.meshgrid(np.arange(nu + 1, dtype=np.float64), np.arange(nv + 1, dtype=np.float64), indexing="xy")
    ja, jb = rng.uniform(-jitter, jitter, a.shape), rng.uniform(-jitter, jitter, a.shape)
    inner = (a > 0) & (a < nu) & (b > 0) & (b < nv)
    a, b = a + ja * inner, b + jb * inner
    v = np.asarray(origin, float) + (a / nu)[..., None] * np.asarray(eu, float) + (b / nv)[..., None] * np.asarray(ev, float)
    idx = lambda i, j: j * (nu + 1) + i
    f = []
    for j in range(nv):
        for i in range(nu):
            p, q, r, s = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            f += [(p, q, r), (p, r, s)] if (i + j) % 2 == 0 else [(p, q, s), (q, r, s)]
    f = np.asarray(f, np.int32)
    return v.reshape(-1, 3).astype(np.float32), f if winding > 0 else np.ascontiguousarray(f[:, ::-1])


def spoiled(vertices, faces, seed=0):
    """The mesh plus a share of triangles that must not be drawn: copies of faces with one vertex moved far behind every camera of the
    rigs used here, with a NaN / an inf vertex, with a repeated vertex and with three collinear snapped positions (a vertex used
    three times), and a face with an index out of range."""
    rng = np.random.default_rng(seed)
    v, f = [np.asarray(vertices, np.float32)], [np.asarray(faces, np.int32)]
    n, m = len(vertices), len(faces)
    pick = rng.choice(m, size=min(m, 200), replace=False)
    extra = np.asarray(vertices, np.float32)[faces[pick, 0]].copy()
    extra[0::4, 2] -= 1000.0     # behind
    extra[1::4, 0] = np.nan
    extra[2::4, 1] = np.inf
    extra[3::4, 2] -= 1000.0
    v.append(extra)
    bad = faces[pick].copy()
    bad[:, 0] = n + np.arange(len(pick))
    f.append(bad)
    dup = faces[rng.choice(m, size=min(m, 100), replace=False)].copy()
    dup[:, 2] = dup[:, 1]        # zero area
    f.append(dup)
    same = faces[rng.choice(m, size=min(m, 50), replace=False)].copy()
    same[:, 1] = same[:, 0]
    same[:, 2] = same[:, 0]      # a point
    f.append(same)
    f.append(np.asarray([[0, 1, n + len(extra) + 7], [-1, 0, 1]], np.int32))  # indices out of range
    order = rng.permutation(sum(len(x) for x in f))
    return np.concatenate(v), np.ascontiguousarray(np.concatenate(f)[order])


def point_cloud(n, target, seed=0):
    """n points in a box around ``target`` (the rigs here look at it from 4 units), with points behind the cameras, non-finite points
    and exact duplicates (equal depths: the lowest index must win) mixed in."""
    rng = np.random.default_rng(seed)
    p = (np.asarray(target, np.float32) + rng.uniform(-1, 1, (n, 3)).astype(np.float32) * np.float32([2.0, 1.6, 1.2])).astype(np.float32)
    k = max(n // 1000, 4)
    p[0:k, 2] -= 100.0
    p[k:2 * k, 0] = np.nan
    p[2 * k:3 * k] = p[3 * k:4 * k]
    p[4 * k:5 * k] *= np.float32(3e4)  # far outside the guard band (or behind)
    return p


# ---- the cases of tests/test_render_io.py (reduced) and tests/test_render_gpu.py (full size) ---------------------------------------------

TARGET = (0.013, -0.021, 5.0)


def case_camera(h, w, distance=4.0, view=1):
    """One camera of tsdf_ref.rig (skew, fx != fy, off-centre principal point) looking at TARGET: (K, E, cam21)."""
    import tsdf_ref as R
    K, E = R.rig(3, h, w, TARGET, distance)
    return K[view], E[view], R.cam21(K[view], E[view])


def mt_lattice(n):
    """The sphere field the 'mt' case extracts its mesh from, and the lattice's placement: (field [n,n,n], origin, voxel)."""
    import tsdf_ref as R
    voxel = np.float32(2.4 / n)
    origin = (np.asarray(TARGET) - 1.2).astype(np.float32)
    return R.sphere_field(n, (0.48 * n, 0.5 * n, 0.49 * n), 0.36 * n), origin, voxel


def case_attributes(vertices, seed=0):
    """(colors [n,3] uint8 random, normals [n,3] float32: the unit direction from TARGET, zero for a tenth of the vertices)."""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, np.float64)
    col = rng.integers(0, 256, (len(v), 3), dtype=np.uint8)
    with np.errstate(all="ignore"):
        d = v - np.asarray(TARGET)
        n = np.nan_to_num(d / np.linalg.norm(d, axis=1)[:, None], nan=0.0, posinf=0.0, neginf=0.0)
    n[rng.random(len(v)) < 0.1] = 0
    return col, n.astype(np.float32)


def compare_oracles(o32, o64):
    """The pixels on which the float32 and float64 oracles took the same decision, and their share: (same [h,w] bool, covered count,
    excluded count)."""
    same = o32["index"] == o64["index"]
    return same, int((o32["index"] >= 0).sum()), int((~same).sum())
