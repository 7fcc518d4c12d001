"""Numpy restatement of csrc/tsdf.hip: the yardstick of tests/test_tsdf_io.py and tests/test_tsdf_gpu.py.  Test
infrastructure, like normals_ref.py: nothing in the product imports it.

``integrate`` takes every decision and does all arithmetic in ``dtype`` in the order the kernel's header comment states (numpy
never contracts a multiply-add and its float32 division is IEEE, so dtype=float32 is expected to reproduce the kernel's bits);
dtype=float64 is the same computation carried out wide: the difference between the two is the rounding noise of the statement itself
and sizes the gates.  ``extract`` is marching tetrahedra on the Kuhn split written as a plain loop over cells, tetrahedra and
triangles: it DEFINES the order of vertices and faces.  The triangle of a case comes from a parity rule evaluated here, not from the
kernel's table, and the vertex set is simply "every edge some triangle refers to", not the kernel's per-sample rule.
"""
from __future__ import annotations

import itertools

import numpy as np

TETS = []          # (corners (0, a, a|b, 7), orientation +1 / -1)
for _a, _b in ((1, 2), (1, 4), (2, 1), (2, 4), (4, 1), (4, 2)):
    _c = 7 ^ _a ^ _b
    _m = np.array([[(v >> bit) & 1 for bit in range(3)] for v in (_a, _b, _c)], float)  # rows = unit vectors of a, b, c
    TETS.append(((0, _a, _a | _b, 7), int(round(np.linalg.det(_m)))))


def _parity(seq):
    return -1 if sum(1 for x, y in itertools.combinations(seq, 2) if x > y) % 2 else 1


def tet_triangles(inside, orient):
    """Triangles of one tetrahedron: ``inside`` = 4 booleans in tetrahedron order -> list of triangles, each three local edges
    (p, q), p < q, wound so that the normal points from inside to outside for a tetrahedron of orientation ``orient``."""
    ins = [p for p in range(4) if inside[p]]
    out = [p for p in range(4) if not inside[p]]
    e = lambda p, q: (min(p, q), max(p, q))
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1:
        i, (j, k, l) = ins[0], out
        tris, sign = [[e(i, j), e(i, k), e(i, l)]], _parity([i, j, k, l]) * orient
    elif len(ins) == 3:
        o, (j, k, l) = out[0], ins
        tris, sign = [[e(o, j), e(o, k), e(o, l)]], -_parity([o, j, k, l]) * orient
    else:
        (a, b), (c, d) = ins, out
        tris, sign = [[e(a, c), e(a, d), e(b, d)], [e(a, c), e(b, d), e(b, c)]], _parity([a, b, c, d]) * orient
    return tris if sign > 0 else [[t[0], t[2], t[1]] for t in tris]


def new_volume(dims, color=True):
    nx, ny, nz = dims
    v = {"tsdf": np.ones((nz, ny, nx), np.float32), "weight": np.zeros((nz, ny, nx), np.float32), "rgb": None, "cweight": None}
    if color:
        v["rgb"] = np.zeros((3, nz, ny, nx), np.float32)
        v["cweight"] = np.zeros((nz, ny, nx), np.float32)
    return v


def widen(vol, dtype):
    return {k: (None if a is None else a.astype(dtype)) for k, a in vol.items()}


def integrate(vol, origin, voxel, trunc, depth, cam, mask=None, image=None, dtype=np.float32):
    """One view into ``vol`` (in place; the planes must already have ``dtype``).  depth [h,w] float32, cam = 21 floats (K row-major,
    then the upper 3x4 of the extrinsic), mask [h,w] uint8 or None, image [h,w,3] uint8 or None."""
    T = dtype
    nz, ny, nx = vol["tsdf"].shape
    h, w = depth.shape
    cam = np.asarray(cam, np.float32).astype(T)
    K, E = cam[:9], cam[9:]
    o = np.asarray(origin, np.float32).astype(T)
    vx, tr = T(np.float32(voxel)), T(np.float32(trunc))
    x = (o[0] + np.arange(nx).astype(T) * vx)[None, None, :]
    y = (o[1] + np.arange(ny).astype(T) * vx)[None, :, None]
    z = (o[2] + np.arange(nz).astype(T) * vx)[:, None, None]
    with np.errstate(all="ignore"):
        pz = ((E[8] * x + E[9] * y) + E[10] * z) + E[11]
        px = ((E[0] * x + E[1] * y) + E[2] * z) + E[3]
        py = ((E[4] * x + E[5] * y) + E[6] * z) + E[7]
        qx = (K[0] * px + K[1] * py) + K[2] * pz
        qy = (K[3] * px + K[4] * py) + K[5] * pz
        qz = (K[6] * px + K[7] * py) + K[8] * pz
        fx = np.floor(qx / qz + T(0.5))
        fy = np.floor(qy / qz + T(0.5))
        ok = (pz > 0) & (fx >= 0) & (fx < T(w)) & (fy >= 0) & (fy < T(h))
        ix = np.where(ok, fx, 0).astype(np.int64)
        iy = np.where(ok, fy, 0).astype(np.int64)
        d = depth.astype(T)[iy, ix]
        ok &= (d > 0) & (d < np.inf)
        if mask is not None:
            ok &= mask[iy, ix] != 0
        sdf = d - pz
        ok &= ~(sdf < -tr)
        obs = np.minimum(T(1), sdf / tr)
        t, wt = vol["tsdf"], vol["weight"]
        t[...] = np.where(ok, (t * wt + obs) / (wt + T(1)), t)
        wt[...] = np.where(ok, wt + T(1), wt)
        if vol["rgb"] is not None and image is not None:
            okc = ok & (sdf <= tr)
            cw = vol["cweight"]
            for ch in range(3):
                b = image[iy, ix, ch].astype(T)
                vol["rgb"][ch] = np.where(okc, (vol["rgb"][ch] * cw + b) / (cw + T(1)), vol["rgb"][ch])
            cw[...] = np.where(okc, cw + T(1), cw)
    return vol


def extract(tsdf, weight, origin, voxel, min_weight=1.0, rgb=None, cweight=None, normals=True, dtype=np.float32):
    """-> dict(vertices [Nv,3], faces [Nt,3] int32, colors [Nv,3] uint8 | None, normals [Nv,3] | None, vmask, ntri [nz,ny,nx] uint8)."""
    T = dtype
    nz, ny, nx = tsdf.shape
    ok = weight >= np.float32(min_weight)
    inside = tsdf < 0
    live = np.zeros((nz, ny, nx), bool)
    mixed = np.zeros((nz, ny, nx), bool)
    if nx > 1 and ny > 1 and nz > 1:
        cl = np.ones((nz - 1, ny - 1, nx - 1), bool)
        n_in = np.zeros((nz - 1, ny - 1, nx - 1), int)
        for c in range(8):
            sl = (slice(c >> 2, nz - 1 + (c >> 2)), slice((c >> 1) & 1, ny - 1 + ((c >> 1) & 1)), slice(c & 1, nx - 1 + (c & 1)))
            cl &= ok[sl]
            n_in += inside[sl]
        live[:-1, :-1, :-1] = cl
        mixed[:-1, :-1, :-1] = cl & (n_in > 0) & (n_in < 8)
    lin = lambda i, j, k: (k * ny + j) * nx + i
    tris = []  # three (owner, class) keys per triangle, in the contract's order
    ntri = np.zeros((nz, ny, nx), np.uint8)
    for k, j, i in zip(*np.nonzero(mixed)):  # np.nonzero walks z, y, x with x fastest
        count = 0
        for corners, orient in TETS:
            ins = [bool(inside[k + (c >> 2), j + ((c >> 1) & 1), i + (c & 1)]) for c in corners]
            for tri in tet_triangles(ins, orient):
                keys = []
                for p, q in tri:
                    lo, hi = corners[p], corners[q]
                    keys.append((lin(i + (lo & 1), j + ((lo >> 1) & 1), k + (lo >> 2)), hi ^ lo))
                tris.append(keys)
                count += 1
        ntri[k, j, i] = count
    edges = sorted({key for t in tris for key in t})
    index = {key: n for n, key in enumerate(edges)}
    faces = np.array([[index[key] for key in t] for t in tris], np.int32).reshape(-1, 3)
    vmask = np.zeros(nz * ny * nx, np.uint8)
    for owner, cls in edges:
        vmask[owner] |= 1 << (cls - 1)
    own = np.array([e[0] for e in edges], np.int64)
    cls = np.array([e[1] for e in edges], np.int64)
    i0, j0, k0 = own % nx, (own // nx) % ny, own // (nx * ny)
    i1, j1, k1 = i0 + (cls & 1), j0 + ((cls >> 1) & 1), k0 + (cls >> 2)
    o = np.asarray(origin, np.float32).astype(T)
    vx = T(np.float32(voxel))
    tw = tsdf.astype(T)
    v0, v1 = tw[k0, j0, i0], tw[k1, j1, i1]
    t = v0 / (v0 - v1)
    verts = np.empty((len(edges), 3), T)
    for c, (a, b) in enumerate(((i0, i1), (j0, j1), (k0, k1))):
        p0, p1 = o[c] + a.astype(T) * vx, o[c] + b.astype(T) * vx
        verts[:, c] = p0 + t * (p1 - p0)
    out = {"vertices": verts, "faces": faces, "colors": None, "normals": None, "vmask": vmask.reshape(nz, ny, nx), "ntri": ntri}
    if rgb is not None:
        cw0, cw1 = cweight[k0, j0, i0], cweight[k1, j1, i1]
        col = np.empty((len(edges), 3), np.uint8)
        for ch in range(3):
            c0, c1 = rgb[ch].astype(T)[k0, j0, i0], rgb[ch].astype(T)[k1, j1, i1]
            cv = np.where((cw0 > 0) & (cw1 > 0), c0 + t * (c1 - c0), np.where(cw0 > 0, c0, np.where(cw1 > 0, c1, T(128))))
            col[:, ch] = np.clip(np.floor(cv + T(0.5)), 0, 255).astype(np.uint8)
        out["colors"] = col
    if normals:
        def grad(i, j, k):
            good = np.ones(len(i), bool)
            g = np.zeros((len(i), 3), T)
            for c, (di, dj, dk) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
                for s in (-1, 1):
                    ii, jj, kk = i + s * di, j + s * dj, k + s * dk
                    inb = (ii >= 0) & (ii < nx) & (jj >= 0) & (jj < ny) & (kk >= 0) & (kk < nz)
                    good &= inb
                    good[inb] &= ok[kk[inb], jj[inb], ii[inb]]
                inb = good.copy()
                g[inb, c] = tw[k[inb] + dk, j[inb] + dj, i[inb] + di] - tw[k[inb] - dk, j[inb] - dj, i[inb] - di]
            return g, good
        g0, ok0 = grad(i0, j0, k0)
        g1, ok1 = grad(i1, j1, k1)
        g = g0 + t[:, None] * (g1 - g0)
        with np.errstate(all="ignore"):
            ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            good = ok0 & ok1 & (ln > 0) & (ln < np.inf)
            out["normals"] = np.where(good[:, None], g / ln[:, None], T(0)).astype(T)
    return out


# ---- topology of an indexed triangle mesh (vectorised numpy) --------------------------------------------------------------------------

def topology(vertices, faces):
    """dict: closed (every undirected edge in exactly two triangles, once per direction), boundary (the undirected edges used once,
    [n,2]), euler = V - E + F, degenerate (triangles that repeat a vertex), unreferenced (vertices no face uses), volume (signed:
    positive for outward winding)."""
    f = np.asarray(faces, np.int64)
    nv = len(vertices)
    d = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    und = np.sort(d, 1)
    key = und[:, 0] * max(nv, 1) + und[:, 1]
    uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    dkey = d[:, 0] * max(nv, 1) + d[:, 1]
    directed_unique = len(np.unique(dkey)) == len(dkey)
    v = np.asarray(vertices, np.float64)
    vol = float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0) if len(f) else 0.0
    return {"closed": bool(len(f) and (cnt == 2).all() and directed_unique), "boundary": und[np.nonzero(cnt[inv] == 1)[0]],
            "max_edge_use": int(cnt.max()) if len(cnt) else 0, "directed_unique": directed_unique,
            "euler": nv - len(uk) + len(f), "degenerate": int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum()),
            "unreferenced": nv - len(np.unique(f)), "volume": vol}


def sphere_field(n, centre, radius, band=3.0):
    k, j, i = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    d = np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2) - radius
    return np.clip(d / band, -1, 1).astype(np.float32)


def torus_field(n, centre, R, r, band=3.0):
    k, j, i = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    q = np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2) - R
    d = np.sqrt(q ** 2 + (k - centre[2]) ** 2) - r
    return np.clip(d / band, -1, 1).astype(np.float32)


# ---- rendered depth maps of analytic surfaces (float64), for the integration tests ----------------------------------------------------

def rig(n_views, h, w, target, distance):
    """Cameras with skew, fx != fy and off-centre principal points looking at ``target`` from ``distance``: (K [n,3,3], E [n,4,4])."""
    Ks, Es = [], []
    for v in range(n_views):
        f = 0.9 * w * (1.0 + 0.03 * v)
        K = np.array([[f, 0.4 + 0.1 * v, w / 2.0 + 1.7 * v - 3.0], [0, f * 1.04, h / 2.0 - 1.3 * v + 2.0], [0, 0, 1]])
        a, b = 0.12 * (v - (n_views - 1) / 2.0), 0.07 * ((v % 3) - 1)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        R = Rx @ Ry
        C = np.asarray(target, float) - R.T @ np.array([0, 0, distance * (1.0 + 0.02 * v)])
        E = np.eye(4)
        E[:3, :3] = R
        E[:3, 3] = -R @ C
        Ks.append(K)
        Es.append(E)
    return np.stack(Ks).astype(np.float32), np.stack(Es).astype(np.float32)


def cam21(K, E):
    return np.concatenate((np.asarray(K, np.float32).reshape(9), np.asarray(E, np.float32)[:3, :4].reshape(12)))


def _rays(K, E, h, w):
    K, E = K.astype(np.float64), E.astype(np.float64)
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dc = np.einsum("ij,jhw->ihw", np.linalg.inv(K), np.stack((u, v, np.ones_like(u))))  # camera-frame ray, z = 1
    R, t = E[:3, :3], E[:3, 3]
    return -(R.T @ t), np.einsum("ij,jhw->ihw", R.T, dc)


def render_plane(K, E, h, w, normal, offset):
    """Depth (camera z) of the plane normal . X = offset; 0 where the ray misses."""
    C, d = _rays(K, E, h, w)
    n = np.asarray(normal, float)
    with np.errstate(all="ignore"):
        s = (offset - n @ C) / np.einsum("i,ihw->hw", n, d)
    return np.where(np.isfinite(s) & (s > 0), s, 0).astype(np.float32)


def render_sphere(K, E, h, w, centre, radius):
    C, d = _rays(K, E, h, w)
    oc = C - np.asarray(centre, float)
    a = (d * d).sum(0)
    b = 2 * np.einsum("i,ihw->hw", oc, d)
    c = oc @ oc - radius * radius
    disc = b * b - 4 * a * c
    with np.errstate(all="ignore"):
        s = (-b - np.sqrt(disc)) / (2 * a)
    return np.where((disc > 0) & (s > 0), s, 0).astype(np.float32)
