"""Numpy side of the block-sparse volume: the yardsticks of tests/test_tsdf_sparse_io.py and
tests/test_tsdf_sparse_gpu.py.  Test infrastructure, like tsdf_ref.py (which it builds on): nothing in the product imports it.

* ``soup`` / ``assert_same_mesh``: two indexed meshes compared as sets of triangles, free of the order of vertices and faces.
* ``mark_blocks``: the marking rule of pmn_tsdf_mark_blocks restated per view; ``needed_blocks``: the exact set it has to cover,
  from tsdf_ref's own projection; ``dilate``: one block in all 26 directions.
* the scenes the tests share, each built once.
"""
from __future__ import annotations

import functools

import numpy as np

import tsdf_ref as R

BLOCK = 8
MARK_SPAN = 8


# ---- order-free mesh comparison -------------------------------------------------------------------------------------------------------

def _records(vertices, colors, normals):
    """One row of uint32 words per vertex: position bits, normal bits, colour bytes."""
    v = np.ascontiguousarray(vertices, np.float32)
    cols = [v.view(np.uint32).reshape(len(v), 3)]
    if normals is not None:
        cols.append(np.ascontiguousarray(normals, np.float32).view(np.uint32).reshape(len(v), 3))
    if colors is not None:
        cols.append(np.asarray(colors, np.uint32).reshape(len(v), 3))
    return np.concatenate(cols, 1)


def _sorted_rows(a):
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def soup(vertices, faces, colors=None, normals=None):
    """(triangles [Nt, 3 * words] sorted, vertex records [Nv, words] sorted).  Every triangle is expanded to its three per-corner
    records, rotated to start at its smallest record (which keeps the winding), and the triangles are sorted."""
    rec = _records(vertices, colors, normals)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    tri = rec[f]                                                   # [Nt, 3, words]
    if len(tri):
        first = np.zeros(len(tri), np.int64)
        for c in (1, 2):                                           # lexicographic minimum of the three corner records
            a, b = tri[np.arange(len(tri)), first], tri[:, c]
            diff = a != b
            at = diff.argmax(1)
            less = diff.any(1) & (b[np.arange(len(tri)), at] < a[np.arange(len(tri)), at])
            first = np.where(less, c, first)
        order = (first[:, None] + np.arange(3)[None]) % 3
        tri = tri[np.arange(len(tri))[:, None], order]
    return _sorted_rows(tri.reshape(len(tri), 3 * rec.shape[1])), _sorted_rows(rec)  # (not -1: a mesh may have no triangle)


def assert_same_mesh(a, b, what=""):
    """a, b = (vertices, faces, colors | None, normals | None)."""
    (ta, va), (tb, vb) = soup(*a), soup(*b)
    assert va.shape == vb.shape and ta.shape == tb.shape, (what, va.shape, vb.shape, ta.shape, tb.shape)
    assert np.array_equal(va, vb), what + ": vertex records differ"
    assert np.array_equal(ta, tb), what + ": triangles differ"


# ---- marking --------------------------------------------------------------------------------------------------------------------------

def n_blocks(dims):
    return tuple(-(-int(n) // BLOCK) for n in dims)


def block_any(samples):
    """[nz,ny,nx] bool per sample -> [nbz,nby,nbx] bool: the blocks that hold a True sample."""
    nz, ny, nx = samples.shape
    nbx, nby, nbz = n_blocks((nx, ny, nz))
    full = np.zeros((nbz * BLOCK, nby * BLOCK, nbx * BLOCK), bool)
    full[:nz, :ny, :nx] = samples
    return full.reshape(nbz, BLOCK, nby, BLOCK, nbx, BLOCK).any((1, 3, 5))


def block_samples(blocks, dims):
    """The inverse view: [nbz,nby,nbx] bool per block -> [nz,ny,nx] bool per sample."""
    nx, ny, nz = dims
    return np.repeat(np.repeat(np.repeat(blocks, BLOCK, 0), BLOCK, 1), BLOCK, 2)[:nz, :ny, :nx]


def dilate(blocks):
    out = blocks.copy()
    for axis in range(3):
        src = out.copy()
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(None, -1), slice(1, None)
        out[tuple(hi)] |= src[tuple(lo)]
        out[tuple(lo)] |= src[tuple(hi)]
    return out


def needed_blocks(dims, origin, voxel, trunc, depth, cam, mask=None):
    """The blocks that hold a sample which the integration maps to a valid pixel of this view with |sdf| <= trunc, through
    tsdf_ref.integrate itself: on a fresh volume with an image, cweight becomes 1 exactly at those samples."""
    vol = R.new_volume(dims, color=True)
    R.integrate(vol, origin, voxel, trunc, depth, cam, mask, np.zeros(depth.shape + (3,), np.uint8))
    return block_any(vol["cweight"] > 0)


def mark_blocks(dims, origin, voxel, trunc, depth, cam, mask=None):
    """The rule of pmn_tsdf_mark_blocks for one view, in float32 in the kernel's order: -> (flags [nbz,nby,nbx] bool, overflow count)."""
    T = np.float32
    nx, ny, nz = dims
    nbx, nby, nbz = n_blocks(dims)
    h, w = depth.shape
    cam = np.asarray(cam, np.float32).astype(np.float64)
    E = np.eye(4)
    E[:3] = cam[9:].reshape(3, 4)
    Ki, Ei = np.linalg.inv(cam[:9].reshape(3, 3)).astype(T), np.linalg.inv(E)[:3].astype(T)
    flags = np.zeros((nbz, nby, nbx), bool)
    with np.errstate(all="ignore"):
        d = depth.astype(T)
        ok = (d > 0) & (d < np.inf)
        if mask is not None:
            ok &= mask != 0
        v, u = np.nonzero(ok)
        d = d[v, u]
        tr, vx = T(np.float32(trunc)), T(np.float32(voxel))
        lo = np.full((len(d), 3), np.inf, T)
        hi = np.full((len(d), 3), -np.inf, T)
        finite = np.ones(len(d), bool)
        for c in range(4):
            cu = u.astype(T) + T(0.5 if c & 1 else -0.5)
            cv = v.astype(T) + T(0.5 if c & 2 else -0.5)
            ray = [(Ki[r, 0] * cu + Ki[r, 1] * cv) + Ki[r, 2] for r in range(3)]
            for z in (np.maximum(d - tr, T(0)), d + tr):
                s = z / ray[2]
                cx, cy = ray[0] * s, ray[1] * s
                for r in range(3):
                    wc = ((Ei[r, 0] * cx + Ei[r, 1] * cy) + Ei[r, 2] * z) + Ei[r, 3]
                    finite &= np.abs(wc) < np.inf
                    lo[:, r] = np.fmin(lo[:, r], wc)
                    hi[:, r] = np.fmax(hi[:, r], wc)
        o = np.asarray(origin, np.float32).astype(T)
        n = np.array([nx, ny, nz])
        fl = np.ceil((lo - o) / vx) - T(1)
        fh = np.floor((hi - o) / vx) + T(1)
        inside = finite & ~((fh < 0) | (fl > (n - 1).astype(T))).any(1)
        b0 = (np.maximum(fl, 0)[inside]).astype(np.int64) // BLOCK
        b1 = (np.minimum(fh, (n - 1).astype(T))[inside]).astype(np.int64) // BLOCK
    wide = ((b1 - b0) >= MARK_SPAN).any(1)
    for (x0, y0, z0), (x1, y1, z1) in zip(b0[~wide], b1[~wide]):
        flags[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = True
    return flags, int((~finite).sum() + wide.sum())


def mark_views(dims, origin, voxel, trunc, views, masks=True):
    flags, over = np.zeros(n_blocks(dims)[::-1], bool), 0
    for d, cam, mask, _ in views:
        f, o = mark_blocks(dims, origin, voxel, trunc, d, cam, mask if masks else None)
        flags |= f
        over += o
    return flags, over


def needed_views(dims, origin, voxel, trunc, views, masks=True):
    need = np.zeros(n_blocks(dims)[::-1], bool)
    for d, cam, mask, _ in views:
        need |= needed_blocks(dims, origin, voxel, trunc, d, cam, mask if masks else None)
    return need


def dense_volume(dims, origin, voxel, trunc, views, masks=True, color=True):
    vol = R.new_volume(dims, color=color)
    for d, cam, mask, image in views:
        R.integrate(vol, origin, voxel, trunc, d, cam, mask if masks else None, image if color else None)
    return vol


def restrict(vol, samples):
    """to_dense()-style planes: the volume where ``samples`` (bool [nz,ny,nx]) is set, tsdf 1 / weight 0 / colour 0 elsewhere."""
    out = {"tsdf": np.where(samples, vol["tsdf"], np.float32(1)), "weight": np.where(samples, vol["weight"], np.float32(0)),
           "rgb": None, "cweight": None}
    if vol["rgb"] is not None:
        out["rgb"] = np.where(samples[None], vol["rgb"], np.float32(0))
        out["cweight"] = np.where(samples, vol["cweight"], np.float32(0))
    return out


def pool_of(vol, keep):
    """Dense planes (tsdf_ref.new_volume's dict, any sides >= 2) as the pool of the blocks ``keep`` ([nbz,nby,nbx] bool) -> dict: blocks
    int32 [B] ascending, table int32 [nbz,nby,nbx], tsdf / weight / cweight [B,8,8,8], rgb [3,B,8,8,8].  The samples of a border block
    beyond the lattice hold what a fresh pool holds (tsdf 1, the rest 0)."""
    nz, ny, nx = vol["tsdf"].shape
    nbz, nby, nbx = keep.shape
    assert (nbx, nby, nbz) == n_blocks((nx, ny, nz))
    blocks = np.nonzero(keep.reshape(-1))[0].astype(np.int32)
    table = np.full(keep.size, -1, np.int32)
    table[blocks] = np.arange(len(blocks), dtype=np.int32)

    def blocked(plane, fill):
        full = np.full((nbz * BLOCK, nby * BLOCK, nbx * BLOCK), fill, np.float32)
        full[:nz, :ny, :nx] = plane
        p = full.reshape(nbz, BLOCK, nby, BLOCK, nbx, BLOCK).transpose(0, 2, 4, 1, 3, 5).reshape(-1, BLOCK, BLOCK, BLOCK)
        return np.ascontiguousarray(p[blocks])

    out = {"blocks": blocks, "table": table.reshape(keep.shape), "tsdf": blocked(vol["tsdf"], 1), "weight": blocked(vol["weight"], 0),
           "rgb": None, "cweight": None}
    if vol["rgb"] is not None:
        out["rgb"] = np.stack([blocked(vol["rgb"][c], 0) for c in range(3)])
        out["cweight"] = blocked(vol["cweight"], 0)
    return out


def mesh_of(vol, origin, voxel, min_weight=1.0):
    m = R.extract(vol["tsdf"], vol["weight"], origin, voxel, min_weight, vol["rgb"], vol["cweight"], True)
    return m["vertices"], m["faces"], m["colors"], m["normals"]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------

DIMS = (40, 48, 56)                                   # 5 x 6 x 7 blocks
VOXEL, TRUNC = np.float32(0.05), np.float32(0.2)
ORIGIN = np.array([-1.03, -1.21, 3.02], np.float32)
CENTRE = ORIGIN.astype(np.float64) + np.array(DIMS) * float(VOXEL) / 2 + [0.011, -0.017, 0.023]
RADIUS = 0.62                                         # 12.4 voxels around a centre 20 / 24 / 28 voxels in: block faces cut it on every axis


def _spoil(d, rng):
    """10 % invalid pixels, NaN / inf / negative depths among them."""
    bad = rng.random(d.shape)
    d = d.copy()
    d[bad < 0.07] = 0.0
    d[(bad >= 0.07) & (bad < 0.08)] = np.nan
    d[(bad >= 0.08) & (bad < 0.09)] = np.inf
    neg = (bad >= 0.09) & (bad < 0.10)
    d[neg] = -d[neg] - 1
    return d


@functools.lru_cache(maxsize=None)
def scene(kind):
    """'A': 4 views of 64 x 80 of a sphere, a fifth of 48 x 64 and a sixth behind the volume looking away; 'B': the same cameras on a
    tilted plane that leaves the lattice through two faces.  General intrinsics (tsdf_ref.rig).  -> list of (depth, cam21, mask, image);
    the lattice is DIMS / ORIGIN / VOXEL / TRUNC.  Built once: treat as read-only."""
    rng = np.random.default_rng(11 if kind == "A" else 12)
    h, w = 64, 80
    K, E = R.rig(5, h, w, CENTRE, 3.0)
    nrm = np.array((0.55, 0.1, 0.83))
    views = []
    for v in range(6):
        hv, wv, Kv, Ev = h, w, K[min(v, 4)].copy(), E[min(v, 4)].copy()
        if v == 4:
            hv, wv = 48, 64
            Kv[:2] *= 0.8
        if v == 5:
            Ev[:3, :3] = np.diag([1.0, -1.0, -1.0]) @ Ev[:3, :3]
            Ev[:3, 3] = np.diag([1.0, -1.0, -1.0]) @ Ev[:3, 3]
        if kind == "A":
            d = R.render_sphere(Kv, Ev, hv, wv, CENTRE, RADIUS)
        else:
            d = R.render_plane(Kv, Ev, hv, wv, nrm, nrm @ CENTRE + 0.013)
        if v == 5:
            d = np.full((hv, wv), 3.0, np.float32)
        d = _spoil(d, rng)
        mask = (rng.random((hv, wv)) > 0.05).astype(np.uint8) * 255
        image = rng.integers(0, 256, (hv, wv, 3), dtype=np.uint8)
        for a in (d, mask, image):
            a.setflags(write=False)
        views.append((d, R.cam21(Kv, Ev), mask, image))
    return views


def look_at(eye, target):
    """World-to-camera extrinsic [4,4] of a camera at ``eye`` looking at ``target`` (z forward)."""
    z = np.asarray(target, float) - np.asarray(eye, float)
    z /= np.linalg.norm(z)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    E = np.eye(4)
    E[:3, :3] = np.stack((x, y, z))
    E[:3, 3] = -E[:3, :3] @ np.asarray(eye, float)
    return E


CORNER_CENTRE = np.array([1.113, 1.287, 1.461])       # of the sphere of the 1024^3 case, from the lattice's origin (0, 0, 0)


@functools.lru_cache(maxsize=None)
def surround_views():
    """Fourteen clean views (six along the axes, eight along the cube diagonals) of 96 x 120 around the sphere of radius RADIUS at
    CORNER_CENTRE: every sample within a cell of the surface is observed, so the mesh is closed."""
    h, w = 96, 120
    K = R.rig(14, h, w, CORNER_CENTRE, 3.0)[0]
    dirs = [np.array(d, float) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    dirs += [np.array((a, b, c), float) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]
    views = []
    for v, dr in enumerate(dirs):
        E = look_at(CORNER_CENTRE + 3.0 * dr / np.linalg.norm(dr), CORNER_CENTRE).astype(np.float32)
        d = R.render_sphere(K[v % 5], E, h, w, CORNER_CENTRE, RADIUS)
        d.setflags(write=False)
        views.append((d, R.cam21(K[v % 5], E), None, None))
    return views
