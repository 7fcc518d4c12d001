"""Brute-force numpy float64 statement of the signed distance from an oriented cloud (pmn_cloud_sdf_blocks, pointcloud.cloud_sdf /
mesh_from_cloud, mesh_cloud.py; include/pmn_hip.h states the definition).  Neighbours come from the full matrix
of squared distances (knn_ref.pair_d2), cut at radius^2 and put in (d2, tie rank) order by a stable sort, as cloud_normals_ref.py
does; the sums, the boundary rule, the clamp and the colour follow in the kernel's order, operation for operation, so the kernel's
planes must equal these bit for bit.  Nothing is shared with the product.  `planes` gives dense [nz,ny,nx] planes that
tsdf_ref.extract meshes; `mark_points` restates SparseTsdfVolume.allocate_points.  The test clouds live here so that the CPU suite
can check them."""
import functools

import numpy as np

import knn_ref as K
import tsdf_ref as T
import tsdf_sparse_ref as S

BLOCK = 8


def positions(origin, voxel, dims):
    """float64 [nz,ny,nx,3]: origin_c + (float)index_c * voxel formed in float32, then widened."""
    o, v = np.asarray(origin, np.float32), np.float32(voxel)
    ax = [(o[c] + np.arange(dims[c], dtype=np.float32) * v).astype(np.float32).astype(np.float64) for c in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], -1)


def neighbours(query, points, k, radius, rank=None, chunk=2048):
    """(idx int64 [n,k], d2 float64 [n,k]): the k nearest points of every query with d2 < radius * radius strictly, ascending
    (d2, rank); -1 / 0 in an empty slot.  ``rank`` [len(points)] breaks ties among equal squares (the product's is the grid's sorted
    position); default: the index itself."""
    q = np.asarray(query, np.float64)
    p = np.asarray(points, np.float32)
    rank = np.arange(len(p)) if rank is None else np.asarray(rank)
    R2 = float(radius) * float(radius)
    idx = np.full((len(q), k), -1, np.int64)
    val = np.zeros((len(q), k), np.float64)
    # a query further than radius from the points' box on some axis has no neighbour: skip it (1.001: far above any rounding)
    lo, hi = p.astype(np.float64).min(0) - 1.001 * float(radius), p.astype(np.float64).max(0) + 1.001 * float(radius)
    near = np.nonzero(((q >= lo) & (q <= hi)).all(1))[0]
    for a in range(0, len(near), chunk):
        rows_q = near[a:a + chunk]
        # pair_d2 takes float32 inputs: the queries are float32 values widened, so the round trip is exact
        d2 = K.pair_d2(q[rows_q].astype(np.float32), p)
        assert np.array_equal(q[rows_q].astype(np.float32).astype(np.float64), q[rows_q])
        r, c = np.nonzero(d2 < R2)
        v = d2[r, c]
        order = np.lexsort((rank[c], v, r))  # stable: row, then d2, then tie rank
        r, c, v = r[order], c[order], v[order]
        start = np.searchsorted(r, np.arange(len(rows_q)))
        slot = np.arange(len(r)) - start[r]
        keep = slot < k
        idx[rows_q[r[keep]], slot[keep]] = c[keep]
        val[rows_q[r[keep]], slot[keep]] = v[keep]
    return idx, val


def planes(points, normals, colors, origin, voxel, dims, trunc, k, radius, boundary, rank=None, lists=None):
    """dict: tsdf, weight [nz,ny,nx] float32, rgb [3,nz,ny,nx] / cweight or None, observed bool, count int, f float64 (unclamped
    distance, NaN where nothing is in range).  ``lists``: `neighbours` of the lattice's positions for this or a larger k, where a
    caller asks for several k (the lists are nested)."""
    nx, ny, nz = dims
    x = positions(origin, voxel, dims).reshape(-1, 3)
    p = np.asarray(points, np.float32).astype(np.float64)
    m = np.asarray(normals, np.float32).astype(np.float64)
    idx, d2 = neighbours(x, points, k, radius, rank) if lists is None else (lists[0][:, :k], lists[1][:, :k])
    R2 = float(radius) * float(radius)
    n = len(x)
    sw, sws, count = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    sc = np.zeros((n, 3))
    col = None if colors is None else np.asarray(colors, np.uint8).astype(np.float64)
    s0 = np.zeros(n)
    for j in range(k):  # rank order
        live = idx[:, j] >= 0
        i = np.maximum(idx[:, j], 0)
        u = 1.0 - d2[:, j] / R2
        u2 = u * u
        w = np.where(live, u2 * u2, 0.0)
        sj = (m[i, 0] * (x[:, 0] - p[i, 0]) + m[i, 1] * (x[:, 1] - p[i, 1])) + m[i, 2] * (x[:, 2] - p[i, 2])
        sj = np.where(live, sj, 0.0)
        if j == 0:
            s0 = sj
        sw = sw + w
        sws = sws + w * sj
        if col is not None:
            sc = sc + w[:, None] * col[i]
        count += live
    t2 = d2[:, 0] - s0 * s0
    observed = (count > 0) & (sw > 0.0) & ~(t2 > float(boundary) * float(boundary))
    with np.errstate(all="ignore"):
        f = sws / sw
        tsdf = np.where(observed, np.fmin(1.0, np.fmax(-1.0, f / float(np.float32(trunc)))).astype(np.float32), np.float32(1))
        weight = np.where(observed, count.astype(np.float32), np.float32(0))
        out = {"tsdf": tsdf.reshape(nz, ny, nx), "weight": weight.reshape(nz, ny, nx), "rgb": None, "cweight": None,
               "observed": observed.reshape(nz, ny, nx), "count": count.reshape(nz, ny, nx), "f": f.reshape(nz, ny, nx)}
        if col is not None:
            rgb = np.where(observed[:, None], (sc / sw[:, None]).astype(np.float32), np.float32(0))
            out["rgb"] = np.ascontiguousarray(rgb.T).reshape(3, nz, ny, nx)
            out["cweight"] = out["weight"].copy()
    return out


def mesh(pl, origin, voxel, min_weight):
    """(vertices, faces, colors | None, normals) of tsdf_ref.extract on the planes."""
    e = T.extract(pl["tsdf"], pl["weight"], origin, voxel, min_weight, pl["rgb"], pl["cweight"], True)
    return e["vertices"], e["faces"], e["colors"], e["normals"]


def mark_points(points, origin, voxel, dims, reach):
    """[nbz,nby,nbx] bool: SparseTsdfVolume.allocate_points' marking BEFORE the dilation: the blocks of the eight corners of the box
    p +- reach grown by one voxel, clipped to the lattice; a box that misses the lattice marks nothing."""
    nbx, nby, nbz = S.n_blocks(dims)
    top = np.asarray(dims, np.float64) - 1.0
    v = float(np.float32(voxel))
    rel = np.asarray(points, np.float32).astype(np.float64) - np.asarray(origin, np.float32).astype(np.float64)
    lo = np.ceil((rel - float(reach)) / v) - 1.0
    hi = np.floor((rel + float(reach)) / v) + 1.0
    inside = ((hi >= 0) & (lo <= top)).all(1)
    ends = (np.maximum(lo[inside], 0.0).astype(np.int64) // BLOCK, np.minimum(hi[inside], top).astype(np.int64) // BLOCK)
    flags = np.zeros((nbz, nby, nbx), bool)
    for corner in range(8):
        bx, by, bz = (ends[(corner >> c) & 1][:, c] for c in range(3))
        flags[bz, by, bx] = True
    return flags


def allocated(points, origin, voxel, dims, reach):
    """The blocks allocate_points builds: the marking dilated by one block."""
    return S.dilate(mark_points(points, origin, voxel, dims, reach))


# ---- the clouds of the tests (each built once: treat as read-only) ------------------------------------------------------------------

SPHERE_RADIUS = 13.4
SPHERE_CENTRE = np.array([19.3, 20.1, 19.7])  # off the lattice of voxel 1 at the origin
FAR = np.array([300.0, -200.0, 650.0])        # the shifted lattice's origin


def _colors(points, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (len(points), 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def sphere(n=3000, shift=(0.0, 0.0, 0.0)):
    """(points float32, normals float32: exact radial directions of the float64 points, colours, centre float64)."""
    rng = np.random.default_rng(21)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = SPHERE_CENTRE + np.asarray(shift, np.float64)
    out = ((c + SPHERE_RADIUS * d).astype(np.float32), d.astype(np.float32), _colors(d, 22), c)
    for a in out:
        a.setflags(write=False)
    return out


PATCH_LO, PATCH_HI = 9.0, 27.0
PATCH_POINT = np.array([18.0, 18.0, 11.3719])                      # the plane passes through it ...
PATCH_NORMAL = np.array([-0.0613579, 0.0237113, 1.0]) / np.linalg.norm([-0.0613579, 0.0237113, 1.0])  # ... slightly tilted, so that no lattice holds it


def patch_distance(v):
    """Signed distance of positions to the patch's plane, positive on the normal's side."""
    return (np.asarray(v, np.float64) - PATCH_POINT) @ PATCH_NORMAL


@functools.lru_cache(maxsize=None)
def patch(n=1200):
    """A planar square over [9, 27]^2 in x, y on the tilted plane above (jittered grid, so that no hole is wider than a voxel), its
    normal at every point, colours."""
    rng = np.random.default_rng(23)
    side = int(np.ceil(np.sqrt(n)))
    g = (np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) + rng.uniform(0.1, 0.9, (side * side, 2)))
    xy = PATCH_LO + g / side * (PATCH_HI - PATCH_LO)
    z = PATCH_POINT[2] - ((xy - PATCH_POINT[:2]) @ PATCH_NORMAL[:2]) / PATCH_NORMAL[2]
    pts = np.concatenate([xy, z[:, None]], 1).astype(np.float32)
    nrm = np.tile(PATCH_NORMAL.astype(np.float32)[None], (len(pts), 1))
    out = (pts, nrm, _colors(pts, 24))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sheet(n=2000, planted=40):
    """tests/knn_ref.py's wavy sheet z = 4 sin(x / 9) cos(y / 7) with ``planted`` outliers; normals = the analytic normals of the
    noise-free sheet at (x, y), upwards (the outliers carry them too)."""
    pts = K.surface_cloud(n, planted / n, 0)[0]
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    gx = 4.0 / 9.0 * np.cos(x / 9.0) * np.cos(y / 7.0)
    gy = -4.0 / 7.0 * np.sin(x / 9.0) * np.sin(y / 7.0)
    nrm = np.stack([-gx, -gy, np.ones_like(gx)], 1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    out = (pts, nrm.astype(np.float32), _colors(pts, 25))
    for a in out:
        a.setflags(write=False)
    return out


def with_normals(points, seed):
    """Random unit normals and colours for a cloud that has none."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(len(points), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.asarray(points, np.float32), d.astype(np.float32), _colors(points, seed + 1)
