"""Numpy restatement of csrc/meshops.hip and patchmatchnet_amd/meshops.py: the yardstick of
tests/test_meshops_io.py and tests/test_meshops_gpu.py.  Test infrastructure, like tsdf_ref.py: nothing in the product imports it.

``components_ref`` is a plain sequential union-find; ``sample_ref`` evaluates the hash on uint64 and the float32 / float64 arithmetic in
the order the kernel's header comment states (numpy never contracts a multiply-add and its sqrt is IEEE), so its bits are expected to be
the kernel's."""
from __future__ import annotations

import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


# ---- components ------------------------------------------------------------------------------------------------------------------

def components_ref(faces, n_vertices):
    """label [Nv] int32: the smallest vertex index of every vertex's component."""
    parent = list(range(n_vertices))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        for p, q in ((a, b), (b, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    return np.array([find(v) for v in range(n_vertices)], np.int32)


def component_sizes_ref(faces, n_vertices):
    """(label, roots ascending int32, face_count int64): every component, those without a face included."""
    label = components_ref(faces, n_vertices)
    roots = np.nonzero(label == np.arange(n_vertices))[0].astype(np.int32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    count = np.bincount(label[faces[:, 0]], minlength=n_vertices)[roots].astype(np.int64)
    return label, roots, count


def remove_components_ref(vertices, faces, colors=None, normals=None, min_faces=0, keep_largest=0):
    """(vertices, faces, colors, normals, components found, components kept) by plain loops over the components."""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nv = len(vertices)
    label, roots, count = component_sizes_ref(faces, nv)
    ranked = sorted(range(len(roots)), key=lambda i: (-int(count[i]), int(roots[i])))
    top = set(ranked[:keep_largest]) if keep_largest > 0 else set(range(len(roots)))
    kept_roots = {int(roots[i]) for i in range(len(roots)) if count[i] >= min_faces and i in top}
    fkeep = np.array([int(label[f[0]]) in kept_roots for f in faces], bool).reshape(-1)
    used = np.zeros(nv, bool)
    used[faces[fkeep].reshape(-1)] = True
    remap = np.full(nv, -1, np.int64)
    remap[used] = np.arange(int(used.sum()))
    pick = lambda a: None if a is None else np.asarray(a)[used]
    return (np.asarray(vertices)[used], remap[faces[fkeep]].astype(np.int32).reshape(-1, 3), pick(colors), pick(normals), len(roots),
            len(kept_roots))


# ---- sampling --------------------------------------------------------------------------------------------------------------------

def mix64(z):
    """The splitmix64 finaliser on uint64 arrays (wrapping arithmetic)."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniforms(seed, face, k):
    """(r1, r2) float32 for arrays of face indices and ranks."""
    key = mix64(np.uint64((int(seed) + GOLDEN) & MASK64))
    with np.errstate(over="ignore"):
        c = ((np.asarray(face, np.uint64) << np.uint64(32)) | np.asarray(k, np.uint64)) + np.uint64(1)
        h = mix64(key + c * np.uint64(GOLDEN))
    r1 = (h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    r2 = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)
    return r1, r2


def face_areas_f32(vertices, faces):
    v = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        return np.sqrt((cx * cx + cy * cy) + cz * cz) * np.float32(0.5)


def face_counts_ref(vertices, faces, density, seed):
    area = face_areas_f32(vertices, faces)
    assert area.dtype == np.float32
    u, _ = uniforms(seed, np.arange(len(area)), np.full(len(area), 0xFFFFFFFF, np.uint64))
    ok = (area > 0) & (area < np.inf)
    with np.errstate(all="ignore"):
        x = np.floor(np.where(ok, area, 0).astype(np.float64) * np.float64(density) + u.astype(np.float64))
    return np.where(ok, np.minimum(x, 2.0 ** 31 - 1), 0).astype(np.int64)


def sample_ref(vertices, faces, density, seed=0, colors=None, return_bary=False):
    """(points [N,3] float32, face [N] int32, colors [N,3] uint8 | None[, barycentrics [N,3] float32])."""
    v = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    counts = face_counts_ref(v, f, density, seed)
    face = np.repeat(np.arange(len(f)), counts)
    start = np.cumsum(counts) - counts
    k = np.arange(len(face)) - start[face]
    r1, r2 = uniforms(seed, face, k)
    s = np.sqrt(r1)
    b0, b1, b2 = np.float32(1) - s, s * (np.float32(1) - r2), s * r2
    A, B, C = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    with np.errstate(all="ignore"):
        pts = (b0[:, None] * A + b1[:, None] * B) + b2[:, None] * C
    assert pts.dtype == np.float32
    col = None
    if colors is not None:
        c = np.asarray(colors, np.uint8).astype(np.float32)
        cv = (b0[:, None] * c[f[face, 0]] + b1[:, None] * c[f[face, 1]]) + b2[:, None] * c[f[face, 2]]
        col = np.clip(np.floor(cv + np.float32(0.5)), 0, 255).astype(np.uint8)
    out = (pts.reshape(-1, 3), face.astype(np.int32), col)
    return out + (np.stack((b0, b1, b2), 1),) if return_bary else out


# ---- meshes ----------------------------------------------------------------------------------------------------------------------

def strip(T):
    """T triangles over T + 2 vertices in a zig-zag band: face i = (i, i + 1, i + 2)."""
    i = np.arange(T + 2)
    v = np.stack((0.5 * i, (i % 2).astype(np.float64), 0.01 * i), 1).astype(np.float32)
    f = np.stack((np.arange(T), np.arange(T) + 1, np.arange(T) + 2), 1).astype(np.int32)
    return v, f


def tetrahedra(M, spacing=3.0):
    """M disjoint tetrahedra (4 vertices, 4 faces each) on a line."""
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    tf = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    v = np.concatenate([base + np.float32([spacing * m, 0, 0]) for m in range(M)]) if M else np.zeros((0, 3), np.float32)
    f = np.concatenate([tf + 4 * m for m in range(M)]) if M else np.zeros((0, 3), np.int32)
    return v.astype(np.float32), f.astype(np.int32)


def icosphere(subdivisions, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """20 * 4^subdivisions faces on a sphere, outward winding, closed (V - E + F = 2)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius + np.asarray(centre, np.float64)).astype(np.float32), np.asarray(f, np.int32)


def join(*meshes):
    """Disjoint union of (vertices, faces) meshes."""
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def permute_faces(faces, seed):
    return np.ascontiguousarray(faces[np.random.default_rng(seed).permutation(len(faces))])


def relabel_vertices(vertices, faces, seed):
    """(vertices', faces', new_of_old): vertex v becomes new_of_old[v]."""
    new_of_old = np.random.default_rng(seed).permutation(len(vertices))
    v2 = np.empty_like(vertices)
    v2[new_of_old] = vertices
    return v2, new_of_old[faces].astype(np.int32), new_of_old
