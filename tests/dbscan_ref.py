"""Brute-force numpy float64 statement of the order-free DBSCAN of DESIGN.md section 33 (pmn_cloud_core, pmn_cloud_dbscan,
pointcloud.cluster_dbscan / select_clusters, cluster_cloud.py).  No spatial index, no union-find, nothing shared with the product: the
matrix of squared distances (knn_ref.pair_d2, in row chunks), a breadth-first search for the components.  The clouds and cases of
tests/test_dbscan_gpu.py live here too so that the CPU suite can check what they contain (tests/test_dbscan_ref.py)."""
import functools
from collections import deque

import numpy as np

import knn_ref as K


def dbscan(points, eps, min_points, chunk=512):
    """(labels int64 [n], core bool [n], sizes int64 [C]) of the definition:
    within eps: sqrt(d2) <= eps; core: at least min_points points within eps, the point itself included; cluster: a connected component
    of the core points under "within eps"; border: not core, joins the cluster of the core point within eps least in (d2, index); noise
    -1; clusters numbered by descending size (core and border members), equal sizes by the lowest index of any member."""
    pts = np.asarray(points, np.float32)
    n, eps = len(pts), float(eps)
    within, d2_rows = [], []
    for a in range(0, n, chunk):
        d2 = K.pair_d2(pts[a:a + chunk], pts)
        within.append(np.sqrt(d2) <= eps)
        d2_rows.append(d2)
    within = np.concatenate(within)
    core = within.sum(1) >= int(min_points)
    comp = np.full(n, -1, np.int64)  # component number in order of discovery
    ncomp = 0
    for s in np.flatnonzero(core):
        if comp[s] >= 0:
            continue
        comp[s] = ncomp
        todo = deque([s])
        while todo:
            i = todo.popleft()
            for j in np.flatnonzero(within[i] & core & (comp < 0)):
                comp[j] = ncomp
                todo.append(j)
        ncomp += 1
    d2 = np.concatenate(d2_rows)
    for i in np.flatnonzero(~core):
        cand = within[i] & core
        if cand.any():
            comp[i] = comp[np.argmin(np.where(cand, d2[i], np.inf))]  # argmin: the first, that is the lowest index, among equals
    sizes = np.bincount(comp[comp >= 0], minlength=ncomp)
    first = np.array([np.flatnonzero(comp == c)[0] for c in range(ncomp)], np.int64)
    order = sorted(range(ncomp), key=lambda c: (-sizes[c], first[c]))
    rank = np.empty(ncomp, np.int64)
    rank[order] = np.arange(ncomp)
    labels = np.full(n, -1, np.int64)
    labels[comp >= 0] = rank[comp[comp >= 0]]
    return labels, core, sizes[order].astype(np.int64)


def select_clusters(labels, sizes, min_cluster_points=0, keep_largest=0):
    """bool [n]: members of the clusters with at least min_cluster_points points that are, with keep_largest > 0, among the keep_largest
    largest (= first); noise never."""
    keep = np.zeros(len(labels), bool)
    for c, s in enumerate(sizes):
        if s >= min_cluster_points and (keep_largest <= 0 or c < keep_largest):
            keep |= labels == c
    return keep


def spacing(points, k=8):
    """The median over the cloud of the mean distance to the k nearest other points: the unit of the surface cloud's eps."""
    return float(np.median(K.knn_mean(K.knn_d2(None, points, k, 1e30, same_cloud=True), 1e30)))


def same_partition(a, b):
    """True when two label vectors describe the same partition with the same noise set, whatever the names of the clusters."""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = {(x, y) for x, y in zip(a[a >= 0].tolist(), b[b >= 0].tolist())}
    return len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs})


# ---- the clouds of the tests ---------------------------------------------------------------------------------------------------

def tie_cloud(low="a"):
    """Two clumps on the x axis, half a unit between their points, their nearest ends at x = -1 and x = +1, and ONE point at the origin:
    with eps = 1 and min_points = 4 the origin is a border point exactly 1 (d2 = 1, bit-equal) from the cores at -1 and +1, which are
    2 apart, so the clumps are two clusters and only the tie-break says which gets it.  ``low``: the clump whose end has the lower
    index ("a": x < 0, "b": x > 0).  A grid sorts x = -1 before x = +1 whatever the indices."""
    xa = [-1.0, -1.5, -2.0, -2.5, -3.0]
    xb = [1.0, 1.5, 2.0, 2.5]
    first, second = (xa, xb) if low == "a" else (xb, xa)
    x = [first[0], second[0], 0.0] + first[1:] + second[1:]
    pts = np.zeros((len(x), 3), np.float32)
    pts[:, 0] = x
    return pts


def chain_cloud(n=4097, step=0.9):
    """n points ``step`` apart along a skew line: with eps = 1 and min_points = 2 every point is core and links only to the next."""
    u = np.array([2.0, 3.0, 6.0]) / 7.0
    return (np.arange(n, dtype=np.float64)[:, None] * step * u[None, :]).astype(np.float32)


def two_chains(n=33):
    """Two parallel chains, half a unit between a chain's points, the chains 1 + 2^-20 apart (exact in float32): with eps = 1 the
    nearest pair across is a last bit too far."""
    x = np.arange(n, dtype=np.float64) * 0.5
    a = np.stack([x, np.zeros(n), np.zeros(n)], 1)
    b = np.stack([x, np.full(n, 1.0 + 2.0 ** -20), np.zeros(n)], 1)
    return np.concatenate([a, b]).astype(np.float32)


def clump(n, seed=9):
    """n random points in a unit box: one cell at cell = 2."""
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def surface():
    pts = K.surface_cloud()[0]
    return pts, spacing(pts)


@functools.lru_cache(maxsize=None)
def floater():
    """(the surface cloud with a dense clump of 41 wrong points 15 units above the sheet -- what consistent mismatches leave behind and
    neither cleaning filter removes --, bool [n]: the clump's points)."""
    pts = surface()[0]
    blob = np.random.default_rng(13).normal(0.0, 0.6, (41, 3)) + np.array([30.0, 30.0, 15.0])
    return np.concatenate([pts, blob.astype(np.float32)]), np.arange(len(pts) + 41) >= len(pts)


def shuffled(pts, seed=21):
    """(the cloud in another order, the permutation: shuffled[k] = pts[perm[k]])."""
    perm = np.random.default_rng(seed).permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), perm


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (points, eps, min_points, expect): the cases of tests/test_dbscan_gpu.py.  expect names what the case must contain
    (checked by tests/test_dbscan_ref.py on the reference alone): "noise", "border", "clusters2" (at least two clusters), "all_core",
    "all_noise", "one" (exactly one cluster)."""
    pts, s = surface()
    n = len(pts)
    out = {}
    for mult in (2.0, 3.0):
        out[f"surface_{mult:g}s_mp1"] = (pts, mult * s, 1, ("all_core", "clusters2"))
        rich = ("noise", "border") if mult == 2.0 else ("noise", "one")  # at 3 spacings every point of the sheet is core
        out[f"surface_{mult:g}s_mp4"] = (pts, mult * s, 4, rich)
        out[f"surface_{mult:g}s_mp10"] = (pts, mult * s, 10, rich)
        out[f"surface_{mult:g}s_mp_n1"] = (pts, mult * s, n + 1, ("all_noise",))
    out["floater"] = (floater()[0], 2.0 * s, 4, ("noise", "border", "clusters2"))
    out["lattice"] = (K.lattice_cloud(), 1.0, 7, ("noise", "border", "one"))
    out["tie_a"] = (tie_cloud("a"), 1.0, 4, ("border", "clusters2"))
    out["tie_b"] = (tie_cloud("b"), 1.0, 4, ("border", "clusters2"))
    chain = chain_cloud()
    out["chain"] = (chain, 1.0, 2, ("all_core", "one"))
    out["chain_reversed"] = (np.ascontiguousarray(chain[::-1]), 1.0, 2, ("all_core", "one"))
    out["chain_shuffled"] = (shuffled(chain)[0], 1.0, 2, ("all_core", "one"))
    out["two_chains"] = (two_chains(), 1.0, 2, ("all_core", "clusters2"))
    dup = K.duplicate_cloud()
    out["duplicates_eps0"] = (dup, 0.0, 2, ("noise", "clusters2"))
    out["duplicates_eps_above"] = (dup, 0.75, 4, ("noise", "border", "clusters2"))
    out["surface_shuffled"] = (shuffled(pts)[0], 2.0 * s, 4, ("noise", "border"))
    out["one_point"] = (np.array([[0.25, -1.5, 3.0]], np.float32), 0.5, 1, ("all_core", "one"))
    out["one_point_noise"] = (np.array([[0.25, -1.5, 3.0]], np.float32), 0.5, 2, ("all_noise",))
    for m in (63, 65, 129):
        out[f"clump_{m}"] = (clump(m), 0.2, 4, ("noise", "border"))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """The reference's (labels, core, sizes) of a case, computed once per process; callers must not write into it."""
    pts, eps, mp, _ = cases()[name]
    out = dbscan(pts, eps, mp)
    for a in out:
        a.setflags(write=False)
    return out
