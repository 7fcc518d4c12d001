"""CPU checks of tests/dbscan_ref.py, the numpy statement of the order-free DBSCAN: against a pure-Python double
loop, against scipy's connected components where scipy imports, and the properties the inputs of tests/test_dbscan_gpu.py must have so
that no GPU test passes vacuously."""
import math

import numpy as np
import pytest

import dbscan_ref as D
import knn_ref as K


def _loop_dbscan(pts, eps, min_points):
    """The definition once more, with nothing but Python floats, lists and loops."""
    p = [[float(v) for v in row] for row in np.asarray(pts, np.float32)]
    n = len(p)

    def d2(i, j):
        dx, dy, dz = p[i][0] - p[j][0], p[i][1] - p[j][1], p[i][2] - p[j][2]
        return dx * dx + dy * dy + dz * dz

    near = [[j for j in range(n) if math.sqrt(d2(i, j)) <= eps] for i in range(n)]
    core = [len(near[i]) >= min_points for i in range(n)]
    comp = [None] * n
    for s in range(n):  # the lowest index of a component names it
        if core[s] and comp[s] is None:
            comp[s], stack = s, [s]
            while stack:
                i = stack.pop()
                for j in near[i]:
                    if core[j] and comp[j] is None:
                        comp[j] = s
                        stack.append(j)
    for i in range(n):
        if not core[i]:
            cand = sorted((d2(i, j), j) for j in near[i] if core[j])
            if cand:
                comp[i] = comp[cand[0][1]]
    names = sorted({c for c in comp if c is not None}, key=lambda c: (-comp.count(c), min(i for i in range(n) if comp[i] == c)))
    labels = [-1 if c is None else names.index(c) for c in comp]
    return labels, core, [comp.count(c) for c in names]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_against_a_pure_python_loop(seed):
    rng = np.random.default_rng(seed)
    pts = (rng.integers(-3, 4, (60, 3)) * 0.5).astype(np.float32)  # a coarse lattice: duplicates, and ties at every distance
    pts[7] = pts[3]
    seen = set()
    for eps, mp in ((0.5, 3), (0.75, 4), (0.0, 2), (1.0, 6), (0.5, 61)):
        labels, core, sizes = D.dbscan(pts, eps, mp, chunk=17)
        want = _loop_dbscan(pts, eps, mp)
        assert labels.tolist() == want[0] and core.tolist() == want[1] and sizes.tolist() == want[2]
        assert labels.dtype == np.int64 and core.dtype == bool and sizes.dtype == np.int64
        seen |= {"border"} if ((labels >= 0) & ~core).any() else set()
        seen |= {"noise"} if (labels < 0).any() else set()
        seen |= {"many"} if len(sizes) > 1 else set()
        seen |= {"tied sizes"} if len(set(sizes.tolist())) < len(sizes) else set()
    assert seen == {"border", "noise", "many", "tied sizes"}
    for a in ((0, 2), (1, 0), (0, 1), (3, 2)):  # select_clusters, stated once more
        keep = D.select_clusters(labels, sizes, *a)
        want = [lab >= 0 and sizes[lab] >= a[0] and (a[1] == 0 or lab < a[1]) for lab in labels.tolist()]
        assert keep.tolist() == want


def test_core_components_against_scipy():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    for name in ("floater", "duplicates_eps_above", "clump_129", "two_chains", "lattice"):
        pts, eps, mp, _ = D.cases()[name]
        labels, core, _ = D.expected(name)
        within = np.sqrt(K.pair_d2(pts, pts)) <= eps
        idx = np.flatnonzero(core)
        ncomp, comp = connected_components(sp.csr_matrix(within[np.ix_(idx, idx)]), directed=False)
        assert ncomp == len(np.unique(labels[core])) and D.same_partition(labels[core], comp)
        assert core.tolist() == (K.radius_count(None, pts, eps, same_cloud=True) + 1 >= mp).tolist()


def test_the_gpu_cases_contain_what_they_are_for():
    for name, (pts, eps, mp, expect) in D.cases().items():
        labels, core, sizes = D.expected(name)
        n = len(pts)
        assert pts.dtype == np.float32 and pts.flags.c_contiguous and n <= 4100 and n % 64 != 0, name
        border, noise = int(((labels >= 0) & ~core).sum()), int((labels < 0).sum())
        assert int(sizes.sum()) == n - noise and (np.diff(sizes) <= 0).all(), name
        have = {"noise": noise > 0, "border": border > 0, "clusters2": len(sizes) >= 2, "one": len(sizes) == 1,
                "all_core": bool(core.all()), "all_noise": noise == n}
        assert expect and all(have[e] for e in expect), (name, have)
    # the lattice: interior points are core, face points border, edge and corner points noise
    pts = K.lattice_cloud().astype(np.float64)
    labels, core, _ = D.expected("lattice")
    on_faces = ((pts == 0) | (pts == np.array([6.0, 5.0, 4.0]))).sum(1)
    assert np.array_equal(core, on_faces == 0) and np.array_equal(labels < 0, on_faces >= 2)


def test_the_tie_cases_really_tie():
    for low, winner in (("a", -1.0), ("b", 1.0)):
        pts = D.tie_cloud(low)
        labels, core, sizes = D.expected(f"tie_{low}")
        mid = int(np.flatnonzero((pts == 0).all(1))[0])
        ends = [int(np.flatnonzero(pts[:, 0] == x)[0]) for x in (-1.0, 1.0)]
        d2 = K.pair_d2(pts[mid:mid + 1], pts)[0]
        assert d2[ends[0]] == d2[ends[1]] == 1.0 and math.sqrt(d2[ends[0]]) <= 1.0  # bit-equal, and on the threshold
        assert not core[mid] and core[ends[0]] and core[ends[1]] and labels[ends[0]] != labels[ends[1]]
        assert sorted(np.flatnonzero(core & (np.sqrt(d2) <= 1.0)).tolist()) == sorted(ends)  # no third candidate
        low_end = ends[0] if winner < 0 else ends[1]
        assert low_end == min(ends) and labels[mid] == labels[low_end]
    # the same points: the two orders differ only in who comes first, and the origin changes sides with it
    assert sorted(map(tuple, D.tie_cloud("a").tolist())) == sorted(map(tuple, D.tie_cloud("b").tolist()))
    # two chains: the nearest pair across is 1 + 2^-20 away, one float32 step of the coordinate above eps
    pts = D.two_chains()
    across = np.sqrt(K.pair_d2(pts[:33], pts[33:]))
    assert across.min() == 1.0 + 2.0 ** -20 and float(np.float32(across.min())) == across.min()
    # duplicates: at eps = 0 exactly the copies find each other
    labels, core, sizes = D.expected("duplicates_eps0")
    dup = K.duplicate_cloud()
    copies = (K.pair_d2(dup, dup) == 0).sum(1)
    assert np.array_equal(core, copies >= 2) and sizes.min() >= 2 and not ((labels >= 0) & ~core).any()


def test_shuffling_the_surface_keeps_the_partition():
    """tests/test_dbscan_gpu.py asks this of the product; it is fair only where the reference itself shows it (a border point with two
    bit-equal nearest cores in different clusters would follow the indices)."""
    pts = D.surface()[0]
    shuf, perm = D.shuffled(pts)
    assert np.array_equal(D.cases()["surface_shuffled"][0], shuf) and not np.array_equal(perm, np.arange(len(pts)))
    a, b = D.expected("surface_2s_mp4"), D.expected("surface_shuffled")
    assert np.array_equal(a[1][perm], b[1]) and D.same_partition(a[0][perm], b[0]) and np.array_equal(a[2], b[2])
    for name in ("chain_reversed", "chain_shuffled"):
        assert np.array_equal(D.expected(name)[0], D.expected("chain")[0])
