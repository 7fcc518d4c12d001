"""CPU checks of the mesher space (tests/mesher_space.py) against the numpy oracle tests/tsdf_ref.py alone: the table covers what it
says it covers -- every corner pattern and every case of every tetrahedron, every edge class with and without a vertex under several
sets of live cells, every planted value at both ends of a crossed edge, every colour boundary, every decision of tsdf_fold_sample met
with equality -- and the oracle is sound there: closed up to the lattice's outer faces, finite, and on the ExactRows the same in float32
and float64.  A GPU failure of tests/test_mesher_space_gpu.py can then only be the kernels'."""
import numpy as np
import pytest

import mesher_space as M
import tsdf_ref as R

BY_NAME = {r.name: r for r in M.EXTRACT_ROWS}
CLASS_CELLS = {c: [m for m in range(8) if m & c == 0] for c in range(1, 8)}  # the cells (owner - m) that contain an edge of class c


def test_the_table_has_the_rows_the_kernels_need():
    names = [r.name for r in M.EXTRACT_ROWS] + [r.name for r in M.EXACT_ROWS]
    assert len(set(names)) == len(names)
    assert {r.dims for r in M.EXTRACT_ROWS if r.kind == "thin"} == set(M.THIN)
    assert {r.min_weight for r in M.EXTRACT_ROWS if r.kind == "holes"} == {1.0, 2.5, 0.0, -1.0}
    assert sum(r.pool for r in M.EXTRACT_ROWS) >= 15 and all(r.what for r in M.EXTRACT_ROWS + M.EXACT_ROWS)
    for r in M.EXTRACT_ROWS:
        x = r.inputs()
        assert x["tsdf"].dtype == np.float32 and x["tsdf"].shape == r.dims[::-1] == x["weight"].shape, r.name
        assert len(M.oracle(r)["faces"]) == 0 if r.empty else len(M.oracle(r)["faces"]) > 0, r.name


@pytest.mark.parametrize("row", [r for r in M.EXTRACT_ROWS if r.kind == "patterns"], ids=lambda r: r.id)
def test_patterns_hold_every_corner_pattern_and_every_case_of_every_tetrahedron(row):
    x = row.inputs()
    live = M.live_cells(x["weight"], row.min_weight)
    pat = M.cell_patterns(x["tsdf"])[live]
    assert live.all() and set(pat.tolist()) == set(range(256)), sorted(set(range(256)) - set(pat.tolist()))
    for t, (corners, _) in enumerate(R.TETS):
        cases = {sum(((p >> c) & 1) << n for n, c in enumerate(corners)) for p in range(256)}
        seen = {sum(((int(p) >> c) & 1) << n for n, c in enumerate(corners)) for p in set(pat.tolist())}
        assert cases == set(range(16)) and set(range(1, 15)) <= seen, (t, sorted(seen))
    mags = np.abs(x["tsdf"]).reshape(-1)
    assert len(np.unique(mags)) == mags.size  # no two corners share a magnitude: no two vertices coincide
    v = M.oracle(row)["vertices"]
    assert len(np.unique(v, axis=0)) == len(v)


@pytest.mark.parametrize("row", [r for r in M.EXTRACT_ROWS if r.kind == "holes"], ids=lambda r: r.id)
def test_holes_show_every_edge_class_with_and_without_a_vertex(row):
    """Per class: crossed edges that carry a vertex, crossed edges that carry none (no live cell contains them), and the different
    non-empty sets of live cells among the cells that contain the edge.  The body diagonal (class 7) lies in one cell only, so it has
    one such set; the others must show at least two."""
    x = row.inputs()
    t, w = x["tsdf"], x["weight"]
    nz, ny, nx = t.shape
    vmask = M.oracle(row)["vmask"]
    live = np.zeros((nz + 1, ny + 1, nx + 1), bool)  # live[k + 1, j + 1, i + 1]: padded so that owner - m never leaves it
    live[1:nz, 1:ny, 1:nx] = M.live_cells(w, row.min_weight)
    weights = set(np.unique(w[~np.isnan(w)]).tolist())
    mw = np.float32(row.min_weight)
    assert np.isnan(w).any() and {float(mw), float(mw + 1), float(np.nextafter(mw, np.float32(-np.inf))), 0.0} <= weights, weights
    report = []
    for c in range(1, 8):
        d = (c & 1, (c >> 1) & 1, c >> 2)
        lo = t[:nz - d[2], :ny - d[1], :nx - d[0]] < 0
        hi = t[d[2]:, d[1]:, d[0]:] < 0
        crossed = lo != hi
        has = ((vmask[:nz - d[2], :ny - d[1], :nx - d[0]] >> (c - 1)) & 1).astype(bool)
        users = np.zeros(crossed.shape, np.int64)
        for m in CLASS_CELLS[c]:
            users |= live[1 - (m >> 2):1 - (m >> 2) + nz - d[2], 1 - ((m >> 1) & 1):1 - ((m >> 1) & 1) + ny - d[1],
                          1 - (m & 1):1 - (m & 1) + nx - d[0]].astype(np.int64) << m
        assert np.array_equal(has, crossed & (users != 0)), c  # the kernel's per-sample rule and the oracle's "edges of triangles" agree
        sets = set(users[crossed & has].tolist())
        report.append((c, int(has.sum()), int((crossed & ~has).sum()), len(sets)))
    text = "; ".join("class %d: %d with a vertex, %d crossed without, %d live-cell sets" % r for r in report)
    print(f"{row.name}: {text}")
    for c, n_with, n_without, n_sets in report:
        assert n_with > 0 and n_without > 0 and n_sets >= min(2, 2 ** len(CLASS_CELLS[c]) - 1), text


def _crossed_ends(row):
    x = row.inputs()
    lo, hi, _ = M.vertex_edges(M.oracle(row)["vmask"])
    t = x["tsdf"]
    return t[lo[2], lo[1], lo[0]], t[hi[2], hi[1], hi[0]]


def test_noise_has_every_planted_value_at_both_ends_of_crossed_edges():
    row = BY_NAME["noise"]
    v0, v1 = _crossed_ends(row)
    b0, b1 = M.bits(v0), M.bits(v1)
    counts = {}
    for s in M.SPECIALS:
        counts[repr(float(s))] = (int((b0 == M.bits(s)).sum()), int((b1 == M.bits(s)).sum()))
    pairs = {f"{float(a)!r}/{float(b)!r}": int(((b0 == M.bits(a)) & (b1 == M.bits(b))).sum()) for a, b in M.PAIRS}
    print(f"noise: crossed edges with the value at (lo, hi): {counts}; planted pairs: {pairs}")
    assert all(a > 0 and b > 0 for a, b in counts.values()), counts
    assert all(n > 0 for n in pairs.values()), pairs
    o32, o64 = M.oracle(row), M.oracle(row, True)
    assert np.isfinite(o32["vertices"]).all() and np.isfinite(o64["vertices"]).all() and np.isfinite(o32["normals"]).all()
    # t of the planted pairs, as IEEE division with denormals gives it: 1 / 2 on the clamp and between the two smallest denormals
    with np.errstate(all="ignore"):
        t = v0 / (v0 - v1)
    for a, b in M.PAIRS[:4]:
        assert (t[(b0 == M.bits(a)) & (b1 == M.bits(b))] == 0.5).all()
    assert (t[(b0 == M.bits(M.PAIRS[4][0])) & (b1 == M.bits(M.PAIRS[4][1]))] == 0).all()
    assert (t[(b0 == M.bits(M.PAIRS[5][0])) & (b1 == M.bits(M.PAIRS[5][1]))] == 1).all()
    d = float(np.abs(o32["vertices"].astype(np.float64) - o64["vertices"]).max())
    print(f"noise: float32 oracle within {d:.2e} of the float64 oracle in position")
    assert d < 1e-4
    pat = M.cell_patterns(row.inputs()["tsdf"])
    print(f"noise: {len(set(pat.reshape(-1).tolist()))} of 256 corner patterns (the patterns rows guarantee all)")


def test_colours_hit_the_rounding_and_clamp_boundaries_with_every_weighting():
    row = BY_NAME["colours"]
    x = row.inputs()
    lo, hi, _ = M.vertex_edges(M.oracle(row)["vmask"])
    at = lambda a, e: a[..., e[2], e[1], e[0]]
    v0, v1 = at(x["tsdf"], lo).astype(np.float64), at(x["tsdf"], hi).astype(np.float64)
    t = v0 / (v0 - v1)
    cw0, cw1 = at(x["cweight"], lo) > 0, at(x["cweight"], hi) > 0
    c0, c1 = at(x["rgb"], lo).astype(np.float64), at(x["rgb"], hi).astype(np.float64)
    both, one = cw0 & cw1, cw0 ^ cw1
    cv = np.where(both, c0 + t * (c1 - c0), np.where(cw0, c0, np.where(cw1, c1, 128.0)))
    half = cv - np.floor(cv) == 0.5
    n = {"both ends weighted": int(both.sum()), "lo only": int((cw0 & ~cw1).sum()), "hi only": int((cw1 & ~cw0).sum()),
         "neither": int((~cw0 & ~cw1).sum()), "k + 0.5, both": int((half & both).sum()), "k + 0.5, one": int((half & one).sum()),
         "k + 0.5, k even": int((half & (np.floor(cv) % 2 == 0)).sum()), "below 0": int((cv < 0).sum()), "-0.5": int((cv == -0.5).sum()),
         "above 255": int((cv > 255).sum()), "255.5": int((cv == 255.5).sum()),
         "just below 0.5": int((cv.astype(np.float32) == np.float32("0.49999997")).sum())}
    print(f"colours: {n}")
    assert all(v > 0 for v in n.values()), n
    zero = x["cweight"] == 0
    assert 0.25 < zero.mean() < 0.42 and np.signbit(x["cweight"][zero]).any()


@pytest.mark.parametrize("row", [r for r in M.EXTRACT_ROWS if r.observed and r.cells], ids=lambda r: r.id)
def test_fully_observed_rows_are_closed_up_to_the_outer_faces(row):
    o = M.oracle(row)
    tp = R.topology(o["vertices"], o["faces"])
    assert tp["max_edge_use"] == 2 and tp["directed_unique"] and tp["degenerate"] == 0 and tp["unreferenced"] == 0, tp
    lo, hi, _ = M.vertex_edges(o["vmask"])
    faces = M.on_outer_faces(lo, hi, row.dims)
    b = tp["boundary"]
    print(f"{row.name}: {len(o['vertices'])} vertices, {len(o['faces'])} faces, {len(b)} boundary edges")
    assert len(b) > 0 and ((faces[b[:, 0]] & faces[b[:, 1]]) != 0).all()
    assert np.isfinite(o["vertices"]).all()


@pytest.mark.parametrize("row", [r for r in M.EXTRACT_ROWS if r.empty], ids=lambda r: r.id)
def test_rows_without_a_surface_give_nothing(row):
    o = M.oracle(row)
    assert o["vertices"].shape == (0, 3) and o["faces"].shape == (0, 3) and not o["vmask"].any() and not o["ntri"].any()
    if row.variant == "dead":
        p = M.cell_patterns(row.inputs()["tsdf"])
        assert ((p > 0) & (p < 255)).any() and not M.live_cells(row.inputs()["weight"], row.min_weight).any()
    if row.variant == "outside":
        t = row.inputs()["tsdf"]
        assert (M.bits(t) == M.bits(np.float32("-0.0"))).any() and (M.bits(t) == 0).any()


@pytest.mark.parametrize("row", M.EXACT_ROWS, ids=lambda r: r.id)
def test_exact_rows_are_the_same_in_float32_and_float64(row):
    o32, o64 = M.oracle_volume(row, np.float32), M.oracle_volume(row, np.float64)
    for k in M.PLANES:
        same = np.array_equal(o32[k].astype(np.float64), o64[k])
        print(f"{row.name}: {k} float32 == float64: {same}; max {float(o64[k].max()):g}")
        assert same or k not in row.claims, k
    assert set(row.claims) >= {"tsdf", "weight", "cweight"}
    assert o32["weight"].max() == len(row.views()) and (o32["weight"] == 0).any() and (o32["cweight"] < o32["weight"]).any()
    masks = [m for _, _, m, _ in row.views() if m is not None]
    assert masks and all(set(np.unique(m).tolist()) == {0, 1, 255} for m in masks)


def test_exact_rows_meet_every_decision_with_equality():
    total = dict.fromkeys(M.EVENTS, 0)
    for row in M.EXACT_ROWS:
        n = M.events(row)
        print(f"{row.name}: {n}")
        for k, v in n.items():
            total[k] += v
    print(f"all exact rows: {total}")
    assert all(v > 0 for v in total.values()), total
    assert len({v[0].shape for r in M.EXACT_ROWS for v in r.views()}) >= 2  # a view of another size
    assert sum(len([m for _, _, m, _ in r.views() if m is not None]) for r in M.EXACT_ROWS) >= 2
