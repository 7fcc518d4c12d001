"""CPU checks of the renderer space (tests/raster_space.py; DESIGN.md section 16, "Raster space"): every generator condition holds,
every family contains what it claims, the scalar reference (written from the header of csrc/render.hip) and the numpy oracle
(tests/render_ref.py) agree on every case in float32 and in float64 with no pixel left out, and the checker reports each of eight
planted mutations of the oracle.  A GPU failure of tests/test_raster_space_gpu.py can then only be the kernels'."""
import inspect
import types

import numpy as np
import pytest

import raster_space as S
import render_ref as RR

ALL = S.mesh_cases() + S.point_cases()


def test_names_are_unique_and_single_renders_are_capped():
    names = [c.name for c in ALL] + [c.name for f in S.fans() for c in f[1]]
    assert len(set(names)) == len(names)
    assert sum(len(f[1]) for f in S.fans()) <= 400
    assert all(c.h <= 129 and c.w <= 70 for c in ALL if c not in S.strips())
    assert {(c.h, c.w) for c in S.clipping()} == set(S.VIEWS) and [(c.h, c.w) for c in S.strips()] == S.STRIPS


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_generator_conditions_and_oracle_agreement(case):
    """The plan is what render_ref.project gives in both precisions; the reference's own conditions hold (asserted inside it); the
    float32 oracle passes the checker at every max_box and the float64 oracle picks the same winners: nothing is excluded."""
    S.check_plan(case)
    ref = S.reference(case)
    col, nrm = S.attributes(case)
    o32 = S.oracle(case, np.float32, col, nrm, True)
    o64 = S.oracle(case, np.float64)
    assert np.array_equal(o64["index"], ref.index) and np.array_equal(o32["index"], o64["index"])  # exclusion share 0
    stats = {}
    assert S.check(case, o32, ref, o32, stats=stats) == []
    assert stats["differ"] == 0 and stats["depth"] <= 1
    if case.faces is not None:
        for max_box in S.MAX_BOXES[1:]:
            got = RR.raster_triangles(case.vertices, case.faces, S.CAM, case.h, case.w, np.float32, max_box, count_hits=True)
            assert tuple(got["counters"]) == ref.counters(max_box) and np.array_equal(got["hits"], ref.hits)


def test_fans_cover_every_centre_inside_exactly_once():
    classes = {(np.sign(dx), np.sign(dy)) for dx, dy in S.RING16}
    assert len(classes) == 8  # dy < 0, dy > 0, dy == 0 with dx of either sign, both diagonals either way
    seen = [0, 0, 0]
    for together, singles, inside in S.fans():
        hits = np.zeros((together.h, together.w), np.int64)
        for c in singles:
            S.check_plan(c)
            for py, px in S.reference(c).covered[0]:
                hits[py, px] += 1
        ref = S.reference(together)
        assert inside.sum() >= 25 and (hits[inside] == 1).all() and hits.max() == 1, together.name
        assert np.array_equal(hits, ref.hits) and len(together.faces) == len(singles)
        for t, c in enumerate(singles):
            assert S.reference(c).covered[0] == ref.covered[t]
        seen = [a + b for a, b in zip(seen, ref.incidences)]
    assert min(seen) >= 100, seen


def test_soup_holds_the_edge_incidences():
    c = S.soup()
    ref = S.reference(c)
    assert len(c.faces) == 1000 and ref.incidences[0] >= 200 and ref.incidences[1] >= 200 and ref.incidences[2] >= 50, ref.incidences
    assert ref.hits.max() >= 3 and (ref.index >= 0).mean() > 0.5
    z = c.vertices[c.faces, 2]
    assert (z == ((8 + np.arange(1000)) / 8).astype(np.float32)[:, None]).all()


def test_perspective_triangles_are_tilted_and_take_both_paths():
    c = S.perspective()
    ref = S.reference(c)
    z = c.vertices[c.faces, 2]
    assert all(len(set(r)) == 3 for r in z.tolist()) and (ref.index >= 0).sum() > 500
    assert 0 < ref.counters(0)[3] < len(c.faces) or ref.counters(0)[3] == len(ref.boxes)
    assert any(not isinstance(d, int) and d.denominator > 8 for d in ref.depth.reshape(-1))  # depths that are not a vertex's


def test_degenerates_and_undrawable_faces_are_what_they_claim():
    c = S.degenerates()
    ref = S.reference(c)
    assert ref.counters() == (0, 0, 3, 0) and all(t not in ref.covered for t in c.claims["zero"])
    assert all(ref.covered[t] == set() for t in c.claims["sliver"])
    sizes = [len(ref.covered[t]) for t in c.claims["corner"]]
    assert sorted(sizes) == [0] * 6 + [1, 1], sizes  # only the right angle that is its triangle's top-left vertex, in both windings
    for t in c.claims["corner"]:
        if ref.covered[t]:
            X, Y = c.plan[c.faces[t][0]][:2] if c.plan[c.faces[t][0]][0] % 256 == 0 and c.plan[c.faces[t][0]][1] % 256 == 0 else c.plan[c.faces[t][2]][:2]
            assert ref.covered[t] == {(Y // 256, X // 256)}
    c = S.not_drawn()
    ref = S.reference(c)
    assert ref.count == [len(c.claims["behind"]), len(c.claims["band"]), 0]
    assert all(t not in ref.covered for t in c.claims["behind"] + c.claims["band"])
    assert all(ref.covered[t] for t in c.claims["drawn"] + c.claims["subnormal"])
    assert {S.GUARD, -S.GUARD, S.GUARD + 1} <= {int(round(float(v[0]) / float(v[2]))) for v in c.vertices if np.isfinite(v).all() and v[2] > 0}
    zs = c.vertices[:, 2]
    assert (zs == 0).sum() >= 2 and np.signbit(zs[zs == 0]).any() and (zs == np.float32(S.SUBNORMAL)).sum() == 2
    assert np.isnan(c.vertices).any() and np.isposinf(c.vertices).any() and np.isneginf(c.vertices).any()
    assert c.faces.min() < 0 and c.faces.max() >= len(c.vertices) and (c.faces == len(c.vertices)).any()


def test_clipping_cases_reach_every_border_and_the_strips_span_the_band():
    for c in S.clipping():
        ref = S.reference(c)
        assert all(ref.covered[t] == set() and t not in ref.boxes for t in c.claims["outside"]), c.name
        assert len(ref.covered[c.claims["whole"]]) == c.h * c.w
        drawn = set().union(*(ref.covered[t] for t in range(8)))
        corners = {(0, 0), (0, c.w - 1), (c.h - 1, 0), (c.h - 1, c.w - 1)}
        assert corners <= drawn, c.name
        assert c.plan and min(p[0] for p in c.plan) < 0 and min(p[1] for p in c.plan) < 0
    for c in S.strips():
        ref = S.reference(c)
        assert len(ref.covered[0]) == 16384 and ref.boxes[0] in ((16384, 1), (1, 16384))
        X = [p[0] for p in c.plan] + [p[1] for p in c.plan]
        assert min(X) == -S.GUARD and max(X) == S.GUARD


def test_box_matrix_and_worklists_have_the_claimed_shapes():
    shapes = set()
    for c in S.box_matrix():
        ref = S.reference(c)
        for t, box in c.claims["boxes"]:
            assert ref.boxes[t] == box and ref.covered[t], (c.name, t)
            shapes.add(box)
        assert ref.counters(1)[3] == sum(bw * bh > 1 for _, (bw, bh) in c.claims["boxes"])
    assert shapes == {(bw, bh) for bw in S.BOX_WIDTHS for bh in S.BOX_HEIGHTS}
    for n, c in zip(S.WORKLIST_LENGTHS, S.worklists()):
        ref = S.reference(c)
        assert len(c.claims["large"]) == n == ref.counters(0)[3] and all(ref.boxes[t] == (9, 9) for t in c.claims["large"])
        assert ref.counters(1 << 40)[3] == 0 and ref.counters(1)[3] >= n
        if n > 1:
            assert min(ref.count) > 0 and len(ref.boxes) > n  # undrawable faces of every kind and small triangles in between
            is_large = np.isin(np.arange(len(c.faces)), c.claims["large"])
            per_wave = [int(is_large[a:a + 64].sum()) for a in range(0, len(c.faces), 64)]
            lanes = {tuple(np.nonzero(is_large[a:a + 64])[0]) for a in range(0, len(c.faces), 64)}
            assert all(0 < k < 64 for k in per_wave[:-1]) and per_wave[-1] < 64 and len(lanes) >= min(3, len(per_wave)), (per_wave, len(lanes))
    assert 8 * S.WORKLIST_LENGTHS[-1] > 8192  # items (entry, slice) against the waves of raster_large_kernel's grid


def test_zbuffer_cases_decide_by_depth_then_index():
    for c in S.zbuffer():
        ref = S.reference(c)
        i, j = c.claims["copies"]
        assert ref.covered[i] == ref.covered[j] and (ref.index == i).any() and not (ref.index == j).any()
        assert (ref.index == 3).sum() == len(ref.covered[3]) and ref.covered[3] & ref.covered[0]  # nearer, higher index
        assert ref.covered[4] & ref.covered[0] and not {(py, px) for py, px in ref.covered[0] if ref.index[py, px] == 4}
    c, perm = S.permuted(S.soup(), 3)
    assert np.array_equal(np.where(S.reference(c).index >= 0, perm[S.reference(c).index], -1), S.reference(S.soup()).index)


def test_point_families_sit_on_their_thresholds():
    for c in S.nearest():
        ref = S.reference(c)
        for t, (X, Y, _) in enumerate(c.plan):
            px, py = (X + 128) >> 8, (Y + 128) >> 8
            assert ref.covered[t] == ({(py, px)} if 0 <= px < c.w and 0 <= py < c.h else set())
        assert {p[0] for p in c.plan} == set(S._nearest_values(c.w)) and {p[1] for p in c.plan} == set(S._nearest_values(c.h))
    assert (S.reference(S.nearest()[0]).hits > 1).any()
    assert [c.claims["Rq"] for c in S.radii()] == [127, 128, 128, 130, 128, 256, 1280, 8192]
    for c in S.radii():
        ref, Rq = S.reference(c), c.claims["Rq"]
        on = sum((256 * px - c.plan[t][0]) ** 2 + (256 * py - c.plan[t][1]) ** 2 == Rq * Rq for t in ref.covered for py, px in ref.covered[t])
        assert on >= (0 if Rq == 127 else 1), c.name  # centres exactly on the disc
        if Rq == 1280:
            X, Y, _ = c.plan[0]
            assert {(Y // 256 + dy, X // 256 + dx) for dx in (3, -3) for dy in (4, -4)} <= ref.covered[0] and on >= 12
        if Rq >= 128:
            assert not ref.covered[14] and not ref.covered[16] and not ref.covered[18] and ref.covered[13] and ref.covered[15] and ref.covered[17]
        borders = set().union(*(ref.covered[t] for t in range(5, 13)))
        assert {(0, 0), (0, c.w - 1), (c.h - 1, 0), (c.h - 1, c.w - 1)} <= borders or Rq < 256
    radii = set().union(*(c.claims["radii"] for c in S.radius_world()))
    assert 32 in radii and min(radii) < 32 and any(256 * 32 * float(z) < c.radius_world for c in S.radius_world() for z in c.vertices[:, 2])
    assert any(256 * 32 * float(z) == c.radius_world for c in S.radius_world() for z in c.vertices[:, 2])
    assert [len(c.vertices) for c in S.clouds()] == list(S.CLOUD_SIZES)
    assert all(min(S.reference(c).count[:2]) > 0 for c in S.clouds()[1:])
    for c in S.ties():
        ref = S.reference(c)
        assert ref.index[2, 2] == 0 and ref.hits[2, 2] >= 3 and ref.index[4, 4] == 5 and ref.index[2, 6] == 6
        p, perm = S.permuted(c, 1)
        rp = S.reference(p)
        assert np.array_equal(rp.depth, ref.depth) and (np.where(rp.index >= 0, perm[rp.index], -1) != ref.index).any()  # a tie moved


# ---- the checker has teeth --------------------------------------------------------------------------------------------------------------

def _mutant(*replacements):
    """A copy of render_ref with source snippets replaced: one planted defect in the oracle's output path."""
    src = inspect.getsource(RR)
    for old, new in replacements:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    mod = types.ModuleType("render_ref_mutant")
    exec(compile(src, "render_ref_mutant", "exec"), mod.__dict__)
    return mod


MUTATIONS = {
    "top-left dx > 0 flipped": ([("top_left = (dy < 0) | ((dy == 0) & (dx > 0))", "top_left = (dy < 0) | ((dy == 0) & (dx < 0))")],
                                lambda: [S.fans()[0][0], S.soup()], 0),
    "the box + 255 dropped": ([("px0 = np.maximum((X3.min(1) + 255) >> 8, 0)", "px0 = np.maximum(X3.min(1) >> 8, 0)"),
                               ("py0 = np.maximum((Y3.min(1) + 255) >> 8, 0)", "py0 = np.maximum(Y3.min(1) >> 8, 0)")],
                              lambda: [S.box_matrix()[0]], 1),
    "GUARD reduced by one": ([("GUARD = 1 << 22 ", "GUARD = (1 << 22) - 1 ")], lambda: [S.not_drawn(), S.strips()[0]], 0),
    "nearest-pixel threshold 129": ([("nx, ny = (x + 128) >> 8, (y + 128) >> 8", "nx, ny = (x + 129) >> 8, (y + 129) >> 8")],
                                    lambda: S.nearest(), 0),
    "disc <= changed to <": ([("(dx * dx + dy * dy <= Rq * Rq)", "(dx * dx + dy * dy < Rq * Rq)")], lambda: [S.radii()[4], S.radii()[6]], 0),
    "tie resolved to the higher index": ([("index = np.full(self.h * self.w, np.iinfo(np.int64).max, np.int64)",
                                           "index = np.full(self.h * self.w, -1, np.int64)"),
                                          ("np.minimum.at(index, pix[win], i[win])", "np.maximum.at(index, pix[win], i[win])")],
                                         lambda: [S.zbuffer()[0], S.nearest()[0], S.ties()[0]], 0),
    "z-buffer min replaced by last wins": ([("""        for pix, d, _ in self.cand:
            np.minimum.at(depth, pix, d)
        for pix, d, i in self.cand:
            win = d == depth[pix]
            np.minimum.at(index, pix[win], i[win])
""", """        for pix, d, i in self.cand:
            depth[pix] = d
            index[pix] = i
""")], lambda: [S.soup(), S.clouds()[5]], 0),
    "one slice of rows skipped": ([("""        ws, inside = _edge_values(S, tt, px << 8, py << 8)
""", """        ws, inside = _edge_values(S, tt, px << 8, py << 8)
        inside = inside & (((py - S["py0"][t]) % 64) // 8 != 1)
""")], lambda: [S.box_matrix()[4], S.strips()[1]], 0),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_the_checker_reports_a_mutated_oracle(name):
    replacements, cases, max_box = MUTATIONS[name]
    mutant = _mutant(*replacements)
    for case in cases():
        ref = S.reference(case)
        assert S.check(case, S.oracle(case, max_box=max_box), ref, max_box=max_box) == []
        fails = S.check(case, S.oracle(case, rr=mutant, max_box=max_box), ref, max_box=max_box)
        print(f"{name} on {case.name}: {fails}")
        assert fails, (name, case.name)
