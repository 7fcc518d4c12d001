"""CPU checks of mesh simplification by vertex clustering on its numpy restatement tests/simplify_ref.py: what
the algorithm promises -- planes stay planes, corners are kept better than by the mean, the clamp, the sqrt(3) * cell bound, the face
bookkeeping, the conditioning -- and the refusals of meshops.simplify_clustering that need no device.  tests/test_simplify_gpu.py holds
the kernels to the same restatement."""
import math

import numpy as np
import pytest
import torch

import meshops_ref as M
import simplify_ref as S

STIFFNESS = 1e-3


def _product():
    from patchmatchnet_amd import _lib, meshops
    assert S.LONG_RUN == _lib.MESH_PLACE_LONG_RUN
    return meshops.simplify_clustering


def _cases():
    plane = S.grid_plane(24)
    sheets = S.two_sheets()
    ico = M.icosphere(3)
    return {"plane": (plane[0], plane[1], 0.4, None), "cube": S.cube(8) + (0.3, None), "two sheets": sheets,
            "icosphere": (ico[0], ico[1], 0.35, None), "fan": S.fan(300) + (0.5, None)}


@pytest.fixture(scope="module")
def results():
    _product()
    return {name: (v, f, cell, S.simplify(v, f, cell, origin=origin, stiffness=STIFFNESS, return_condition=True))
            for name, (v, f, cell, origin) in _cases().items()}


def test_header_states_the_constants():
    import os
    from patchmatchnet_amd import _lib
    _product()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pmn_hip.h")).read()
    assert f"#define PMN_MESH_PLACE_LONG_RUN {_lib.MESH_PLACE_LONG_RUN}" in hdr
    assert f"#define PMN_MESH_SIMPLIFY_MAX_FACES {_lib.MESH_SIMPLIFY_MAX_FACES}" in hdr
    assert 3 * _lib.MESH_SIMPLIFY_MAX_FACES <= 2 ** 31 - 1 < 3 * (_lib.MESH_SIMPLIFY_MAX_FACES + 1)
    assert "once per corner" in hdr  # the weight of a face with several corners in one cluster is stated


def test_flat_grid_stays_on_its_plane(results):
    """Every vertex of z = 0.5 x + 0.25 y + 3 is exact in float32; a cluster's float32 mean is off the plane by at most the rounding
    of its three coordinates, (0.5 + 0.25 + 1) * ulp32(8) / 2 < 9e-7, and the minimiser keeps stiffness / (1 + stiffness) of that:
    below 1e-9 before the one rounding to float32; after it, below the 9e-7 of three rounded coordinates."""
    _product()
    v, f, cell, r = results["plane"]
    assert len(r["faces"]) and len(r["faces"]) < len(f) / 4
    for key, tol in (("exact", 1e-9), ("vertices", 9e-7)):
        p = r[key].astype(np.float64)
        off = np.abs(p[:, 2] - (0.5 * p[:, 0] + 0.25 * p[:, 1] + 3.0)).max()
        print(f"flat grid, {len(p)} representatives ({key}): largest distance from the plane {off:.3e}")
        assert off <= tol


def test_quadric_placement_keeps_the_cube_corners(results):
    """The unit cube at 8 squares an edge, cell 0.3: in the eight clusters that hold a corner, the quadric representative is nearer the
    true corner than the cluster's mean (DESIGN.md section 28 records both distances)."""
    _product()
    v, f, cell, r = results["cube"]
    mean = S.simplify(v, f, cell, placement="mean")
    assert np.array_equal(mean["faces"], r["faces"]) and np.array_equal(mean["vertex_map"], r["vertex_map"])
    worst_q, best_m = 0.0, np.inf
    for corner in np.ndindex(2, 2, 2):
        i = int(np.flatnonzero((v == np.float32(corner)).all(1))[0])
        k = r["vertex_map"][i]
        assert k >= 0
        dq = float(np.linalg.norm(r["exact"][k].astype(np.float64) - corner))
        dm = float(np.linalg.norm(mean["vertices"][k].astype(np.float64) - corner))
        print(f"cube corner {corner}: quadric {dq:.6f}, mean {dm:.6f}")
        assert dq < dm
        worst_q, best_m = max(worst_q, dq), min(best_m, dm)
    print(f"cube corners: largest quadric distance {worst_q:.6f}, smallest mean distance {best_m:.6f}")


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def test_no_representative_leaves_its_cell(results):
    _product()
    clamped = 0
    for name, (v, f, cell, r) in results.items():
        ctr = r["origin"] + (r["cells"] + 0.5) * cell
        x = r["exact_all"] - ctr
        eps = 2.0 * np.spacing(np.abs(ctr) + cell)  # (ctr + x) - ctr is x up to two float64 roundings
        assert (np.abs(x) <= cell / 2 + eps).all(), name  # before the rounding to float32: inside
        clamped += int((np.abs(x) >= cell / 2 - eps).sum())
        rep = r["exact_all"].astype(np.float32).astype(np.float64)
        over = np.maximum(np.abs(rep - ctr) - cell / 2, 0.0)
        assert (over <= _ulp32(rep)).all(), name
    v, f, cell, r = results["two sheets"]
    x = r["exact_all"] - (r["origin"] + (r["cells"] + 0.5) * cell)
    print(f"coordinates at the clamp: {clamped} in all cases, {int((np.abs(x) >= cell / 2 - 1e-12).sum())} of the two sheets")
    assert (x[:, 0] <= -cell / 2 + 1e-12).any()  # the sheets' planes meet left of their cells: the clamp is what holds these


def test_every_vertex_is_within_sqrt3_cells_of_its_representative(results):
    _product()
    for name, (v, f, cell, r) in results.items():
        for placement in ("quadric", "mean"):
            rep = r["exact_all"] if placement == "quadric" else r["mean_all"]
            d = np.linalg.norm(v.astype(np.float64) - rep[r["cluster"]].astype(np.float32).astype(np.float64), axis=1)
            print(f"{name} ({placement}): largest distance vertex - representative {d.max():.4f} = {d.max() / cell:.3f} cells")
            assert d.max() <= math.sqrt(3.0) * cell


def _check_bookkeeping(v, f, r):
    faces, vmap = r["faces"], r["vertex_map"]
    n = len(r["vertices"])
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    assert (faces[:, 0] < faces[:, 1]).all() and (faces[:, 0] < faces[:, 2]).all()  # rotated: the smallest index first
    assert len(S.face_set(faces)) == len(faces)  # unique per orientation
    if len(faces):
        assert faces.min() == 0 and faces.max() == n - 1 and len(np.unique(faces)) == n
    assert vmap.shape == (len(v),) and vmap.min() >= -1 and vmap.max() == n - 1
    # vertex_map is the faces' own map: an input face whose corners map to three different outputs is an output face
    t = vmap[np.asarray(f, np.int64)]
    alive = (t >= 0).all(1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    shift = t[alive].argmin(1)
    rot = np.stack([t[alive][np.arange(int(alive.sum())), (shift + k) % 3] for k in range(3)], 1)
    assert S.face_set(rot) == S.face_set(faces)
    # ... in input order, the first of equals
    firsts, seen = [], set()
    for row in map(tuple, rot.tolist()):
        if row not in seen:
            seen.add(row)
            firsts.append(row)
    assert firsts == list(map(tuple, faces.tolist()))


def test_face_bookkeeping(results):
    _product()
    for name, (v, f, cell, r) in results.items():
        _check_bookkeeping(v, f, r)
        print(f"{name}: {len(v)} vertices, {len(f)} faces -> {len(r['vertices'])} vertices, {len(r['faces'])} faces")
    # duplicates, an opposite pair, degenerate faces and an unreferenced vertex
    v, f, cell, r = results["icosphere"]
    v2 = np.concatenate([v, [[0.0, 0.0, 0.0]]]).astype(np.float32)
    f2 = np.concatenate([f[:40], f, f[100:130, ::-1], [[3, 3, 9], [5, 5, 5]]]).astype(np.int32)
    r2 = S.simplify(v2, f2, cell)
    _check_bookkeeping(v2, f2, r2)
    assert r2["vertex_map"][-1] == -1
    flipped = S.face_set(r2["faces"]) - S.face_set(r["faces"])
    assert flipped and all((a, c, b) in S.face_set(r["faces"]) for a, b, c in flipped)  # both orientations stay
    assert len(r2["faces"]) == len(r["faces"]) + len(flipped)


def test_face_order_does_not_matter(results):
    _product()
    for name in ("icosphere", "cube", "fan"):
        v, f, cell, r = results[name]
        for g in (np.ascontiguousarray(f[::-1]), M.permute_faces(f, 3)):
            p = S.simplify(v, g, cell)
            assert S.face_set(p["faces"]) == S.face_set(r["faces"]), name
            assert np.array_equal(p["vertex_map"], r["vertex_map"]), name
            assert p["exact"].tobytes() == r["exact"].tobytes(), name  # the sums run in the faces' own order, not the array's


def test_condition_number_is_bounded(results):
    _product()
    bound = (1.0 + STIFFNESS) / STIFFNESS
    for name, (v, f, cell, r) in results.items():
        worst = float(r["condition_all"].max())
        print(f"{name}: largest condition number over {len(r['condition_all'])} clusters {worst:.3f} (bound {bound:.1f})")
        assert worst <= bound * (1.0 + 1e-9)
    v, f, cell, r = results["icosphere"]
    for s in (1e-6, 1.0):
        c = S.simplify(v, f, cell, stiffness=s, return_condition=True)["condition_all"].max()
        assert c <= (1.0 + s) / s * (1.0 + 1e-9)


def test_float64_agrees_with_the_extended_reference(results):
    _product()
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than float64 on this platform"
    for name, (v, f, cell, r) in results.items():
        origin = _cases()[name][3]
        ext = S.simplify(v, f, cell, origin=origin, stiffness=STIFFNESS, dtype=np.longdouble)
        gap = float(np.abs(r["exact"].astype(np.longdouble) - ext["exact"]).max()) if len(ext["exact"]) else 0.0
        print(f"{name}: max |float64 - longdouble| = {gap:.3e}")
        assert np.array_equal(ext["faces"], r["faces"]) and gap <= 1e-10


def test_refusals_that_need_no_device():
    from patchmatchnet_amd import PmnError
    simplify = _product()
    v, f = M.icosphere(1)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(PmnError, match="ROCm GPU|cuda|device"):
        simplify(tv, tf, 0.5)
    for cell in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(PmnError, match="cell must be positive and finite"):
            simplify(tv, tf, cell)
    for s in (0.0, -1e-3, float("inf"), float("nan")):
        with pytest.raises(PmnError, match="stiffness must be positive and finite"):
            simplify(tv, tf, 0.5, stiffness=s)
    with pytest.raises(PmnError, match="placement"):
        simplify(tv, tf, 0.5, placement="median")
