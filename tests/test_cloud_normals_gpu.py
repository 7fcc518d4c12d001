"""GPU checks of normals from neighbourhoods (pmn_knn_normals, pointcloud.knn_normals / estimate_normals, cloud_normals.py) against
tests/cloud_normals_ref.py.

What is float64 in the kernel is compared bit for bit: the count; the moments behind the covariance, recomputed on the host from the
lists knn_distance returns for the same grid; the surface variation and the normal itself against the host model of the kernel's Jacobi
sweeps (the same operations in the same order: a difference is a contraction or an ordering bug).  Independently of that model the
normal must lie within 1e-6 rad of numpy.linalg.eigh's vector wherever the reference's (l1 - l0) / l2 >= 1e-3 (the float32 rounding of
a unit vector is about 5e-8, the float64 Jacobi error at that gap about 1e-12) and have length 1 to 2^-23, for every k, cloud and
query mode (k = 1 has no normals).  On the sphere and the sheet at most 1 % of the clouds' own points may be left out of the eigh
comparison for a small gap (the reference leaves out 0 % at k = 8, 9, 16, 17, 20, 32 and 0.33 % at k = 3).  At k = 2 that limit cannot
hold -- a neighbourhood is three points, 3.47 % (sphere) and 2.28 % (sheet) of which are nearly collinear -- so there the limit is
4 %; the separate query sets have limits of their own (LEFT_OUT).  The lattice's and the duplicates' symmetric neighbourhoods have
equal eigenvalues by construction: they are compared where the gap allows, with no limit on how many."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_normals_ref as R
import knn_ref as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
KS = (1, 2, 3, 8, 9, 16, 17, 20, 32)  # across every capacity (8, 16, 32)
BIG = 1000.0
UNIT = 2.0 ** -23
# (same_cloud, k == 2) -> the share of the sphere's or the sheet's points that may drop out of the eigh comparison for a small gap.
# Measured with the reference alone (numpy): the clouds' own points 0 % at k = 8 .. 32 and 0.33 % at k = 3, but 3.47 % (sphere) and
# 2.28 % (sheet) at k = 2, where a neighbourhood is three points and that many triples are nearly collinear; of the 131 separate
# queries (half of them off the surface, where the plane through a query and its neighbours is arbitrary) at most 7, 5.3 %.
LEFT_OUT = {(True, False): 0.01, (True, True): 0.04, (False, False): 0.06, (False, True): 0.06}


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _clouds():
    """name -> (points, cell of the grid, max_dist)"""
    rng = np.random.default_rng(1)
    return {"sphere": (R.sphere_cloud()[0], 1.5, BIG),
            "sheet": (R.sheet_cloud(), 2.5, 5.0),            # the 40 planted outliers have fewer than two neighbours within 5
            "lattice": (K.lattice_cloud(), 0.5, 1.5),        # ties at every rank, points on cell faces, lists cut by max_dist
            "duplicates": (K.duplicate_cloud(), 0.7, 0.8),
            "one_point": (np.array([[1.0, 2.0, 3.0]], np.float32), 1.0, BIG),
            "two_points": (np.array([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0]], np.float32), 1.0, BIG),
            "three_points": (np.array([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0], [1.0, 2.25, 3.5]], np.float32), 1.0, BIG),
            "line": (K.axis_cloud(), 1.0, BIG),
            "one_cell": ((rng.uniform(0.0, 0.4, (90, 3)) + 5.0).astype(np.float32), 10.0, BIG)}


@pytest.fixture(scope="module")
def cases():
    """(name, same_cloud) -> dict(points, query, grid, max_dist, idx): the grid and the reference's 32 nearest, ties in the grid's
    sorted order, computed once and read by every k."""
    from patchmatchnet_amd import pointcloud as PC
    out = {}
    for name, (pts, cell, max_dist) in _clouds().items():
        grid = PC.build_grid(_dev(pts), cell)
        pos = np.empty(len(pts), np.int64)
        pos[grid.perm.cpu().numpy()] = np.arange(len(pts))  # original index -> sorted position
        for same in (True, False):
            query = None if same else K.far_queries(pts)
            out[name, same] = {"points": pts, "query": query, "grid": grid, "max_dist": max_dist,
                               "idx": R.neighbours(query, pts, 32, max_dist, same, rank=pos)}
    return out


def _run(PC, case, k, same, **kw):
    got = PC.knn_normals(None if same else _dev(case["query"]), case["grid"], k, case["max_dist"], same_cloud=same,
                         return_variation=True, return_count=True, **kw)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.float64 and got[2].dtype == torch.int32
    return tuple(t.cpu().numpy() for t in got)


@pytest.mark.parametrize("k", KS)
def test_normals_match_the_reference(cases, k):
    from patchmatchnet_amd import pointcloud as PC
    zero_seen = {}
    for (name, same), case in cases.items():
        tag = (name, same, k)
        pts, query, grid, max_dist = case["points"], case["query"], case["grid"], case["max_dist"]
        q = pts if same else query
        ref = R.normals(query, pts, k, max_dist, same, idx=case["idx"])
        normal, variation, count = _run(PC, case, k, same)
        assert normal.shape == (len(q), 3) and variation.shape == (len(q),) and count.shape == (len(q),)
        # the neighbour set: the count, and the moments of the lists the distance kernel reports for the same grid
        assert np.array_equal(count, ref["count"]), tag
        _, idx = PC.knn_distance(None if same else _dev(query), grid, k, max_dist, same_cloud=same, return_index=True)
        c, s, M = R.moments(q, pts, idx.cpu().numpy())
        assert np.array_equal(c, ref["count"]) and np.array_equal(s, ref["s"]) and np.array_equal(R.covariance(c, s, M), ref["C"]), tag
        # float64 outputs and the zero pattern: the host model, bit for bit
        assert np.array_equal((normal == 0).all(1), ~ref["valid"]), tag
        assert np.array_equal(variation, ref["variation"]), tag
        assert np.array_equal(normal, ref["normal"].astype(np.float32)), tag
        # a call that asks for the normal alone returns the same normal
        alone = PC.knn_normals(None if same else _dev(query), grid, k, max_dist, same_cloud=same)
        assert np.array_equal(alone.cpu().numpy(), normal), tag
        # against eigh, and the length
        valid = ref["valid"]
        zero_seen[name, same] = int((~valid).sum())
        if valid.any():
            assert np.abs(np.linalg.norm(normal[valid].astype(np.float64), axis=1) - 1.0).max() <= UNIT, tag
        e = R.normals(query, pts, k, max_dist, same, idx=case["idx"], solver=R.eigh)
        ok = valid & e["valid"] & (R.gap(e["values"]) >= 1e-3)
        if name in ("sphere", "sheet"):
            left_out = int((valid & ~ok).sum())
            print(f"{tag}: {left_out} of {len(q)} points left out for a small gap")
            assert left_out <= LEFT_OUT[same, k == 2] * len(q), tag
        if ok.any():
            ang = R.angle(normal[ok], e["normal"][ok], signed=False)
            print(f"{tag}: max angle to eigh {ang.max():.3e} rad over {int(ok.sum())} points")
            assert ang.max() <= 1e-6, tag
    # degenerate neighbourhoods occur exactly where the reference has them (asserted above); these are the ones it must have
    for name in ("line", "one_point", "two_points"):
        assert zero_seen[name, True] == len(cases[name, True]["points"])
    assert zero_seen["three_points", True] == (3 if k == 1 else 0)
    assert zero_seen["sheet", True] >= (1800 if k == 1 else 30)        # the planted outliers: fewer than two neighbours in range
    assert zero_seen["duplicates", True] > 0                            # a point whose neighbours are all copies of it
    assert zero_seen["sheet", False] >= 50                              # far queries: nothing within max_dist
    if k >= 2:
        assert zero_seen["sphere", True] == 0


@pytest.mark.parametrize("k", KS)
def test_cloud_of_k_plus_one_points(k):
    """k + 1 points: every list is exactly full under same_cloud; one point fewer and every list has a capped slot."""
    from patchmatchnet_amd import pointcloud as PC
    base = R.sphere_cloud(40, seed=9)[0]
    for n in (k, k + 1):
        pts = base[:n]
        grid = PC.build_grid(_dev(pts), 4.0)
        pos = np.empty(n, np.int64)
        pos[grid.perm.cpu().numpy()] = np.arange(n)
        ref = R.normals(None, pts, k, BIG, True, rank=pos)
        normal, variation, count = (t.cpu().numpy() for t in PC.knn_normals(None, grid, k, BIG, same_cloud=True, return_variation=True,
                                                                            return_count=True))
        assert (count == n - 1).all() and np.array_equal(count, ref["count"])
        assert np.array_equal(variation, ref["variation"]) and np.array_equal(normal, ref["normal"].astype(np.float32))
        assert np.array_equal((normal == 0).all(1), ~ref["valid"]) and ref["valid"].all() == (n >= 3)


def test_results_do_not_depend_on_the_grid_or_the_run():
    """Four grids (cells far below the spacing, about k points per cell, one cell for everything, a shifted origin) and two runs: the
    same bits.  (Not the lattice: there the k-th rank is tied between different points and the tie goes to the grid's sorted order.)"""
    from patchmatchnet_amd import pointcloud as PC
    for name, max_dist in (("sphere", BIG), ("sheet", 3.0), ("duplicates", 0.8)):
        pts = _clouds()[name][0]
        p = _dev(pts)
        lo = pts.min(0).astype(np.float64)
        grids = [PC.build_grid(p, 0.1), PC.build_grid(p, 3.0), PC.build_grid(p, 1000.0),
                 PC.build_grid(p, 3.0, origin=(lo - [7.25, 100.0, 55.5]).tolist())]
        views = np.array([[300.0, -200.0, 650.0], [0.0, 0.0, 0.0]])
        for k in (8, 20):
            for kw in ({}, {"viewpoints": views}):
                want = None
                for g in grids + grids[:1]:
                    got = [t.cpu().numpy() for t in PC.knn_normals(None, g, k, max_dist, same_cloud=True, return_variation=True,
                                                                   return_count=True, **kw)]
                    want = got if want is None else want
                    assert all(np.array_equal(a, b) for a, b in zip(got, want)), (name, k)
        # a separate query set with its order (a small max_dist: the far queries would walk thousands of 0.1-unit shells)
        q = _dev(K.far_queries(pts))
        want = None
        for g in grids + grids[:1]:
            got = [t.cpu().numpy() for t in PC.knn_normals(q, g, 16, min(max_dist, 3.0), return_variation=True, return_count=True)]
            want = got if want is None else want
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), name


def test_orientation_to_viewpoints(cases):
    from patchmatchnet_amd import pointcloud as PC
    case = cases["sphere", True]
    pts, centre = R.sphere_cloud()
    q = pts.astype(np.float64)
    # the centre as the single viewpoint: every normal points inwards
    n_in = PC.knn_normals(None, case["grid"], 16, BIG, same_cloud=True, viewpoints=centre[None]).cpu().numpy().astype(np.float64)
    assert ((n_in * (centre - q)).sum(1) > 0).all()
    # a viewpoint outside along each axis, and one more exactly as far from some points as another: the nearest, the lowest index
    views = np.concatenate([centre + 40.0 * s * np.eye(3)[a][None] for a in range(3) for s in (1.0, -1.0)])
    for k in (3, 16, 20):
        for same in (True, False):
            c = cases["sphere", same]
            ref = R.normals(c["query"], pts, k, BIG, same, viewpoints=views, idx=c["idx"])
            for v in (views, torch.from_numpy(views).to(DEV)):  # host numbers or a float64 tensor on the device
                got = PC.knn_normals(None if same else _dev(c["query"]), c["grid"], k, BIG, same_cloud=same, viewpoints=v)
                assert np.array_equal(got.cpu().numpy(), ref["normal"].astype(np.float32)), (k, same)
    out = PC.knn_normals(None, case["grid"], 16, BIG, same_cloud=True, viewpoints=views).cpu().numpy().astype(np.float64)
    j, e = R.nearest_viewpoint(pts, views)
    assert len(np.unique(j)) == 6 and ((out * e).sum(1) > 0).all() and ((out * (q - centre)).sum(1) > 0).all()  # outwards
    # one layer of a lattice, z = 0: the normal is exactly (0, 0, 1); two viewpoints mirrored in the plane are an exact tie
    x, y = np.meshgrid(np.arange(9.0), np.arange(8.0), indexing="ij")
    layer = np.random.default_rng(4).permutation(np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], 1)).astype(np.float32)
    grid = PC.build_grid(_dev(layer), 2.0)
    up = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(layer), 1))
    assert np.array_equal(PC.knn_normals(None, grid, 8, BIG, same_cloud=True).cpu().numpy(), up)
    below, above = [4.0, 4.0, -7.0], [4.0, 4.0, 7.0]
    assert np.array_equal(PC.knn_normals(None, grid, 8, BIG, same_cloud=True, viewpoints=[below, above]).cpu().numpy(), -up)
    assert np.array_equal(PC.knn_normals(None, grid, 8, BIG, same_cloud=True, viewpoints=[above, below]).cpu().numpy(), up)
    assert np.array_equal(PC.knn_normals(None, grid, 8, BIG, same_cloud=True, viewpoints=[[99.0, 0, 9.0], below, above]).cpu().numpy(), -up)
    # n . (c - q) == 0: a viewpoint inside the plane keeps the canonical sign, and one a hair below does not
    assert np.array_equal(PC.knn_normals(None, grid, 8, BIG, same_cloud=True, viewpoints=[[100.0, 3.0, 0.0]]).cpu().numpy(), up)
    assert np.array_equal(PC.knn_normals(None, grid, 8, BIG, same_cloud=True, viewpoints=[[100.0, 3.0, -1e-300]]).cpu().numpy(), -up)
    # the full lattice with viewpoints on lattice points: products of exactly 0 occur, and the reference decides them the same way
    c = cases["lattice", True]
    lat_views = np.array([[3.0, 2.0, 2.0], [0.0, 0.0, 0.0], [6.0, 5.0, 4.0], [3.0, 9.0, 2.0]])
    for k in (8, 20):
        ref = R.normals(None, c["points"], k, c["max_dist"], True, viewpoints=lat_views, idx=c["idx"])
        got = PC.knn_normals(None, c["grid"], k, c["max_dist"], same_cloud=True, viewpoints=lat_views)
        assert np.array_equal(got.cpu().numpy(), ref["normal"].astype(np.float32)), k


def test_estimate_normals_and_orient_like():
    from patchmatchnet_amd import pointcloud as PC
    pts, centre = R.sphere_cloud()
    p = _dev(pts)
    plain, variation, count = PC.estimate_normals(p, return_variation=True, return_count=True)
    cell = PC.default_cell(p)
    grid = PC.build_grid(p, cell)
    want = PC.knn_normals(None, grid, 16, PC.CLEAN_MAX_DIST_CELLS * cell, same_cloud=True, return_variation=True, return_count=True)
    assert torch.equal(plain, want[0]) and torch.equal(variation, want[1]) and torch.equal(count, want[2])
    assert torch.equal(PC.estimate_normals(p, k=8, max_dist=3.0, cell=2.0), PC.knn_normals(None, PC.build_grid(p, 2.0), 8, 3.0, same_cloud=True))
    assert torch.equal(PC.estimate_normals(p, viewpoints=centre[None]),
                       PC.knn_normals(None, grid, 16, PC.CLEAN_MAX_DIST_CELLS * cell, same_cloud=True, viewpoints=centre[None]))
    # orient_like: radial directions, a third of them inwards -- far from perpendicular to any normal, so the set is not in doubt
    rng = np.random.default_rng(6)
    like = pts.astype(np.float64) - centre
    like = (like / np.linalg.norm(like, axis=1, keepdims=True) * np.where(rng.random(len(pts)) < 0.33, -1.0, 1.0)[:, None]).astype(np.float32)
    n0 = plain.cpu().numpy()
    dot = (n0.astype(np.float64) * like.astype(np.float64)).sum(1)
    assert np.abs(dot).min() > 0.9 and 0 < (dot < 0).sum() < len(pts)
    got = PC.estimate_normals(p, orient_like=_dev(like)).cpu().numpy()
    assert np.array_equal(got, np.where((dot < 0)[:, None], -n0, n0))
    got3 = PC.estimate_normals(p, orient_like=_dev(like), return_count=True)
    assert np.array_equal(got3[0].cpu().numpy(), got) and torch.equal(got3[1], count)


def test_argument_checks():
    from patchmatchnet_amd import pointcloud as PC
    from patchmatchnet_amd._lib import PmnError
    pts = _dev(K.duplicate_cloud())
    grid = PC.build_grid(pts, 1.0)
    with pytest.raises(PmnError, match="no CPU fallback"):
        PC.knn_normals(pts.cpu(), grid, 4, 1.0)
    with pytest.raises(PmnError, match="no CPU fallback"):
        PC.estimate_normals(pts.cpu())
    with pytest.raises(PmnError, match="expected float32"):
        PC.knn_normals(pts.double(), grid, 4, 1.0)
    with pytest.raises(PmnError, match=r"contiguous \[n,3\]"):
        PC.knn_normals(pts[:, :2], grid, 4, 1.0)
    for k in (0, 33, 2.5, True):
        with pytest.raises(PmnError, match="k must be"):
            PC.knn_normals(pts, grid, k, 1.0)
    for bad in (float("inf"), float("nan"), 0.0, -1.0):
        with pytest.raises(PmnError, match="max_dist"):
            PC.knn_normals(pts, grid, 4, bad)
    for bad in (float("inf"), float("nan"), -1e-9):
        with pytest.raises(PmnError, match="line_ratio"):
            PC.knn_normals(pts, grid, 4, 1.0, line_ratio=bad)
    with pytest.raises(PmnError, match="same_cloud"):
        PC.knn_normals(pts, grid, 4, 1.0, same_cloud=True)
    for bad in (np.zeros((0, 3)), np.zeros((4097, 3)), np.zeros((5, 2)), np.zeros(3), [[0.0, float("nan"), 0.0]]):
        with pytest.raises(PmnError, match="viewpoints"):
            PC.knn_normals(pts, grid, 4, 1.0, viewpoints=bad)
    with pytest.raises(PmnError, match="viewpoints: expected float64"):
        PC.knn_normals(pts, grid, 4, 1.0, viewpoints=torch.zeros((2, 3), device=DEV))
    with pytest.raises(PmnError, match="viewpoints are on"):
        PC.knn_normals(pts, grid, 4, 1.0, viewpoints=torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(PmnError, match="not both"):
        PC.estimate_normals(pts, viewpoints=[[0.0, 0.0, 0.0]], orient_like=pts)
    for bad in (pts.cpu(), pts.double(), pts[:-1].contiguous()):
        with pytest.raises(PmnError, match="orient_like"):
            PC.estimate_normals(pts, orient_like=bad)
    with pytest.raises(PmnError, match="the grid on"):
        PC.knn_normals(pts, grid._replace(xyz=grid.xyz.cpu()), 4, 1.0)
    # the entry point validates before launching
    L = PC._lib.lib()
    a = PC._grid_args(grid)
    n = len(pts)
    out = torch.zeros((n, 3), dtype=torch.float32, device=DEV)
    views = torch.zeros((2, 3), dtype=torch.float64, device=DEV)
    q, o, v = pts.data_ptr(), out.data_ptr(), views.data_ptr()
    assert L.pmn_knn_normals(*a, q, None, n, 4, 1.0, 0, None, 0, 1e-6, None, None, None, None) == -1       # no normal
    assert L.pmn_knn_normals(*a, None, None, n, 4, 1.0, 0, None, 0, 1e-6, o, None, None, None) == -1       # no query
    assert L.pmn_knn_normals(None, *a[1:], q, None, n, 4, 1.0, 0, None, 0, 1e-6, o, None, None, None) == -1
    assert L.pmn_knn_normals(*a, q, None, n, 0, 1.0, 0, None, 0, 1e-6, o, None, None, None) == -1
    assert L.pmn_knn_normals(*a, q, None, n, 33, 1.0, 0, None, 0, 1e-6, o, None, None, None) == -1
    assert L.pmn_knn_normals(*a, q, None, n, 4, float("inf"), 0, None, 0, 1e-6, o, None, None, None) == -1
    assert L.pmn_knn_normals(*a, q, None, n, 4, 0.0, 0, None, 0, 1e-6, o, None, None, None) == -1
    assert L.pmn_knn_normals(*a, q, None, n - 1, 4, 1.0, 1, None, 0, 1e-6, o, None, None, None) == -1      # same_cloud, n_from != n_to
    assert L.pmn_knn_normals(*a, q, None, n, 4, 1.0, 0, None, 2, 1e-6, o, None, None, None) == -1          # viewpoints missing
    assert L.pmn_knn_normals(*a, q, None, n, 4, 1.0, 0, v, -1, 1e-6, o, None, None, None) == -1
    assert L.pmn_knn_normals(*a, q, None, n, 4, 1.0, 0, v, 4097, 1e-6, o, None, None, None) == -1
    assert L.pmn_knn_normals(*a, q, None, n, 4, 1.0, 0, None, 0, -1.0, o, None, None, None) == -1
    assert L.pmn_knn_normals(*a, q, None, n, 4, 1.0, 0, None, 0, float("nan"), o, None, None, None) == -1
    assert L.pmn_knn_normals(*a, q, None, n, 4, 1.0, 0, None, 0, float("inf"), o, None, None, None) == -1
    torch.cuda.synchronize()
    assert not out.any()  # nothing was launched


def _cli(args, timeout=120):
    return subprocess.run([sys.executable, os.path.join(ROOT, "cloud_normals.py")] + args, capture_output=True, text=True, timeout=timeout,
                          cwd=ROOT, env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})


def _body(path, n_bytes):
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    assert len(body) % n_bytes == 0
    return head.decode(), np.frombuffer(body, np.uint8).reshape(-1, n_bytes)


def test_cloud_normals_end_to_end(tmp_path):
    """One run of the tool on a file without normals, one with --drop_degenerate on its output (normals replaced, --orient
    existing), and the written file drawn shaded."""
    from patchmatchnet_amd import _lib, ply, pointcloud as PC, render
    pts = R.sheet_cloud(1500, seed=3)
    colors = np.random.default_rng(4).integers(0, 256, (len(pts), 3)).astype(np.uint8)
    src, dst, rep = str(tmp_path / "fused.ply"), str(tmp_path / "out" / "fused_normals.ply"), str(tmp_path / "report.json")
    ply.write_ply(src, pts, colors)
    view = [30.0, 30.0, 400.0]
    r = _cli(["--input", src, "--output", dst, "--k", "12", "--cell", "2.5", "--max_dist", "5.0", "--viewpoint"] + [str(v) for v in view] +
             ["--report", rep])
    assert r.returncode == 0, r.stderr
    want, variation, count = PC.estimate_normals(_dev(pts), k=12, max_dist=5.0, cell=2.5, viewpoints=[view], return_variation=True,
                                                 return_count=True)
    want = want.cpu().numpy()
    has = (want != 0).any(1)
    assert 30 <= (~has).sum() < 100  # the planted outliers
    head_in, rec_in = _body(src, 15)
    head_out, rec_out = _body(dst, 27)
    assert np.array_equal(rec_out[:, :12], rec_in[:, :12]) and np.array_equal(rec_out[:, 24:], rec_in[:, 12:])  # positions, colours
    assert np.array_equal(rec_out[:, 12:24], want.view(np.uint8).reshape(-1, 12))
    assert head_out + "end_header\n" == ply.header(len(pts), True, True).decode() and "property float nx" not in head_in
    assert ((want.astype(np.float64) * (np.array(view) - pts.astype(np.float64))).sum(1)[has] > 0).all()  # every normal faces the viewpoint
    js = json.load(open(rep))
    f = js["files"][0]
    assert js["abi"] == _lib.ABI_VERSION and js["k"] == 12 and js["orient"] == "viewpoint" and js["drop_degenerate"] is False
    assert (f["n"], f["k"], f["cell"], f["max_dist"], f["written"]) == (len(pts), 12, 2.5, 5.0, len(pts))
    assert f["zero_normals"] == int((~has).sum()) and f["capped"] == int((count < 12).sum())
    assert abs(f["mean_variation"] - float(variation[torch.from_numpy(has).to(DEV)].mean())) <= 1e-15
    line = [ln for ln in r.stdout.splitlines() if "points read" in ln]
    assert len(line) == 1 and f"{len(pts)} points read, {int((~has).sum())} without a normal" in line[0]
    # its own output as input: the normals are replaced, their side kept, and the zero-normal points dropped
    dst2 = str(tmp_path / "dropped.ply")
    r = _cli(["--input", dst, "--output", dst2, "--k", "12", "--cell", "2.5", "--max_dist", "5.0", "--orient", "existing",
              "--drop_degenerate"])
    assert r.returncode == 0, r.stderr
    _, rec2 = _body(dst2, 27)
    assert np.array_equal(rec2, rec_out[has])
    r = _cli(["--input", src, "--output", dst2, "--orient", "existing"])
    assert r.returncode == 2 and "needs normals" in r.stderr
    # the written file is usable where it is meant to be used: render.py's shading reads the normals
    model = render.upload_model(ply.read_ply_model(dst2), DEV)
    assert model["normals"] is not None and model["faces"] is None
    Ks, Es = render.orbit_cameras(np.concatenate([pts.min(0), pts.max(0)]), 1, 96, 128)
    rr = render.Renderer(DEV)
    args = (model["vertices"], Ks[0], Es[0], 96, 128, model["colors"], model["normals"])
    shaded = rr.render_points(*args, radius_px=1.0, shade=True)[2].clone()
    flat = rr.render_points(*args, radius_px=1.0, shade=False)[2].clone()
    drawn = int((rr.render_points(*args, radius_px=1.0, shade=False)[1] >= 0).sum())
    assert drawn > 500 and int((shaded != flat).any(2).sum()) > drawn // 10
    # ... which the input could not be: without normals, shading changes nothing
    bare = render.upload_model(ply.read_ply_model(src), DEV)
    args = (bare["vertices"], Ks[0], Es[0], 96, 128, bare["colors"], None)
    assert torch.equal(rr.render_points(*args, radius_px=1.0, shade=True)[2].clone(), rr.render_points(*args, radius_px=1.0, shade=False)[2])


def test_cloud_normals_scan_list_and_cameras(tmp_path):
    """--scan_list with --mvs_folder: every scan's cloud is oriented to its own cameras."""
    from patchmatchnet_amd import ply, pointcloud as PC
    (tmp_path / "list.txt").write_text("scan1\nscan9\n")
    want = {}
    for scan, seed, height in (("scan1", 5, 300.0), ("scan9", 6, -300.0)):
        pts = R.sheet_cloud(900, planted=0, seed=seed)
        ply.write_ply(str(tmp_path / "out" / scan / "fused.ply"), pts, np.full((len(pts), 3), 7, np.uint8))
        os.makedirs(tmp_path / "mvs" / scan / "cams")
        centres = []
        for i, (cx, cy) in enumerate(((10.0, 10.0), (50.0, 50.0), (30.0, 20.0))):
            C = np.array([cx, cy, height])
            E = np.eye(4)
            E[:3, 3] = -C
            centres.append(C)
            with open(tmp_path / "mvs" / scan / "cams" / f"{i:08d}_cam.txt", "w") as f:
                f.write("extrinsic\n" + "\n".join(" ".join(repr(float(v)) for v in row) for row in E) + "\n\nintrinsic\n"
                        "100 0 50\n0 100 40\n0 0 1\n\n1.0 2.0\n")
        want[scan] = (pts, PC.estimate_normals(_dev(pts), viewpoints=np.array(centres)).cpu().numpy(), height)
    r = _cli(["--input", str(tmp_path / "out"), "--scan_list", str(tmp_path / "list.txt"), "--mvs_folder", str(tmp_path / "mvs")])
    assert r.returncode == 0, r.stderr
    for scan, (pts, normal, height) in want.items():
        _, rec = _body(str(tmp_path / "out" / scan / "fused_normals.ply"), 27)
        assert np.array_equal(rec[:, 12:24], normal.view(np.uint8).reshape(-1, 12))
        assert (np.sign(normal[:, 2]) == np.sign(height)).all()
