"""GPU checks of the k-nearest-neighbour and radius searches (pmn_knn_distance, pmn_radius_count), the cleaning filters of
patchmatchnet_amd/pointcloud.py and clean_cloud.py against the brute-force numpy float64 statements of tests/knn_ref.py.

Squared distances, means and counts follow the definition in un-contracted float64, so they are compared bit for bit
(np.array_equal); indices are checked by their properties (a tie may be broken either way by an argsort), the filters' keep masks
exactly, on inputs whose reference shows no mean within a relative 1e-9 of the threshold (the product's mu and sigma are float64 sums
in another order: a few ulp)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import knn_ref as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
KS = (1, 2, 8, 9, 20, 32)
BIG = 1000.0  # a max_dist that cuts nothing inside a cloud


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _clouds():
    """name -> (points, cell of the grid, a max_dist that cuts some lists part way)"""
    rng = np.random.default_rng(1)
    return {"surface": (K.surface_cloud()[0], 2.5, 1.5),
            "lattice": (K.lattice_cloud(), 0.5, 1.5),  # spacing 1: every point on a cell face; neighbours at 1, sqrt 2 | sqrt 3, 2
            "duplicates": (K.duplicate_cloud(), 0.7, 0.8),
            "one_point": (np.array([[1.0, 2.0, 3.0]], np.float32), 1.0, 1.0),
            "one_cell": ((rng.uniform(0.0, 0.4, (90, 3)) + 5.0).astype(np.float32), 10.0, 0.1),
            "axis": (K.axis_cloud(), 1.0, 0.5)}


@pytest.fixture(scope="module")
def clouds():
    return _clouds()


@pytest.fixture(scope="module")
def rows(clouds):
    """(name, same_cloud) -> (queries, sorted rows of the full matrix): computed once, read by every k."""
    out = {}
    for name, (pts, _, _) in clouds.items():
        q = K.far_queries(pts)
        out[name, True] = (None, K.sorted_d2(None, pts, True))
        out[name, False] = (q, K.sorted_d2(q, pts, False))
    return out


def _check_rows(PC, pts, grid, query, same, k, max_dist, want_rows, tag):
    """One call against the reference; returns (partly capped rows, fully capped rows)."""
    want = K.knn_d2(query, pts, k, max_dist, same, rows=want_rows)
    mean, d2, idx = PC.knn_distance(None if same else _dev(query), grid, k, max_dist, same_cloud=same, return_d2=True,
                                    return_index=True)
    mean, d2, idx = mean.cpu().numpy(), d2.cpu().numpy(), idx.cpu().numpy()
    n = len(pts) if same else len(query)
    assert d2.shape == (n, k) and d2.dtype == np.float64 and idx.shape == (n, k) and idx.dtype == np.int64 and mean.shape == (n,)
    assert np.array_equal(d2, want), tag
    assert np.array_equal(mean, K.knn_mean(want, max_dist)), tag
    # a second call that asks for the mean alone gives the same mean
    assert np.array_equal(PC.knn_distance(None if same else _dev(query), grid, k, max_dist, same_cloud=same).cpu().numpy(), mean), tag
    # indices: in range or -1 exactly where the slot is capped, distinct, never the query itself, and each reproduces its d2
    cap = float(max_dist) * float(max_dist)
    capped = want == cap
    assert np.array_equal(idx < 0, capped) and (idx[capped] == -1).all() and (idx < len(pts)).all(), tag
    q = pts if same else query
    for i in range(n):
        live = idx[i][idx[i] >= 0]
        assert len(np.unique(live)) == len(live), tag
        if same:
            assert i not in live, tag
        assert np.array_equal(K.pair_d2(q[i:i + 1], pts[live])[0], d2[i][:len(live)]), tag
    ncap = capped.sum(1)
    return int(((ncap > 0) & (ncap < k)).sum()), int((ncap == k).sum())


@pytest.mark.parametrize("k", KS)
def test_knn_matches_brute_force(clouds, rows, k):
    from patchmatchnet_amd import pointcloud as PC
    seen = {}
    for name, (pts, cell, cut) in clouds.items():
        assert len(pts) % 64 != 0
        grid = PC.build_grid(_dev(pts), cell)
        for same in (True, False):
            query, want_rows = rows[name, same]
            for max_dist in (cut, BIG):
                seen[name, same, max_dist] = _check_rows(PC, pts, grid, query, same, k, max_dist, want_rows, (name, same, k, max_dist))
    # the cases really occur: lists cut part way and queries with no neighbour at all (the planted outliers, the far queries)
    if k >= 8:
        assert seen["surface", True, 1.5][0] > 0 and seen["lattice", True, 1.5][0] > 0
    assert seen["surface", True, 1.5][1] > 0 and seen["surface", False, BIG][1] > 0 and seen["one_point", True, BIG][1] == 1


@pytest.mark.parametrize("k", KS)
def test_knn_fewer_points_than_k(k):
    """A cloud of k points (k - 1 neighbours under same_cloud, k for a separate query) and one of k + 1."""
    from patchmatchnet_amd import pointcloud as PC
    base = K.duplicate_cloud(67, seed=9)
    for n in (k, k + 1):
        pts = base[:n]
        grid = PC.build_grid(_dev(pts), 0.9)
        query = K.far_queries(pts, n=27)
        for same in (True, False):
            part, _ = _check_rows(PC, pts, grid, query, same, k, BIG, None, (n, same, k))
            assert (part > 0) == (same and n == k and k > 1)


def test_knn_ties_go_to_the_lower_sorted_index(clouds):
    """On the lattice every rank is tied.  Within a run of equal d2 the returned points ascend in the grid's sorted order, and a run
    cut by k holds the lowest sorted positions among all points at that distance."""
    from patchmatchnet_amd import pointcloud as PC
    pts = clouds["lattice"][0]
    for cell in (0.5, 3.0):
        grid = PC.build_grid(_dev(pts), cell)
        perm = grid.perm.cpu().numpy()
        pos = np.empty(len(pts), np.int64)
        pos[perm] = np.arange(len(pts))  # original index -> sorted position
        full = K.pair_d2(pts, pts)
        for k in (2, 9, 20):
            _, d2, idx = PC.knn_distance(None, grid, k, BIG, same_cloud=True, return_d2=True, return_index=True)
            d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
            for i in range(len(pts)):
                for v in np.unique(d2[i]):
                    got = pos[idx[i][d2[i] == v]]
                    assert (np.diff(got) > 0).all()
                    tied = np.sort(pos[np.flatnonzero((full[i] == v) & (np.arange(len(pts)) != i))])
                    assert np.array_equal(got, tied[:len(got)])


def test_radius_count_matches_brute_force(clouds):
    from patchmatchnet_amd import pointcloud as PC
    radii = {"lattice": (0.0, 0.4, 1.0, 2.0, 3.7),      # 1.0 and 2.0 are lattice spacings: "<=" on the rooted value
             "surface": (0.0, 0.01, 1.0, 9.0),
             "duplicates": (0.0, 1e-3, 0.5, 4.0),
             "one_point": (0.0, 1.0), "one_cell": (0.0, 0.05, 1.0), "axis": (0.0, 0.01, 0.5, 7.0)}
    for name, (pts, cell, _) in clouds.items():
        grid = PC.build_grid(_dev(pts), cell)
        query = K.far_queries(pts)
        for r in radii[name]:
            for same in (True, False):
                got = PC.radius_count(None if same else _dev(query), grid, r, same_cloud=same)
                assert got.dtype == torch.int32
                assert np.array_equal(got.cpu().numpy(), K.radius_count(query, pts, r, same)), (name, r, same)
    lat = clouds["lattice"][0]
    assert K.radius_count(None, lat, 1.0, True).max() == 6 and K.radius_count(None, lat, 0.4, True).max() == 0
    assert K.radius_count(None, clouds["duplicates"][0], 0.0, True).max() >= 1  # a duplicate at distance 0 is a neighbour


def test_results_do_not_depend_on_the_grid(clouds):
    """Cells far below the point spacing (1.1), about k points per cell, one cell for everything; a shifted origin."""
    from patchmatchnet_amd import pointcloud as PC
    pts = clouds["surface"][0]
    p = _dev(pts)
    k, max_dist, radius = 20, 3.0, 2.0
    want = K.knn_d2(None, pts, k, max_dist, True)
    wc = K.radius_count(None, pts, radius, True)
    grids = [PC.build_grid(p, 0.1), PC.build_grid(p, 3.0), PC.build_grid(p, 1000.0), PC.build_grid(p, 3.0, origin=[-7.25, -100.0, -55.5])]
    for g in grids:
        mean, d2 = PC.knn_distance(None, g, k, max_dist, same_cloud=True, return_d2=True)
        assert np.array_equal(d2.cpu().numpy(), want) and np.array_equal(mean.cpu().numpy(), K.knn_mean(want, max_dist))
        assert np.array_equal(PC.radius_count(None, g, radius, same_cloud=True).cpu().numpy(), wc)


def _no_near_tie(mean, threshold):
    return (np.abs(mean - threshold) > 1e-9 * abs(threshold)).all()


def test_filters_match_the_reference(clouds):
    from patchmatchnet_amd import pointcloud as PC
    for name, k, ratio, max_dist in (("surface", 20, 2.0, 5.0), ("surface", 8, 1.0, 3.0), ("lattice", 8, 1.0, 2.0),
                                     ("duplicates", 8, 1.0, 2.0)):
        pts = clouds[name][0]
        keep, mean, threshold = K.statistical_outliers(pts, k, ratio, max_dist)
        assert _no_near_tie(mean, threshold) and keep.any() and not keep.all()
        for cell in (None, clouds[name][1]):
            gk, gm, gt = PC.statistical_outliers(_dev(pts), k=k, std_ratio=ratio, max_dist=max_dist, cell=cell)
            assert gk.dtype == torch.bool and isinstance(gt, float)
            assert np.array_equal(gm.cpu().numpy(), mean) and abs(gt - threshold) <= 1e-12 * threshold
            assert np.array_equal(gk.cpu().numpy(), keep), (name, k)
    for name, radius, least in (("surface", 2.0, 4), ("surface", 1.0, 2), ("lattice", 1.0, 5), ("duplicates", 0.0, 1)):
        pts = clouds[name][0]
        keep, count = K.radius_outliers(pts, radius, least)
        assert keep.any() and not keep.all()
        gk, gc = PC.radius_outliers(_dev(pts), radius, least)
        assert np.array_equal(gc.cpu().numpy(), count) and np.array_equal(gk.cpu().numpy(), keep), (name, radius)
    # default max_dist and cell: nothing to compare bit for bit (the cap follows the cell), but the call runs and keeps most points
    gk, _, _ = PC.statistical_outliers(_dev(clouds["surface"][0]))
    assert 0.9 < float(gk.float().mean()) < 1.0


def test_filters_remove_the_planted_outliers():
    """The reference (k = 20, 2 sigma, max_dist 5) removes every planted point farther than 2.0 from the sheet -- the farthest it
    keeps is 1.73 off, the nearest it removes 3.15 -- and 0.6 % of the surface points; radius 2.0 with 4 neighbours removes every
    planted point farther than 2.0 and 2.7 % of the surface points.  The product must do the same."""
    from patchmatchnet_amd import pointcloud as PC
    pts, planted, offset = K.surface_cloud()
    far = planted & (offset > 2.0)
    assert far.sum() >= 50
    for ref_keep, got, share in ((K.statistical_outliers(pts, 20, 2.0, 5.0)[0], PC.statistical_outliers(_dev(pts), 20, 2.0, 5.0)[0], 0.01),
                                 (K.radius_outliers(pts, 2.0, 4)[0], PC.radius_outliers(_dev(pts), 2.0, 4)[0], 0.03)):
        for keep in (ref_keep, got.cpu().numpy()):
            assert not keep[far].any()
            assert (~keep[~planted]).mean() <= share


def test_wrapper_errors(clouds):
    from patchmatchnet_amd import pointcloud as PC
    from patchmatchnet_amd._lib import PmnError
    pts = _dev(clouds["duplicates"][0])
    grid = PC.build_grid(pts, 1.0)
    with pytest.raises(PmnError, match="no CPU fallback"):
        PC.knn_distance(pts.cpu(), grid, 4, 1.0)
    with pytest.raises(PmnError, match="no CPU fallback"):
        PC.radius_count(pts.cpu(), grid, 1.0)
    with pytest.raises(PmnError, match="no CPU fallback"):
        PC.statistical_outliers(pts.cpu())
    with pytest.raises(PmnError, match="no CPU fallback"):
        PC.radius_outliers(pts.cpu(), 1.0, 2)
    for k in (0, 33, 2.5):
        with pytest.raises(PmnError, match="k must be"):
            PC.knn_distance(pts, grid, k, 1.0)
    for bad in (float("inf"), float("nan"), 0.0, -1.0):
        with pytest.raises(PmnError, match="max_dist"):
            PC.knn_distance(pts, grid, 4, bad)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(PmnError, match="radius"):
            PC.radius_count(pts, grid, bad)
    with pytest.raises(PmnError, match="same_cloud"):
        PC.knn_distance(pts, grid, 4, 1.0, same_cloud=True)
    with pytest.raises(PmnError, match="same_cloud"):
        PC.radius_count(pts, grid, 1.0, same_cloud=True)
    nan = pts.clone()
    nan[3, 1] = float("nan")
    with pytest.raises(PmnError, match="non-finite"):
        PC.knn_distance(nan, grid, 4, 1.0)
    with pytest.raises(PmnError, match="non-finite"):
        PC.statistical_outliers(nan)
    if torch.cuda.device_count() > 1:
        with pytest.raises(PmnError, match="the grid on"):
            PC.knn_distance(pts.to("cuda:1"), grid, 4, 1.0)
    # the device check itself, on any machine: a grid whose tensors sit elsewhere
    other = grid._replace(xyz=grid.xyz.cpu())
    with pytest.raises(PmnError, match="the grid on"):
        PC.knn_distance(pts, other, 4, 1.0)
    with pytest.raises(PmnError, match="the grid on"):
        PC.radius_count(pts, other, 1.0)
    # the entry points validate before launching
    L = PC._lib.lib()
    a = PC._grid_args(grid)
    n = len(pts)
    assert L.pmn_knn_distance(*a, pts.data_ptr(), None, n, 0, 1.0, 0, None, None, None, None) == -1
    assert L.pmn_knn_distance(*a, pts.data_ptr(), None, n, 33, 1.0, 0, None, None, None, None) == -1
    assert L.pmn_knn_distance(*a, pts.data_ptr(), None, n, 4, float("inf"), 0, None, None, None, None) == -1
    assert L.pmn_knn_distance(*a, pts.data_ptr(), None, n - 1, 4, 1.0, 1, None, None, None, None) == -1  # same_cloud, n_from != n_to
    assert L.pmn_radius_count(*a, pts.data_ptr(), None, n, -1.0, 0, pts.data_ptr(), None) == -1
    assert L.pmn_radius_count(*a, pts.data_ptr(), None, n, 1.0, 0, None, None) == -1


def _run(args, timeout=120):
    return subprocess.run([sys.executable, os.path.join(ROOT, "clean_cloud.py")] + args, capture_output=True, text=True, timeout=timeout,
                          cwd=ROOT, env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})


def _body(path, n_bytes):
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    assert len(body) % n_bytes == 0
    return head.decode(), np.frombuffer(body, np.uint8).reshape(-1, n_bytes)


@pytest.mark.parametrize("normals", [False, True])
def test_clean_cloud_end_to_end(tmp_path, normals):
    from patchmatchnet_amd import _lib, fusion
    pts, _, _ = K.surface_cloud(3000, seed=2)
    rng = np.random.default_rng(4)
    colors = rng.integers(0, 256, (len(pts), 3)).astype(np.uint8)
    nrm = rng.normal(size=(len(pts), 3)).astype(np.float32) if normals else None
    src, dst, rep = str(tmp_path / "fused.ply"), str(tmp_path / "out" / "fused_clean.ply"), str(tmp_path / "report.json")
    fusion.write_ply(src, pts, colors, nrm)
    keep, mean, threshold = K.statistical_outliers(pts, 20, 2.0, 5.0)
    assert _no_near_tie(mean, threshold)
    r = _run(["--input", src, "--output", dst, "--method", "statistical", "--k", "20", "--std_ratio", "2.0", "--max_dist", "5.0",
              "--report", rep])
    assert r.returncode == 0, r.stderr
    width = 27 if normals else 15
    head_in, rec_in = _body(src, width)
    head_out, rec_out = _body(dst, width)
    assert np.array_equal(rec_out, rec_in[keep])
    assert head_out == head_in.replace(f"element vertex {len(pts)}", f"element vertex {int(keep.sum())}")
    line = [ln for ln in r.stdout.splitlines() if "points read" in ln]
    assert len(line) == 1 and f"{len(pts)} points read, {int(keep.sum())} kept, {int((~keep).sum())} removed" in line[0]
    js = json.load(open(rep))
    assert js["abi"] == _lib.ABI_VERSION and js["method"] == "statistical" and js["k"] == 20 and js["max_dist"] == 5.0
    f = js["files"][0]
    assert (f["points"], f["kept"], f["removed"]) == (len(pts), int(keep.sum()), int((~keep).sum()))
    assert abs(f["threshold"] - threshold) <= 1e-12 * threshold


def test_clean_cloud_folder_and_scan_list(tmp_path):
    from patchmatchnet_amd import fusion
    want = {}
    for scan, seed in (("scan1", 5), ("scan9", 6)):
        pts, _, _ = K.surface_cloud(1500, seed=seed)
        fusion.write_ply(str(tmp_path / scan / "fused.ply"), pts, np.full((len(pts), 3), 7, np.uint8))
        want[scan] = K.radius_outliers(pts, 2.5, 3)[0]
    (tmp_path / "list.txt").write_text("scan1\nscan9\n")
    rep = str(tmp_path / "r.json")
    r = _run(["--input", str(tmp_path), "--scan_list", str(tmp_path / "list.txt"), "--method", "radius", "--radius", "2.5",
              "--min_neighbors", "3", "--report", rep])
    assert r.returncode == 0, r.stderr
    assert len([ln for ln in r.stdout.splitlines() if "points read" in ln]) == 2
    for scan, keep in want.items():
        _, rec_in = _body(str(tmp_path / scan / "fused.ply"), 15)
        _, rec_out = _body(str(tmp_path / scan / "fused_clean.ply"), 15)
        assert np.array_equal(rec_out, rec_in[keep])
    js = json.load(open(rep))
    assert [f["kept"] for f in js["files"]] == [int(want["scan1"].sum()), int(want["scan9"].sum())] and js["radius"] == 2.5


def test_realistic_size_agrees_with_nn_distance():
    """~1 M points, statistical, k = 20, default cell and max_dist; no brute force: the first neighbour of 100 k separate queries
    must be the one pmn_nn_distance finds, to the bit."""
    from patchmatchnet_amd import pointcloud as PC
    n = 1_000_003
    rng = np.random.default_rng(0)
    xy = rng.uniform(0.0, 600.0, (n, 2))
    z = 40.0 * np.sin(xy[:, 0] / 90.0) * np.cos(xy[:, 1] / 70.0) + rng.normal(0.0, 0.05, n)
    z[::53] += rng.uniform(-300.0, 300.0, len(z[::53]))
    pts = _dev(np.stack([xy[:, 0], xy[:, 1], z], 1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep, mean, threshold = PC.statistical_outliers(pts, k=20)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    removed = int((~keep).sum())
    print(f"statistical_outliers, {n} points, k = 20: {t1 - t0:.3f} s, threshold {threshold:.4f}, {removed} removed")
    assert n // 53 // 2 < removed < n // 20 and bool(torch.isfinite(mean).all())
    cell = PC.default_cell(pts)
    grid = PC.build_grid(pts, cell)
    m = 100_003
    q = np.stack([rng.uniform(-50.0, 650.0, m), rng.uniform(-50.0, 650.0, m), rng.uniform(-60.0, 60.0, m)], 1)
    q = _dev(q)
    max_dist = PC.CLEAN_MAX_DIST_CELLS * cell
    _, d2 = PC.knn_distance(q, grid, 20, max_dist, return_d2=True)
    d = PC.nn_distance(q, grid, max_dist)
    capped = d2[:, 0] == max_dist * max_dist
    assert torch.equal(torch.where(capped, torch.full_like(d, max_dist), torch.sqrt(d2[:, 0])), d)
    assert torch.equal(capped, d == max_dist) and 0 < int(capped.sum()) < m
    assert bool((d2[:, 1:] >= d2[:, :-1]).all())
