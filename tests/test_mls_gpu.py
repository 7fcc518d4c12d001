"""GPU checks of moving least squares (pmn_knn_mls, pointcloud.knn_mls / smooth_mls) against tests/mls_ref.py, the host model of the
kernel: the same float64 operations in the same order, so every output -- position, normal, displacement, status, count -- is
compared bit for bit; a difference is a contraction, an ordering bug or a wrong neighbour.  (That the model itself is right is
tests/test_mls_ref.py's business, on the CPU.)  The clouds are those of tests/test_cloud_normals_gpu.py with their cells and their
max_dist as the radius, plus the sphere at a radius of three spacings, where the quadric's step is taken: at a radius of 1000 its
second-order pivots fail and every point of the sphere ends on the plane."""
import numpy as np
import pytest
import torch

import cloud_normals_ref as R
import knn_ref as K
import mls_ref as M
from test_cloud_normals_gpu import _clouds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = (1, 2, 5, 8, 9, 16, 17, 32)  # every capacity (8, 16, 32) and its edge
BIG = 1000.0
OUTPUTS = ("position", "normal", "displacement", "status", "count")


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _sorted_pos(grid, n):
    pos = np.empty(n, np.int64)
    pos[grid.perm.cpu().numpy()] = np.arange(n)  # original index -> sorted position
    return pos


@pytest.fixture(scope="module")
def cases():
    """(name, same_cloud) -> dict(points, query, grid, radius, idx): the grid and the reference's 32 nearest, ties in the grid's sorted
    order, computed once and read by every k and degree."""
    from patchmatchnet_amd import pointcloud as PC
    clouds = dict(_clouds())
    clouds["sphere_near"] = (clouds["sphere"][0], 1.5, 3.0)
    out = {}
    for name, (pts, cell, radius) in clouds.items():
        grid = PC.build_grid(_dev(pts), cell)
        pos = _sorted_pos(grid, len(pts))
        for same in (True, False):
            query = None if same else K.far_queries(pts)
            out[name, same] = {"points": pts, "query": query, "grid": grid, "radius": radius,
                               "idx": R.neighbours(query, pts, 32, radius, same, rank=pos)}
    return out


def _run(PC, case, k, same, degree, **kw):
    got = PC.knn_mls(None if same else _dev(case["query"]), case["grid"], k, case["radius"], same_cloud=same, degree=degree,
                     return_normal=True, return_displacement=True, return_status=True, return_count=True, **kw)
    assert [t.dtype for t in got] == [torch.float32, torch.float32, torch.float64, torch.int32, torch.int32]
    return dict(zip(OUTPUTS, (t.cpu().numpy() for t in got)))


def _same(got, ref, tag):
    for name in OUTPUTS:
        assert got[name].shape == ref[name].shape and np.array_equal(got[name], ref[name]), (tag, name)
    stay = ref["status"] == 0
    assert not got["normal"][stay].any() and not got["displacement"][stay].any(), tag


@pytest.mark.parametrize("k", KS)
def test_mls_matches_the_model(cases, k):
    from patchmatchnet_amd import pointcloud as PC
    seen = {}
    for (name, same), case in cases.items():
        pts, query = case["points"], case["query"]
        q = pts if same else query
        for degree in (1, 2):
            tag = (name, same, k, degree)
            ref = M.mls(query, pts, k, case["radius"], same, degree, idx=case["idx"])
            got = _run(PC, case, k, same, degree)
            _same(got, ref, tag)
            stay = ref["status"] == 0
            assert np.array_equal(got["position"][stay].view(np.uint32), np.ascontiguousarray(q[stay]).view(np.uint32)), tag
            moved = ~stay
            if moved.any():
                assert np.abs(np.linalg.norm(got["normal"][moved].astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -22, tag
            # a call that asks for the position alone returns the same positions
            alone = PC.knn_mls(None if same else _dev(query), case["grid"], k, case["radius"], same_cloud=same, degree=degree)
            assert np.array_equal(alone.cpu().numpy(), got["position"]), tag
            seen[name, same, degree] = np.bincount(ref["status"], minlength=3)
    # the three outcomes occur where they must (they equal the model's above; these are the ones the model must have)
    for name in ("line", "one_point", "two_points"):
        for degree in (1, 2):
            assert seen[name, True, degree][0] == len(cases[name, True]["points"])
    assert seen["sheet", False, 2][0] >= 13                                  # far queries: nothing within the radius
    assert seen["sphere", True, 2][2] == 0                                   # the radius of 1000: the plane stands
    if k >= 2:
        assert seen["sphere", True, 1][1] == 1500
    if k >= 5:
        assert seen["sphere_near", True, 2][2] > 1000 and seen["sheet", True, 2][2] > 1000 and seen["lattice", True, 2][2] > 0
    else:
        assert all(seen[name, same, 2][2] == 0 for name, same, _ in seen)   # fewer than six members


def test_the_tail_of_a_wave():
    from patchmatchnet_amd import pointcloud as PC
    base = R.sphere_cloud(65, seed=8)[0]
    for n in (63, 64, 65):
        pts = base[:n]
        grid = PC.build_grid(_dev(pts), 5.0)
        case = {"points": pts, "query": None, "grid": grid, "radius": 12.0}
        for degree in (1, 2):
            ref = M.mls(None, pts, 8, 12.0, True, degree, rank=_sorted_pos(grid, n))
            _same(_run(PC, case, 8, True, degree), ref, (n, degree))
            assert (ref["status"] == degree).sum() > n // 2


@pytest.mark.parametrize("k", KS)
def test_cloud_of_k_plus_one_points(k):
    """k + 1 points: every list is exactly full under same_cloud; one point fewer and every list has a capped slot."""
    from patchmatchnet_amd import pointcloud as PC
    base = R.sphere_cloud(40, seed=9)[0]
    for n in (k, k + 1):
        pts = base[:n]
        grid = PC.build_grid(_dev(pts), 4.0)
        case = {"points": pts, "query": None, "grid": grid, "radius": 25.0}   # the sphere's diameter is 20: everything is in range
        for degree in (1, 2):
            ref = M.mls(None, pts, k, 25.0, True, degree, rank=_sorted_pos(grid, n))
            got = _run(PC, case, k, True, degree)
            assert (got["count"] == n - 1).all()
            _same(got, ref, (k, n, degree))
            assert (ref["status"] > 0).all() == (n >= 3)


def test_two_runs_and_any_order_give_the_same_bits(cases):
    """The result of a query does not depend on the run or on which lane of which wave computes it: `order` only assigns the lanes."""
    from patchmatchnet_amd import pointcloud as PC
    L = PC._lib.lib()
    rng = np.random.default_rng(12)
    for name in ("sheet", "sphere_near", "lattice"):
        for same in (True, False):
            case = cases[name, same]
            query = case["grid"].xyz if same else _dev(case["query"])
            n = int(query.shape[0])
            want = _run(PC, case, 16, same, 2)
            again = _run(PC, case, 16, same, 2)
            assert all(np.array_equal(want[o], again[o]) for o in OUTPUTS), name
            order = _dev(rng.permutation(n), np.int32)
            out = [torch.empty((n, 3), dtype=torch.float32, device=DEV), torch.empty((n, 3), dtype=torch.float32, device=DEV),
                   torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV),
                   torch.empty(n, dtype=torch.int32, device=DEV)]
            rc = L.pmn_knn_mls(*PC._grid_args(case["grid"]), query.data_ptr(), order.data_ptr(), n, 16, float(case["radius"]), int(same), 2,
                               1e-6, *(t.data_ptr() for t in out), None)
            assert rc == 0
            torch.cuda.synchronize()
            for o, t in zip(OUTPUTS, out):
                assert np.array_equal(PC._unsort(t, case["grid"], same).cpu().numpy(), want[o]), (name, same, o)


def test_smooth_mls_is_chained_knn_mls():
    from patchmatchnet_amd import pointcloud as PC
    pts = _dev(M.noisy_sphere()[0])
    for degree in (1, 2):
        got, normals, report = PC.smooth_mls(pts, radius=3.0, k=16, degree=degree, iterations=2, return_normals=True)
        first = PC.knn_mls(None, PC._clean_grid(pts, None), 16, 3.0, same_cloud=True, degree=degree)
        second, n2, status = PC.knn_mls(None, PC._clean_grid(first, None), 16, 3.0, same_cloud=True, degree=degree, return_normal=True,
                                        return_status=True)
        assert torch.equal(got, second) and torch.equal(normals, n2) and not torch.equal(first, second)
        assert report["status"] == torch.bincount(status.long(), minlength=3).cpu().tolist() and report["status"][degree] == 1500
        assert (report["radius"], report["k"], report["degree"], report["iterations"]) == (3.0, 16, degree, 2)
        moved = (second.double() - pts.double()).norm(dim=1)
        assert report["mean_displacement"] == float(moved.mean()) and report["max_displacement"] == float(moved.max())
        spacing = PC.cloud_spacing(pts)
        assert report["spacing"] == spacing and report["max_displacement_spacings"] == float(moved.max()) / spacing
    # the default radius is MLS_RADIUS_SPACINGS spacings of the input, and one iteration is one call
    got, report = PC.smooth_mls(pts)
    assert report["radius"] == PC.MLS_RADIUS_SPACINGS * PC.cloud_spacing(pts) and report["k"] == 32 and report["degree"] == 2
    assert torch.equal(got, PC.knn_mls(None, PC._clean_grid(pts, None), 32, report["radius"], same_cloud=True))
    assert PC.smooth_mls(pts, radius_spacings=2.0)[1]["radius"] == 2.0 * PC.cloud_spacing(pts)


def test_argument_checks():
    from patchmatchnet_amd import pointcloud as PC
    from patchmatchnet_amd._lib import PmnError
    pts = _dev(K.duplicate_cloud())
    grid = PC.build_grid(pts, 1.0)
    with pytest.raises(PmnError, match="no CPU fallback"):
        PC.knn_mls(pts.cpu(), grid, 4, 1.0)
    with pytest.raises(PmnError, match="no CPU fallback"):
        PC.smooth_mls(pts.cpu())
    with pytest.raises(PmnError, match="expected float32"):
        PC.knn_mls(pts.double(), grid, 4, 1.0)
    with pytest.raises(PmnError, match=r"contiguous \[n,3\]"):
        PC.knn_mls(pts[:, :2], grid, 4, 1.0)
    for k in (0, 33, 2.5, True):
        with pytest.raises(PmnError, match="k must be"):
            PC.knn_mls(pts, grid, k, 1.0)
    for bad in (float("inf"), float("nan"), 0.0, -1.0, 1e200, 1e-200):
        with pytest.raises(PmnError, match="radius"):
            PC.knn_mls(pts, grid, 4, bad)
    for bad in (0, 3, 1.5, True):
        with pytest.raises(PmnError, match="degree must be"):
            PC.knn_mls(pts, grid, 4, 1.0, degree=bad)
    for bad in (float("inf"), float("nan"), -1e-9):
        with pytest.raises(PmnError, match="line_ratio"):
            PC.knn_mls(pts, grid, 4, 1.0, line_ratio=bad)
    with pytest.raises(PmnError, match="same_cloud"):
        PC.knn_mls(pts, grid, 4, 1.0, same_cloud=True)
    with pytest.raises(PmnError, match="the grid on"):
        PC.knn_mls(pts, grid._replace(xyz=grid.xyz.cpu()), 4, 1.0)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(PmnError, match="iterations"):
            PC.smooth_mls(pts, iterations=bad)
    with pytest.raises(PmnError, match="cell must be"):
        PC.smooth_mls(pts, cell=0.0)
    with pytest.raises(PmnError, match="radius_spacings"):
        PC.smooth_mls(pts, radius_spacings=0.0)
    with pytest.raises(PmnError, match="give radius"):
        PC.smooth_mls(_dev(np.ones((1, 3))))  # a single point has no spacing
    # the entry point validates before launching
    L = PC._lib.lib()
    a = PC._grid_args(grid)
    n = len(pts)
    out = torch.zeros((n, 3), dtype=torch.float32, device=DEV)
    q, o = pts.data_ptr(), out.data_ptr()
    tail = (None, None, None, None, None)
    assert L.pmn_knn_mls(*a, q, None, n, 4, 1.0, 0, 2, 1e-6, None, *tail) == -1       # no position
    assert L.pmn_knn_mls(*a, None, None, n, 4, 1.0, 0, 2, 1e-6, o, *tail) == -1       # no query
    assert L.pmn_knn_mls(None, *a[1:], q, None, n, 4, 1.0, 0, 2, 1e-6, o, *tail) == -1
    assert L.pmn_knn_mls(*a, q, None, 0, 4, 1.0, 0, 2, 1e-6, o, *tail) == -1
    assert L.pmn_knn_mls(*a, q, None, n, 0, 1.0, 0, 2, 1e-6, o, *tail) == -1
    assert L.pmn_knn_mls(*a, q, None, n, 33, 1.0, 0, 2, 1e-6, o, *tail) == -1
    assert L.pmn_knn_mls(*a, q, None, n, 4, float("inf"), 0, 2, 1e-6, o, *tail) == -1
    assert L.pmn_knn_mls(*a, q, None, n, 4, float("nan"), 0, 2, 1e-6, o, *tail) == -1
    assert L.pmn_knn_mls(*a, q, None, n, 4, 0.0, 0, 2, 1e-6, o, *tail) == -1
    assert L.pmn_knn_mls(*a, q, None, n, 4, -1.0, 0, 2, 1e-6, o, *tail) == -1
    assert L.pmn_knn_mls(*a, q, None, n, 4, 1e200, 0, 2, 1e-6, o, *tail) == -1        # the square is not finite
    assert L.pmn_knn_mls(*a, q, None, n, 4, 1e-200, 0, 2, 1e-6, o, *tail) == -1       # the square is 0
    assert L.pmn_knn_mls(*a, q, None, n - 1, 4, 1.0, 1, 2, 1e-6, o, *tail) == -1      # same_cloud, n_from != n_to
    assert L.pmn_knn_mls(*a, q, None, n, 4, 1.0, 0, 0, 1e-6, o, *tail) == -1          # degree
    assert L.pmn_knn_mls(*a, q, None, n, 4, 1.0, 0, 3, 1e-6, o, *tail) == -1
    assert L.pmn_knn_mls(*a, q, None, n, 4, 1.0, 0, 2, -1.0, o, *tail) == -1
    assert L.pmn_knn_mls(*a, q, None, n, 4, 1.0, 0, 2, float("nan"), o, *tail) == -1
    assert L.pmn_knn_mls(*a, q, None, n, 4, 1.0, 0, 2, float("inf"), o, *tail) == -1
    torch.cuda.synchronize()
    assert not out.any()  # nothing was launched
