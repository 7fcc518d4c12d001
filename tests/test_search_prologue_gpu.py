"""What the five query searches share before the walk (csrc/pc_grid.hpp: pc_query and the capacity dispatch), on one 130-point cloud:
query counts around the 64 lanes of a wave, taken through an order array, and the grid's own points in identity order; k on both
sides of every capacity of the k-best list.  pmn_nn_distance, pmn_knn_distance, pmn_radius_count, pmn_knn_normals and pmn_knn_mls
against the numpy models of knn_ref, cloud_normals_ref and mls_ref, bit for bit as their own tests compare; and the raw entries on
buffers 64 rows longer than the queries, of which no row past the last query may be written."""
import numpy as np
import pytest
import torch

import cloud_normals_ref as R
import knn_ref as K
import mls_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 63, 64, 65, 130)    # a lone lane, one short of a wave, a full wave, one lane into the second, two waves and two lanes
KS = (8, 9, 16, 17, 32)      # the last k of a capacity and the first of the next
REACH = 2.5                  # cuts some lists part way, and the far queries' altogether
PAD = 64
MLS_OUTPUTS = ("position", "normal", "displacement", "status", "count")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


@pytest.fixture(scope="module")
def case():
    """The cloud, its grid, 130 separate queries, and per same_cloud the reference's sorted rows and 32 nearest (ties in the grid's
    sorted order): computed once, read by every n and k -- the first n queries' rows are the first n rows."""
    from patchmatchnet_amd import pointcloud as PC
    pts = K.duplicate_cloud(130)
    query = K.far_queries(pts, n=130)
    assert len(pts) == 130 and len(query) == 130
    grid = PC.build_grid(_dev(pts), 0.9)
    pos = np.empty(len(pts), np.int64)
    pos[grid.perm.cpu().numpy()] = np.arange(len(pts))  # original index -> sorted position
    return {"points": pts, "query": query, "grid": grid,
            "rows": {same: K.sorted_d2(query, pts, same) for same in (False, True)},
            "idx": {same: R.neighbours(query, pts, 32, REACH, same, rank=pos) for same in (False, True)}}


def _calls(case):
    """(same_cloud, n, the queries on the host, the argument for the wrappers)"""
    for n in NS:
        yield False, n, case["query"][:n], _dev(case["query"][:n])
    yield True, len(case["points"]), case["points"], None


def test_nn_distance_and_radius_count(case):
    from patchmatchnet_amd import pointcloud as PC
    pts, grid = case["points"], case["grid"]
    cap = REACH * REACH
    for same, n, q, arg in _calls(case):
        got = PC.radius_count(arg, grid, REACH, same_cloud=same).cpu().numpy()
        assert got.shape == (n,) and np.array_equal(got, K.radius_count(q, pts, REACH, same)), (same, n)
        if same:
            continue  # pmn_nn_distance has no same_cloud: below, the grid's own points are ordinary queries, each its own nearest
        d2 = K.knn_d2(q, pts, 1, REACH, False, rows=case["rows"][False][:n])[:, 0]
        dist, idx = PC.nn_distance(arg, grid, REACH, return_index=True)
        dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
        assert np.array_equal(dist, np.where(d2 == cap, REACH, np.sqrt(d2))), n
        # the index: -1 exactly where capped, else a point at that distance (the first met wins among equals: any of them)
        assert np.array_equal(idx < 0, d2 == cap) and (idx[idx < 0] == -1).all(), n
        assert ((idx < 0).sum() > 0) == (n == 130), n  # the far queries are the last
        live = idx >= 0
        assert np.array_equal(K.pair_d2(q, pts)[np.flatnonzero(live), idx[live]], d2[live]), n
    own = PC.nn_distance(_dev(pts), grid, REACH).cpu().numpy()
    assert own.shape == (len(pts),) and not own.any()


@pytest.mark.parametrize("k", KS)
def test_knn_distance(case, k):
    from patchmatchnet_amd import pointcloud as PC
    pts, grid = case["points"], case["grid"]
    for same, n, q, arg in _calls(case):
        want = K.knn_d2(q, pts, k, REACH, same, rows=case["rows"][same][:n])
        mean, d2, idx = (t.cpu().numpy() for t in PC.knn_distance(arg, grid, k, REACH, same_cloud=same, return_d2=True,
                                                                  return_index=True))
        assert d2.shape == (n, k) and idx.shape == (n, k) and mean.shape == (n,)
        assert np.array_equal(d2, want) and np.array_equal(mean, K.knn_mean(want, REACH)), (same, n, k)
        assert np.array_equal(idx, case["idx"][same][:n, :k]), (same, n, k)


@pytest.mark.parametrize("k", KS)
def test_knn_normals(case, k):
    from patchmatchnet_amd import pointcloud as PC
    pts, grid = case["points"], case["grid"]
    for same, n, q, arg in _calls(case):
        ref = R.normals(q, pts, k, REACH, same, idx=case["idx"][same][:n])
        normal, variation, count = (t.cpu().numpy() for t in PC.knn_normals(arg, grid, k, REACH, same_cloud=same,
                                                                            return_variation=True, return_count=True))
        assert normal.shape == (n, 3) and normal.dtype == np.float32
        assert np.array_equal(count, ref["count"]) and np.array_equal(variation, ref["variation"]), (same, n, k)
        assert np.array_equal(normal, ref["normal"].astype(np.float32)), (same, n, k)


@pytest.mark.parametrize("k", KS)
def test_knn_mls(case, k):
    from patchmatchnet_amd import pointcloud as PC
    pts, grid = case["points"], case["grid"]
    for same, n, q, arg in _calls(case):
        for degree in (1, 2):
            ref = M.mls(q, pts, k, REACH, same, degree, idx=case["idx"][same][:n])
            got = PC.knn_mls(arg, grid, k, REACH, same_cloud=same, degree=degree, return_normal=True, return_displacement=True,
                             return_status=True, return_count=True)
            for name, t in zip(MLS_OUTPUTS, got):
                t = t.cpu().numpy()
                assert t.shape == ref[name].shape and np.array_equal(t, ref[name]), (same, n, k, degree, name)


def _padded(n, row, dtype, sentinel):
    return torch.full((n + PAD,) + row, sentinel, dtype=dtype, device=DEV)


def test_no_row_past_the_last_query_is_written(case):
    """The raw entries on outputs PAD rows longer than the queries and filled with a sentinel: rows [0, n) are what the wrapper
    returns (checked against the models above), every row from n on still holds the sentinel."""
    from patchmatchnet_amd import pointcloud as PC
    grid = case["grid"]
    L, a = PC._lib.lib(), PC._grid_args(grid)
    F64, F32, I32 = torch.float64, torch.float32, torch.int32
    for same, n, _, arg in _calls(case):
        query = grid.xyz if same else arg
        order = None if same else PC._cell_order(query, grid)
        head = a + (query.data_ptr(), order.data_ptr() if order is not None else None, n)
        s, stream = int(same), PC._stream(query)
        # entry -> (its padded outputs with their sentinels, the call, the wrapper's outputs in the same order)
        runs = {}
        o = [_padded(n, (), F64, -7.0), _padded(n, (), I32, -77)]
        # (pmn_nn_distance has no same_cloud: the grid's sorted points are then ordinary queries in identity order)
        runs["nn_distance"] = (o, lambda o: L.pmn_nn_distance(*head, REACH, o[0].data_ptr(), o[1].data_ptr(), stream),
                               (PC._unsort(PC.nn_distance(query, grid, REACH), grid, same), None))
        o = [_padded(n, (17,), F64, -7.0), _padded(n, (17,), I32, -77), _padded(n, (), F64, -7.0)]
        mean, d2 = PC.knn_distance(arg, grid, 17, REACH, same_cloud=same, return_d2=True)
        runs["knn_distance"] = (o, lambda o: L.pmn_knn_distance(*head, 17, REACH, s, *(t.data_ptr() for t in o), stream), (d2, None, mean))
        o = [_padded(n, (), I32, -77)]
        runs["radius_count"] = (o, lambda o: L.pmn_radius_count(*head, REACH, s, o[0].data_ptr(), stream),
                                (PC.radius_count(arg, grid, REACH, same_cloud=same),))
        o = [_padded(n, (3,), F32, -7.0), _padded(n, (), F64, -7.0), _padded(n, (), I32, -77)]
        runs["knn_normals"] = (o, lambda o: L.pmn_knn_normals(*head, 9, REACH, s, None, 0, 1e-6, *(t.data_ptr() for t in o), stream),
                               PC.knn_normals(arg, grid, 9, REACH, same_cloud=same, return_variation=True, return_count=True))
        o = [_padded(n, (3,), F32, -7.0), _padded(n, (3,), F32, -7.0), _padded(n, (), F64, -7.0), _padded(n, (), I32, -77),
             _padded(n, (), I32, -77)]
        runs["knn_mls"] = (o, lambda o: L.pmn_knn_mls(*head, 32, REACH, s, 2, 1e-6, *(t.data_ptr() for t in o), stream),
                           PC.knn_mls(arg, grid, 32, REACH, same_cloud=same, degree=2, return_normal=True, return_displacement=True,
                                      return_status=True, return_count=True))
        for entry, (outs, call, want) in runs.items():
            tag = (entry, same, n)
            assert call(outs) == 0, tag
            for j, t in enumerate(outs):
                sentinel = -77 if t.dtype == I32 else -7.0
                assert bool((t[n:] == sentinel).all()), tag + (j,)
                assert not bool((t[:n] == sentinel).any()), tag + (j,)
                if want[j] is not None:
                    assert torch.equal(PC._unsort(t[:n], grid, same), want[j]), tag + (j,)
