"""The scalar checks of the cloud functions of patchmatchnet_amd/pointcloud.py, message for message, without a device: every call
below fails in a check that comes before the first launch, so host tensors stand in for the grid and the points.  Where a function
looks at its tensors first, the message pinned is that of the device check (no CPU fallback), which is then what a bad setting
meets.  The WHOLE string is compared: the texts, their "function: " prefix and the order in which a function's checks fire are part
of the interface.

One case has two accepted outcomes.  A reach whose square overflows (1e200) is refused with the function's reach message wherever the
square is formed as a product; knn_distance, knn_normals and radius_count formed it as float ** 2, which raises OverflowError before
the message is reached.  Either the message in full or that OverflowError passes; nothing else does."""
import numpy as np
import pytest
import torch

from patchmatchnet_amd import pointcloud as PC
from patchmatchnet_amd._lib import PmnError

INF, NAN = float("inf"), float("nan")
ON_CPU = "tensor is on cpu; patchmatchnet_amd runs only on a ROCm GPU (no CPU fallback)"
SAME = "same_cloud=True queries the grid's own points; pass query=None"
BAD_K = (0, 33, 2.5, True)
BAD_REACH = (0.0, -1.0, INF, NAN)  # 1e200, whose square overflows, has cases of its own


def _host_cloud(n=12):
    return torch.from_numpy(np.random.default_rng(0).uniform(0.0, 4.0, (n, 3)).astype(np.float32))


@pytest.fixture(scope="module")
def pts():
    return _host_cloud()


@pytest.fixture(scope="module")
def grid(pts):
    """A stand-in Grid of host tensors: what _sort_into_grid gives for host points."""
    g = PC._sort_into_grid(pts, 1.0)
    assert not g.xyz.is_cuda
    return g


def _raises(message, fn, *args, **kw):
    with pytest.raises(PmnError) as e:
        fn(*args, **kw)
    assert str(e.value) == message


def _raises_or_overflows(message, fn, *args, **kw):
    with pytest.raises((PmnError, OverflowError)) as e:
        fn(*args, **kw)
    if isinstance(e.value, PmnError):
        assert str(e.value) == message


def test_knn_distance(pts, grid):
    for k in BAD_K:
        _raises(f"knn_distance: k must be an integer in 1..32, got {k!r}", PC.knn_distance, pts, grid, k, 1.0)
        _raises(f"knn_distance: k must be an integer in 1..32, got {k!r}", PC.knn_distance, None, grid, k, NAN, same_cloud=True)  # k first
    for v in BAD_REACH:
        _raises(f"knn_distance: max_dist must be positive and finite, got {v}", PC.knn_distance, pts, grid, 4, v)
    _raises_or_overflows("knn_distance: max_dist must be positive and finite, got 1e+200", PC.knn_distance, pts, grid, 4, 1e200)
    _raises(f"knn_distance: {SAME}", PC.knn_distance, pts, grid, 4, 1.0, same_cloud=True)
    _raises(f"query: {ON_CPU}", PC.knn_distance, pts, grid, 4, 1.0)
    _raises(f"query: {ON_CPU}", PC.knn_distance, pts, grid, np.int64(32), 1e-200)  # a square that underflows is no error here


def test_radius_count(pts, grid):
    for v in (-1.0, INF, NAN):
        _raises(f"radius_count: radius must be finite and >= 0, got {v}", PC.radius_count, pts, grid, v)
    _raises_or_overflows("radius_count: radius must be finite and >= 0, got 1e+200", PC.radius_count, pts, grid, 1e200)
    _raises(f"radius_count: {SAME}", PC.radius_count, pts, grid, 1.0, same_cloud=True)
    _raises(f"query: {ON_CPU}", PC.radius_count, pts, grid, 0.0)  # 0 is a radius


def test_knn_normals(pts, grid):
    for k in BAD_K:
        _raises(f"knn_normals: k must be an integer in 1..32, got {k!r}", PC.knn_normals, pts, grid, k, 1.0)
    for v in BAD_REACH:
        _raises(f"knn_normals: max_dist must be positive and finite, got {v}", PC.knn_normals, pts, grid, 4, v)
        _raises(f"knn_normals: max_dist must be positive and finite, got {v}", PC.knn_normals, pts, grid, 4, v, line_ratio=-1.0)
    _raises_or_overflows("knn_normals: max_dist must be positive and finite, got 1e+200", PC.knn_normals, pts, grid, 4, 1e200)
    for v in (-1e-6, INF, NAN):
        _raises(f"knn_normals: line_ratio must be finite and >= 0, got {v}", PC.knn_normals, pts, grid, 4, 1.0, line_ratio=v)
    _raises(f"knn_normals: {SAME}", PC.knn_normals, pts, grid, 4, 1.0, same_cloud=True)
    _raises(f"query: {ON_CPU}", PC.knn_normals, pts, grid, 4, 1.0, viewpoints=[[0.0, 0.0, NAN]])  # viewpoints come after the query


def test_knn_mls(pts, grid):
    for k in BAD_K:
        _raises(f"knn_mls: k must be an integer in 1..32, got {k!r}", PC.knn_mls, pts, grid, k, 1.0)
    for v in BAD_REACH + (1e200, 1e-200):
        _raises(f"knn_mls: radius and its square must be positive and finite, got {v}", PC.knn_mls, pts, grid, 4, v)
        _raises(f"knn_mls: radius and its square must be positive and finite, got {v}", PC.knn_mls, pts, grid, 4, v, degree=3)
    for d in (3, 0, 2.0, True):
        _raises(f"knn_mls: degree must be 1 or 2, got {d!r}", PC.knn_mls, pts, grid, 4, 1.0, degree=d)
        _raises(f"knn_mls: degree must be 1 or 2, got {d!r}", PC.knn_mls, pts, grid, 4, 1.0, degree=d, line_ratio=-1.0)
    for v in (-1e-6, INF, NAN):
        _raises(f"knn_mls: line_ratio must be finite and >= 0, got {v}", PC.knn_mls, pts, grid, 4, 1.0, line_ratio=v)
    _raises(f"knn_mls: {SAME}", PC.knn_mls, pts, grid, 4, 1.0, same_cloud=True)
    _raises(f"query: {ON_CPU}", PC.knn_mls, pts, grid, 4, 1.0, degree=1)


def _host_volume():
    """A SparseTsdfVolume that counts as allocated, of host tensors: cloud_sdf reads blocks, tsdf and rgb before its device check."""
    from patchmatchnet_amd.tsdf import SparseTsdfVolume
    v = object.__new__(SparseTsdfVolume)
    v.blocks = torch.zeros(1, dtype=torch.int32)
    v.tsdf = torch.ones((1, 8, 8, 8), dtype=torch.float32)
    v.rgb = None
    return v


def test_cloud_sdf(pts, grid):
    vol, nrm = _host_volume(), torch.zeros_like(pts)
    _raises("cloud_sdf: volume must be a tsdf.SparseTsdfVolume", PC.cloud_sdf, None, grid, nrm, k=0)
    for k in BAD_K:
        _raises(f"cloud_sdf: k must be an integer in 1..32, got {k!r}", PC.cloud_sdf, vol, grid, nrm, k=k, radius=NAN)
    for v in BAD_REACH + (1e200, 1e-200):
        _raises(f"cloud_sdf: radius and its square must be positive and finite, got {v}", PC.cloud_sdf, vol, grid, nrm, radius=v,
                boundary=1.0)
        _raises(f"cloud_sdf: boundary and its square must be positive and finite, got {v}", PC.cloud_sdf, vol, grid, nrm, radius=1.0,
                boundary=v)
    _raises("cloud_sdf: radius and its square must be positive and finite, got -2.0", PC.cloud_sdf, vol, grid, nrm, radius=-2, boundary=0)
    _raises("cloud_sdf: the grid is on cpu, the volume on cpu (no CPU fallback)", PC.cloud_sdf, vol, grid, nrm)


def test_functions_that_look_at_their_points_first(pts, grid):
    """mesh_from_cloud, cluster_dbscan, radius_outliers and smooth_mls check the points' device before any setting."""
    nrm = torch.zeros_like(pts)
    for k in BAD_K:
        _raises(f"points: {ON_CPU}", PC.mesh_from_cloud, pts, nrm, k=k)
    _raises(f"points: {ON_CPU}", PC.mesh_from_cloud, pts, nrm, radius=-1.0)
    for m in (2.5, True, 0):
        _raises(f"points: {ON_CPU}", PC.cluster_dbscan, pts, 0.5, m)
    for v in BAD_REACH[1:] + (1e200,):
        _raises(f"points: {ON_CPU}", PC.cluster_dbscan, pts, v, 4)
        _raises(f"points: {ON_CPU}", PC.radius_outliers, pts, v, 2)
    _raises(f"points: {ON_CPU}", PC.radius_outliers, pts, 1.0, 2.5)
    for v in BAD_REACH + (1e200,):
        _raises(f"points: {ON_CPU}", PC.smooth_mls, pts, radius=v)
    _raises(f"points: {ON_CPU}", PC.smooth_mls, pts, radius=1.0, k=33, degree=3, iterations=0)


def test_segment_planes(pts):
    for name, lo, bad in (("hypotheses", 1, (0, 2.5, True)), ("seed", 0, (-1, 1.5, False)), ("refine", 0, (-1, 0.5, True))):
        for v in bad:
            _raises(f"segment_planes: {name} must be an integer >= {lo}, got {v!r}", PC.segment_planes, pts, 0.1, **{name: v})
            _raises(f"segment_plane: {name} must be an integer >= {lo}, got {v!r}", PC.segment_plane, pts, 0.1, **{name: v})
    _raises("segment_planes: hypotheses must be an integer >= 1, got 0", PC.segment_planes, pts, 0.1, hypotheses=0, seed=-1, max_planes=0)
    for name in ("max_planes", "min_inliers"):
        for v in (0, 2.5, True):
            _raises(f"segment_planes: {name} must be an integer >= 1, got {v!r}", PC.segment_planes, pts, 0.1, **{name: v})
    _raises("segment_planes: max_planes must be an integer >= 1, got 0", PC.segment_planes, pts, 0.1, max_planes=0, min_inliers=0)
    _raises("segment_planes: normal_angle must lie in [0, 90] degrees, got 91", PC.segment_planes, pts, 0.1, normal_angle=91)
    _raises("segment_planes: normal_angle needs normals", PC.segment_planes, pts, 0.1, normal_angle=30.0)
    _raises(f"points: {ON_CPU}", PC.segment_planes, pts, 0.1)
    _raises(f"points: {ON_CPU}", PC.segment_planes, pts, -1.0)  # the threshold is checked with the points
    _raises(f"points: {ON_CPU}", PC.segment_planes, pts)        # no threshold: the spacing of the points is asked for first


def test_select_clusters():
    labels, sizes = torch.zeros(5, dtype=torch.int64), torch.tensor([5])
    for name in ("min_cluster_points", "keep_largest"):
        for v in (-1, 2.5, True):
            _raises(f"select_clusters: {name} must be an integer >= 0, got {v!r}", PC.select_clusters, labels, sizes, **{name: v})
    _raises("select_clusters: min_cluster_points must be an integer >= 0, got -1", PC.select_clusters, labels, sizes, -1, -1)
    _raises("select_clusters: labels: expected a 1-D int64 tensor on a ROCm GPU (no CPU fallback)", PC.select_clusters, labels, sizes)
    _raises("select_clusters: labels: expected a 1-D int64 tensor on a ROCm GPU (no CPU fallback)", PC.select_clusters, labels, sizes, 3, 2)
