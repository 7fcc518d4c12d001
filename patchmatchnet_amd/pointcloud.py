"""DTU accuracy / completeness of a fused point cloud on the device (reference evaluations/dtu/BaseEvalMain_web.m,
PointCompareMain.m, MaxDistCP.m, reducePts_haa.m, ComputeStat_web.m -- MATLAB with CPU KD-trees).

The two searches are HIP kernels (csrc/pointcloud.hip): pmn_reduce_round, the greedy 0.2-unit reduction of the method's cloud, and
pmn_nn_distance, the nearest-neighbour distance in both directions.  Both read a uniform grid over sorted points; building it is
plumbing and uses torch on the device (cell coordinates -> 63-bit key -> torch.sort), as are the masks and the statistics (a gather
from the ObsMask volume, a dot product, boolean selects, one sort for the median, float64 sums: a few elementwise launches per scan).
There is no CPU path: the searches refuse host tensors.  The clouds come from ply.read_ply_vertices.

The same grid serves cloud cleaning (clean_cloud.py): pmn_knn_distance and pmn_radius_count are the k nearest
neighbours and the number of points within a radius, and statistical_outliers / radius_outliers the two filters built on them.
cluster_dbscan (cluster_cloud.py) takes a cloud apart into its dense pieces over the same grid: pmn_cloud_core and
pmn_cloud_dbscan (csrc/cloud_cluster.hip).  segment_plane / segment_planes (segment_cloud.py) find the dominant planes
by seeded RANSAC: pmn_plane_score and pmn_plane_inliers (csrc/cloud_plane.hip) need no grid.  knn_mls / smooth_mls (smooth_cloud.py,
DESIGN.md 36) move every point onto a surface fitted to its neighbourhood, moving least squares: pmn_knn_mls (csrc/cloud_mls.hip).

Semantics: every distance is sqrt(dx*dx + dy*dy + dz*dz) of the float32 PLY coordinates widened to float64; the visiting
order of the reduction is an explicit, seeded permutation (the MATLAB draws an unseeded randperm), and for a given order the result is
the sequential greedy set exactly; nn_distance returns min(d, max_dist) where MaxDistCP.m returns some value >= MaxDist (the one stated
deviation: every consumer keeps only distances < 20).
"""
from __future__ import annotations

import ctypes
import os
import time
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import PmnError, check
from .ply import read_ply_vertices  # noqa: F401  (the clouds and meshes that are scored)

# defaults chosen from the sweep recorded in DESIGN.md 13
NN_CELL = 2.0          # cell of the nearest-neighbour grids, in scene units (DTU: millimetres)
REDUCE_CELL_RATIO = 2  # cell of the reduction's grid = REDUCE_CELL_RATIO * dst
ROUNDS_PER_READ = 4    # rounds of the reduction enqueued between two reads of the undecided counters
# defaults of the cleaning filters, chosen from the sweep recorded in DESIGN.md 23 (profiles/clean_cloud_measure.log)
CLEAN_CELL_POINTS = 8.0      # default_cell: mean number of points per occupied cell at which the doubling stops
CLEAN_MAX_DIST_CELLS = 16.0  # default max_dist of statistical_outliers, in cells


# ---- mask files ---------------------------------------------------------------------------------------------------------------

def _load_fields(path: str, fields) -> Dict[str, np.ndarray]:
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    if path.endswith(".npz"):
        with np.load(path) as z:
            missing = [k for k in fields if k not in z.files]
            if missing:
                raise ValueError(f"{path}: no field {missing[0]!r}")
            return {k: z[k] for k in fields}
    try:
        import scipy.io
    except ImportError as e:
        raise PmnError(f"{path}: reading .mat files needs scipy (scipy.io.loadmat); convert the file to .npz with the same field "
                       f"names ({', '.join(fields)}) to do without it") from e
    m = scipy.io.loadmat(path, variable_names=list(fields))
    missing = [k for k in fields if k not in m]
    if missing:
        raise ValueError(f"{path}: no field {missing[0]!r}")
    return {k: m[k] for k in fields}


def load_obs_mask(path: str) -> Tuple[np.ndarray, np.ndarray, float]:
    """ObsMask/ObsMask<scan>_10.mat (or an .npz with the same field names) -> (ObsMask bool [s1,s2,s3], BB float64 [2,3], Res)."""
    m = _load_fields(path, ("ObsMask", "BB", "Res"))
    obs = np.asarray(m["ObsMask"]).astype(bool)
    bb = np.asarray(m["BB"], np.float64)
    if obs.ndim != 3 or bb.shape != (2, 3):
        raise ValueError(f"{path}: ObsMask must be 3-D and BB 2x3, got {obs.shape} and {bb.shape}")
    return obs, bb, float(np.asarray(m["Res"], np.float64).reshape(-1)[0])


def load_plane(path: str) -> np.ndarray:
    """ObsMask/Plane<scan>.mat (or .npz): P, the 4 plane coefficients, float64 [4]."""
    p = np.asarray(_load_fields(path, ("P",))["P"], np.float64).reshape(-1)
    if p.shape != (4,):
        raise ValueError(f"{path}: P must have 4 entries, got {p.shape}")
    return p


# ---- grid -----------------------------------------------------------------------------------------------------------------------

class Grid(NamedTuple):
    """Uniform grid over sorted points (layout: include/pmn_hip.h, ABI 25)."""
    xyz: torch.Tensor     # [n,3] float32, ascending key order
    keys: torch.Tensor    # [n] int64
    perm: torch.Tensor    # [n] int64: xyz == points[perm]
    origin: Tuple[float, float, float]
    cell: float
    dims: Tuple[int, int, int]


def _points(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise PmnError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise PmnError(f"{name}: tensor is on {t.device}; patchmatchnet_amd runs only on a ROCm GPU (no CPU fallback)")
    if t.dtype != torch.float32:
        raise PmnError(f"{name}: expected float32, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
        raise PmnError(f"{name}: expected a contiguous [n,3] tensor, got {tuple(t.shape)}")
    if t.shape[0] < 1 or t.shape[0] >= 2 ** 31 - 64:
        raise PmnError(f"{name}: between 1 and 2^31 - 65 points, got {t.shape[0]}")
    bad = int((~torch.isfinite(t)).any(1).sum())
    if bad:
        raise PmnError(f"{name}: {bad} points have non-finite coordinates")
    return t


def _cells(points: torch.Tensor, origin, cell: float) -> torch.Tensor:
    """floor((double(p) - origin) / cell), int64 [n,3]: the expression of the kernels (csrc/pointcloud.hip pc_cell)."""
    o = torch.tensor(origin, dtype=torch.float64, device=points.device)
    return torch.floor((points.double() - o) / cell).clamp_(-2.0 ** 30, 2.0 ** 30).long()


def _keys(points: torch.Tensor, origin, cell: float):
    """(keys int64 [n], dims): the key (c.z * dims.y + c.y) * dims.x + c.x of every point's cell and the cells per axis."""
    c = _cells(points, origin, cell)
    dims = (c.max(0).values + 1).cpu().tolist()
    return (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0], dims


def build_grid(points: torch.Tensor, cell: float, origin=None) -> Grid:
    """Sorts ``points`` ([n,3] float32 on the device) into the cells of a uniform grid of side ``cell`` whose corner is ``origin``
    (default: the per-axis minimum of the points; a given origin must not exceed it)."""
    return _sort_into_grid(_points(points, "points"), cell, origin)


def _sort_into_grid(points: torch.Tensor, cell: float, origin=None, what: str = "build_grid") -> Grid:
    """build_grid without the device check: meshops.build_face_grid also sorts host tensors (its cover property is tested there).
    ``what`` names the caller in the errors."""
    cell = float(cell)
    if not (cell > 0.0 and np.isfinite(cell)):
        raise PmnError(f"{what}: cell must be positive and finite, got {cell}")
    lo = points.min(0).values.double().cpu().numpy()
    origin = lo if origin is None else np.asarray(origin, np.float64).reshape(3)
    if not np.isfinite(origin).all() or (origin > lo).any():
        raise PmnError(f"{what}: origin {origin.tolist()} must be finite and not above the points' minimum {lo.tolist()}")
    keys, dims = _keys(points, origin.tolist(), cell)
    if max(dims) > 2 ** 30 or dims[0] * dims[1] * dims[2] >= 2 ** 62:
        raise PmnError(f"{what}: a grid of {dims} cells does not fit a 63-bit key (PMN_ERR_SHAPE); use a larger cell")
    keys, perm = torch.sort(keys)
    return Grid(points[perm].contiguous(), keys, perm, tuple(float(v) for v in origin), cell, tuple(int(d) for d in dims))


def _grid_args(g: Grid):
    return (g.xyz.data_ptr(), g.keys.data_ptr(), int(g.xyz.shape[0]), (ctypes.c_double * 3)(*g.origin), float(g.cell),
            (ctypes.c_int * 3)(*g.dims))


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def nn_distance(query: torch.Tensor, grid: Grid, max_dist: float, return_index: bool = False):
    """pmn_nn_distance: float64 [n] distance from every query point to the nearest point of ``grid``, capped at ``max_dist``.
    ``return_index``: also int64 [n], the index into the points ``grid`` was built from (-1 where the result is the cap)."""
    query = _points(query, "query")
    if query.device != grid.xyz.device:
        raise PmnError(f"nn_distance: query is on {query.device}, the grid on {grid.xyz.device}")
    if not (max_dist > 0.0 and np.isfinite(max_dist)):
        raise PmnError(f"nn_distance: max_dist must be positive and finite, got {max_dist}")
    n = int(query.shape[0])
    order = _cell_order(query, grid)
    dist = torch.empty(n, dtype=torch.float64, device=query.device)
    index = torch.empty(n, dtype=torch.int32, device=query.device) if return_index else None
    with torch.cuda.device(query.device):
        check(_lib.lib().pmn_nn_distance(*_grid_args(grid), query.data_ptr(), order.data_ptr(), n, float(max_dist), dist.data_ptr(),
                                         index.data_ptr() if return_index else None, _stream(query)), "pmn_nn_distance")
    if not return_index:
        return dist
    idx = index.long()
    return dist, torch.where(idx >= 0, grid.perm[idx.clamp_min(0)], idx)


def _cell_order(query: torch.Tensor, grid: Grid) -> torch.Tensor:
    """int32 [n]: the queries in the order of their own cells (the lanes of a wave then walk the same cells)."""
    qc = _cells(query, grid.origin, grid.cell).clamp_(-1, max(grid.dims))
    side = max(grid.dims) + 2
    return torch.argsort(((qc[:, 2] + 1) * side + (qc[:, 1] + 1)) * side + (qc[:, 0] + 1)).int()


def _search_query(what: str, query: Optional[torch.Tensor], grid: Grid, same_cloud: bool):
    """(query tensor, order or None) of a k-nearest / radius search.  ``same_cloud``: the grid's own sorted points in identity order
    (they ARE in cell order), so that query i is grid point i as the kernels' flag states."""
    if same_cloud:
        if query is not None:
            raise PmnError(f"{what}: same_cloud=True queries the grid's own points; pass query=None")
        return grid.xyz, None
    query = _points(query, "query")
    if query.device != grid.xyz.device:
        raise PmnError(f"{what}: query is on {query.device}, the grid on {grid.xyz.device}")
    return query, _cell_order(query, grid)


def _unsort(t: torch.Tensor, grid: Grid, same_cloud: bool) -> torch.Tensor:
    """Rows of a same_cloud result (grid-sorted) back in the order of the points the grid was built from."""
    if not same_cloud:
        return t
    out = torch.empty_like(t)
    out[grid.perm] = t
    return out


def _check_int(what: str, name: str, v, lo: int) -> None:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
        raise PmnError(f"{what}: {name} must be an integer >= {lo}, got {v!r}")


def _check_k(what: str, k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 32:
        raise PmnError(f"{what}: k must be an integer in 1..32, got {k!r}")
    return int(k)


def _check_reach(what: str, name: str, v, positive_square: bool = False) -> None:
    """The cap of a k-nearest search.  The kernels compare squares, and where they divide by the cap's it must not have underflowed."""
    square = float(v) * float(v)  # (** raises OverflowError where the product is infinite)
    if not (v > 0.0 and np.isfinite(v) and np.isfinite(square) and (square > 0.0 or not positive_square)):
        raise PmnError(f"{what}: {name} {'and its square must be' if positive_square else 'must be'} positive and finite, got {v}")


def _query_search(entry: str, grid: Grid, query: Optional[torch.Tensor], same_cloud: bool, scalars, outputs) -> list:
    """The C entry ``entry`` ("pmn_" + the public function's name) on the checked query: ``scalars`` are its arguments between n_from
    and the outputs (a tensor goes as its pointer), or a function of the query's device that returns them; ``outputs`` its outputs as
    (shape of a row, dtype, wanted).  Returns the wanted ones, rows in the caller's order; the others are passed as null."""
    query, order = _search_query(entry[4:], query, grid, same_cloud)
    n, dev = int(query.shape[0]), query.device
    args = scalars(dev) if callable(scalars) else scalars
    outs = [torch.empty((n,) + shape, dtype=dtype, device=dev) if wanted else None for shape, dtype, wanted in outputs]
    with torch.cuda.device(dev):
        check(getattr(_lib.lib(), entry)(*_grid_args(grid), query.data_ptr(), order.data_ptr() if order is not None else None, n,
                                         *(a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args),
                                         *(t.data_ptr() if t is not None else None for t in outs), _stream(query)), entry)
    return [_unsort(t, grid, same_cloud) for t in outs if t is not None]


def _one_or_tuple(out: list):
    return out[0] if len(out) == 1 else tuple(out)


def knn_distance(query: Optional[torch.Tensor], grid: Grid, k: int, max_dist: float, same_cloud: bool = False,
                 return_d2: bool = False, return_index: bool = False):
    """pmn_knn_distance: float64 [n], the mean distance from every query point to its ``k`` (1..32) nearest points of ``grid``; a
    neighbour slot for which no point lies nearer than ``max_dist`` counts as ``max_dist`` (pmn_nn_distance's cap).
    ``return_d2``: also float64 [n,k], the squared distances ascending (max_dist * max_dist in a capped slot); ``return_index``: also
    int64 [n,k], indices into the points ``grid`` was built from (-1 in a capped slot; ties at equal d2 go to the point that comes
    first in the grid's sorted order).  The lists cost 8 k n and 4 k n bytes: the cleaning filters ask for the mean alone.
    ``same_cloud``: the queries are the grid's own points (``query`` must be None); a point is never its own neighbour (excluded by
    index: an exact duplicate at distance 0 is a neighbour), and row i of every result belongs to point i of the original cloud."""
    k = _check_k("knn_distance", k)
    _check_reach("knn_distance", "max_dist", max_dist)
    out = _query_search("pmn_knn_distance", grid, query, same_cloud, (k, float(max_dist), int(bool(same_cloud))),
                        [((k,), torch.float64, return_d2), ((k,), torch.int32, return_index), ((), torch.float64, True)])
    if return_index:  # sorted positions -> indices into the points the grid was built from
        idx = out[-2].long()
        out[-2] = torch.where(idx >= 0, grid.perm[idx.clamp_min(0)], idx)
    return _one_or_tuple(out[-1:] + out[:-1])  # the mean comes first


def radius_count(query: Optional[torch.Tensor], grid: Grid, radius: float, same_cloud: bool = False) -> torch.Tensor:
    """pmn_radius_count: int32 [n], the number of points of ``grid`` within ``radius`` of every query point (sqrt(d2) <= radius on
    the float64 distance).  ``same_cloud``: as knn_distance; the point itself is not counted."""
    if not (radius >= 0.0 and np.isfinite(radius) and np.isfinite(float(radius) ** 2)):
        raise PmnError(f"radius_count: radius must be finite and >= 0, got {radius}")
    return _query_search("pmn_radius_count", grid, query, same_cloud, (float(radius), int(bool(same_cloud))),
                         [((), torch.int32, True)])[0]


def default_cell(points: torch.Tensor, target: float = CLEAN_CELL_POINTS) -> float:
    """The cell of a cleaning grid: doubled from a small start until the occupied cells hold ``target`` points on average (occupied
    cells counted with torch.unique on the keys).  Only the time of a search depends on it, never its result."""
    points = _points(points, "points")
    n = int(points.shape[0])
    lo = points.min(0).values.double()
    extent = float((points.max(0).values.double() - lo).max())
    if not extent > 0.0:
        return 1.0
    # no arrangement of n points over this extent (not even a line) reaches the target below extent * target / n; 2^-20 of the extent
    # keeps the key inside 63 bits
    cell = extent * max(min(target / n, 1.0) / 2.0, 2.0 ** -20)
    origin = lo.cpu().tolist()
    while cell < extent:
        if n / int(torch.unique(_keys(points, origin, cell)[0]).numel()) >= target:
            break
        cell *= 2.0
    return cell


def _clean_grid(points: torch.Tensor, cell: Optional[float]) -> Grid:
    return build_grid(points, default_cell(points) if cell is None else cell)


def statistical_outliers(points: torch.Tensor, k: int = 20, std_ratio: float = 2.0, max_dist: Optional[float] = None,
                         cell: Optional[float] = None):
    """Statistical outlier removal (PCL StatisticalOutlierRemoval, Open3D remove_statistical_outlier) on the device:
    (keep bool [n], mean float64 [n], threshold float).  mean[i] is the mean distance from point i to its ``k`` nearest other points
    (knn_distance, same_cloud); threshold = mu + std_ratio * sigma over the n means, sigma with n - 1 in the denominator as in both
    libraries (0 for a single point), float64 on the device; keep = mean <= threshold.  That is PCL's rule; Open3D keeps mean <
    threshold, which differs only for a mean exactly on the threshold.
    Deviation: the search is capped at ``max_dist`` (default CLEAN_MAX_DIST_CELLS cells) so that a far outlier does not walk empty
    shells for ever.  A point with fewer than k neighbours inside max_dist -- or a cloud of fewer than k + 1 points, where PCL and
    Open3D average what there is -- has capped slots that count as max_dist each: its mean is a lower bound of the true one, still
    far above any surface point's.  ``cell`` (default: default_cell) changes the time only."""
    points = _points(points, "points")
    if not np.isfinite(std_ratio):
        raise PmnError(f"statistical_outliers: std_ratio must be finite, got {std_ratio}")
    grid = _clean_grid(points, cell)
    if max_dist is None:
        max_dist = CLEAN_MAX_DIST_CELLS * grid.cell
    mean = knn_distance(None, grid, k, max_dist, same_cloud=True)
    sigma = mean.std(unbiased=True) if mean.numel() > 1 else mean.new_zeros(())
    threshold = float(mean.mean() + float(std_ratio) * sigma)
    return mean <= threshold, mean, threshold


def radius_outliers(points: torch.Tensor, radius: float, min_neighbors: int, cell: Optional[float] = None):
    """Radius outlier removal (PCL RadiusOutlierRemoval, Open3D remove_radius_outlier) on the device: (keep bool [n], count int32
    [n]); count[i] is the number of OTHER points within ``radius`` (<=) of point i and keep = count >= min_neighbors.  ``cell``
    (default: default_cell, but not below radius / 8 so that the walk stays within a few shells) changes the time only."""
    points = _points(points, "points")
    _check_int("radius_outliers", "min_neighbors", min_neighbors, 0)
    if not (radius >= 0.0 and np.isfinite(radius)):
        raise PmnError(f"radius_outliers: radius must be finite and >= 0, got {radius}")
    if cell is None:
        cell = max(default_cell(points), float(radius) / 8.0)
    count = radius_count(None, build_grid(points, cell), radius, same_cloud=True)
    return count >= int(min_neighbors), count


# ---- density clustering ------------------------------------------------------------------------------------------------

def cluster_dbscan(points: torch.Tensor, eps: float, min_points: int, cell: Optional[float] = None):
    """DBSCAN on the device with an order-free border rule (pmn_cloud_core, pmn_cloud_dbscan): (labels int64 [n] in the
    order of ``points``, core bool [n], sizes int64 [C]).  Distances are radius_count's: "within eps" is sqrt(d2) <= eps on the float64
    distance of the float32 coordinates.
    Core: a point with at least ``min_points`` points within ``eps`` of it, itself included (sklearn's and Open3D's rule).  Cluster: a
    connected component of the core points under "within eps".  Border: a point that is not core but has a core point within eps; it
    joins the cluster of the core point least in (d2, index in ``points``) order.  Open3D's cluster_dbscan and sklearn's DBSCAN give a
    border point to whichever cluster reaches it first, which depends on their visiting order; that rule is REPLACED here, so a border
    point that two clusters can reach may be labelled differently from theirs (core flags, the core points' partition and the noise set
    agree).  Noise: every other point, label -1.  Clusters are numbered 0 .. C - 1 by descending size (core and border members),
    equal sizes by the lowest index in ``points`` of any member; sizes[c] is the size of cluster c.
    The result is a function of (points, eps, min_points): ``cell`` (default: default_cell, but not below eps / 8 so that the walk stays
    within a few shells) changes the time only, and so do the sort inside the grid, the launch shape and the run.  The relabelling from
    the kernels' roots to size ranks is a handful of torch ops on the device."""
    points = _points(points, "points")
    _check_int("cluster_dbscan", "min_points", min_points, 1)
    if not (eps >= 0.0 and np.isfinite(eps) and np.isfinite(float(eps) * float(eps))):
        raise PmnError(f"cluster_dbscan: eps must be finite and >= 0, got {eps}")
    if cell is None:
        cell = max(default_cell(points), float(eps) / 8.0)
    grid = build_grid(points, cell)
    n, dev = int(points.shape[0]), points.device
    core = torch.empty(n, dtype=torch.uint8, device=dev)
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    label = torch.empty(n, dtype=torch.int32, device=dev)
    orig = grid.perm.int()
    L, args = _lib.lib(), _grid_args(grid)
    with torch.cuda.device(dev):
        check(L.pmn_cloud_core(*args, float(eps), int(min_points), core.data_ptr(), _stream(points)), "pmn_cloud_core")
        check(L.pmn_cloud_dbscan(*args, float(eps), core.data_ptr(), orig.data_ptr(), parent.data_ptr(), label.data_ptr(),
                                 _stream(points)), "pmn_cloud_dbscan")
    # roots (sorted indices) -> ranks by (size descending, lowest original index ascending); the second key is unique per cluster.
    # (Integer scatters into tables of n entries instead of unique's sort were measured slower: one large cluster is one address.)
    member = label >= 0
    roots, inverse, counts = torch.unique(label[member].long(), return_inverse=True, return_counts=True)
    first = torch.full((int(roots.numel()),), n, dtype=torch.int64, device=dev).scatter_reduce_(0, inverse, grid.perm[member], "amin")
    order = torch.argsort((n - counts) * (2 ** 31) + first)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(int(order.numel()), dtype=torch.int64, device=dev)
    ranked = torch.full((n,), -1, dtype=torch.int64, device=dev)
    ranked[member] = rank[inverse]
    return _unsort(ranked, grid, True), _unsort(core.bool(), grid, True), counts[order]


def select_clusters(labels: torch.Tensor, sizes: torch.Tensor, min_cluster_points: int = 0, keep_largest: int = 0) -> torch.Tensor:
    """bool [n]: the points of cluster_dbscan's clusters that hold at least ``min_cluster_points`` points and, with ``keep_largest`` > 0,
    are among the ``keep_largest`` first (labels are size ranks, so those are the largest, ties as cluster_dbscan breaks them).  Noise
    (label -1) is never kept."""
    _check_int("select_clusters", "min_cluster_points", min_cluster_points, 0)
    _check_int("select_clusters", "keep_largest", keep_largest, 0)
    for name, t in (("labels", labels), ("sizes", sizes)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int64 or t.dim() != 1:
            raise PmnError(f"select_clusters: {name}: expected a 1-D int64 tensor on a ROCm GPU (no CPU fallback)")
    if labels.device != sizes.device:
        raise PmnError(f"select_clusters: labels are on {labels.device}, sizes on {sizes.device}")
    good = sizes >= int(min_cluster_points)
    if keep_largest > 0:
        good = good & (torch.arange(int(sizes.numel()), device=sizes.device) < int(keep_largest))
    good = torch.cat([good, good.new_zeros(1)])  # label -1 reads the last entry
    return good[labels]


# ---- planes ------------------------------------------------------------------------------------------------------------
# Named settings, chosen by reasoning and not measured optima: 1024 hypotheses find a plane that holds a fifth of the cloud with
# probability 1 - (1 - 0.2^3)^1024 > 0.999; three refits because a least-squares fit of the inliers of a good hypothesis moves little
# after the first.  A threshold of two spacings is the band a surface sampled at that spacing fills.
PLANE_HYPOTHESES = 1024
PLANE_REFITS = 3
PLANE_THRESHOLD_SPACINGS = 2.0


def _plane_inputs(what: str, points, normals, active, threshold, min_cos):
    """The checked point inputs of plane_score / plane_inliers: (points, normals or None, active uint8 or None)."""
    points = _points(points, "points")
    n, dev = int(points.shape[0]), points.device
    if not (isinstance(threshold, (int, float, np.floating, np.integer)) and threshold >= 0.0 and np.isfinite(threshold)):
        raise PmnError(f"{what}: threshold must be finite and >= 0, got {threshold!r}")
    if not (isinstance(min_cos, (int, float, np.floating, np.integer)) and 0.0 <= min_cos <= 1.0):
        raise PmnError(f"{what}: min_cos must lie in [0, 1], got {min_cos!r}")
    if min_cos > 0.0 and normals is None:
        raise PmnError(f"{what}: min_cos > 0 needs normals")
    if normals is not None:
        normals = _per_point(normals, "normals", what, torch.float32, n, dev)
        if not normals.is_contiguous():
            raise PmnError(f"{what}: normals must be contiguous")
        bad = int((~torch.isfinite(normals)).any(1).sum())
        if bad:
            raise PmnError(f"{what}: {bad} normals are not finite")
    if active is not None:
        if not isinstance(active, torch.Tensor) or not active.is_cuda or active.device != dev:
            raise PmnError(f"{what}: active must be a tensor on {dev} (no CPU fallback)")
        if active.dtype not in (torch.bool, torch.uint8) or tuple(active.shape) != (n,):
            raise PmnError(f"{what}: active: expected bool or uint8 [{n}], got {active.dtype} {tuple(active.shape)}")
        active = (active != 0).to(torch.uint8).contiguous()
    return points, normals, active


def plane_score(points: torch.Tensor, planes: torch.Tensor, threshold: float, normals: Optional[torch.Tensor] = None,
                active: Optional[torch.Tensor] = None, min_cos: float = 0.0) -> torch.Tensor:
    """pmn_plane_score: int32 [H], the number of inliers of every row (a, b, c, d) of ``planes`` (float64 [H,4] on the device) among
    ``points``: fabs(a * x + b * y + c * z + d) <= threshold in float64 and, with ``min_cos`` > 0, fabs(a * nx + b * ny + c * nz) >=
    min_cos on ``normals``; points with ``active`` (bool or uint8 [n]) == 0 never count; a row with a non-finite entry scores 0.
    More than 4096 rows are scored in several calls."""
    points, normals, active = _plane_inputs("plane_score", points, normals, active, threshold, min_cos)
    dev = points.device
    if not isinstance(planes, torch.Tensor) or not planes.is_cuda or planes.device != dev:
        raise PmnError(f"plane_score: planes must be a tensor on {dev} (no CPU fallback)")
    if planes.dtype != torch.float64 or planes.dim() != 2 or planes.shape[1] != 4 or planes.shape[0] < 1 or not planes.is_contiguous():
        raise PmnError(f"plane_score: planes: expected a contiguous float64 [H,4] tensor with H >= 1, got {planes.dtype} "
                       f"{tuple(planes.shape)}")
    H = int(planes.shape[0])
    counts = torch.empty(H, dtype=torch.int32, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        for h0 in range(0, H, _lib.PLANE_MAX_HYPOTHESES):
            h1 = min(H, h0 + _lib.PLANE_MAX_HYPOTHESES)
            check(L.pmn_plane_score(points.data_ptr(), normals.data_ptr() if normals is not None else None,
                                    active.data_ptr() if active is not None else None, int(points.shape[0]), planes[h0:h1].data_ptr(),
                                    h1 - h0, float(threshold), float(min_cos), counts[h0:h1].data_ptr(), _stream(points)),
                  "pmn_plane_score")
    return counts


def plane_frame(points: torch.Tensor, active: Optional[torch.Tensor] = None):
    """(centre, extent), float64 [3] each on the host: the centre (lo + hi) * 0.5 of the bounding box of the active points, in float64
    from the float32 coordinates, and the bound max(hi - centre, centre - lo) of |p - centre| that plane_inliers scales its sums by."""
    p = points if active is None else points[active != 0]
    if p.shape[0] < 1:
        raise PmnError("plane_frame: no active point")
    lo, hi = p.min(0).values.double().cpu().numpy(), p.max(0).values.double().cpu().numpy()
    centre = (lo + hi) * 0.5
    return centre, np.maximum(hi - centre, centre - lo)


def plane_inliers(points: torch.Tensor, plane, threshold: float, normals: Optional[torch.Tensor] = None,
                  active: Optional[torch.Tensor] = None, min_cos: float = 0.0, centre=None, extent=None, return_mask: bool = True,
                  scratch: Optional[torch.Tensor] = None):
    """pmn_plane_inliers: (mask bool [n] on the device or None, sums float64 [10] on the device) of ONE ``plane`` (4 finite floats on
    the host), with plane_score's inlier test.  sums over the inliers, with a = p - centre: [0] their number, [1..3] the sum of a,
    [4..9] of ax ax, ax ay, ax az, ay ay, ay az, az az -- exact up to one rounding each, hence the same bits on every run.  ``centre``
    and ``extent`` default to plane_frame(points, active); a given extent must bound |p - centre| over the active points."""
    points, normals, active = _plane_inputs("plane_inliers", points, normals, active, threshold, min_cos)
    n, dev = int(points.shape[0]), points.device
    plane = np.asarray(plane, np.float64).reshape(-1)
    if plane.shape != (4,) or not np.isfinite(plane).all():
        raise PmnError(f"plane_inliers: plane must be 4 finite numbers, got {plane.tolist()}")
    if centre is None or extent is None:
        if centre is not None or extent is not None:
            raise PmnError("plane_inliers: give centre and extent together, or neither")
        centre, extent = plane_frame(points, active)
    centre, extent = np.asarray(centre, np.float64).reshape(-1), np.asarray(extent, np.float64).reshape(-1)
    if centre.shape != (3,) or extent.shape != (3,) or not np.isfinite(centre).all() or not np.isfinite(extent).all() \
            or (extent < 0.0).any():
        raise PmnError(f"plane_inliers: centre must be 3 finite numbers and extent 3 finite numbers >= 0, got {centre.tolist()} and "
                       f"{extent.tolist()}")
    words = _lib.plane_scratch(n)
    if scratch is None:
        scratch = torch.empty(words, dtype=torch.int64, device=dev)
    elif not isinstance(scratch, torch.Tensor) or scratch.device != dev or scratch.dtype != torch.int64 or scratch.dim() != 1 \
            or scratch.numel() < words or not scratch.is_contiguous():
        raise PmnError(f"plane_inliers: scratch must be a contiguous int64 tensor of at least {words} words on {dev}")
    mask = torch.empty(n, dtype=torch.uint8, device=dev) if return_mask else None
    sums = torch.empty(_lib.PLANE_SUMS, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().pmn_plane_inliers(points.data_ptr(), normals.data_ptr() if normals is not None else None,
                                           active.data_ptr() if active is not None else None, n, (ctypes.c_double * 4)(*plane.tolist()),
                                           float(threshold), float(min_cos), (ctypes.c_double * 3)(*centre.tolist()),
                                           (ctypes.c_double * 3)(*extent.tolist()), scratch.data_ptr(), int(scratch.numel()),
                                           mask.data_ptr() if return_mask else None, sums.data_ptr(), _stream(points)),
              "pmn_plane_inliers")
    return (mask.bool() if return_mask else None), sums


def _plane_sign(nrm: np.ndarray) -> np.ndarray:
    """The sign rule: the component of largest magnitude is positive, ties go to the lowest axis (np.argmax takes the first)."""
    k = np.argmax(np.abs(nrm), axis=-1)
    s = np.where(np.take_along_axis(nrm, k[..., None], -1)[..., 0] < 0.0, -1.0, 1.0)
    return nrm * s[..., None]


def plane_hypotheses(triplets, indices=None) -> np.ndarray:
    """The planes through ``triplets`` ([H,3,3]: H times three points, any float type, taken as float64), float64 [H,4] on the host;
    DESIGN.md 34 states every expression.  u = p1 - p0, v = p2 - p0, w = u x v, l2 = w . w; a row is NaN when l2 is not > 0 or, with
    ``indices`` ([H,3] integers), when two of its indices coincide; else nrm = w / sqrt(l2) with the sign rule of _plane_sign and
    d = -(nrm . p0)."""
    p = np.asarray(triplets, np.float64)
    if p.ndim != 3 or p.shape[1:] != (3, 3):
        raise PmnError(f"plane_hypotheses: expected [H,3,3] points, got {p.shape}")
    u, v = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    w = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    l2 = w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]
    bad = ~(l2 > 0.0)
    if indices is not None:
        t = np.asarray(indices)
        bad |= (t[:, 0] == t[:, 1]) | (t[:, 0] == t[:, 2]) | (t[:, 1] == t[:, 2])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        nrm = _plane_sign(w / np.sqrt(l2)[:, None])
        d = -(nrm[:, 0] * p[:, 0, 0] + nrm[:, 1] * p[:, 0, 1] + nrm[:, 2] * p[:, 0, 2])
    planes = np.concatenate([nrm, d[:, None]], 1)
    planes[bad | ~np.isfinite(planes).all(1)] = np.nan
    return planes


def plane_from_sums(sums, centre) -> Optional[np.ndarray]:
    """The least-squares plane of plane_inliers' ten ``sums`` (host float64): the mean m = sums[1:4] / count, the covariance
    C_cd = S_cd / count - m_c * m_d, the eigenvector of np.linalg.eigh's smallest eigenvalue under the sign rule, through centre + m.
    None with fewer than 3 inliers or a result that is not finite."""
    s, c = np.asarray(sums, np.float64), np.asarray(centre, np.float64)
    cnt = s[0]
    if cnt < 3.0:
        return None
    m = s[1:4] / cnt
    C = np.empty((3, 3), np.float64)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[i, j] = C[j, i] = s[4 + k] / cnt - m[i] * m[j]
    if not np.isfinite(C).all():
        return None
    nrm = _plane_sign(np.linalg.eigh(C)[1][:, 0])
    d = -(nrm[0] * (c[0] + m[0]) + nrm[1] * (c[1] + m[1]) + nrm[2] * (c[2] + m[2]))
    plane = np.array([nrm[0], nrm[1], nrm[2], d], np.float64)
    return plane if np.isfinite(plane).all() else None


def plane_rmse(sums, centre, plane) -> float:
    """sqrt(mean r * r) over the inliers from the ten sums, on the host: with e = a cx + b cy + c cz + d the residual is
    r = n . a + e for a = p - centre, so sum r r = n^T S n + 2 e n . s + count e e (clamped at 0 before the root)."""
    s, c, p = np.asarray(sums, np.float64), np.asarray(centre, np.float64), np.asarray(plane, np.float64)
    if s[0] < 1.0:
        return 0.0
    e = p[0] * c[0] + p[1] * c[1] + p[2] * c[2] + p[3]
    q = (p[0] * p[0] * s[4] + p[1] * p[1] * s[7] + p[2] * p[2] * s[9]
         + 2.0 * (p[0] * p[1] * s[5] + p[0] * p[2] * s[6] + p[1] * p[2] * s[8]))
    total = q + 2.0 * e * (p[0] * s[1] + p[1] * s[2] + p[2] * s[3]) + s[0] * e * e
    return float(np.sqrt(max(total, 0.0) / s[0]))


def _min_cos(what: str, normals, normal_angle) -> float:
    if normal_angle is None:
        return 0.0
    if not (isinstance(normal_angle, (int, float, np.floating, np.integer)) and 0.0 <= normal_angle <= 90.0):
        raise PmnError(f"{what}: normal_angle must lie in [0, 90] degrees, got {normal_angle!r}")
    if normals is None:
        raise PmnError(f"{what}: normal_angle needs normals")
    return min(1.0, max(0.0, float(np.cos(np.radians(float(normal_angle))))))


def _plane_settings(what: str, points, threshold, hypotheses, seed, refine):
    for name, v, lo in (("hypotheses", hypotheses, 1), ("seed", seed, 0), ("refine", refine, 0)):
        _check_int(what, name, v, lo)
    return PLANE_THRESHOLD_SPACINGS * cloud_spacing(points) if threshold is None else threshold


def _segment_one(what: str, points, normals, active, threshold: float, min_cos: float, hypotheses: int, refine: int, rng):
    """One plane of the active points, the generator ``rng`` going on from where it stands."""
    n, dev = int(points.shape[0]), points.device
    idx = torch.arange(n, device=dev) if active is None else torch.nonzero(active, as_tuple=False)[:, 0]
    m = int(idx.numel())
    if m < 3:
        raise PmnError(f"{what}: a plane needs 3 active points, got {m}")
    trip = rng.integers(0, m, size=(hypotheses, 3))
    drawn = points[idx[torch.from_numpy(trip).to(dev)]].cpu().numpy()  # [H,3,3]: the 3H points, gathered on the device
    planes = plane_hypotheses(drawn, trip)
    if np.isnan(planes).any(1).all():
        raise PmnError(f"{what}: all {hypotheses} hypotheses are invalid (repeated or collinear points)")
    counts = plane_score(points, torch.from_numpy(planes).to(dev), threshold, normals, active, min_cos).cpu().numpy()
    best = int(np.argmax(counts))
    centre, extent = plane_frame(points, active)
    scratch = torch.empty(_lib.plane_scratch(n), dtype=torch.int64, device=dev)
    kw = dict(normals=normals, active=active, min_cos=min_cos, centre=centre, extent=extent, scratch=scratch)
    plane = planes[best]
    mask, sums = plane_inliers(points, plane, threshold, **kw)
    sums = sums.cpu().numpy()
    refits = 0
    for _ in range(refine):
        new = plane_from_sums(sums, centre)
        if new is None:
            break
        mask2, sums2 = plane_inliers(points, new, threshold, **kw)
        sums2 = sums2.cpu().numpy()
        if sums2[0] < sums[0]:  # a refit that loses inliers is rejected and ends the loop
            break
        same = bool(torch.equal(mask2, mask))
        plane, mask, sums, refits = new, mask2, sums2, refits + 1
        if same:
            break
    return {"plane": plane, "inliers": mask, "count": int(sums[0]), "rmse": plane_rmse(sums, centre, plane), "hypothesis": best,
            "refits": refits}


def segment_plane(points: torch.Tensor, threshold: Optional[float] = None, hypotheses: int = PLANE_HYPOTHESES, seed: int = 0,
                  refine: int = PLANE_REFITS, normals: Optional[torch.Tensor] = None, normal_angle: Optional[float] = None,
                  active: Optional[torch.Tensor] = None) -> dict:
    """The dominant plane of a cloud (Open3D segment_plane, PCL SACSegmentation) on the device: seeded RANSAC scored by pmn_plane_score
    and refitted by least squares over pmn_plane_inliers' exact sums.  Returns a dict: ``plane`` float64 [4] (a, b, c, d
    with a unit normal whose largest component is positive), ``inliers`` bool [n] on the device, ``count``, ``rmse`` (of the residuals
    of the inliers), ``hypothesis`` (the index of the winning draw) and ``refits`` (the refits that were accepted, at most ``refine``).
    A point is an inlier when fabs(a x + b y + c z + d) <= ``threshold`` (default: PLANE_THRESHOLD_SPACINGS times cloud_spacing) and,
    with ``normal_angle`` (degrees, needs ``normals``), its normal lies within that angle of the plane's, either way round.
    ``hypotheses`` triplets of the active points are drawn by np.random.Generator(PCG64(seed)); the highest count wins, ties go to the
    lowest index.  Every output is a function of (points, normals, active, settings, seed), bit for bit; the ORDER of the points
    matters, through the draw.  PmnError with fewer than 3 active points or when every hypothesis is invalid."""
    threshold = _plane_settings("segment_plane", points, threshold, hypotheses, seed, refine)
    min_cos = _min_cos("segment_plane", normals, normal_angle)
    points, normals, active = _plane_inputs("segment_plane", points, normals, active, threshold, min_cos)
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    return _segment_one("segment_plane", points, normals, active, float(threshold), min_cos, int(hypotheses), int(refine), rng)


def segment_planes(points: torch.Tensor, threshold: Optional[float] = None, max_planes: int = 1, min_inliers: int = 3,
                   hypotheses: int = PLANE_HYPOTHESES, seed: int = 0, refine: int = PLANE_REFITS,
                   normals: Optional[torch.Tensor] = None, normal_angle: Optional[float] = None,
                   active: Optional[torch.Tensor] = None) -> dict:
    """Up to ``max_planes`` planes, one after the other: after a plane is accepted its inliers leave the active set and the SAME
    generator goes on drawing.  Extraction stops after ``max_planes``, when the best plane holds fewer than ``min_inliers`` points (it is
    not accepted), or when fewer than 3 active points are left.  Returns a dict: ``labels`` int64 [n] on the device (-1, or the plane's
    index in order of extraction), ``planes`` float64 [k,4], ``counts`` (list of k) and ``results`` (segment_plane's dict per plane)."""
    threshold = _plane_settings("segment_planes", points, threshold, hypotheses, seed, refine)
    _check_int("segment_planes", "max_planes", max_planes, 1)
    _check_int("segment_planes", "min_inliers", min_inliers, 1)
    min_cos = _min_cos("segment_planes", normals, normal_angle)
    points, normals, active = _plane_inputs("segment_planes", points, normals, active, threshold, min_cos)
    n, dev = int(points.shape[0]), points.device
    left = torch.ones(n, dtype=torch.uint8, device=dev) if active is None else active.clone()
    if int(left.sum()) < 3:
        raise PmnError(f"segment_planes: a plane needs 3 active points, got {int(left.sum())}")
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    labels = torch.full((n,), -1, dtype=torch.int64, device=dev)
    results = []
    while len(results) < max_planes and int(left.sum()) >= 3:
        one = _segment_one("segment_planes", points, normals, left, float(threshold), min_cos, int(hypotheses), int(refine), rng)
        if one["count"] < min_inliers:
            break
        labels[one["inliers"]] = len(results)
        left[one["inliers"]] = 0
        results.append(one)
    return {"labels": labels, "planes": np.array([r["plane"] for r in results], np.float64).reshape(-1, 4),
            "counts": [r["count"] for r in results], "results": results}


def _viewpoints(what: str, viewpoints, device) -> Optional[torch.Tensor]:
    """None, or the viewpoints as a contiguous float64 [V,3] tensor on ``device`` (a tensor there already, or host numbers)."""
    if viewpoints is None:
        return None
    if isinstance(viewpoints, torch.Tensor):
        if viewpoints.device != device:
            raise PmnError(f"{what}: viewpoints are on {viewpoints.device}, the grid on {device}")
        if viewpoints.dtype != torch.float64:
            raise PmnError(f"{what}: viewpoints: expected float64, got {viewpoints.dtype}")
        v = viewpoints
    else:
        v = torch.as_tensor(np.asarray(viewpoints, np.float64)).to(device)
    if v.dim() != 2 or v.shape[1] != 3 or not 1 <= v.shape[0] <= _lib.NORMAL_MAX_VIEWPOINTS:
        raise PmnError(f"{what}: viewpoints: expected [V,3] with 1 <= V <= {_lib.NORMAL_MAX_VIEWPOINTS}, got {tuple(v.shape)}")
    if not bool(torch.isfinite(v).all()):
        raise PmnError(f"{what}: viewpoints have non-finite coordinates")
    return v.contiguous()


def knn_normals(query: Optional[torch.Tensor], grid: Grid, k: int, max_dist: float, same_cloud: bool = False, viewpoints=None,
                line_ratio: float = 1e-6, return_variation: bool = False, return_count: bool = False):
    """pmn_knn_normals: float32 [n,3], the normal of every query point from the point itself and its ``k`` (1..32) nearest points of
    ``grid`` nearer than ``max_dist`` (knn_distance's search): the eigenvector of least variance of their covariance, float64 on the
    device (include/pmn_hip.h states every operation).  (0, 0, 0) where fewer than two neighbours lie in range, where all points
    coincide, or where they lie on a line (second eigenvalue <= ``line_ratio`` times the largest).
    Sign: the component of largest magnitude is positive, or with ``viewpoints`` ([V,3], V <= 4096; a float64 tensor on the grid's
    device or host numbers) the normal faces the viewpoint nearest to the point -- a heuristic, a cloud does not say which camera saw
    a point.  Unlike the C entry, which only enqueues, this wrapper waits for the device when viewpoints are given: it checks them
    for non-finite values (one host read) and uploads host numbers first.  ``return_variation``: also float64 [n], the surface variation l0 / (l0 + l1 + l2), 0 where the normal is;
    ``return_count``: also int32 [n], the neighbours used (less than k where slots were capped).  ``same_cloud``: as knn_distance."""
    k = _check_k("knn_normals", k)
    _check_reach("knn_normals", "max_dist", max_dist)
    if not (line_ratio >= 0.0 and np.isfinite(line_ratio)):
        raise PmnError(f"knn_normals: line_ratio must be finite and >= 0, got {line_ratio}")

    def scalars(dev):  # the viewpoints go to the query's device, and are checked after the query
        views = _viewpoints("knn_normals", viewpoints, dev)
        return k, float(max_dist), int(bool(same_cloud)), views, int(views.shape[0]) if views is not None else 0, float(line_ratio)

    return _one_or_tuple(_query_search("pmn_knn_normals", grid, query, same_cloud, scalars,
                                       [((3,), torch.float32, True), ((), torch.float64, return_variation), ((), torch.int32, return_count)]))


def estimate_normals(points: torch.Tensor, k: int = 16, max_dist: Optional[float] = None, cell: Optional[float] = None,
                     viewpoints=None, orient_like: Optional[torch.Tensor] = None, line_ratio: float = 1e-6,
                     return_variation: bool = False, return_count: bool = False):
    """Normals of a cloud from its own neighbourhoods (Open3D estimate_normals with knn = k + 1): builds the cleaning grid
    (default_cell; ``max_dist`` defaults to CLEAN_MAX_DIST_CELLS cells, as in statistical_outliers) and calls knn_normals with
    same_cloud.  Orientation: ``viewpoints`` as in knn_normals, or ``orient_like``, float32 [n,3] on the device (for example the
    depth-map normals of an ``eval.py --normals 1`` cloud): a normal n is negated where n . orient_like < 0 (float64 torch on the
    device, on the rounded normal); giving both is an error.  ``cell`` changes the time only."""
    points = _points(points, "points")
    if viewpoints is not None and orient_like is not None:
        raise PmnError("estimate_normals: give viewpoints or orient_like, not both")
    if orient_like is not None:
        if not isinstance(orient_like, torch.Tensor) or orient_like.device != points.device:
            raise PmnError(f"estimate_normals: orient_like must be a tensor on {points.device} (no CPU fallback)")
        if orient_like.dtype != torch.float32 or tuple(orient_like.shape) != tuple(points.shape):
            raise PmnError(f"estimate_normals: orient_like: expected float32 {tuple(points.shape)}, got {orient_like.dtype} "
                           f"{tuple(orient_like.shape)}")
    grid = _clean_grid(points, cell)
    if max_dist is None:
        max_dist = CLEAN_MAX_DIST_CELLS * grid.cell
    out = knn_normals(None, grid, k, max_dist, same_cloud=True, viewpoints=viewpoints, line_ratio=line_ratio,
                      return_variation=return_variation, return_count=return_count)
    if orient_like is not None:
        normal = out[0] if isinstance(out, tuple) else out
        against = (normal.double() * orient_like.double()).sum(1) < 0
        normal = torch.where(against[:, None], -normal, normal)
        out = (normal,) + out[1:] if isinstance(out, tuple) else normal
    return out


# ---- moving least squares ------------------------------------------------------------------------------------------------
# A SETTING, not a measurement: three spacings hold about 28 neighbours of a point of a regularly sampled surface (pi * 3^2), the k
# the tool defaults to; no sweep stands behind the figure.  It is an argument of smooth_mls and a flag of smooth_cloud.py.
MLS_RADIUS_SPACINGS = 3.0   # default radius of smooth_mls = this times cloud_spacing


def knn_mls(query: Optional[torch.Tensor], grid: Grid, k: int, radius: float, same_cloud: bool = False, degree: int = 2,
            line_ratio: float = 1e-6, return_normal: bool = False, return_displacement: bool = False, return_status: bool = False,
            return_count: bool = False):
    """pmn_knn_mls: float32 [n,3], every query point projected onto the surface fitted to its ``k`` (1..32) nearest points of ``grid``
    nearer than ``radius`` (knn_distance's search), weighted by (1 - d2 / radius^2)^4: the plane through the weighted centroid along
    the two directions of largest variance (``degree`` 1), or the quadric over that plane (``degree`` 2, from 6 members on; it falls
    back to the plane when its normal equations are too ill-conditioned or when it would move the point beyond ``radius``), float64 on
    the device (include/pmn_hip.h states every operation).  A point with fewer than three members, or whose neighbourhood lies on a
    line (second eigenvalue <= ``line_ratio`` times the largest), stays where it is.  ``return_normal``: also float32 [n,3], the fitted
    surface's unit normal at the projection, its largest component positive (0 0 0 where the point stayed); ``return_displacement``:
    also float64 [n], how far the point moved; ``return_status``: also int32 [n], 0 not fitted, 1 plane, 2 quadric; ``return_count``:
    also int32 [n], the neighbours in range.  ``same_cloud``: as knn_distance; the point itself then joins the fit with weight 1."""
    k = _check_k("knn_mls", k)
    _check_reach("knn_mls", "radius", radius, positive_square=True)
    if isinstance(degree, bool) or not isinstance(degree, (int, np.integer)) or int(degree) not in (1, 2):
        raise PmnError(f"knn_mls: degree must be 1 or 2, got {degree!r}")
    if not (line_ratio >= 0.0 and np.isfinite(line_ratio)):
        raise PmnError(f"knn_mls: line_ratio must be finite and >= 0, got {line_ratio}")
    return _one_or_tuple(_query_search("pmn_knn_mls", grid, query, same_cloud,
                                       (k, float(radius), int(bool(same_cloud)), int(degree), float(line_ratio)),
                                       [((3,), torch.float32, True), ((3,), torch.float32, return_normal),
                                        ((), torch.float64, return_displacement), ((), torch.int32, return_status),
                                        ((), torch.int32, return_count)]))


def smooth_mls(points: torch.Tensor, radius: Optional[float] = None, k: int = 32, degree: int = 2, iterations: int = 1,
               cell: Optional[float] = None, return_normals: bool = False, radius_spacings: float = MLS_RADIUS_SPACINGS):
    """Moving-least-squares smoothing of a cloud by its own neighbourhoods (PCL MovingLeastSquares without upsampling): (positions
    float32 [n,3] in the order of ``points``, report dict), with ``return_normals`` (positions, normals float32 [n,3], report).
    Every iteration builds the cleaning grid (default_cell, or ``cell``) from the current positions and calls knn_mls with
    same_cloud; ``radius`` defaults to ``radius_spacings`` (MLS_RADIUS_SPACINGS) times cloud_spacing(points) of the INPUT and is
    the same in every iteration.  The number and the order of the points never change; a point that could not be fitted stays where it was.  report:
    radius, spacing (None when the radius was given and the cloud has none), k, degree, iterations, status = the points that were
    [not fitted, projected onto a plane, projected onto a quadric] in the last iteration, and mean_displacement / max_displacement
    from the input position to the final one, in scene units and (``_spacings``) in units of the spacing."""
    points = _points(points, "points")
    _check_int("smooth_mls", "iterations", iterations, 1)
    if cell is not None and not (float(cell) > 0.0 and np.isfinite(float(cell))):
        raise PmnError(f"smooth_mls: cell must be positive and finite, got {cell}")
    if not (float(radius_spacings) > 0.0 and np.isfinite(float(radius_spacings))):
        raise PmnError(f"smooth_mls: radius_spacings must be positive and finite, got {radius_spacings}")
    spacing = cloud_spacing(points) if int(points.shape[0]) > 1 else 0.0
    if radius is None:
        radius = float(radius_spacings) * spacing
        if not (radius > 0.0 and np.isfinite(radius)):
            raise PmnError(f"smooth_mls: the cloud's spacing is {spacing}; give radius")
    current, normal, status = points, None, None
    for _ in range(int(iterations)):
        grid = _clean_grid(current, cell)
        current, normal, status = knn_mls(None, grid, k, radius, same_cloud=True, degree=degree, return_normal=True, return_status=True)
    moved = (current.double() - points.double()).norm(dim=1)
    mean, largest = float(moved.mean()), float(moved.max())
    unit = spacing if spacing > 0.0 and np.isfinite(spacing) else None
    report = {"radius": float(radius), "spacing": unit, "k": int(k), "degree": int(degree), "iterations": int(iterations),
              "status": torch.bincount(status.long(), minlength=3).cpu().tolist(), "mean_displacement": mean, "max_displacement": largest,
              "mean_displacement_spacings": mean / unit if unit else None, "max_displacement_spacings": largest / unit if unit else None}
    return (current, normal, report) if return_normals else (current, report)


# ---- a surface from an oriented cloud -------------------------------------------------------------------------------
# SETTINGS, not measurements: the ratios below were chosen by reasoning (a sample should see about a ring of neighbours on either side,
# the band should hold the marching cells next to the surface, a boundary is cut about half a support away from the last point) and
# no sweep stands behind them.  Each is an argument of mesh_from_cloud and a flag of mesh_cloud.py.
SDF_SPACING_K = 8           # s = the median over the cloud of the mean distance to this many nearest other points
SDF_VOXEL_SPACINGS = 1.0    # voxel = this times s
SDF_RADIUS_VOXELS = 3.0     # radius = this times voxel; trunc = radius
SDF_BOUNDARY_RADII = 0.5    # boundary = this times radius


def _per_point(t, name: str, what: str, dtype, n: int, device) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise PmnError(f"{what}: {name}: expected a torch.Tensor")
    if not t.is_cuda or t.device != device:
        raise PmnError(f"{what}: {name} is on {t.device}, the points on {device} (no CPU fallback)")
    if t.dtype != dtype:
        raise PmnError(f"{what}: {name}: expected {dtype}, got {t.dtype}")
    if tuple(t.shape) != (n, 3):
        raise PmnError(f"{what}: {name}: expected [{n},3], got {tuple(t.shape)}")
    return t


def cloud_sdf(volume, grid: Grid, normals: torch.Tensor, colors: Optional[torch.Tensor] = None, k: int = 16,
              radius: Optional[float] = None, boundary: Optional[float] = None) -> None:
    """pmn_cloud_sdf_blocks: fills the pool planes of ``volume`` (a tsdf.SparseTsdfVolume after allocate_points) with the signed
    distance to the oriented cloud of ``grid``: per sample the ``k`` (1..32) nearest points within ``radius``, f = sum w n . (x - p) /
    sum w with w = (1 - d2 / radius^2)^4 in rank order, unobserved (tsdf 1, weight 0) where no point is in range or where the nearest
    point's tangent plane is met further than ``boundary`` from it; weight = the number of neighbours (include/pmn_hip.h states every
    operation).  ``normals`` float32 [n,3] and ``colors`` uint8 [n,3] (given exactly when the volume has colour planes) are in the
    ORIGINAL order of the points the grid was built from; they are gathered through grid.perm here.  ``radius`` defaults to the grid's
    cell, ``boundary`` to half the radius.  One launch; every argument is checked before it."""
    from .tsdf import SparseTsdfVolume
    if not isinstance(volume, SparseTsdfVolume):
        raise PmnError("cloud_sdf: volume must be a tsdf.SparseTsdfVolume")
    volume._allocated("cloud_sdf")
    k = _check_k("cloud_sdf", k)
    radius = float(grid.cell) if radius is None else float(radius)
    boundary = SDF_BOUNDARY_RADII * radius if boundary is None else float(boundary)
    _check_reach("cloud_sdf", "radius", radius, positive_square=True)
    _check_reach("cloud_sdf", "boundary", boundary, positive_square=True)
    if not isinstance(grid.xyz, torch.Tensor) or not grid.xyz.is_cuda or grid.xyz.device != volume.tsdf.device:
        raise PmnError(f"cloud_sdf: the grid is on {getattr(grid.xyz, 'device', None)}, the volume on {volume.tsdf.device} "
                       f"(no CPU fallback)")
    n, dev = int(grid.xyz.shape[0]), grid.xyz.device
    normals = _per_point(normals, "normals", "cloud_sdf", torch.float32, n, dev)
    if (colors is not None) != (volume.rgb is not None):
        raise PmnError("cloud_sdf: colors must be given exactly when the volume has colour planes")
    if colors is not None:
        colors = _per_point(colors, "colors", "cloud_sdf", torch.uint8, n, dev)
    bad = int((~torch.isfinite(normals)).any(1).sum())
    if bad:
        raise PmnError(f"cloud_sdf: {bad} normals are not finite")
    nrm = normals[grid.perm].contiguous()
    col = colors[grid.perm].contiguous() if colors is not None else None
    dims = (ctypes.c_int * 3)(*volume.dims)
    origin = (ctypes.c_float * 3)(*[float(v) for v in volume.origin])
    with torch.cuda.device(dev):
        check(_lib.lib().pmn_cloud_sdf_blocks(*_grid_args(grid), nrm.data_ptr(), col.data_ptr() if col is not None else None,
                                              volume.blocks.data_ptr(), int(volume.blocks.shape[0]), dims, origin, volume.voxel,
                                              volume.trunc, k, radius, boundary, volume.tsdf.data_ptr(), volume.weight.data_ptr(),
                                              volume.rgb.data_ptr() if col is not None else None,
                                              volume.cweight.data_ptr() if col is not None else None, _stream(grid.xyz)),
              "pmn_cloud_sdf_blocks")


def cloud_spacing(points: torch.Tensor, k: int = SDF_SPACING_K) -> float:
    """s, the spacing mesh_from_cloud sizes its voxel from: the median (the lower of the two middle values) over the cloud of
    knn_distance's mean distance to the ``k`` nearest other points, on the cleaning grid with its default cap."""
    points = _points(points, "points")
    grid = _clean_grid(points, None)
    return float(knn_distance(None, grid, k, CLEAN_MAX_DIST_CELLS * grid.cell, same_cloud=True).median())


def mesh_from_cloud(points: torch.Tensor, normals: torch.Tensor, colors: Optional[torch.Tensor] = None, voxel: Optional[float] = None,
                    radius: Optional[float] = None, trunc: Optional[float] = None, k: int = 16, boundary: Optional[float] = None,
                    min_neighbors: int = 3, max_blocks: Optional[int] = None, normals_out: bool = True):
    """A surface mesh from an oriented cloud: (vertices [Nv,3] float32, faces [Nt,3] int32, colors [Nv,3] uint8 | None,
    normals [Nv,3] float32 | None, info dict), on the device.  ``points`` float32 [n,3], ``normals`` float32 [n,3] (for example
    estimate_normals'), ``colors`` uint8 [n,3] or None.  A point whose normal is zero or not finite -- cloud_normals.py's degenerate
    points -- is dropped and counted in info.  Defaults (the SDF_* settings above, none of them measured): voxel = s = cloud_spacing,
    radius = 3 voxels, trunc = radius, boundary = radius / 2.  The lattice is tsdf.choose_grid's for the sparse volume (1st..99th
    percentile box of the points grown by radius; when it would exceed the virtual lattice the voxel grows, with the defaults that
    follow it, and info["note"] says so); the search grid's cell is radius.  Then SparseTsdfVolume.allocate_points(points, radius),
    cloud_sdf and extract(min_weight=min_neighbors): a vertex needs ``min_neighbors`` points within radius of both ends of its edge."""
    from . import ops, tsdf
    points = _points(points, "points")
    n, dev = int(points.shape[0]), points.device
    normals = _per_point(normals, "normals", "mesh_from_cloud", torch.float32, n, dev)
    if colors is not None:
        colors = _per_point(colors, "colors", "mesh_from_cloud", torch.uint8, n, dev)
    k = _check_k("mesh_from_cloud", k)
    if isinstance(min_neighbors, bool) or not isinstance(min_neighbors, (int, np.integer)) or not 1 <= int(min_neighbors) <= k:
        raise PmnError(f"mesh_from_cloud: min_neighbors must be an integer in 1..k, got {min_neighbors!r}")
    for name, v in (("voxel", voxel), ("radius", radius), ("trunc", trunc), ("boundary", boundary)):
        if v is not None and not (float(v) > 0.0 and np.isfinite(float(v))):
            raise PmnError(f"mesh_from_cloud: {name} must be positive and finite, got {v}")
    max_blocks = tsdf.MAX_BLOCKS if max_blocks is None else int(max_blocks)
    good = torch.isfinite(normals).all(1) & (normals != 0).any(1)
    dropped = n - int(good.sum())
    if dropped == n:
        raise PmnError("mesh_from_cloud: no point has a normal (all are zero or not finite); cloud_normals.py estimates them")
    if dropped:
        points, normals = points[good].contiguous(), normals[good].contiguous()
        colors = colors[good].contiguous() if colors is not None else None
    s = None
    if voxel is None:
        s = cloud_spacing(points)
        voxel = SDF_VOXEL_SPACINGS * s
        if not (voxel > 0.0 and np.isfinite(voxel)):
            raise PmnError(f"mesh_from_cloud: the cloud's spacing is {s}; give voxel")
    voxel, note = float(voxel), None
    while True:  # a voxel that has to grow takes the defaults that depend on it along
        r = SDF_RADIUS_VOXELS * voxel if radius is None else float(radius)
        origin, grown, _, dims, why = tsdf.choose_grid(points, voxel=voxel, trunc=r, max_voxels=tsdf.MAX_VIRTUAL_VOXELS,
                                                       limit_name="the virtual lattice's", max_axis=ops.SPARSE_MAX_AXIS - 1)
        if why is None:
            break
        voxel, note = grown, why
    radius = r
    trunc = radius if trunc is None else float(trunc)
    boundary = SDF_BOUNDARY_RADII * radius if boundary is None else float(boundary)
    volume = tsdf.SparseTsdfVolume(origin, voxel, dims, trunc, dev, color=colors is not None, max_blocks=max_blocks)
    grid = build_grid(points, radius)
    blocks = volume.allocate_points(points, radius)
    cloud_sdf(volume, grid, normals, colors, k=int(k), radius=radius, boundary=boundary)
    vertices, faces, vcolors, vnormals = volume.extract(min_weight=float(min_neighbors), normals=normals_out)
    nb = volume.nblocks
    info = {"points": n, "dropped": dropped, "s": s, "voxel": volume.voxel, "radius": radius, "trunc": volume.trunc,
            "boundary": boundary, "k": int(k), "min_neighbors": int(min_neighbors), "dims": tuple(volume.dims),
            "origin": [float(v) for v in volume.origin], "blocks": blocks, "blocks_marked": volume.marked,
            "block_share": blocks / float(nb[0] * nb[1] * nb[2]), "observed": int((volume.weight > 0).sum()),
            "vertices": int(vertices.shape[0]), "faces": int(faces.shape[0]), "note": note}
    return vertices, faces, vcolors, vnormals, info


def reduce_points(points: torch.Tensor, dst: float, order=None, seed: int = 0, cell: Optional[float] = None,
                  return_rounds: bool = False):
    """reducePts_haa.m on the device: bool [n], the greedy maximal set of points no two of which are within ``dst`` (<=) of each
    other, for the visiting order ``order`` (a permutation of 0..n-1, tensor or array; default: numpy's default_rng(seed)
    permutation, drawn on the host).  The result is the sequential greedy set of that order, bit for bit, on every run.
    ``cell``: the grid's cell (default REDUCE_CELL_RATIO * dst)."""
    points = _points(points, "points")
    n = int(points.shape[0])
    dst = float(dst)
    if not (dst >= 0.0 and np.isfinite(dst)):
        raise PmnError(f"reduce_points: dst must be finite and >= 0, got {dst}")
    if order is None:
        order = np.random.default_rng(seed).permutation(n)
    order = torch.as_tensor(np.asarray(order.cpu()) if isinstance(order, torch.Tensor) else np.asarray(order)).long().to(points.device)
    if order.shape != (n,) or int(order.min()) != 0 or int(order.max()) != n - 1 or int(torch.unique(order).numel()) != n:
        raise PmnError(f"reduce_points: order must be a permutation of 0..{n - 1}")
    if cell is None:
        cell = REDUCE_CELL_RATIO * dst if dst > 0 else 1.0
    grid = build_grid(points, cell)
    rank = torch.empty(n, dtype=torch.int32, device=points.device)
    rank[order] = torch.arange(n, dtype=torch.int32, device=points.device)
    rank = rank[grid.perm].contiguous()
    state = torch.zeros(n, dtype=torch.uint8, device=points.device)
    L = _lib.lib()
    args = _grid_args(grid)
    rounds = 0
    with torch.cuda.device(points.device):
        while True:
            counters = torch.zeros(ROUNDS_PER_READ, dtype=torch.int32, device=points.device)
            for k in range(ROUNDS_PER_READ):
                check(L.pmn_reduce_round(*args, dst, rank.data_ptr(), state.data_ptr(), counters[k:].data_ptr(), _stream(points)),
                      "pmn_reduce_round")
            left = counters.cpu().tolist()
            if 0 in left:
                rounds += left.index(0) + 1
                break
            rounds += ROUNDS_PER_READ
    keep = torch.empty(n, dtype=torch.bool, device=points.device)
    keep[grid.perm] = state == 1
    return (keep, rounds) if return_rounds else keep


# ---- masks and statistics (PointCompareMain.m:32-53, ComputeStat_web.m:52-68) -----------------------------------------------------------

def matlab_round(x: torch.Tensor) -> torch.Tensor:
    """MATLAB round: halves away from zero (torch.round rounds halves to even)."""
    t = torch.trunc(x)
    return t + torch.sign(x) * ((x - t).abs() >= 0.5)


def data_in_mask(xyz: torch.Tensor, obs_mask: torch.Tensor, bb: np.ndarray, res: float) -> torch.Tensor:
    """Qv = round((Qdata - BB(1,:)) / Res + 1), 1-based, inside size(ObsMask) and ObsMask(Qv) set; float64 from the float32 points."""
    lo = torch.tensor(np.asarray(bb, np.float64)[0], dtype=torch.float64, device=xyz.device)
    qv = matlab_round((xyz.double() - lo) / float(res) + 1.0)
    shape = torch.tensor(tuple(obs_mask.shape), dtype=torch.float64, device=xyz.device)
    inside = ((qv > 0) & (qv <= shape)).all(1)
    iv = (qv.clamp(1.0, 2.0 ** 40).long() - 1).minimum(torch.tensor(tuple(obs_mask.shape), device=xyz.device) - 1)
    return inside & (obs_mask[iv[:, 0], iv[:, 1], iv[:, 2]] != 0)


def above_plane(xyz: torch.Tensor, plane: np.ndarray) -> torch.Tensor:
    """P' * [Qstl; 1] > 0 in float64."""
    p = [float(v) for v in np.asarray(plane, np.float64).reshape(4)]
    q = xyz.double()
    return q[:, 0] * p[0] + q[:, 1] * p[1] + q[:, 2] * p[2] + p[3] > 0


def in_blocks(xyz: torch.Tensor, bb: np.ndarray, search_dist: float) -> torch.Tensor:
    """True for the points inside one of MaxDistCP.m's blocks [Low, Low + MaxDist), Low = BB(1,:) + k * MaxDist, k = 0 ..
    floor((BB(2,:) - BB(1,:)) / MaxDist) per axis, with the bounds computed as the MATLAB computes them."""
    bb = np.asarray(bb, np.float64)
    q = xyz.double()
    out = torch.ones(len(q), dtype=torch.bool, device=xyz.device)
    for a in range(3):
        k = np.arange(int(np.floor((bb[1, a] - bb[0, a]) / search_dist)) + 1, dtype=np.float64)
        low = torch.tensor(bb[0, a] + k * search_dist, dtype=torch.float64, device=xyz.device)
        high = low + search_dist
        out &= ((q[:, a, None] >= low) & (q[:, a, None] < high)).any(1)
    return out


def _stats(d: torch.Tensor, prefix: str) -> Dict[str, float]:
    n = int(d.numel())
    nan = float("nan")
    out = {f"{prefix}_n": n, f"{prefix}_mean": nan, f"{prefix}_median": nan, f"{prefix}_var": nan}
    if n:
        s = torch.sort(d).values
        out[f"{prefix}_mean"] = float(d.mean())
        out[f"{prefix}_median"] = float((s[(n - 1) // 2] + s[n // 2]) / 2)  # numpy / MATLAB median, not torch.median
    if n > 1:
        out[f"{prefix}_var"] = float(d.var(unbiased=True))
    return out


def dtu_score_scan(data_xyz: torch.Tensor, stl_xyz: torch.Tensor, obs_mask, bb, res: float, plane, dst: float = 0.2,
                   max_dist: float = 20.0, search_dist: float = 60.0, seed: int = 0, nn_cell: Optional[float] = None,
                   mesh=None) -> Dict:
    """PointCompareMain.m + the statistics of BaseEvalMain_web.m / ComputeStat_web.m for one scan.  data_xyz / stl_xyz: [n,3] float32
    on the device (the vertices of the method's PLY and of stl%03d_total.ply); obs_mask, bb, res, plane: load_obs_mask / load_plane.
    ``max_dist``: the outlier threshold of the statistics (20); ``search_dist``: MaxDistCP's block size and cap (60).
    ``mesh`` = (vertices, faces) of the method's surface: the stl -> data leg (completeness) is then the exact distance to that surface
    (meshops.point_mesh_distance against the whole mesh), with the blocks and the ``search_dist`` cap unchanged; the
    data -> stl leg is unchanged.
    Returns n_data_in, n_data_reduced, reduce_rounds, acc_n/mean/median/var, comp_n/mean/median/var and seconds per phase."""
    data_xyz = _points(data_xyz, "data_xyz")
    stl_xyz = _points(stl_xyz, "stl_xyz")
    dev = data_xyz.device
    nn_cell = NN_CELL if nn_cell is None else float(nn_cell)
    obs = torch.as_tensor(np.ascontiguousarray(np.asarray(obs_mask), dtype=np.uint8)).to(dev)
    if obs.dim() != 3:
        raise PmnError(f"dtu_score_scan: ObsMask must be 3-D, got {tuple(obs.shape)}")

    def clock():
        torch.cuda.synchronize(dev)
        return time.perf_counter()

    t0 = clock()
    keep, rounds = reduce_points(data_xyz, dst, seed=seed, return_rounds=True)
    qd = data_xyz[keep].contiguous()
    t1 = clock()

    def blocked(frm, to):  # MaxDistCP.m: a from-point in no block keeps MaxDist
        d = nn_distance(frm, build_grid(to, nn_cell), search_dist)
        return torch.where(in_blocks(frm, bb, search_dist), d, torch.full_like(d, search_dist))

    d_data = blocked(qd, stl_xyz)
    t2 = clock()
    if mesh is None:
        d_stl = blocked(stl_xyz, qd)
    else:
        from . import meshops
        d_stl = meshops.point_mesh_distance(stl_xyz, meshops.build_face_grid(mesh[0], mesh[1]), search_dist)
        d_stl = torch.where(in_blocks(stl_xyz, bb, search_dist), d_stl, torch.full_like(d_stl, search_dist))
    t3 = clock()
    acc = d_data[data_in_mask(qd, obs, bb, res)]
    comp = d_stl[above_plane(stl_xyz, plane)]
    out = {"n_data_in": int(data_xyz.shape[0]), "n_data_reduced": int(qd.shape[0]), "reduce_rounds": rounds}
    out.update(_stats(acc[acc < max_dist], "acc"))
    out.update(_stats(comp[comp < max_dist], "comp"))
    t4 = clock()
    out["seconds"] = {"reduce": t1 - t0, "data_to_stl": t2 - t1, "stl_to_data": t3 - t2, "statistics": t4 - t3}
    return out


def totals(per_scan) -> Dict[str, float]:
    """BaseEvalMain_web.m:98-99: mean over the scans of the per-scan means; overall = (acc + comp) / 2."""
    acc = float(np.mean([s["acc_mean"] for s in per_scan])) if per_scan else float("nan")
    comp = float(np.mean([s["comp_mean"] for s in per_scan])) if per_scan else float("nan")
    return {"acc": acc, "comp": comp, "overall": (acc + comp) / 2}
