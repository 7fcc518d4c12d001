"""Rigid registration of two point clouds and the Tanks and Temples F-score on the device (tests/tnt_ref.py is the numpy
statement the module is held to).

The three kernels are csrc/registration.hip: pmn_icp_accumulate (one ICP iteration: nearest-neighbour search over a pointcloud.Grid
and the seventeen sums of the matched pairs in one pass), pmn_voxel_mean (the voxel-mean downsample) and pmn_crop_prism (the crop
volume).  Grids, sorts and boolean selects are torch on the device, as in pointcloud.py; the 3 x 3 SVD of an iteration, the
trajectory alignment and the file readers are numpy float64 on the host.  There is no CPU path: the kernels refuse host tensors.
"""
from __future__ import annotations

import ctypes
import json
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import pointcloud as PC
from ._lib import PmnError, check

# per-scene distance threshold tau of the training scenes (written from memory of the toolbox: DESIGN.md 17; eval_tnt.py --tau overrides)
SCENE_TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01,
             "Truck": 0.005}
# (voxel / tau, ICP distance / tau) of the two voxel rounds and the distance of the thinned round; ICP iterations per round
ROUND_A = (1.0, 80.0)
ROUND_B = (0.5, 20.0)
ROUND_C_DIST = 2.0
ICP_ITERATIONS = 20
MAX_POINTS = 4_000_000
HIST_MAX_TAU = 5.0
HIST_BINS = 100
ICP_CELL_DIVISOR = 4.0  # an ICP round's grid cell = max(2 voxels, distance / this): a far outlier walks at most six shells


# ---- files --------------------------------------------------------------------------------------------------------------------------

class CropVolume(NamedTuple):
    """The toolbox's crop volume: a polygon extruded along one coordinate axis."""
    polygon: np.ndarray  # [k,3] float64, the vertices in cyclic order (the coordinate along ``axis`` is ignored)
    axis: int            # 0 | 1 | 2
    axis_min: float
    axis_max: float


def read_crop_json(path: str) -> CropVolume:
    """<Scene>.json of the toolbox: bounding_polygon ([k][3]), orthogonal_axis ("X" | "Y" | "Z"), axis_min, axis_max."""
    with open(path) as f:
        js = json.load(f)
    for key in ("bounding_polygon", "orthogonal_axis", "axis_min", "axis_max"):
        if key not in js:
            raise ValueError(f"{path}: no field {key!r}")
    poly = np.asarray(js["bounding_polygon"], np.float64)
    axis = "xyz".find(str(js["orthogonal_axis"]).lower())
    if poly.ndim != 2 or poly.shape[1] != 3 or len(poly) < 3:
        raise ValueError(f"{path}: bounding_polygon must be [k >= 3][3], got {poly.shape}")
    if axis < 0 or len(str(js["orthogonal_axis"])) != 1:
        raise ValueError(f"{path}: orthogonal_axis must be X, Y or Z, got {js['orthogonal_axis']!r}")
    return CropVolume(poly, axis, float(js["axis_min"]), float(js["axis_max"]))


def read_trajectory_log(path: str) -> np.ndarray:
    """A trajectory .log of the toolbox -> [m,4,4] float64 camera-to-world matrices: per camera a line of three integers, then the
    four rows of the matrix."""
    with open(path) as f:
        rows = [ln.split() for ln in f if ln.strip()]
    if not rows or len(rows) % 5:
        raise ValueError(f"{path}: {len(rows)} non-empty lines is not a multiple of 5 (a header line and four matrix rows per camera)")
    out = np.empty((len(rows) // 5, 4, 4), np.float64)
    for i in range(len(out)):
        head, mat = rows[5 * i], rows[5 * i + 1:5 * i + 5]
        try:
            [int(v) for v in head]
            ok = len(head) == 3 and all(len(r) == 4 for r in mat)
            out[i] = np.asarray(mat, np.float64) if ok else 0
        except ValueError:
            ok = False
        if not ok:
            raise ValueError(f"{path}: camera {i}: expected three integers and a 4 x 4 matrix")
    return out


def read_transform(path: str) -> np.ndarray:
    """A 4 x 4 matrix in a text file (<Scene>_trans.txt)."""
    m = np.loadtxt(path, dtype=np.float64)
    if m.shape != (4, 4):
        raise ValueError(f"{path}: expected a 4 x 4 matrix, got {m.shape}")
    return m


# ---- host-side alignment ------------------------------------------------------------------------------------------------------------

def _rotation(H: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """R = V diag(1, 1, det(V U^T)) U^T for H = U S V^T = sum (a - mean a)(b - mean b)^T: the rotation that takes the a onto the b;
    also S and the diagonal (the reflection fix)."""
    U, S, Vt = np.linalg.svd(H)
    D = np.array([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0])
    return Vt.T @ np.diag(D) @ U.T, S, D


def umeyama(a, b, with_scale: bool = True) -> np.ndarray:
    """The closed-form similarity (rigid motion if not ``with_scale``) that takes the points a [m,3] onto b [m,3] in the least-squares
    sense, as a 4 x 4 matrix; float64 on the host.  This is the alignment of two camera trajectories by their centres."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or a.ndim != 2 or a.shape[1] != 3 or len(a) < 3:
        raise PmnError(f"umeyama: two [m >= 3][3] arrays, got {a.shape} and {b.shape}")
    ma, mb = a.mean(0), b.mean(0)
    da, db = a - ma, b - mb
    R, S, D = _rotation(da.T @ db)
    var = float((da * da).sum())
    if with_scale and not var > 0.0:
        raise PmnError("umeyama: the source points coincide")
    s = float((S * D).sum()) / var if with_scale else 1.0
    T = np.eye(4)
    T[:3, :3] = s * R
    T[:3, 3] = mb - s * R @ ma
    return T


def kabsch_from_sums(sums, centre) -> np.ndarray:
    """The rigid update of one ICP iteration from pmn_icp_accumulate's seventeen sums (count, sum a, sum b, sum a b^T row-major,
    sum |p' - q|^2; a = p' - centre, b = q - centre): H = sum a b^T - sum a (sum b)^T / n, the SVD with the reflection fix, then
    t = (mean b + centre) - R (mean a + centre).  4 x 4 float64."""
    s = np.asarray(sums, np.float64).reshape(17)
    c = np.asarray(centre, np.float64).reshape(3)
    n = s[0]
    if not n >= 3:
        raise PmnError(f"icp: {int(n)} matched pairs, a rigid motion needs 3")
    sa, sb = s[1:4], s[4:7]
    H = s[7:16].reshape(3, 3) - np.outer(sa, sb) / n
    R, _, _ = _rotation(H)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (sb / n + c) - R @ (sa / n + c)
    return T


# ---- checked wrappers ---------------------------------------------------------------------------------------------------------------

def _pose12(pose, what: str):
    p = np.asarray(pose, np.float64)
    if p.shape == (4, 4):
        if not np.array_equal(p[3], [0.0, 0.0, 0.0, 1.0]):
            raise PmnError(f"{what}: the last row of a 4 x 4 pose must be 0 0 0 1")
        p = p[:3]
    if p.shape != (3, 4) or not np.isfinite(p).all():
        raise PmnError(f"{what}: pose must be a finite 3 x 4 or 4 x 4 matrix, got shape {p.shape}")
    return (ctypes.c_double * 12)(*p.reshape(-1).tolist())


def grid_centre(grid: PC.Grid) -> np.ndarray:
    """Centre of the bounding box of a grid's points, float64 [3]."""
    lo, hi = grid.xyz.min(0).values.double(), grid.xyz.max(0).values.double()
    return ((lo + hi) / 2).cpu().numpy()


def query_order(points: torch.Tensor, grid: PC.Grid, pose=None) -> torch.Tensor:
    """int32 [n]: the points in the order of the grid cells they (under ``pose``) fall into, so that the lanes of a wave walk the same
    cells.  Any order gives the same result."""
    q = points if pose is None else transform(points, pose)
    qc = PC._cells(q, grid.origin, grid.cell).clamp_(-1, max(grid.dims))
    side = max(grid.dims) + 2
    return torch.argsort(((qc[:, 2] + 1) * side + (qc[:, 1] + 1)) * side + (qc[:, 0] + 1)).int()


def icp_accumulate(src: torch.Tensor, grid: PC.Grid, pose, centre, max_dist: float, order: Optional[torch.Tensor] = None,
                   scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pmn_icp_accumulate: float64 [17] on the device (count, sum a, sum b, sum a b^T, sum |p' - q|^2 over the pairs nearer than
    ``max_dist``; include/pmn_hip.h).  ``order``: int32 [n] permutation or None; ``scratch``: int64 [>= _lib.icp_scratch(n)] to reuse."""
    src = PC._points(src, "src")
    n = int(src.shape[0])
    if src.device != grid.xyz.device:
        raise PmnError(f"icp_accumulate: src is on {src.device}, the grid on {grid.xyz.device}")
    if not (max_dist > 0.0 and np.isfinite(max_dist)):
        raise PmnError(f"icp_accumulate: max_dist must be positive and finite, got {max_dist}")
    c = np.asarray(centre, np.float64).reshape(-1)
    if c.shape != (3,) or not np.isfinite(c).all():
        raise PmnError(f"icp_accumulate: centre must be 3 finite numbers, got {c.tolist()}")
    if order is not None and (order.dtype != torch.int32 or order.shape != (n,) or order.device != src.device or not order.is_contiguous()):
        raise PmnError(f"icp_accumulate: order must be a contiguous int32 [{n}] tensor on {src.device}")
    words = _lib.icp_scratch(n)
    if scratch is None:
        scratch = torch.empty(words, dtype=torch.int64, device=src.device)
    elif scratch.dtype != torch.int64 or scratch.numel() < words or scratch.device != src.device or not scratch.is_contiguous():
        raise PmnError(f"icp_accumulate: scratch must be a contiguous int64 tensor of at least {words} elements on {src.device}")
    sums = torch.empty(_lib.ICP_SUMS, dtype=torch.float64, device=src.device)
    with torch.cuda.device(src.device):
        check(_lib.lib().pmn_icp_accumulate(*PC._grid_args(grid), src.data_ptr(), order.data_ptr() if order is not None else None, n,
                                            _pose12(pose, "icp_accumulate"), (ctypes.c_double * 3)(*c.tolist()), float(max_dist),
                                            scratch.data_ptr(), int(scratch.numel()), sums.data_ptr(), PC._stream(src)),
              "pmn_icp_accumulate")
    return sums


def voxel_mean(xyz: torch.Tensor, starts: torch.Tensor, attr: Optional[torch.Tensor] = None):
    """pmn_voxel_mean: the float32 means [m,3] (and [m,C]) of the runs [starts[r], starts[r + 1]) of ``xyz`` (and ``attr``)."""
    xyz = PC._points(xyz, "xyz")
    n = int(xyz.shape[0])
    if starts.dtype != torch.int64 or starts.dim() != 1 or starts.numel() < 2 or starts.device != xyz.device or not starts.is_contiguous():
        raise PmnError("voxel_mean: starts must be a contiguous int64 [m + 1] tensor on the points' device")
    m = int(starts.numel()) - 1
    if int(starts[0]) != 0 or int(starts[-1]) != n or m > n or not bool((starts[1:] > starts[:-1]).all()):
        raise PmnError(f"voxel_mean: starts must increase strictly from 0 to {n}")
    C = 0
    if attr is not None:
        if (not attr.is_cuda or attr.device != xyz.device or attr.dtype != torch.float32 or attr.dim() != 2 or attr.shape[0] != n
                or not attr.is_contiguous() or not 1 <= attr.shape[1] <= _lib.VOXEL_MAX_CHANNELS):
            raise PmnError(f"voxel_mean: attr must be a contiguous float32 [{n}, 1..{_lib.VOXEL_MAX_CHANNELS}] tensor on {xyz.device}")
        C = int(attr.shape[1])
    out = torch.empty(m, 3, dtype=torch.float32, device=xyz.device)
    out_attr = torch.empty(m, C, dtype=torch.float32, device=xyz.device) if C else None
    with torch.cuda.device(xyz.device):
        check(_lib.lib().pmn_voxel_mean(xyz.data_ptr(), attr.data_ptr() if C else None, C, n, starts.data_ptr(), m, out.data_ptr(),
                                        out_attr.data_ptr() if C else None, PC._stream(xyz)), "pmn_voxel_mean")
    return out if attr is None else (out, out_attr)


def crop(points: torch.Tensor, volume: CropVolume, pose=None) -> torch.Tensor:
    """pmn_crop_prism: bool [n], True for the points that (under ``pose``, if given) lie inside ``volume``."""
    points = PC._points(points, "points")
    poly = np.asarray(volume.polygon, np.float64)
    if poly.ndim != 2 or poly.shape[1] != 3 or not 3 <= len(poly) <= _lib.CROP_MAX_VERTICES or not np.isfinite(poly).all():
        raise PmnError(f"crop: the polygon must be finite [3..{_lib.CROP_MAX_VERTICES}][3], got {poly.shape}")
    if volume.axis not in (0, 1, 2):
        raise PmnError(f"crop: axis must be 0, 1 or 2, got {volume.axis}")
    if np.isnan(volume.axis_min) or np.isnan(volume.axis_max):
        raise PmnError("crop: axis_min / axis_max must not be NaN")
    uv = [a for a in (0, 1, 2) if a != volume.axis]
    poly2 = torch.from_numpy(np.ascontiguousarray(poly[:, uv])).to(points.device)
    mask = torch.empty(points.shape[0], dtype=torch.uint8, device=points.device)
    with torch.cuda.device(points.device):
        check(_lib.lib().pmn_crop_prism(points.data_ptr(), int(points.shape[0]), poly2.data_ptr(), len(poly), int(volume.axis),
                                        float(volume.axis_min), float(volume.axis_max),
                                        _pose12(pose, "crop") if pose is not None else None, mask.data_ptr(), PC._stream(points)),
              "pmn_crop_prism")
    return mask.bool()


# ---- clouds -------------------------------------------------------------------------------------------------------------------------

def transform(points: torch.Tensor, pose) -> torch.Tensor:
    """float32 [n,3]: r0 * x + r1 * y + r2 * z + t per row in float64 (the kernels' expression), rounded to float32."""
    P = np.asarray(pose, np.float64)[:3]
    p = points.double()
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    rows = [float(P[r, 0]) * x + float(P[r, 1]) * y + float(P[r, 2]) * z + float(P[r, 3]) for r in range(3)]
    return torch.stack(rows, 1).float().contiguous()


def voxel_downsample(points: torch.Tensor, voxel: float, attr: Optional[torch.Tensor] = None):
    """One point per occupied voxel of side ``voxel``: the mean of the voxel's points (and of their ``attr`` rows), float32.  The
    lattice's corner is min(points) - voxel / 2; voxels come in ascending (z, y, x) order and the points of a voxel are summed in input
    order (the sort by voxel key is stable)."""
    points = PC._points(points, "points")
    voxel = float(voxel)
    if not (voxel > 0.0 and np.isfinite(voxel)):
        raise PmnError(f"voxel_downsample: voxel must be positive and finite, got {voxel}")
    origin = points.min(0).values.double().cpu().numpy() - voxel / 2
    c = PC._cells(points, origin.tolist(), voxel)
    dims = (c.max(0).values + 1).cpu().tolist()
    if max(dims) > 2 ** 30 or dims[0] * dims[1] * dims[2] >= 2 ** 62:
        raise PmnError(f"voxel_downsample: a lattice of {dims} voxels does not fit a 63-bit key; use a larger voxel")
    keys = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    keys, perm = torch.sort(keys, stable=True)
    n = int(points.shape[0])
    first = torch.nonzero(keys[1:] != keys[:-1]).reshape(-1) + 1
    starts = torch.cat([first.new_zeros(1), first, first.new_full((1,), n)]).contiguous()
    return voxel_mean(points[perm].contiguous(), starts, None if attr is None else attr[perm].contiguous())


def thin(points: torch.Tensor, max_points: int) -> torch.Tensor:
    """Every k-th point, k the smallest stride that leaves at most ``max_points``."""
    k = max(1, -(-int(points.shape[0]) // int(max_points)))
    return points[::k].contiguous()


# ---- ICP ----------------------------------------------------------------------------------------------------------------------------

def icp(src: torch.Tensor, grid: PC.Grid, init, max_dist: float, max_iter: int = 20, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6,
        with_scale: bool = False) -> Dict:
    """Point-to-point ICP of ``src`` onto the cloud of ``grid``, from the 4 x 4 pose ``init``.  An iteration is one pmn_icp_accumulate
    call with the target's bounding-box centre, one 17-double download and kabsch_from_sums on the host; the update is composed onto
    the pose.  Stops after ``max_iter`` updates, or when the changes of fitness and of RMSE since the previous iteration are both below
    ``rel_fitness`` / ``rel_rmse`` times the previous value.  Returns pose (4 x 4 float64), fitness (matched / n), rmse (of the matched
    pairs), iterations (updates applied) and history (fitness, rmse per evaluation).  PmnError when fewer than 3 pairs match."""
    if with_scale:
        raise PmnError("icp: with_scale is not supported: the seventeen sums hold no sum of |a|^2 (use umeyama for a similarity)")
    pose = np.array(np.asarray(init, np.float64), copy=True)
    if pose.shape != (4, 4):
        raise PmnError(f"icp: init must be 4 x 4, got {pose.shape}")
    src = PC._points(src, "src")
    n = int(src.shape[0])
    centre = grid_centre(grid)
    order = query_order(src, grid, pose)
    scratch = torch.empty(_lib.icp_scratch(n), dtype=torch.int64, device=src.device)
    history: List[Tuple[float, float]] = []
    updates = 0
    while True:
        s = icp_accumulate(src, grid, pose, centre, max_dist, order, scratch).cpu().numpy()
        if s[0] < 3:
            raise PmnError(f"icp: {int(s[0])} of {n} points have a neighbour within {max_dist}; a rigid motion needs 3 pairs")
        fitness, rmse = float(s[0]) / n, float(np.sqrt(s[16] / s[0]))
        if history:
            pf, pr = history[-1]
            done = abs(fitness - pf) < rel_fitness * pf and abs(rmse - pr) < rel_rmse * pr
        else:
            done = False
        history.append((fitness, rmse))
        if done or updates >= max_iter:
            break
        pose = kabsch_from_sums(s, centre) @ pose
        updates += 1
    return {"pose": pose, "fitness": fitness, "rmse": rmse, "iterations": updates, "history": history}


# ---- the protocol -------------------------------------------------------------------------------------------------------------------

def f_score(d_est: torch.Tensor, d_gt: torch.Tensor, tau: float, hist_max: float, bins: int = HIST_BINS) -> Dict:
    """precision = 100 #{d_est < tau} / #est, recall likewise over d_gt, F = 2 P R / (P + R) (0 when both are 0), and the cumulative
    histograms (percent of the points nearer than each of ``bins`` equal steps up to ``hist_max``)."""
    n_est, n_gt = int(d_est.numel()), int(d_gt.numel())
    hit_est, hit_gt = int((d_est < tau).sum()), int((d_gt < tau).sum())
    P, R = 100.0 * hit_est / n_est, 100.0 * hit_gt / n_gt
    edges = np.linspace(0.0, hist_max, bins + 1)
    e = torch.tensor(edges[1:], dtype=torch.float64, device=d_est.device)

    def cum(d):
        return (100.0 * torch.searchsorted(torch.sort(d).values, e, right=False).double() / d.numel()).cpu().tolist()

    return {"precision": P, "recall": R, "fscore": 2 * P * R / (P + R) if P + R > 0 else 0.0, "n_est": n_est, "n_gt": n_gt,
            "n_est_within_tau": hit_est, "n_gt_within_tau": hit_gt, "hist_edges": edges[1:].tolist(),
            "precision_curve": cum(d_est), "recall_curve": cum(d_gt)}


def _keep(points: torch.Tensor, mask: torch.Tensor, what: str) -> torch.Tensor:
    out = points[mask].contiguous()
    if out.shape[0] < 1:
        raise PmnError(f"tnt_score: no point of {what} lies inside the crop volume")
    return out


def tnt_score(est: torch.Tensor, gt: torch.Tensor, volume: Optional[CropVolume], tau: float, init=None, register: bool = True,
              round_a=ROUND_A, round_b=ROUND_B, round_c_dist: float = ROUND_C_DIST, icp_iterations: int = ICP_ITERATIONS,
              max_points: int = MAX_POINTS, hist_max: Optional[float] = None, bins: int = HIST_BINS,
              return_distances: bool = False, mesh=None):
    """The Tanks and Temples protocol: from the 4 x 4 ``init`` (identity if None) three ICP rounds bring ``est`` into
    the frame of ``gt`` (skipped unless ``register``), then both clouds are cropped, voxel-downsampled at tau / 2 and cropped again, and
    the capped nearest-neighbour distances in both directions give precision, recall and F-score at ``tau``.  ``volume`` None: no crop.
    ``mesh`` = (vertices, faces) of the reconstruction in ``est``'s frame: the ground-truth -> reconstruction leg (recall) is then the
    exact distance to that surface (meshops.point_mesh_distance against the whole mesh, moved by the final pose) and not
    the distance to the nearest point of ``est``; the other leg is unchanged.
    Returns f_score's dict plus pose and rounds (fitness, rmse, iterations per round); with ``return_distances`` also the two float64
    distance tensors."""
    est, gt = PC._points(est, "est"), PC._points(gt, "gt")
    tau = float(tau)
    if not (tau > 0.0 and np.isfinite(tau)):
        raise PmnError(f"tnt_score: tau must be positive and finite, got {tau}")
    hist_max = HIST_MAX_TAU * tau if hist_max is None else float(hist_max)
    pose = np.eye(4) if init is None else np.array(np.asarray(init, np.float64), copy=True)
    if pose.shape != (4, 4):
        raise PmnError(f"tnt_score: init must be 4 x 4, got {pose.shape}")

    def cropped(points, what):
        return points if volume is None else _keep(points, crop(points, volume), what)

    gt_c = cropped(gt, "the ground truth")
    rounds = []
    if register:
        for name, voxel, dist in (("A", round_a[0] * tau, round_a[1] * tau), ("B", round_b[0] * tau, round_b[1] * tau),
                                  ("C", None, round_c_dist * tau)):
            moved = cropped(transform(est, pose), "the reconstruction")
            if voxel is None:
                source, target, spacing = thin(moved, max_points), thin(gt_c, max_points), tau
            else:
                source, target, spacing = voxel_downsample(moved, voxel), voxel_downsample(gt_c, voxel), voxel
            cell = max(2.0 * spacing, dist / ICP_CELL_DIVISOR)
            r = icp(source, PC.build_grid(target, cell), np.eye(4), dist, max_iter=icp_iterations)
            pose = r["pose"] @ pose
            rounds.append({"round": name, "fitness": r["fitness"], "rmse": r["rmse"], "iterations": r["iterations"],
                           "n_source": int(source.shape[0]), "n_target": int(target.shape[0])})

    def prepared(points, what):
        return cropped(voxel_downsample(cropped(points, what), tau / 2), what)

    est_s, gt_s = prepared(transform(est, pose), "the reconstruction"), prepared(gt, "the ground truth")
    d_est = PC.nn_distance(est_s, PC.build_grid(gt_s, tau), hist_max)
    if mesh is None:
        d_gt = PC.nn_distance(gt_s, PC.build_grid(est_s, tau), hist_max)
    else:
        from . import meshops
        d_gt = meshops.point_mesh_distance(gt_s, meshops.build_face_grid(transform(mesh[0], pose), mesh[1]), hist_max)
    out = f_score(d_est, d_gt, tau, hist_max, bins)
    out.update({"tau": tau, "pose": pose.tolist(), "rounds": rounds})
    return (out, d_est, d_gt) if return_distances else out
