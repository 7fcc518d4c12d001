"""The camera space: one row per rig that feeds pmn_stage_projections and the warp (pmn_differentiable_warping, the gather kernels),
with the yardsticks the tests read them against.  Every rig of the rest of the suite is DTU (f ~ 2892 W / 1600, cameras a few degrees
apart, looking at (0, 0, 650)); the rows here are what COLMAP imports and Tanks and Temples bring: scenes of unit scale, world origins
far from the cameras, inward-facing rings with a source camera inside the reference's depth range, reference cameras turned by 90 and
180 degrees in the world (every pivot order of the 4x4 inverse), rolled cameras, skewed / cropped intrinsics and source maps of other
sizes than the reference's.

Conventions.  Intrinsics are given for a reference image of (H0, W0) = (24, 32) / scale0 pixels, so that the coarsest stage's map is
24 x 32; stage s scales rows 0, 1 by scale0 * 2**s (net.py:225-231).  The warp tests use a 24 x 32 reference map at every stage: at
stage s > 0 that is the central window of the stage's map, every view cropped alike (`cropped`: the principal points move by the
window's offset, as they do for a cropped image; the top-left window would look past every source).  A source view's map is (round(h * rh), round(w * rw)) for its ratio
(rh, rw): the source projection addresses pixels of a map as large as the reference's, and grid_sample rescales to the map it is
given (module.py:170-181).

Plain helper module (no tests here): tests/test_camera_space.py checks the table on the CPU (the reference alone meets every
condition the GPU tests lean on), tests/test_camera_space_gpu.py runs it on the device, tests/kernel_space.py takes rig rows from it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Dict, List, Tuple

import numpy as np

import ref64 as R

H_MAP, W_MAP, D_MAP = 24, 32, 8      # the warp tests' reference map and hypothesis count
CLASSES = ("inside", "border", "outside", "behind")

# The pivot rows Gauss-Jordan with partial pivoting can choose for columns 0 and 1 of a projection whose last row is (0, 0, 0, 1):
# row 3 has zeros in columns 0..2, so column 0 picks among rows 0..2, column 1 among rows 1, 2, and columns 2, 3 have no choice.
PATTERNS = tuple((a, b, 2, 3) for a in (0, 1, 2) for b in (1, 2))


@dataclass(frozen=True)
class Rig:
    name: str
    intrinsics: np.ndarray          # [B,V,3,3] float32, view 0 = reference
    extrinsics: np.ndarray          # [B,V,4,4] float32
    depth_min: np.ndarray           # [B] float32
    depth_max: np.ndarray           # [B] float32
    ratios: Tuple[Tuple[float, float], ...]  # per view (rh, rw): map size relative to the reference's (view 0: (1, 1))
    nstages: int = 3
    scale0: float = 0.125
    shares: Dict[str, float] = field(default_factory=dict)  # class -> the minimum share of samples tests/test_camera_space.py asserts

    @property
    def B(self) -> int:
        return self.intrinsics.shape[0]

    @property
    def V(self) -> int:
        return self.intrinsics.shape[1]

    def scales(self) -> List[float]:
        return [self.scale0 * 2.0 ** s for s in range(self.nstages)]

    def map_size(self, v: int, h: int = H_MAP, w: int = W_MAP) -> Tuple[int, int]:
        rh, rw = self.ratios[v]
        return max(2, int(round(h * rh))), max(2, int(round(w * rw)))


# ---- building blocks ------------------------------------------------------------------------------------------------------------------

def _rot(axis: str, deg: float) -> np.ndarray:
    a = math.radians(deg)
    c, s = round(math.cos(a), 15), round(math.sin(a), 15)  # (quarter and half turns: exact zeros, not 6e-17)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis].astype(np.float64)


def look_at(C, target, roll_deg: float = 0.0) -> np.ndarray:
    """World-to-camera [4,4] of a camera at C looking at ``target`` (x right, y down, z forward), rolled about its axis."""
    C, target = np.asarray(C, np.float64), np.asarray(target, np.float64)
    z = target - C
    z /= np.linalg.norm(z)
    up = np.array([0.0, -1.0, 0.0]) if abs(z[1]) < 0.99 else np.array([0.0, 0.0, 1.0])
    x = np.cross(-up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = _rot("z", roll_deg) @ np.stack([x, y, z])
    E = np.eye(4)
    E[:3, :3] = Rm
    E[:3, 3] = -Rm @ C
    return E


def _K(f, W0, H0, fy=None, skew=0.0, cx=None, cy=None) -> np.ndarray:
    return np.array([[f, skew, W0 / 2.0 if cx is None else cx], [0, f if fy is None else fy, H0 / 2.0 if cy is None else cy],
                     [0, 0, 1]], np.float64)


def _pack(name, Ks, Es, dmin, dmax, ratios, **kw) -> Rig:
    intr = np.asarray(Ks, np.float64).astype(np.float32)
    extr = np.asarray(Es, np.float64).astype(np.float32)
    B = intr.shape[0]
    return Rig(name, intr, extr, np.full(B, dmin, np.float32) if np.isscalar(dmin) else np.asarray(dmin, np.float32),
               np.full(B, dmax, np.float32) if np.isscalar(dmax) else np.asarray(dmax, np.float32), tuple(ratios), **kw)


def _scene(rng, V, scale, base_lo, base_hi, target_z, f_rel=0.8, scale0=0.125, jitter=0.05):
    """A reference camera at the origin looking down +z and V - 1 sources ``base_lo .. base_hi`` away from it in seeded directions
    (x, y and a little z), looking at (0, 0, target_z) with seeded jitter and roll.  f = f_rel * W0."""
    W0, H0 = W_MAP / scale0, H_MAP / scale0
    Ks, Es = [], []
    for v in range(V):
        if v == 0:
            C, roll = np.zeros(3), 0.0
        else:
            d = rng.standard_normal(3) * np.array([1.0, 0.6, 0.25])
            C = d / np.linalg.norm(d) * rng.uniform(base_lo, base_hi) * scale
            roll = rng.uniform(-8.0, 8.0)
        tgt = np.array([0.0, 0.0, target_z * scale]) + (jitter * scale * rng.standard_normal(3) if v else 0.0)
        Es.append(look_at(C, tgt, roll))
        Ks.append(_K(f_rel * W0 * (1.0 + (0.03 * rng.standard_normal() if v else 0.0)), W0, H0))
    return Ks, Es


def _shift_world(Es, T) -> List[np.ndarray]:
    """The same cameras in a world whose origin is moved by -T: X_world' = X_world + T."""
    out = []
    for E in Es:
        E2 = E.copy()
        E2[:3, 3] = E[:3, 3] - E[:3, :3] @ np.asarray(T, np.float64)
        out.append(E2)
    return out


def _turn_world(Es, Q) -> List[np.ndarray]:
    """The same cameras in a world rotated by Q: X_world' = Q X_world (every camera's rotation becomes R Q^T)."""
    out = []
    for E in Es:
        E2 = E.copy()
        E2[:3, :3] = E[:3, :3] @ Q.T
        out.append(E2)
    return out


def pivot_pattern(P_ref: np.ndarray) -> Tuple[int, int, int, int]:
    """The pivot row stage_projections_kernel's Gauss-Jordan picks for each column of the float32 P_ref: the first row (at or below
    the diagonal) of strictly largest magnitude, in float64.  Rows are numbered as they stand when the column is reached (the
    kernel's `piv`)."""
    A = np.asarray(np.asarray(P_ref, np.float32), np.float64).copy()
    out = []
    for col in range(4):
        piv = col
        for r in range(col + 1, 4):
            if abs(A[r, col]) > abs(A[piv, col]):
                piv = r
        A[[col, piv]] = A[[piv, col]]
        out.append(piv)
        A[col] /= A[col, col]
        for r in range(4):
            if r != col:
                A[r] -= A[r, col] * A[col]
    return tuple(out)


def swaps(P_ref: np.ndarray) -> Tuple[Tuple[int, int], ...]:
    """The (column, row) exchanges the kernel's predicated swaps perform for P_ref: `sw` of (col, r) is true exactly for these."""
    A = np.asarray(np.asarray(P_ref, np.float32), np.float64).copy()
    out = []
    for col in range(4):
        piv = col
        for r in range(col + 1, 4):
            if abs(A[r, col]) > abs(A[piv, col]):
                piv = r
        if piv != col:
            out.append((col, piv))
        A[[col, piv]] = A[[piv, col]]
        A[col] /= A[col, col]
        for r in range(4):
            if r != col:
                A[r] -= A[r, col] * A[col]
    return tuple(out)


# ---- the rigs -------------------------------------------------------------------------------------------------------------------------

def _dtu() -> Rig:
    import synth
    intr, extr = synth.general_cameras(5, int(H_MAP / 0.125), int(W_MAP / 0.125))
    return Rig("dtu", intr, extr, np.float32([425.0]), np.float32([935.0]), ((1.0, 1.0),) * 5,
               shares={"inside": 0.5, "border": 0.02, "outside": 0.2})


def _unit() -> Rig:
    Ks, Es = [], []
    for b in range(2):  # two samples that differ: seeds, baselines and focal lengths
        rng = np.random.default_rng(11 + b)
        k, e = _scene(rng, 3, 1.0, 0.3, 1.0, 3.0 + b, f_rel=0.8 + 0.1 * b)
        Ks.append(k)
        Es.append(e)
    return _pack("unit", Ks, Es, 0.5, 8.0, ((1.0, 1.0),) * 3, shares={"inside": 0.4, "border": 0.02, "outside": 0.3})


FAR_SHIFT = (1.0e3, -2.0e3, 5.0e2)


def _far_origin() -> Rig:
    rng = np.random.default_rng(11)
    Ks, Es = _scene(rng, 3, 1.0, 0.3, 1.0, 3.0)
    return _pack("far_origin", [Ks], [_shift_world(Es, FAR_SHIFT)], 0.5, 8.0, ((1.0, 1.0),) * 3,
                 shares={"inside": 0.4, "border": 0.02, "outside": 0.3})


def _ring() -> Rig:
    """8 cameras (f = 0.4 W) on a circle of radius 3 in the x-z plane looking at its centre; the one opposite the reference is pulled in to
    radius 1.5, so it stands at depth 4.5 of the reference's range 0.5 .. 6 and looks straight back at it."""
    rng = np.random.default_rng(7)
    scale0 = 0.125
    W0, H0 = W_MAP / scale0, H_MAP / scale0
    Ks, Es = [], []
    for i in range(8):
        th = math.radians(45.0 * i)
        rad = 1.5 if i == 4 else 3.0
        C = np.array([rad * math.sin(th), 0.15 * rng.standard_normal() if i else 0.0, -rad * math.cos(th)])
        Es.append(look_at(C, 0.05 * rng.standard_normal(3) if i else np.zeros(3), rng.uniform(-5, 5) if i else 0.0))
        Ks.append(_K(0.4 * W0, W0, H0))
    return _pack("ring", [Ks], [Es], 0.5, 6.0, ((1.0, 1.0),) * 8, nstages=4,
                 shares={"inside": 0.3, "border": 0.02, "outside": 0.3, "behind": 0.02})


# Rotations of the world for rig `turned` (X_world' = Q X_world: the reference camera's rotation becomes Q^T), two per pivot pattern.
# With P = K_s [R | t] over (0, 0, 0, 1), K_s the intrinsics at the stage's scale (f = 25.6, principal point (16, 12)):
#  * column 0 takes row 1 when the camera is rolled by a quarter turn (|P10| > |P00|);
#  * column 0 takes row 2 when the world's x axis vanishes within a pixel of the image origin, K_s R[:, 0] ~ (0, 0, 1): the camera
#    yawed by about a quarter turn and turned further by half its field of view;
#  * column 1 takes row 2 when, after the elimination of column 0, the minor of rows 0, 1 is the smaller one: the world's z axis lies
#    nearly in the image plane, K_s^-T R[:, 2] with a third component below 1 / f (the camera pitched, or yawed, by a quarter turn
#    less the angle of the principal point).
# ("turn", ((axis, degrees), ...)): turns applied left to right.  ("x_at", (px, py, phi)): the world's x axis vanishes at pixel
# (px, py), the rest turned by phi about it.  ("z_in", (axis, dz, phi)): the world's z axis along the camera's ``axis`` tilted to
# that plane (dz: how far off), the rest turned by phi about it.  tests/test_camera_space.py asserts the pattern each one gives.
TURNS = (
    ((0, 1, 2, 3), "turn", (("y", 180.0),)),
    ((0, 1, 2, 3), "turn", (("x", 180.0), ("z", 7.0))),
    ((1, 1, 2, 3), "turn", (("z", 90.0),)),
    ((1, 1, 2, 3), "turn", (("z", -90.0), ("y", 180.0))),
    ((0, 2, 2, 3), "z_in", ("y", 0.0, 0.0)),
    ((0, 2, 2, 3), "z_in", ("y", 0.02, 120.0)),
    ((1, 2, 2, 3), "z_in", ("x", 0.0, 30.0)),
    ((1, 2, 2, 3), "z_in", ("x", 0.02, 200.0)),
    ((2, 1, 2, 3), "x_at", (0.3, -0.4, 90.0)),
    ((2, 1, 2, 3), "x_at", (-0.5, 0.2, 270.0)),
    ((2, 2, 2, 3), "x_at", (0.3, -0.4, 0.0)),
    ((2, 2, 2, 3), "x_at", (-0.5, 0.2, 180.0)),
)
TURNED_SCALE0 = 0.25


def _frame(c, phi_deg: float, pole) -> np.ndarray:
    """Unit vectors (a, b) completing c to a right-handed frame a x b = c, turned by phi about c."""
    a0 = np.cross(pole, c)
    a0 /= np.linalg.norm(a0)
    b0 = np.cross(c, a0)
    phi = math.radians(phi_deg)
    a = math.cos(phi) * a0 + math.sin(phi) * b0
    return a, np.cross(c, a)


def turn_matrix(kind: str, params) -> np.ndarray:
    W0, H0 = W_MAP / TURNED_SCALE0, H_MAP / TURNED_SCALE0
    f, cx, cy = 0.8 * W0 * TURNED_SCALE0, W0 / 2.0 * TURNED_SCALE0, H0 / 2.0 * TURNED_SCALE0
    if kind == "turn":
        Q = np.eye(3)
        for axis, deg in params:
            Q = _rot(axis, deg) @ Q
        return Q
    if kind == "x_at":
        px, py, phi = params
        u = np.array([(px - cx) / f, (py - cy) / f, 1.0])
        u /= np.linalg.norm(u)
        v, n = _frame(u, phi, np.array([0.0, 1.0, 0.0]))  # rows (u, v, u x v)
        return np.stack([u, v, n])
    if kind == "z_in":
        axis, dz, phi = params
        c = np.array([1.0, 0.0, cx / f + dz]) if axis == "x" else np.array([0.0, 1.0, cy / f + dz])
        c /= np.linalg.norm(c)
        a, b = _frame(c, phi, np.array([0.0, 0.0, 1.0]))  # rows (a, b, c)
        return np.stack([a, b, c])
    raise ValueError(kind)


def _turned() -> Rig:
    Ks, Es = [], []
    for b, (_pat, kind, params) in enumerate(TURNS):
        rng = np.random.default_rng(40 + b)
        k, e = _scene(rng, 2, 1.0, 0.3, 1.0, 3.0, scale0=TURNED_SCALE0)
        Ks.append(k)
        Es.append(_turn_world(e, turn_matrix(kind, params)))
    return _pack("turned", Ks, Es, 0.5, 8.0, ((1.0, 1.0),) * 2, nstages=1, scale0=TURNED_SCALE0,
                 shares={"inside": 0.5, "border": 0.02, "outside": 0.2})


def _mixed() -> Rig:
    """Per-view fx != fy, skew, principal points outside the centre third (cropped images), source maps half, one and a half and
    (0.75, 1.25) times the reference's, and source 1 two units in FRONT of the reference, looking back at it."""
    rng = np.random.default_rng(28)
    scale0 = 0.125
    W0, H0 = W_MAP / scale0, H_MAP / scale0
    Ks, Es = _scene(rng, 4, 1.0, 0.4, 0.9, 3.0)
    Es[1] = look_at(np.array([0.3, -0.2, 2.0]), np.array([0.1, 0.0, -1.0]), 4.0)
    pp = ((0.22, 0.75), (0.8, 0.2), (0.15, 0.3), (0.7, 0.85))
    for v in range(4):
        fx = 0.8 * W0 * (1.0 + 0.1 * v)
        Ks[v] = _K(fx, W0, H0, fy=fx * (0.85 + 0.1 * v), skew=0.02 * fx * (-1) ** v, cx=pp[v][0] * W0, cy=pp[v][1] * H0)
    return _pack("mixed", [Ks], [Es], 0.5, 8.0, ((1.0, 1.0), (0.5, 0.5), (1.5, 1.5), (0.75, 1.25)),
                 shares={"inside": 0.05, "border": 0.02, "outside": 0.5, "behind": 0.1})


def _wide() -> Rig:
    Ks, Es = [], []
    for b in range(2):
        rng = np.random.default_rng(31 + b)
        k, e = _scene(rng, 11, 30.0, 0.02, 5.0 / 3.0 / 30.0, 1.0 + 0.5 * b, jitter=0.02)
        Ks.append(k)
        Es.append(e)
    return _pack("wide", Ks, Es, 5.0, 200.0, ((1.0, 1.0),) * 11, nstages=4,
                 shares={"inside": 0.5, "border": 0.02, "outside": 0.1})


@lru_cache(maxsize=None)
def rigs() -> Dict[str, Rig]:
    return {r.name: r for r in (_dtu(), _unit(), _far_origin(), _ring(), _turned(), _mixed(), _wide())}


RIG_NAMES = ("dtu", "unit", "far_origin", "ring", "turned", "mixed", "wide")


# ---- yardsticks -------------------------------------------------------------------------------------------------------------------------

def stage_proj(rig: Rig, scale: float, dtype=np.float64, intr=None) -> np.ndarray:
    """net.py:225-229 on the rig's float32 inputs, every operation in ``dtype``: proj [B,V,4,4] with proj[:3,:4] = (K, rows 0 and 1
    scaled) @ E[:3,:4]."""
    K = np.array(rig.intrinsics if intr is None else intr, dtype)
    E = np.array(rig.extrinsics, dtype)
    K[:, :, :2] = K[:, :, :2] * np.dtype(dtype).type(scale)
    proj = E.copy()
    # the product term by term, k ascending, every operation rounded once (a BLAS matmul may fuse or reorder: an ulp of P_ref, which
    # an entry of its inverse that is a cancellation -- a turned camera has them -- shows at full size)
    Ke, Ee = K[:, :, :, :, None], E[:, :, None, :3, :4]
    proj[:, :, :3, :4] = (Ke[:, :, :, 0] * Ee[:, :, :, 0] + Ke[:, :, :, 1] * Ee[:, :, :, 1]) + Ke[:, :, :, 2] * Ee[:, :, :, 2]
    return proj


def projections(rig: Rig, scale: float, dtype=np.float64, intr=None) -> np.ndarray:
    """The reference's sequence (net.py:225-231, module.py:148) -> rel [B,V-1,4,4] = proj_src @ inverse(proj_ref), in ``dtype``:
    float32 runs the reference's own operations (np.linalg.inv on float32 is LAPACK's sgesv, as torch.inverse), float64 the same
    on the same float32 inputs."""
    proj = stage_proj(rig, scale, dtype, intr)
    inv = np.linalg.inv(proj[:, 0])
    assert inv.dtype == np.dtype(dtype)
    return np.stack([np.matmul(proj[:, v], inv) for v in range(1, rig.V)], 1)


def positions(P, depth, h: int, w: int, hs: int, ws: int, dtype=np.float64, xy=None):
    """module.py:161-181 in ``dtype`` -> (ix, iy, front) [D,h,w]: ref64.warp_positions, which also returns what it decided.
    ``xy``: reference pixels (x, y) of depth's shape instead of the h x w grid."""
    ix, iy, det = R.warp_positions(P, depth, h, w, hs, ws, dtype=dtype, details=True, xy=xy)
    return ix, iy, det["front"]


def cropped(rig: Rig, stage: int, h: int = H_MAP, w: int = W_MAP) -> np.ndarray:
    """The rig's float32 intrinsics with every view cropped to the central h x w window of stage ``stage``'s map (h 2**s x w 2**s):
    the principal point moves by the window's offset, given at full resolution (an exact float32 operand at these sizes)."""
    intr = rig.intrinsics.copy()
    scale = rig.scales()[stage]
    intr[:, :, 0, 2] -= np.float32((w * 2 ** stage - w) / 2.0 / scale)
    intr[:, :, 1, 2] -= np.float32((h * 2 ** stage - h) / 2.0 / scale)
    return intr


def ramps(hs: int, ws: int) -> np.ndarray:
    """[3,hs,ws] float32: x index, y index, ones.  Bilinear sampling with zero padding gives (sum w x, sum w y, sum w): the
    position the kernel sampled at and the weight of the taps that survived."""
    y, x = np.meshgrid(np.arange(hs, dtype=np.float32), np.arange(ws, dtype=np.float32), indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, np.ones_like(x)]))


def hypotheses(rig: Rig, b: int, D: int = D_MAP, h: int = H_MAP, w: int = W_MAP, seed: int = 0) -> np.ndarray:
    """[D,h,w] float32 depths spread over the sample's range: level k sits at fraction (k + u) / D of it, u seeded per pixel; even
    levels are spaced in depth, odd ones in inverse depth."""
    rng = np.random.default_rng(1000 * seed + 17 * b + sum(map(ord, rig.name)))
    lo, hi = float(rig.depth_min[b]), float(rig.depth_max[b])
    f = (np.arange(D).reshape(D, 1, 1) + rng.random((D, h, w))) / D
    lin = lo + f * (hi - lo)
    inv = 1.0 / (1.0 / hi + f * (1.0 / lo - 1.0 / hi))
    return np.where((np.arange(D) % 2 == 0).reshape(D, 1, 1), lin, inv).astype(np.float32)


def classify(ix, iy, front, hs: int, ws: int) -> Dict[str, np.ndarray]:
    """Masks of the four sample classes (float64 positions): all four taps inside the map; exactly one tap row OR column outside;
    no tap inside; behind the camera.  (A sample with a row AND a column outside is in none.)"""
    x0, y0 = np.floor(ix), np.floor(iy)
    xin = (x0 >= 0) & (x0 + 1 <= ws - 1)
    yin = (y0 >= 0) & (y0 + 1 <= hs - 1)
    xedge = (x0 == -1) | (x0 == ws - 1)
    yedge = (y0 == -1) | (y0 == hs - 1)
    xout = (x0 < -1) | (x0 > ws - 1)
    yout = (y0 < -1) | (y0 > hs - 1)
    return {"inside": front & xin & yin, "border": front & ((xedge & yin) | (xin & yedge)), "outside": front & (xout | yout),
            "behind": ~front}


@dataclass
class WarpCase:
    """One call of the warp: rig, stage, source view -> everything the tests compare, for all B samples."""
    stage: int
    view: int
    h: int
    w: int
    hs: int
    ws: int
    P: np.ndarray        # [B,4,4] float32: the float32 restatement's relative projection (what the kernel is given)
    depth: np.ndarray    # [B,D,h,w] float32
    pos64: tuple         # (ix, iy, front, pz) [B,D,h,w], float64 operations
    pos32: tuple         # the same in float32
    want: np.ndarray     # [B,3,D,h,w] float64 bilinear sampling of the ramps at pos64
    ref32: np.ndarray    # [B,3,D,h,w] the float32 restatement: float32 positions, float32 bilinear
    near: np.ndarray     # [B,D,h,w] samples whose float64 pz is within the restatements' largest pz difference of 1e-3


def _pos(P, depth, h, w, hs, ws, dtype):
    out = []
    for b in range(P.shape[0]):
        ix, iy, det = R.warp_positions(P[b], depth[b], h, w, hs, ws, dtype=dtype, details=True)
        out.append((ix, iy, det["front"], det["pz"]))
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def _plant_front_crossings(P, depth, rig) -> None:
    """Row h // 2 of hypothesis level 1 gets, where the range allows it, the depth at which the pixel's ray meets pz = 1e-3 in the
    source camera, moved by -3 .. +12 float32 steps along the row: pz a few 1e-7 on both sides of the front test, positions of
    1e4 - 1e5 px on the front side."""
    B, D, h, w = depth.shape
    y = h // 2
    for b in range(B):
        Pb = P[b].astype(np.float64)
        x = np.arange(w, dtype=np.float64)
        rz = Pb[2, 0] * x + Pb[2, 1] * y + Pb[2, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            d0 = ((1e-3 - Pb[2, 3]) / rz).astype(np.float32)
        ok = np.isfinite(d0) & (d0 > rig.depth_min[b]) & (d0 < rig.depth_max[b])
        steps = (np.arange(w) % 16 - 3).astype(np.float32)
        d = d0 + steps * np.spacing(d0)
        depth[b, 1, y, ok] = d[ok]


def warp_case(rig: Rig, stage: int, view: int, h: int = H_MAP, w: int = W_MAP, D: int = D_MAP, scale=None) -> WarpCase:
    """``scale``: the whole image at that scale on an h x w map (the large rows) instead of stage ``stage``'s central window."""
    hs, ws = rig.map_size(view, h, w)
    if scale is None:
        P = projections(rig, rig.scales()[stage], np.float32, cropped(rig, stage, h, w))[:, view - 1]
    else:
        P = projections(rig, scale, np.float32)[:, view - 1]
    depth = np.stack([hypotheses(rig, b, D, h, w, seed=stage) for b in range(rig.B)])
    if rig.name == "ring":
        _plant_front_crossings(P, depth, rig)
    p64, p32 = _pos(P, depth, h, w, hs, ws, np.float64), _pos(P, depth, h, w, hs, ws, np.float32)
    src = ramps(hs, ws)
    want = np.stack([R.bilinear(src, p64[0][b], p64[1][b]) for b in range(rig.B)])
    ref32 = np.stack([R.bilinear(src, p32[0][b], p32[1][b], dtype=np.float32) for b in range(rig.B)])
    with np.errstate(invalid="ignore"):
        dz = np.abs(p32[3].astype(np.float64) - p64[3])
    near = np.abs(p64[3] - 1e-3) <= (dz.max() if dz.size else 0.0)
    return WarpCase(stage, view, h, w, hs, ws, P, depth, p64, p32, want, ref32, near)


LARGE = ("dtu", "far_origin")      # rigs that also run once at 296 x 400 with 4 hypotheses: fp32 position error grows with the coordinate
H_LARGE, W_LARGE, D_LARGE = 296, 400, 4


@lru_cache(maxsize=None)
def large_case(name: str) -> WarpCase:
    rig = rigs()[name]
    return warp_case(rig, 0, 1, H_LARGE, W_LARGE, D_LARGE, scale=W_LARGE * rig.scale0 / W_MAP)


@lru_cache(maxsize=None)
def warp_cases(name: str) -> Tuple[WarpCase, ...]:
    """Every (stage, source view) of the rig at the 24 x 32 map, computed once."""
    rig = rigs()[name]
    return tuple(warp_case(rig, s, v) for s in range(rig.nstages) for v in range(1, rig.V))


def position_error(a: tuple, b: tuple, hs: int, ws: int, mask=None) -> float:
    """Largest difference in source pixels between two position sets (ix, iy, front, ...) over samples both call front and that lie
    within one map size of the source image in ``b`` (further out no tap is reached and fp32 positions of 1e6 px carry errors of
    pixels that change nothing)."""
    ok = a[2] & b[2] & (b[0] > -ws) & (b[0] < 2 * ws) & (b[1] > -hs) & (b[1] < 2 * hs)
    if mask is not None:
        ok = ok & mask
    if not ok.any():
        return 0.0
    return float(max(np.abs(a[0].astype(np.float64) - b[0])[ok].max(), np.abs(a[1].astype(np.float64) - b[1])[ok].max()))


# ---- pmn_stage_projections by what it is for: where a reference pixel lands in the source image ----------------------------------------

def projection_samples(rig: Rig, stage: int, n: int = 512, D: int = 8):
    """Seeded reference pixels (x, y) [D,n] over stage ``stage``'s whole map (h 2**s x w 2**s, sub-pixel positions included) and
    depths [B,D,n] spanning each sample's range."""
    rng = np.random.default_rng(77 + stage + sum(map(ord, rig.name)))
    h, w = H_MAP * 2 ** stage, W_MAP * 2 ** stage
    x = np.broadcast_to(rng.uniform(0, w - 1, n).astype(np.float32), (D, n))
    y = np.broadcast_to(rng.uniform(0, h - 1, n).astype(np.float32), (D, n))
    f = (np.arange(D).reshape(D, 1) + rng.random((D, n))) / D
    lo, hi = rig.depth_min.astype(np.float64).reshape(-1, 1, 1), rig.depth_max.astype(np.float64).reshape(-1, 1, 1)
    return (x, y), (lo + f * (hi - lo)).astype(np.float32), h, w


def projection_error(rel: np.ndarray, rig: Rig, stage: int) -> float:
    """Largest difference in source pixels between where ``rel`` [B,V-1,4,4] and the float64 projections send projection_samples,
    both through float64 positions, over samples that are front and within one map size of the source image."""
    want = projections(rig, rig.scales()[stage], np.float64)
    xy, depth, h, w = projection_samples(rig, stage)
    worst = 0.0
    for b in range(rig.B):
        for v in range(1, rig.V):
            hs, ws = rig.map_size(v, h, w)
            a = positions(rel[b, v - 1], depth[b], h, w, hs, ws, np.float64, xy)
            t = positions(want[b, v - 1], depth[b], h, w, hs, ws, np.float64, xy)
            worst = max(worst, position_error(a, t, hs, ws))
    return worst


# ---- the kernel's inverse, restated (for reasoning about its swaps on the CPU) ------------------------------------------------------------

def gauss_jordan_port(P_ref: np.ndarray, negate=None) -> np.ndarray:
    """stage_projections_kernel's inverse of the float32 P_ref, operation by operation in float64, rounded to float32: per column
    the first row of strictly largest magnitude, the exchange as predicated swaps `sw = (piv == r)` for r = col+1 .. 3, scaling,
    elimination.  ``negate`` = (col, r): that one `sw` negated."""
    A = np.zeros((4, 8))
    A[:, :4] = np.asarray(P_ref, np.float32).astype(np.float64)
    A[:, 4:] = np.eye(4)
    with np.errstate(all="ignore"):
        for col in range(4):
            piv = col
            for r in range(col + 1, 4):
                if abs(A[r, col]) > abs(A[piv, col]):
                    piv = r
            for r in range(col + 1, 4):
                sw = piv == r
                if negate == (col, r):
                    sw = not sw
                if sw:
                    A[[col, r]] = A[[r, col]]
            A[col] = A[col] * (1.0 / A[col, col])
            for r in range(4):
                if r != col:
                    A[r] = A[r] - A[r, col] * A[col]
        return A[:, 4:].astype(np.float32)


SW_CONDITIONS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def exact_inverse(P: np.ndarray) -> np.ndarray:
    """The inverse of the float32 matrix in rational arithmetic, rounded once to float64.  (np.linalg.inv in float64 leaves ~1e-19
    where an entry of a turned camera's inverse is exactly zero; the kernel's inverse has a true zero there, and one float32 ulp of
    1e-19 would then be the bound: the yardstick has to be better than what it measures.)"""
    from fractions import Fraction
    A = [[Fraction(float(np.float32(P[i, j]))) for j in range(4)] + [Fraction(int(i == j)) for j in range(4)] for i in range(4)]
    for c in range(4):
        p = next(r for r in range(c, 4) if A[r][c] != 0)
        A[c], A[p] = A[p], A[c]
        inv = 1 / A[c][c]
        A[c] = [x * inv for x in A[c]]
        for r in range(4):
            if r != c and A[r][c] != 0:
                f = A[r][c]
                A[r] = [x - f * y for x, y in zip(A[r], A[c])]
    return np.array([[float(A[i][4 + j]) for j in range(4)] for i in range(4)], np.float64)


def inverse_gate(got: np.ndarray, P_ref: np.ndarray):
    """(worst ratio, passes): ``got`` against the inverse of the float32 P_ref (exact, rounded to float64) entry by entry; an entry
    may differ by 4 x the float32 LAPACK inverse's own error there, at least one float32 ulp of the entry."""
    P32 = np.asarray(P_ref, np.float32)
    want = exact_inverse(P32)
    lapack = np.linalg.inv(P32).astype(np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    bound = np.maximum(4.0 * np.abs(lapack - want), ulp)
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(got, np.float64) - want)
    d = np.where(np.isfinite(d), d, np.inf)
    return float((d / bound).max()), bool((d <= bound).all())


def pivot_cases():
    """pattern -> (b of rig `turned` with that pattern, ...): the samples test (b) observes the kernel's inverse on."""
    rig = rigs()["turned"]
    P = stage_proj(rig, rig.scale0, np.float32)
    out: Dict[tuple, list] = {}
    for b in range(rig.B):
        out.setdefault(pivot_pattern(P[b, 0]), []).append(b)
    return out
