"""The mesher space: one row per input of the TSDF mesher (csrc/tsdf.hip, DESIGN.md sections 15 and 18) at the places where such kernels
go wrong and smooth fields never go.  Extraction rows (ExtractRow) feed pmn_mt_count / pmn_mt_emit and their pool twins: a lattice that
holds each of the 256 corner patterns in a cell of its own, in three orientations; uniform noise with +-0, float32 denormals and the
clamp values +-1 planted; the same with weights on, one ulp below and above min_weight and NaN; colours on the rounding and clamp
boundaries with cweight zero on either end; lattices of one sample, one cell, thin slabs, sides off and on the 64 x 4 workgroup and
the 8^3 block; fields without a surface.  Integration rows (ExactRow) feed pmn_tsdf_integrate and pmn_tsdf_integrate_blocks rigs in
which every number is a small dyadic rational, so that float32 and float64 take the same decisions and give the same values, and every
comparison of tsdf_fold_sample is met with equality: pc.z == 0, projections on pixel borders, fx == w, fx == -1, sdf == -trunc and
sdf == +trunc.

Plain helper module (no tests here): tests/test_mesher_space.py checks the table on the CPU against the oracle tests/tsdf_ref.py alone
(coverage of every pattern, value and event; exactness of the ExactRows), tests/test_mesher_space_gpu.py runs every row on the device.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List, Tuple

import numpy as np

import tsdf_ref as R

F = np.float32
OFF_ORIGIN, OFF_VOXEL = (-3.25, 100.5, 0.125), 0.37  # the off-origin lattice of tests/test_tsdf_gpu.py
NOISE_DIMS = (17, 13, 11)
# planted sample values: both zeros, the smallest denormals, a larger denormal, the clamp values
SPECIALS = tuple(F(s) for s in ("0.0", "-0.0", "1e-45", "-1e-45", "-1e-39", "1.0", "-1.0"))
# planted (lo, hi) pairs along x: both ends on the clamp, both ends denormal (t = 0.5 only under IEEE division with denormals kept),
# a zero against a denormal (t = 0 and t = 1)
PAIRS = tuple((F(a), F(b)) for a, b in (("1.0", "-1.0"), ("-1.0", "1.0"), ("1e-45", "-1e-45"), ("-1e-45", "1e-45"), ("0.0", "-1e-45"),
                                        ("-1e-45", "-0.0"), ("-1e-39", "1e-45")))
# planted colours: k + 0.5 for even and odd k (floorf(cv + 0.5f) is neither rintf nor truncation), the float32 below 0.5 (cv + 0.5f rounds
# to 1: not roundf either), both sides of both clamps
COLOUR_SPECIALS = tuple(F(s) for s in ("0.5", "100.5", "127.5", "254.5", "255.5", "-0.5", "0.49999997", "-3.0", "300.0", "0.0", "255.0"))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- extraction rows ------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class ExtractRow:
    name: str
    what: str                 # what the row is there for
    kind: str                 # patterns | noise | holes | colours | thin | none
    dims: Tuple[int, int, int]
    min_weight: float = 1.0
    seed: int = 0
    variant: str = ""         # patterns: the thin axis; none: inside | outside | dead

    @property
    def id(self) -> str:
        return self.name

    @property
    def observed(self) -> bool:
        """Every sample is observed: the surface is closed up to the lattice's outer faces."""
        return self.kind in ("patterns", "noise", "colours", "thin")

    @property
    def cells(self) -> bool:
        return min(self.dims) >= 2

    @property
    def pool(self) -> bool:
        """The block-sparse entry points take it (sides >= 2, min_weight > 0)."""
        return self.cells and self.min_weight > 0

    @property
    def empty(self) -> bool:
        return self.kind == "none" or not self.cells

    def inputs(self) -> Dict[str, object]:
        """dict(tsdf, weight [nz,ny,nx], rgb [3,nz,ny,nx] | None, cweight | None, origin, voxel, min_weight); built once, read-only."""
        return _inputs(self)


def patterns_field(seed: int) -> np.ndarray:
    """[2,32,32]: cell (2a, 2b, 0) has corner pattern 16 b + a (bit c = corner c inside); every sample is a corner of exactly one such
    cell, and every magnitude differs, so no two vertices coincide."""
    k, j, i = np.meshgrid(np.arange(2), np.arange(32), np.arange(32), indexing="ij")
    p = 16 * (j // 2) + i // 2
    c = (i & 1) | ((j & 1) << 1) | (k << 2)
    mag = np.random.default_rng(seed).permutation(2048).reshape(2, 32, 32) / 2048.0 * 0.9 + 0.05
    return np.where((p >> c) & 1, -mag, mag).astype(F)


def noise_field(dims, rng, pairs: bool) -> np.ndarray:
    nx, ny, nz = dims
    t = rng.uniform(-1, 1, (nz, ny, nx)).astype(F)
    u = rng.random(t.shape)
    for n, s in enumerate(SPECIALS):
        t[(u >= 0.03 * n) & (u < 0.03 * (n + 1))] = s
    if pairs:
        for n, (lo, hi) in enumerate(PAIRS):
            t[n % nz, (3 * n + 1) % ny, 4:6] = (lo, hi)
    return t


def hole_weights(shape, min_weight: float, rng) -> np.ndarray:
    """Weights on every side of the threshold: 0, the float32 next to min_weight towards 0 and towards -inf (the same number for a
    positive threshold; for -1.0 and 0.0 only the second is below it), min_weight, min_weight + 1, NaN."""
    mw = F(min_weight)
    u = rng.random(shape)
    w = np.where(u < 0.55, mw, mw + F(1)).astype(F)
    w[u < 0.16] = np.nan
    w[u < 0.13] = np.nextafter(mw, F(-np.inf))
    w[u < 0.09] = np.nextafter(mw, F(0))
    w[u < 0.05] = 0
    return w


@lru_cache(maxsize=None)
def _inputs(row: ExtractRow):
    rng = np.random.default_rng(1000 + row.seed)
    nx, ny, nz = row.dims
    origin, voxel = OFF_ORIGIN, OFF_VOXEL
    rgb = cw = None
    if row.kind == "patterns":
        t = patterns_field(row.seed)
        t = {"z": t, "x": t.transpose(1, 2, 0), "y": t.transpose(2, 0, 1)}[row.variant]
        origin, voxel = (0.5, -2.0, 1.0), 0.5
    elif row.kind == "none" and row.variant in ("inside", "outside"):
        t = rng.uniform(0.1, 1, (nz, ny, nx)).astype(F)
        if row.variant == "outside":  # zeros of either sign are outside
            u = rng.random(t.shape)
            t[u < 0.2] = F(0)
            t[u < 0.1] = F("-0.0")
        else:
            t = -t
    else:
        t = noise_field(row.dims, rng, pairs=row.dims == NOISE_DIMS)
    t = np.ascontiguousarray(t, F)
    assert t.shape == (nz, ny, nx)
    w = np.ones_like(t)
    if row.kind == "holes":
        w = hole_weights(t.shape, row.min_weight, rng)
    if row.kind == "none" and row.variant == "dead":  # mixed signs, but every cell holds a sample of an even x: none is live
        w[:, :, ::2] = 0
    if row.kind == "colours":
        u = rng.random((3,) + t.shape)
        rgb = rng.uniform(-20, 275, u.shape).astype(F)
        for n, s in enumerate(COLOUR_SPECIALS):
            rgb[(u >= 0.055 * n) & (u < 0.055 * (n + 1))] = s
        u = rng.random(t.shape)
        cw = np.where(u < 0.7, F(1), F(2.5)).astype(F)
        cw[u < 0.34] = 0
        cw[u < 0.05] = F("-0.0")
    out = {"tsdf": t, "weight": w, "rgb": rgb, "cweight": cw, "origin": origin, "voxel": voxel, "min_weight": row.min_weight}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


THIN = ((1, 1, 1), (5, 1, 7), (2, 2, 2), (65, 2, 2), (2, 5, 2), (2, 2, 300), (130, 3, 2), (9, 8, 16))


def _extract_rows() -> List[ExtractRow]:
    rows = [ExtractRow(f"patterns-thin-{ax}", "all 256 corner patterns, each in a cell of its own: MT_CASES, MT_NEGATIVE, mt_vertex_index",
                       "patterns", {"z": (32, 32, 2), "x": (2, 32, 32), "y": (32, 2, 32)}[ax], variant=ax, seed=n)
            for n, ax in enumerate("zxy")]
    rows.append(ExtractRow("noise", "ambiguous and saddle cells everywhere; +-0, denormals and +-1 at either end of crossed edges",
                           "noise", NOISE_DIMS, seed=3))
    for n, mw in enumerate((1.0, 2.5, 0.0, -1.0)):
        rows.append(ExtractRow(f"noise-holes-{mw}", "users / live: every combination of live cells round an edge; weights next to the threshold",
                               "holes", NOISE_DIMS, min_weight=mw, seed=4 + n))
    rows.append(ExtractRow("colours", "floorf(cv + 0.5f) on k + 0.5, both clamps, cweight zero on one, the other and both ends",
                           "colours", NOISE_DIMS, seed=8))
    for n, dims in enumerate(THIN):
        rows.append(ExtractRow("lattice-%dx%dx%d" % dims, "no cell, one cell, slabs, sides off and on the workgroup and block borders",
                               "thin", dims, seed=9 + n))
    for n, v in enumerate(("inside", "outside", "dead")):
        rows.append(ExtractRow(f"no-surface-{v}", "no vertex and no face: emit is skipped, the outputs are empty", "none", (9, 7, 5),
                               variant=v, seed=20 + n))
    return rows


EXTRACT_ROWS = _extract_rows()


@lru_cache(maxsize=None)
def oracle(row: ExtractRow, wide: bool = False):
    """tsdf_ref.extract of the row, float32 (or float64); computed once, shared by the tests."""
    x = row.inputs()
    return R.extract(x["tsdf"], x["weight"], x["origin"], x["voxel"], x["min_weight"], x["rgb"], x["cweight"], True,
                     np.float64 if wide else np.float32)


def cell_patterns(tsdf) -> np.ndarray:
    """[nz-1,ny-1,nx-1]: bit c = corner c of the cell is inside."""
    nz, ny, nx = tsdf.shape
    p = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        p |= (tsdf[c >> 2:nz - 1 + (c >> 2), (c >> 1) & 1:ny - 1 + ((c >> 1) & 1), c & 1:nx - 1 + (c & 1)] < 0).astype(np.int64) << c
    return p


def live_cells(weight, min_weight) -> np.ndarray:
    nz, ny, nx = weight.shape
    ok = weight >= F(min_weight)
    live = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        live &= ok[c >> 2:nz - 1 + (c >> 2), (c >> 1) & 1:ny - 1 + ((c >> 1) & 1), c & 1:nx - 1 + (c & 1)]
    return live


def vertex_edges(vmask):
    """The edge of every vertex, in the contract's order (owner, then class), from a vmask plane: (i0, j0, k0), (i1, j1, k1), class."""
    nz, ny, nx = vmask.shape
    own, cls = np.nonzero((vmask.reshape(-1, 1) >> np.arange(7)) & 1)
    cls = cls + 1
    lo = np.stack((own % nx, own // nx % ny, own // (nx * ny)))
    return lo, lo + np.stack((cls & 1, (cls >> 1) & 1, cls >> 2)), cls


def on_outer_faces(lo, hi, dims) -> np.ndarray:
    """Per vertex, the mask of the lattice's six outer faces its edge lies in."""
    m = np.zeros(lo.shape[1], np.int64)
    for ax in range(3):
        m |= ((lo[ax] == 0) & (hi[ax] == 0)).astype(np.int64) << (2 * ax)
        m |= ((lo[ax] == dims[ax] - 1) & (hi[ax] == dims[ax] - 1)).astype(np.int64) << (2 * ax + 1)
    return m


# ---- integration rows -----------------------------------------------------------------------------------------------------------------

DEPTHS = (0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0)
INVALID = (0.0, np.inf, -1.0, np.nan)
K_DYADIC = ((4, 0, 3.5), (0, 4, 2.5), (0, 0, 1))
PLANES = ("tsdf", "weight", "rgb", "cweight")


@dataclass(frozen=True)
class ExactRow:
    name: str
    what: str
    dims: Tuple[int, int, int] = (12, 10, 14)
    origin: Tuple[float, float, float] = (-1.0, -0.75, -0.5)
    rotation: Tuple[Tuple[int, ...], ...] = ((1, 0, 0), (0, 1, 0), (0, 0, 1))  # a signed permutation: products stay exact
    translation: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    K: Tuple[Tuple[float, ...], ...] = K_DYADIC
    n_views: int = 2
    same_depth: bool = False  # every view sees one depth map (differently spoilt and masked) and one image: thirds stay exact
    second_size: Tuple[int, int] = ()  # (h, w) of the last view; its K is the row's at half the focal length
    claims: Tuple[str, ...] = PLANES  # the planes on which float32 and float64 agree exactly
    seed: int = 0
    voxel: float = 0.25
    trunc: float = 0.5

    @property
    def id(self) -> str:
        return self.name

    def views(self):
        """list of (depth [h,w] float32, cam21, mask [h,w] uint8 | None, image [h,w,3] uint8 | None); built once, read-only."""
        return _views(self)


def _depth_map(rng, h, w):
    d = rng.choice(np.array(DEPTHS, F), (h, w))
    return _spoil(d, rng, 0.24)


def _spoil(d, rng, share):
    d = d.copy()
    u = rng.random(d.shape)
    for n, bad in enumerate(INVALID):
        d[(u >= share / 4 * n) & (u < share / 4 * (n + 1))] = bad
    return d


@lru_cache(maxsize=None)
def _views(row: ExactRow):
    rng = np.random.default_rng(2000 + row.seed)
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = np.array(row.rotation, float), row.translation
    h, w = 7, 9
    base, image = rng.choice(np.array(DEPTHS, F), (h, w)), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    views = []
    for v in range(row.n_views):
        hv, wv, K = h, w, np.array(row.K, float)
        if row.second_size and v == row.n_views - 1:
            (hv, wv), K = row.second_size, K * np.array([[0.5, 1, 1], [1, 0.5, 1], [1, 1, 1]]) - np.array([[0, 0, 1], [0, 0, 1], [0, 0, 0]])
        if row.same_depth and (hv, wv) == (h, w):
            d, img = _spoil(base, rng, 0.16), (image if v < 2 else None)  # the last view brings no colour
        else:
            d, img = _depth_map(rng, hv, wv), rng.integers(0, 256, (hv, wv, 3), dtype=np.uint8)
        mask = None if v == row.n_views - 1 else rng.choice(np.array([0, 1, 255], np.uint8), (hv, wv), p=(0.15, 0.4, 0.45))
        for a in (d, mask, img):
            if a is not None:
                a.setflags(write=False)
        views.append((d, R.cam21(K, E), mask, img))
    return views


EXACT_ROWS = [
    ExactRow("dyadic", "three views of one camera: pc.z == 0 on the plane z = 0, pixel borders, fx == w, both ends of the band; weights to 3",
             n_views=3, same_depth=True, seed=0),
    ExactRow("dyadic-shifted", "the lattice one voxel further out in x and y: fx == -1 and fy == -1", dims=(13, 11, 14),
             origin=(-1.25, -1.0, -0.5), seed=1),
    ExactRow("look-minus-x", "the camera looks along -x; the lattice plane x = 0.5 has pc.z == 0", rotation=((0, 1, 0), (0, 0, -1), (-1, 0, 0)),
             translation=(0.0, 0.0, 0.5), seed=2),
    ExactRow("look-plus-y", "the camera looks along +y; the lattice plane y = -0.5 has pc.z == 0", rotation=((1, 0, 0), (0, 0, -1), (0, 1, 0)),
             translation=(0.0, 0.5, 0.5), seed=3),
    ExactRow("two-sizes", "a 7 x 9 view and a 5 x 6 view in one launch: fy == h, per-view w in the pixel index", second_size=(5, 6), seed=4),
    ExactRow("general-k", "K's third row is (0.25, 0, 1): samples with pc.z == 0 project INTO the image, only the test on pc.z keeps them out",
             K=((1, 0, 3.5), (0, 1, 2.5), (0.25, 0, 1)), seed=5),
]


def oracle_volume(row: ExactRow, dtype, color: bool = True):
    vol = R.widen(R.new_volume(row.dims, color=color), dtype)
    for d, cam, mask, image in row.views():
        R.integrate(vol, row.origin, row.voxel, row.trunc, d, cam, mask, image if color else None, dtype=dtype)
    return vol


EVENTS = ("pz_zero", "pz_zero_in_image", "pz_behind", "on_pixel_border", "fx_eq_w", "fx_eq_minus_1", "fy_eq_h", "fy_eq_minus_1",
          "depth_zero", "depth_inf", "depth_negative", "depth_nan", "mask_0", "mask_1", "mask_255", "sdf_eq_minus_trunc",
          "sdf_one_voxel_below", "sdf_eq_plus_trunc", "sdf_one_voxel_past")


def events(row: ExactRow) -> Dict[str, int]:
    """How often every decision of tsdf_fold_sample is met with equality (and every kind of pixel is read), counted over the samples and
    views of the row in float64."""
    nx, ny, nz = row.dims
    n = dict.fromkeys(EVENTS, 0)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = [row.origin[c] + a.astype(np.float64) * row.voxel for c, a in enumerate((i, j, k))]
    for d, cam, mask, _ in row.views():
        h, w = d.shape
        K, E = cam[:9].astype(np.float64).reshape(3, 3), cam[9:].astype(np.float64).reshape(3, 4)
        pc = [E[r, 0] * p[0] + E[r, 1] * p[1] + E[r, 2] * p[2] + E[r, 3] for r in range(3)]
        q = [K[r, 0] * pc[0] + K[r, 1] * pc[1] + K[r, 2] * pc[2] for r in range(3)]
        with np.errstate(all="ignore"):
            ux, uy = q[0] / q[2] + 0.5, q[1] / q[2] + 0.5
            fx, fy = np.floor(ux), np.floor(uy)
            inimg = (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
            front = pc[2] > 0
            n["pz_zero"] += int((pc[2] == 0).sum())
            n["pz_behind"] += int((pc[2] < 0).sum())
            ix, iy = np.where(inimg, fx, 0).astype(int), np.where(inimg, fy, 0).astype(int)
            dd = d.astype(np.float64)[iy, ix]
            mm = np.full(dd.shape, 255) if mask is None else mask[iy, ix]
            valid = (dd > 0) & (dd < np.inf)
            n["pz_zero_in_image"] += int(((pc[2] == 0) & inimg & valid & (mm != 0)).sum())
            n["on_pixel_border"] += int((front & inimg & ((ux == fx) | (uy == fy))).sum())
            n["fx_eq_w"] += int((front & (fx == w) & (fy >= 0) & (fy < h)).sum())
            n["fx_eq_minus_1"] += int((front & (fx == -1) & (fy >= 0) & (fy < h)).sum())
            n["fy_eq_h"] += int((front & (fy == h) & (fx >= 0) & (fx < w)).sum())
            n["fy_eq_minus_1"] += int((front & (fy == -1) & (fx >= 0) & (fx < w)).sum())
            seen = front & inimg
            n["depth_zero"] += int((seen & (dd == 0)).sum())
            n["depth_inf"] += int((seen & (dd == np.inf)).sum())
            n["depth_negative"] += int((seen & (dd < 0)).sum())
            n["depth_nan"] += int((seen & np.isnan(dd)).sum())
            if mask is not None:
                for b in (0, 1, 255):
                    n[f"mask_{b}"] += int((seen & valid & (mm == b)).sum())
            sdf = np.where(seen & valid & (mm != 0), dd - pc[2], np.nan)
            n["sdf_eq_minus_trunc"] += int((sdf == -row.trunc).sum())
            n["sdf_one_voxel_below"] += int((sdf == -row.trunc - row.voxel).sum())
            n["sdf_eq_plus_trunc"] += int((sdf == row.trunc).sum())
            n["sdf_one_voxel_past"] += int((sdf == row.trunc + row.voxel).sum())
    return n


if __name__ == "__main__":
    for r in EXTRACT_ROWS:
        o = oracle(r)
        print(f"{r.name}: {len(o['vertices'])} vertices, {len(o['faces'])} faces")
    for r in EXACT_ROWS:
        print(r.name, events(r))
