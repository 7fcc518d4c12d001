"""A surface mesh from a scan's depth maps: a dense truncated-signed-distance volume integrated on the device
(pmn_tsdf_integrate), its iso-surface by marching tetrahedra (pmn_mt_count / pmn_mt_emit), the grid heuristics of mesh.py (the PLY
mesh files are ply.write_ply_mesh / ply.read_ply_mesh); and the same volume stored in 8 x 8 x 8 blocks near the surface only (section 18: SparseTsdfVolume), for scenes whose
dense lattice would not fit.  There is no CPU path: the volumes refuse a host device."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import PmnError
from .ply import PLY_FACE, mesh_header, read_ply_mesh, write_ply_mesh  # noqa: F401  (mesh.ply)

MAX_VOXELS = 2 ** 29  # mesh.py --max_voxels: 24 B per sample with colour = 12.9 GB
MAX_BLOCKS = 2 ** 20  # mesh.py --max_blocks: as many pooled samples
MAX_VIRTUAL_VOXELS = 2 ** 36  # mesh.py --volume sparse: the virtual lattice (its block table then stays below ops.SPARSE_MAX_TABLE)


class _Volume:
    """What the two volumes share: where the lattice sits, and the batching of ``integrate``.  A subclass supplies ``_integrate_views``,
    the op call of one launch."""

    def _place(self, origin, voxel: float, trunc: float, device) -> None:
        name = type(self).__name__
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise PmnError(f"{name}: device {self.device} is not a ROCm GPU (no CPU fallback)")
        self.origin = np.asarray(origin, np.float32).reshape(3).copy()
        self.voxel, self.trunc = float(np.float32(voxel)), float(np.float32(trunc))
        if not (np.isfinite(self.origin).all() and np.isfinite(self.voxel) and self.voxel > 0 and np.isfinite(self.trunc) and self.trunc > 0):
            raise PmnError(f"{name}: origin must be finite, voxel and trunc positive and finite")

    def _allocated(self, what) -> None:
        """Raises where the planes do not exist yet."""

    def integrate(self, maps: torch.Tensor, slots: Sequence[int], sizes: Sequence[Tuple[int, int]], cams, masks=None, images=None,
                  batch: int = 8) -> None:
        """Folds the views in, ``batch`` per launch, in the given order (see ops.tsdf_integrate for the arguments; any batch size
        leaves the same bits).  For a SparseTsdfVolume the views should be those ``allocate`` saw: a surface outside the allocated
        band is not integrated."""
        self._allocated("integrate")
        if not 1 <= int(batch) <= _lib.TSDF_MAX_VIEWS:
            raise PmnError(f"{type(self).__name__}.integrate: batch must be 1 .. {_lib.TSDF_MAX_VIEWS}")
        cams = np.asarray(cams, np.float32).reshape(len(slots), 21)
        for a in range(0, len(slots), int(batch)):
            b = min(a + int(batch), len(slots))
            self._integrate_views(maps, slots[a:b], sizes[a:b], cams[a:b], None if masks is None else masks[a:b],
                                  None if images is None or self.rgb is None else images[a:b])


class TsdfVolume(_Volume):
    """nx x ny x nz samples, sample (i,j,k) at origin + (i,j,k) * voxel (world units); planes tsdf (1), weight (0) and, with
    ``color``, rgb and cweight (0), all float32 on ``device``."""

    def __init__(self, origin, voxel: float, dims: Sequence[int], trunc: float, device, color: bool = True) -> None:
        self._place(origin, voxel, trunc, device)
        nx, ny, nz = (int(d) for d in dims)
        if min(nx, ny, nz) < 2 or nz > 65535 or nx * ny * nz > 2 ** 31 - 1:
            raise PmnError(f"TsdfVolume: dims {nx} x {ny} x {nz} must be >= 2 per axis, nz <= 65535, fewer than 2^31 samples")
        self.dims, device = (nx, ny, nz), self.device
        self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=device)
        self.rgb = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=device) if color else None
        self.cweight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=device) if color else None

    def _integrate_views(self, maps, slots, sizes, cams, masks, images) -> None:
        ops.tsdf_integrate(self.tsdf, self.weight, self.rgb, self.cweight, self.origin, self.voxel, self.trunc, maps, slots, sizes, cams,
                           masks, images)

    def extract(self, min_weight: float = 1.0, normals: bool = True):
        """(vertices [Nv,3] float32, faces [Nt,3] int32, colors [Nv,3] uint8 | None, normals [Nv,3] float32 | None) on the device."""
        return ops.mt_extract(self.tsdf, self.weight, self.origin, self.voxel, min_weight, self.rgb, self.cweight, normals)


class SparseTsdfVolume(_Volume):
    """The lattice of TsdfVolume (``dims`` = nx x ny x nz VIRTUAL samples) of which only the 8 x 8 x 8 blocks near some view's surface
    exist.  ``allocate`` builds, from the views that will be integrated, ``blocks`` (int32 [B]: the linear block
    index of every slot, ascending), ``table`` (int32 [nbz,nby,nbx]: slot or -1) and the pool planes tsdf (1), weight (0) [B,8,8,8] and,
    with ``color``, rgb [3,B,8,8,8] and cweight (0).  ``integrate`` and ``extract`` then give, sample for sample and triangle for
    triangle, what TsdfVolume gives on the same lattice fed the same views."""

    def __init__(self, origin, voxel: float, dims: Sequence[int], trunc: float, device, color: bool = True,
                 max_blocks: int = MAX_BLOCKS) -> None:
        self._place(origin, voxel, trunc, device)
        self.dims = tuple(int(d) for d in dims)
        self.nblocks = ops.sparse_blocks(self.dims)  # (nbx, nby, nbz)
        if not 1 <= int(max_blocks) <= ops.SPARSE_MAX_BLOCKS:
            raise PmnError(f"SparseTsdfVolume: max_blocks must be 1 .. {ops.SPARSE_MAX_BLOCKS}")
        self.color, self.max_blocks = bool(color), int(max_blocks)
        self.blocks = self.table = self.tsdf = self.weight = self.rgb = self.cweight = None
        self.marked = self.needed = 0  # blocks the views marked; blocks after the dilation (set even when allocate raises)

    @staticmethod
    def _dilate(flags: torch.Tensor) -> torch.Tensor:
        """One block in all 26 directions: a box maximum, one axis at a time (uint8 slices: plumbing)."""
        for axis in range(3):
            grown = flags.clone()
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(None, -1), slice(1, None)
            grown[tuple(hi)] |= flags[tuple(lo)]
            grown[tuple(lo)] |= flags[tuple(hi)]
            flags = grown
        return flags

    def allocate(self, maps: torch.Tensor, slots: Sequence[int], sizes: Sequence[Tuple[int, int]], cams, masks=None) -> int:
        """Marks the blocks near the surface of the given views (see ops.tsdf_mark_blocks for the arguments), dilates them by one block
        and builds list, table and pool.  Returns the number of blocks B.  PmnError if a pixel's box was too large to mark (a wild
        depth: mask it), if nothing was marked, or if B > max_blocks."""
        nbx, nby, nbz = self.nblocks
        flags = torch.zeros((nbz, nby, nbx), dtype=torch.uint8, device=self.device)
        overflow = torch.zeros(1, dtype=torch.int32, device=self.device)
        cams = np.asarray(cams, np.float32).reshape(len(slots), 21)
        V = _lib.TSDF_MAX_VIEWS
        for a in range(0, len(slots), V):
            ops.tsdf_mark_blocks(flags, overflow, self.dims, self.origin, self.voxel, self.trunc, maps, slots[a:a + V], sizes[a:a + V],
                                 cams[a:a + V], None if masks is None else masks[a:a + V])
        blocks = torch.nonzero(self._dilate(flags).reshape(-1)).reshape(-1)  # ascending; synchronises
        over, self.marked, self.needed = int(overflow.item()), int(flags.sum(dtype=torch.int64).item()), int(blocks.numel())
        del flags
        if over:
            raise PmnError(f"SparseTsdfVolume.allocate: {over} pixels have a depth whose +-trunc section covers more than "
                           f"{_lib.TSDF_MARK_SPAN} blocks of {ops.SPARSE_BLOCK} samples on an axis (or no finite position); mask them, or "
                           f"use a larger voxel")
        if self.needed == 0:
            raise PmnError("SparseTsdfVolume.allocate: no valid pixel's surface lies inside the lattice (0 blocks)")
        if self.needed > self.max_blocks:
            raise PmnError(f"SparseTsdfVolume.allocate: {self.needed} blocks needed, max_blocks is {self.max_blocks}")
        B = self.needed
        self.blocks = blocks.to(torch.int32)
        self.table = torch.full((nbz, nby, nbx), -1, dtype=torch.int32, device=self.device)
        self.table.view(-1)[blocks] = torch.arange(B, dtype=torch.int32, device=self.device)
        shape = (B,) + (ops.SPARSE_BLOCK,) * 3
        self.tsdf = torch.ones(shape, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.rgb = torch.zeros((3,) + shape, dtype=torch.float32, device=self.device) if self.color else None
        self.cweight = torch.zeros(shape, dtype=torch.float32, device=self.device) if self.color else None
        return B

    def allocate_points(self, points: torch.Tensor, reach: float) -> int:
        """``allocate`` for a cloud instead of views (pointcloud.cloud_sdf): marks the blocks that the box
        p +- ``reach``, grown by one voxel as ops.tsdf_mark_blocks grows its boxes, of any point touches, dilates them by one block
        and builds list, table and pool.  ``points``: float32 [n,3] on the volume's device.  The marking is torch (plumbing): the
        blocks of the box's eight corners, which with the dilation cover the whole box because ``reach`` may not exceed 8 voxels (a
        box then spans at most three blocks per axis, and the middle one lies next to both ends).  A box that misses the virtual
        lattice marks nothing.  Returns the number of blocks B.  PmnError if nothing was marked or if B > max_blocks."""
        if not isinstance(points, torch.Tensor) or not points.is_cuda or self.device.index not in (None, points.device.index) or \
                points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
            raise PmnError(f"SparseTsdfVolume.allocate_points: points must be a float32 [n,3] tensor on {self.device}")
        reach = float(reach)
        if not (np.isfinite(reach) and reach > 0 and reach <= ops.SPARSE_BLOCK * self.voxel):
            raise PmnError(f"SparseTsdfVolume.allocate_points: reach must be positive and at most {ops.SPARSE_BLOCK} voxels "
                           f"({ops.SPARSE_BLOCK * self.voxel:.6g}), got {reach}")
        if not bool(torch.isfinite(points).all()):
            raise PmnError("SparseTsdfVolume.allocate_points: points have non-finite coordinates")
        nbx, nby, nbz = self.nblocks
        S = ops.SPARSE_BLOCK
        top = torch.tensor([d - 1 for d in self.dims], dtype=torch.float64, device=self.device)
        rel = points.double() - torch.from_numpy(self.origin.astype(np.float64)).to(self.device)
        lo = torch.ceil((rel - reach) / self.voxel) - 1.0   # sample indices of the box, +- one voxel
        hi = torch.floor((rel + reach) / self.voxel) + 1.0
        inside = ((hi >= 0) & (lo <= top)).all(1)
        ends = (lo[inside].clamp_min(0.0).long() // S, torch.minimum(hi[inside], top).long() // S)  # first and last block per axis
        flags = torch.zeros(nbz * nby * nbx, dtype=torch.uint8, device=self.device)
        for corner in range(8):
            bx, by, bz = (ends[(corner >> c) & 1][:, c] for c in range(3))
            flags[(bz * nby + by) * nbx + bx] = 1
        flags = flags.view(nbz, nby, nbx)
        blocks = torch.nonzero(self._dilate(flags).reshape(-1)).reshape(-1)  # ascending; synchronises
        self.marked, self.needed = int(flags.sum(dtype=torch.int64).item()), int(blocks.numel())
        del flags
        if self.needed == 0:
            raise PmnError("SparseTsdfVolume.allocate_points: no point lies within reach of the lattice (0 blocks)")
        if self.needed > self.max_blocks:
            raise PmnError(f"SparseTsdfVolume.allocate_points: {self.needed} blocks needed, max_blocks is {self.max_blocks}")
        B = self.needed
        self.blocks = blocks.to(torch.int32)
        self.table = torch.full((nbz, nby, nbx), -1, dtype=torch.int32, device=self.device)
        self.table.view(-1)[blocks] = torch.arange(B, dtype=torch.int32, device=self.device)
        shape = (B,) + (S,) * 3
        self.tsdf = torch.ones(shape, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.rgb = torch.zeros((3,) + shape, dtype=torch.float32, device=self.device) if self.color else None
        self.cweight = torch.zeros(shape, dtype=torch.float32, device=self.device) if self.color else None
        return B

    def _allocated(self, what):
        if self.blocks is None:
            raise PmnError(f"SparseTsdfVolume.{what}: call allocate() first")

    def _integrate_views(self, maps, slots, sizes, cams, masks, images) -> None:
        ops.tsdf_integrate_blocks(self.tsdf, self.weight, self.rgb, self.cweight, self.blocks, self.dims, self.origin, self.voxel,
                                  self.trunc, maps, slots, sizes, cams, masks, images)

    def extract(self, min_weight: float = 1.0, normals: bool = True):
        """What TsdfVolume.extract returns, in pool order: the same triangles, vertex for vertex the same bits."""
        self._allocated("extract")
        return ops.mt_extract_blocks(self.tsdf, self.weight, self.table, self.blocks, self.dims, self.origin, self.voxel, min_weight,
                                     self.rgb, self.cweight, normals)

    def to_dense(self):
        """(tsdf, weight, rgb | None, cweight | None) as dense [nz,ny,nx] planes: the pool scattered, tsdf 1 / weight 0 elsewhere (for
        tests and debugging: it needs the dense lattice's memory)."""
        self._allocated("to_dense")
        nbx, nby, nbz = self.nblocks
        nx, ny, nz = self.dims
        S = ops.SPARSE_BLOCK
        idx = self.blocks.long()

        def scatter(pool, fill):
            full = torch.full((nbz * nby * nbx, S, S, S), fill, dtype=torch.float32, device=self.device)
            full[idx] = pool
            return full.view(nbz, nby, nbx, S, S, S).permute(0, 3, 1, 4, 2, 5).reshape(nbz * S, nby * S, nbx * S)[:nz, :ny, :nx].contiguous()

        rgb = None if self.rgb is None else torch.stack([scatter(self.rgb[c], 0.0) for c in range(3)])
        return scatter(self.tsdf, 1.0), scatter(self.weight, 0.0), rgb, None if self.cweight is None else scatter(self.cweight, 0.0)


def camera21(K, E) -> np.ndarray:
    """The 21 floats pmn_tsdf_integrate reads per view: K row-major (at the MAP's size), then the upper 3x4 of the extrinsic."""
    return np.concatenate((np.asarray(K, np.float32).reshape(9), np.asarray(E, np.float32)[:3, :4].reshape(12)))


def backproject(depth: torch.Tensor, mask: Optional[torch.Tensor], K, E, stride: int = 1):
    """World points [n,3] (float32, on the device) and depth / fx [n] of the valid (finite, > 0, mask != 0) pixels of one view, every
    ``stride``-th pixel per axis: the evidence choose_grid sizes the volume from (elementwise torch: plumbing, not a kernel)."""
    h, w = depth.shape
    d = depth[::stride, ::stride]
    ok = torch.isfinite(d) & (d > 0)
    if mask is not None:
        ok &= mask[::stride, ::stride] != 0
    v, u = torch.meshgrid(torch.arange(0, h, stride, device=depth.device, dtype=torch.float32),
                          torch.arange(0, w, stride, device=depth.device, dtype=torch.float32), indexing="ij")
    K64, E64 = np.asarray(K, np.float64), np.asarray(E, np.float64)
    Kinv = torch.from_numpy(np.linalg.inv(K64)).to(depth.device, torch.float32)
    Einv = torch.from_numpy(np.linalg.inv(E64)).to(depth.device, torch.float32)
    z = d[ok]
    pix = torch.stack((u[ok], v[ok], torch.ones_like(z)), 1)
    cam = (pix @ Kinv.T) * z[:, None]
    return cam @ Einv[:3, :3].T + Einv[:3, 3], z / float(K64[0, 0])


def choose_grid(points: torch.Tensor, footprint: Optional[torch.Tensor] = None, voxel: Optional[float] = None,
                trunc: Optional[float] = None, bounds: Optional[Sequence[float]] = None, max_voxels: int = MAX_VOXELS,
                limit_name: str = "--max_voxels", max_axis: Optional[int] = None):
    """Bounds and voxel size for a scan -> (origin float32[3], voxel, trunc, (nx, ny, nz), note).  ``points`` [n,3] are the
    back-projected masked pixels, ``footprint`` [n] their depth / fx.  voxel defaults to 2 x the median footprint (a sample is then
    seen by several pixels' worth of evidence), trunc to 4 x voxel, the box to the 1st..99th percentile of the points per axis grown by
    trunc on every side (``bounds`` = xmin ymin zmin xmax ymax zmax is taken as given).  If the lattice would exceed ``max_voxels``
    samples the voxel grows (trunc with it, when trunc was not given) and ``note`` says so, naming the limit ``limit_name``; it is None
    otherwise.  The dense volume's nz <= 65535 also bounds the grid unless ``max_axis`` (a bound on every axis) is given.  Works on any device (a sort per axis)."""
    if voxel is None:
        if footprint is None or footprint.numel() == 0:
            raise PmnError("choose_grid: no valid pixel to size the voxel from")
        voxel = 2.0 * float(footprint.float().median())
    voxel = float(voxel)
    if not (np.isfinite(voxel) and voxel > 0):
        raise PmnError("choose_grid: voxel must be positive and finite")
    auto_trunc = trunc is None
    trunc = 4.0 * voxel if auto_trunc else float(trunc)
    if not (np.isfinite(trunc) and trunc > 0):
        raise PmnError("choose_grid: trunc must be positive and finite")
    if bounds is None:
        if points is None or points.numel() == 0:
            raise PmnError("choose_grid: no valid pixel to bound the volume with")
        srt = torch.sort(points.float(), 0).values
        n = srt.shape[0]
        lo = srt[int(np.floor(0.01 * (n - 1)))].tolist()
        hi = srt[int(np.ceil(0.99 * (n - 1)))].tolist()
        grow = True
    else:
        if len(bounds) != 6 or not np.isfinite(np.asarray(bounds, float)).all() or any(bounds[c + 3] <= bounds[c] for c in range(3)):
            raise PmnError("choose_grid: bounds must be xmin ymin zmin xmax ymax zmax with max > min")
        lo, hi, grow = list(bounds[:3]), list(bounds[3:]), False
    note = None
    while True:
        g = trunc if grow else 0.0
        dims = tuple(max(int(np.ceil((hi[c] - lo[c] + 2 * g) / voxel)) + 1, 2) for c in range(3))
        if dims[0] * dims[1] * dims[2] <= max_voxels and (dims[2] <= 65535 if max_axis is None else max(dims) <= max_axis):
            break
        factor = max((dims[0] * dims[1] * dims[2] / float(max_voxels)) ** (1.0 / 3.0), 1.01)
        voxel *= factor
        if auto_trunc:
            trunc = 4.0 * voxel
        note = "the grid would exceed %s %d: voxel enlarged to %.6g%s" % (limit_name, max_voxels, voxel,
                                                                          " (trunc %.6g)" % trunc if auto_trunc else "")
    g = trunc if grow else 0.0
    origin = np.asarray([lo[c] - g for c in range(3)], np.float32)
    return origin, voxel, trunc, dims, note
