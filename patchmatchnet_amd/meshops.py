"""Operations on an indexed triangle mesh: the connected components of its vertices (pmn_mesh_components), the
removal of small components -- the floaters of a TSDF mesh -- and points drawn on the triangles at a fixed density per unit area
(pmn_mesh_face_samples / pmn_mesh_sample), which is what a surface is scored by.  A mesh is ``vertices`` [Nv,3] float32 and ``faces``
[Nt,3] int32 on a ROCm GPU, as ops.mt_extract returns them.  There is no CPU path: everything that launches refuses a host tensor.
tests/meshops_ref.py restates all of it in numpy.  build_face_grid / point_mesh_distance (pmn_mesh_distance) are
the exact distance from points to the surface itself; tests/mesh_distance_ref.py is their numpy form.  simplify_clustering (DESIGN.md
section 28, pmn_mesh_remap_faces / pmn_mesh_cluster_place) shrinks a mesh to one vertex per occupied cell; tests/simplify_ref.py is its
numpy form.  vertex_adjacency, smooth_taubin / smooth_laplacian (pmn_mesh_smooth) and vertex_normals (pmn_mesh_vertex_normals) are
DESIGN.md section 30: noise removal and the normals of the geometry itself; tests/smooth_ref.py is their numpy form."""
from __future__ import annotations

import ctypes
import math
import time
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import PmnError, check
from .ops import _dev_as, _ptr, _stream
from .pointcloud import Grid, _cell_order, _cells, _points, _sort_into_grid
from .registration import voxel_mean

INT32_MAX = 2 ** 31 - 1
# settings of build_face_grid, chosen from the sweep recorded in DESIGN.md 25 (profiles/mesh_distance_bench.log); they change the time
# of a search only, never its result
FACE_CELL_EDGES = 2.0    # default cell = FACE_CELL_EDGES * the median over the faces of the longest edge
FACE_COVER_CELLS = 1.0   # default cover = FACE_COVER_CELLS * cell
FACE_MAX_LEVEL = 16      # a face is split (conceptually) at most into 4^16 parts
FACE_ENTRY_LIMIT = 2 ** 31 - 64


def _faces(faces: torch.Tensor, what: str) -> torch.Tensor:
    faces = _dev_as(faces, f"{what}: faces", torch.int32)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise PmnError(f"{what}: faces must be [Nt,3], got {tuple(faces.shape)}")
    return faces


def _per_vertex(t: Optional[torch.Tensor], name: str, dtype: torch.dtype, nv: int, dev, what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = _dev_as(t, f"{what}: {name}", dtype)
    if tuple(t.shape) != (nv, 3) or t.device != dev:
        raise PmnError(f"{what}: {name} must be [{nv},3] on {dev}, got {tuple(t.shape)} on {t.device}")
    return t


def _raise_invalid(what: str, bad: int, nv: int) -> None:
    raise PmnError(f"{what}: {bad} faces have a vertex index outside 0..{nv - 1}")


def _enqueue_components(faces: torch.Tensor, nv: int):
    """(label, invalid) with the three launches of pmn_mesh_components enqueued; nothing is read back."""
    dev = faces.device
    label = torch.empty(nv, dtype=torch.int32, device=dev)
    invalid = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().pmn_mesh_components(faces.data_ptr() if faces.shape[0] else None, faces.shape[0], nv, label.data_ptr(),
                                             invalid.data_ptr(), _stream(faces)), "pmn_mesh_components")
    return label, invalid


def components(faces: torch.Tensor, n_vertices: int):
    """(label [Nv] int32, roots [C] int32 ascending, face_count [C] int64).  label[v] is the smallest vertex index of v's component (two
    vertices are connected when a face names both; a vertex no face names is a component of its own, with 0 faces); roots are the
    distinct labels and face_count[i] the faces of roots[i].  A function of the mesh alone, bit for bit.  PmnError, with their number,
    if faces name a vertex outside 0..Nv-1 (none is dereferenced).  The counting is integer torch (bincount); one host read."""
    faces = _faces(faces, "components")
    nv = int(n_vertices)
    if not 1 <= nv <= INT32_MAX - 255 or faces.shape[0] > INT32_MAX - 255:
        raise PmnError(f"components: n_vertices must be 1 .. 2^31 - 256 and at most as many faces, got {nv} / {faces.shape[0]}")
    label, invalid = _enqueue_components(faces, nv)
    bad = int(invalid.item())  # the host read (torch.nonzero below would synchronise anyway)
    if bad:
        _raise_invalid("components", bad, nv)
    roots = torch.nonzero(label == torch.arange(nv, dtype=torch.int32, device=faces.device)).reshape(-1)
    per_root = torch.bincount(label[faces[:, 0].long()].long(), minlength=nv)
    return label, roots.to(torch.int32), per_root[roots]


def _kept_components(roots: torch.Tensor, face_count: torch.Tensor, min_faces: int, keep_largest: int) -> torch.Tensor:
    """bool [C]: at least min_faces faces and, with keep_largest = K > 0, among the K largest by face count (ties: the smaller root)."""
    keep = face_count >= min_faces
    if keep_largest > 0:
        order = torch.sort(face_count, descending=True, stable=True).indices  # roots ascend, so a tie keeps the smaller root first
        top = torch.zeros_like(keep)
        top[order[:keep_largest]] = True
        keep &= top
    return keep


def remove_components(vertices: torch.Tensor, faces: torch.Tensor, colors: Optional[torch.Tensor] = None,
                      normals: Optional[torch.Tensor] = None, min_faces: int = 0, keep_largest: int = 0, return_counts: bool = False):
    """(vertices, faces, colors, normals) without the components that have fewer than ``min_faces`` faces or, with ``keep_largest`` =
    K > 0, are not among the K largest by face count (ties go to the smaller root).  Kept faces and kept vertices keep their order, a
    vertex that no kept face names is dropped, the indices are remapped with a cumulative sum; one host read sizes the outputs.
    ``min_faces=0, keep_largest=0`` returns its inputs unchanged -- the very same tensors, on any device; everything else raises
    PmnError for a tensor that is not on a ROCm GPU.  With ``return_counts`` the result gains (components found, components kept)."""
    min_faces, keep_largest = int(min_faces), int(keep_largest)
    if min_faces < 0 or keep_largest < 0:
        raise PmnError("remove_components: min_faces and keep_largest must be >= 0")
    if min_faces == 0 and keep_largest == 0:
        return (vertices, faces, colors, normals) + (((None, None),) if return_counts else ())
    what = "remove_components"
    faces = _faces(faces, what)
    vertices = _dev_as(vertices, f"{what}: vertices", torch.float32)
    dev, nv, nt = faces.device, vertices.shape[0], faces.shape[0]
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.device != dev:
        raise PmnError(f"{what}: vertices must be [Nv,3] on {dev}")
    colors = _per_vertex(colors, "colors", torch.uint8, nv, dev, what)
    normals = _per_vertex(normals, "normals", torch.float32, nv, dev, what)
    if nv == 0:
        if nt:
            _raise_invalid(what, nt, 0)
        return (vertices, faces, colors, normals) + (((0, 0),) if return_counts else ())
    label, roots, face_count = components(faces, nv)
    keep = _kept_components(roots, face_count, min_faces, keep_largest)
    root_kept = torch.zeros(nv, dtype=torch.bool, device=dev)
    root_kept[roots.long()] = keep
    named = torch.zeros(nv, dtype=torch.bool, device=dev)
    named[faces.reshape(-1).long()] = True
    vkeep = root_kept[label.long()] & named                # named by a kept face: its whole component is kept
    fkeep = root_kept[label[faces[:, 0].long()].long()]
    vscan = torch.cumsum(vkeep, 0, dtype=torch.int64)      # inclusive: new index + 1 where kept
    fscan = torch.cumsum(fkeep, 0, dtype=torch.int64)
    zero = torch.zeros((), dtype=torch.int64, device=dev)
    nkv, nkf, nkc = torch.stack((vscan[-1], fscan[-1] if nt else zero, keep.sum())).tolist()  # the host read that sizes the outputs
    vidx = torch.searchsorted(vscan, torch.arange(1, nkv + 1, dtype=torch.int64, device=dev))  # the j-th kept vertex
    fidx = torch.searchsorted(fscan, torch.arange(1, nkf + 1, dtype=torch.int64, device=dev))
    new_faces = (vscan[faces[fidx].long()] - 1).to(torch.int32)
    out = (vertices[vidx], new_faces, None if colors is None else colors[vidx], None if normals is None else normals[vidx])
    return out + (((int(roots.shape[0]), int(nkc)),) if return_counts else ())


def sample_surface(vertices: torch.Tensor, faces: torch.Tensor, density: Optional[float] = None, spacing: Optional[float] = None,
                   seed: int = 0, colors: Optional[torch.Tensor] = None):
    """Points on the triangles at ``density`` points per unit area (``spacing`` s means density 1 / s^2; exactly one of the two), a
    function of (mesh, density, seed) alone: (points [N,3] float32, face [N] int32, colors [N,3] uint8 or None), ordered by face and by
    rank within the face.  A face gets floor(area * density + u) samples with u uniform in [0, 1) (unbiased rounding; float64), placed
    uniformly (b0, b1, b2) = (1 - sqrt(r1), sqrt(r1) (1 - r2), sqrt(r1) r2); all randomness is a counter-based hash of (seed, face,
    rank) (include/pmn_hip.h).  Zero-area faces and faces with a vertex that is not finite get none.  PmnError for faces that name a
    vertex outside the array (none is dereferenced) and for a total above 2^31 - 1.  One host read (the total)."""
    what = "sample_surface"
    if (density is None) == (spacing is None):
        raise PmnError(f"{what}: give exactly one of density and spacing")
    if spacing is not None:
        spacing = float(spacing)
        if not (spacing > 0.0 and spacing < float("inf")):
            raise PmnError(f"{what}: spacing must be positive and finite")
        density = 1.0 / spacing ** 2
    density = float(density)
    if not (density > 0.0 and density < float("inf")):
        raise PmnError(f"{what}: density must be positive and finite")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise PmnError(f"{what}: seed must be 0 .. 2^64 - 1")
    faces = _faces(faces, what)
    vertices = _dev_as(vertices, f"{what}: vertices", torch.float32)
    dev, nv, nt = faces.device, vertices.shape[0], faces.shape[0]
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.device != dev:
        raise PmnError(f"{what}: vertices must be [Nv,3] on {dev}")
    if nv > INT32_MAX - 255 or nt > INT32_MAX - 255:
        raise PmnError(f"{what}: at most 2^31 - 256 vertices and faces")
    colors = _per_vertex(colors, "colors", torch.uint8, nv, dev, what)
    if nt and not nv:
        _raise_invalid(what, nt, 0)
    total = 0
    with torch.cuda.device(dev):
        L = _lib.lib()
        if nt:
            counts = torch.empty(nt, dtype=torch.int32, device=dev)
            invalid = torch.zeros(1, dtype=torch.int32, device=dev)
            check(L.pmn_mesh_face_samples(vertices.data_ptr(), nv, faces.data_ptr(), nt, density, seed, counts.data_ptr(),
                                          invalid.data_ptr(), _stream(faces)), "pmn_mesh_face_samples")
            scan = torch.cumsum(counts, 0, dtype=torch.int64)
            total, bad = torch.stack((scan[-1], invalid[0].long())).tolist()  # the feature's one host read
            if bad:
                _raise_invalid(what, bad, nv)
            if total > INT32_MAX:
                raise PmnError(f"{what}: {total} samples exceed 2^31 - 1; use a lower density")
        points = torch.empty((total, 3), dtype=torch.float32, device=dev)
        face = torch.empty(total, dtype=torch.int32, device=dev)
        out_colors = torch.empty((total, 3), dtype=torch.uint8, device=dev) if colors is not None else None
        if total:
            check(L.pmn_mesh_sample(vertices.data_ptr(), nv, faces.data_ptr(), nt, _ptr(colors), scan.data_ptr(), total, seed,
                                    points.data_ptr(), face.data_ptr(), _ptr(out_colors), _stream(faces)), "pmn_mesh_sample")
    return points, face, out_colors


# ---- distance to the surface -------------------------------------------------------------------------------------

class FaceGrid(NamedTuple):
    """The search structure of point_mesh_distance: a pointcloud.Grid over reference points of the faces (include/pmn_hip.h,
    pmn_mesh_distance).  Every point of face f lies within ``radius`` of one of the reference points that ``entry_face`` maps to f."""
    grid: Grid                # over the reference points (float32), sorted
    entry_face: torch.Tensor  # [E] int32: the face of every sorted reference point
    vertices: torch.Tensor    # [Nv,3] float32, the caller's
    faces: torch.Tensor       # [Nt,3] int32, the caller's
    levels: torch.Tensor      # [Nt] int64: face f has 4^levels[f] reference points
    radius: float             # R, the float32 rounding of the reference points included
    cover: float


def _mesh_any_device(vertices: torch.Tensor, faces: torch.Tensor, what: str):
    for t, name, dtype in ((vertices, "vertices", torch.float32), (faces, "faces", torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous():
            raise PmnError(f"{what}: {name}: expected a contiguous {dtype} tensor")
        if t.dim() != 2 or t.shape[1] != 3:
            raise PmnError(f"{what}: {name} must be [n,3], got {tuple(t.shape)}")
    if vertices.device != faces.device:
        raise PmnError(f"{what}: vertices are on {vertices.device}, faces on {faces.device}")
    if not 1 <= vertices.shape[0] <= INT32_MAX - 255 or not 1 <= faces.shape[0] <= INT32_MAX - 255:
        raise PmnError(f"{what}: between 1 and 2^31 - 256 vertices and faces, got {vertices.shape[0]} and {faces.shape[0]}")


def build_face_grid(vertices: torch.Tensor, faces: torch.Tensor, cell: Optional[float] = None,
                    cover: Optional[float] = None) -> FaceGrid:
    """Sorts reference points of the faces into a uniform grid of side ``cell`` and fixes the covering radius R of point_mesh_distance.
    A face whose vertices all lie within ``cover`` of its centroid has one reference point, the centroid.  A larger face gets the 4^L
    centroids of its conceptual L-fold midpoint split (the 2^L x 2^L lattice of similar triangles), L the smallest level at which a
    part's vertices lie within ``cover`` of the part's centroid; they are computed in float64 from their barycentric weights
    (3 i + 1 or 2) / (3 * 2^L) and all name the ORIGINAL face: no geometry is subdivided.  A part is convex, so each of its points is
    within the part's radius of its centroid; R is the largest such radius plus sqrt(3) * 2^-23 * max |coordinate| for the rounding of
    the reference points to float32 (twice its bound; the rest covers the float64 arithmetic).  Degenerate faces are faces like any
    other; a face with an index outside 0..Nv-1 is placed by its clamped indices here and refused by point_mesh_distance.
    Defaults: ``cell`` = FACE_CELL_EDGES * the median longest edge, ``cover`` = FACE_COVER_CELLS * cell; neither changes a result.
    Torch on the tensors' device -- a host tensor works too (nothing launches) -- with no loop over faces; one host read for the
    defaults and one for the sizes.  PmnError for vertices that are not finite, a cell or cover that is not positive and finite, and
    for 2^31 - 64 reference points or more (it names the largest face and the cover)."""
    what = "build_face_grid"
    _mesh_any_device(vertices, faces, what)
    nv, nt, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    bad = int((~torch.isfinite(vertices)).any(1).sum())
    if bad:
        raise PmnError(f"{what}: {bad} vertices have non-finite coordinates")
    idx = faces.long().clamp(0, nv - 1)
    v64 = vertices.double()
    A, B, C = v64[idx[:, 0]], v64[idx[:, 1]], v64[idx[:, 2]]
    longest = torch.stack(((B - A).norm(dim=1), (C - B).norm(dim=1), (A - C).norm(dim=1))).max(0).values
    G = (A + B + C) / 3.0
    rf = torch.stack(((A - G).norm(dim=1), (B - G).norm(dim=1), (C - G).norm(dim=1))).max(0).values
    if cell is None:
        med, top = float(longest.median()), float(longest.max())
        cell = FACE_CELL_EDGES * (med if med > 0.0 else (top if top > 0.0 else 1.0))
    cell = float(cell)
    if not (cell > 0.0 and math.isfinite(cell)):
        raise PmnError(f"{what}: cell must be positive and finite, got {cell}")
    cover = FACE_COVER_CELLS * cell if cover is None else float(cover)
    if not (cover > 0.0 and math.isfinite(cover)):
        raise PmnError(f"{what}: cover must be positive and finite, got {cover}")
    # the level: the smallest L with rf * 2^-L <= cover (the parts are similar to the face at scale 2^-L, so is their radius)
    levels = torch.ceil(torch.log2(rf / cover)).clamp(0, FACE_MAX_LEVEL).long()
    levels = (levels + (rf / (torch.ones_like(levels) << levels).double() > cover).long()).clamp(max=FACE_MAX_LEVEL)
    counts = torch.ones_like(levels) << (2 * levels)
    total = int(counts.sum())
    if total >= FACE_ENTRY_LIMIT:
        f = int(rf.argmax())
        raise PmnError(f"{what}: {total} reference points reach the limit of 2^31 - 64: face {f} (vertices within {float(rf[f]):.6g} of "
                       f"its centroid) would need {int(counts[f])} at cover {cover:.6g}; use a larger cover")
    part_radius = float((rf / (torch.ones_like(levels) << levels).double()).max())
    # entry k of a face with N = 2^L: row i of the lattice holds 2 (N - i) - 1 parts (upright and inverted alternating), N^2 - k parts
    # are left from k on, and (N - i)^2 from row i on
    fid = torch.repeat_interleave(torch.arange(nt, device=dev), counts)
    k = torch.arange(total, device=dev) - (torch.cumsum(counts, 0) - counts)[fid]
    N = torch.ones_like(k) << levels[fid]
    left = N * N - k
    s = torch.ceil(torch.sqrt(left.double())).long()
    s = s - ((s - 1) * (s - 1) >= left).long() + (s * s < left).long()  # the integer ceil(sqrt(left)), whatever the float one gave
    i = N - s
    t = k - (2 * N * i - i * i)
    j, inverted = t >> 1, t & 1
    den = (3 * N).double()
    w0 = (3 * i + 1 + inverted).double() / den
    w1 = (3 * j + 1 + inverted).double() / den
    w2 = (3 * (N - 1 - inverted - i - j) + 1 + inverted).double() / den
    ref = (w0[:, None] * A[fid] + w1[:, None] * B[fid] + w2[:, None] * C[fid]).float().contiguous()
    radius = part_radius * (1.0 + 2.0 ** -40) + math.sqrt(3.0) * 2.0 ** -23 * float(vertices.abs().max())
    grid = _sort_into_grid(ref, cell, what=what)
    return FaceGrid(grid, fid[grid.perm].int().contiguous(), vertices, faces, levels, radius, cover)


def point_mesh_distance(query: torch.Tensor, face_grid: FaceGrid, max_dist: float, return_face: bool = False,
                        return_closest: bool = False):
    """pmn_mesh_distance: float64 [n], the exact distance from every query point ([n,3] float32 on the device, any finite position) to
    the nearest triangle of the mesh ``face_grid`` was built from, capped at ``max_dist`` with nn_distance's convention (a face counts
    only when d < max_dist).  ``return_face``: also int64 [n], the index into the mesh's faces, the lower index among faces at
    bit-equal distance, -1 at the cap; ``return_closest``: also float64 [n,3], the nearest point on that face, NaN at the cap.  A
    function of (mesh, query) alone.  PmnError if a face names a vertex outside the mesh (none is dereferenced); one host read."""
    what = "point_mesh_distance"
    if not isinstance(face_grid, FaceGrid):
        raise PmnError(f"{what}: face_grid must come from build_face_grid")
    query = _points(query, "query")
    g = face_grid.grid
    for t, name in ((g.xyz, "grid"), (g.keys, "keys"), (face_grid.entry_face, "entry_face"), (face_grid.vertices, "vertices"),
                    (face_grid.faces, "faces")):
        if not isinstance(t, torch.Tensor) or t.device != query.device:
            raise PmnError(f"{what}: query is on {query.device}, the face grid's {name} on {getattr(t, 'device', type(t).__name__)}")
    # a FaceGrid is a plain tuple anyone can put together: what the kernel indexes is checked before raw pointers go to it
    _mesh_any_device(face_grid.vertices, face_grid.faces, what)
    n_ref = int(g.xyz.shape[0]) if g.xyz.dim() == 2 else -1
    if g.xyz.dtype != torch.float32 or g.xyz.dim() != 2 or g.xyz.shape[1] != 3 or not g.xyz.is_contiguous() or n_ref < 1:
        raise PmnError(f"{what}: the face grid's points must be a contiguous float32 [n,3] tensor, n >= 1")
    for t, name, dtype in ((g.keys, "keys", torch.int64), (face_grid.entry_face, "entry_face", torch.int32)):
        if t.dtype != dtype or tuple(t.shape) != (n_ref,) or not t.is_contiguous():
            raise PmnError(f"{what}: the face grid's {name} must be a contiguous {dtype} [{n_ref}] tensor, got {t.dtype} {tuple(t.shape)}")
    if not (isinstance(face_grid.radius, float) and face_grid.radius >= 0.0 and math.isfinite(face_grid.radius)):
        raise PmnError(f"{what}: the face grid's radius must be finite and >= 0, got {face_grid.radius!r}")
    if not (max_dist > 0.0 and math.isfinite(max_dist) and math.isfinite(float(max_dist) * float(max_dist))):
        raise PmnError(f"{what}: max_dist must be positive and finite, got {max_dist}")
    n, dev = int(query.shape[0]), query.device
    order = _cell_order(query, g)
    dist = torch.empty(n, dtype=torch.float64, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev) if return_face else None
    closest = torch.empty((n, 3), dtype=torch.float64, device=dev) if return_closest else None
    invalid = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().pmn_mesh_distance(g.xyz.data_ptr(), g.keys.data_ptr(), int(g.xyz.shape[0]), (ctypes.c_double * 3)(*g.origin),
                                           float(g.cell), (ctypes.c_int * 3)(*g.dims), face_grid.entry_face.data_ptr(),
                                           float(face_grid.radius), face_grid.vertices.data_ptr(), int(face_grid.vertices.shape[0]),
                                           face_grid.faces.data_ptr(), int(face_grid.faces.shape[0]), query.data_ptr(),
                                           order.data_ptr(), n, float(max_dist), dist.data_ptr(), _ptr(face), _ptr(closest),
                                           invalid.data_ptr(), _stream(query)), "pmn_mesh_distance")
    bad = int(invalid.item())
    if bad:
        _raise_invalid(what, bad, int(face_grid.vertices.shape[0]))
    out = (dist,) + ((face.long(),) if return_face else ()) + ((closest,) if return_closest else ())
    return out[0] if len(out) == 1 else out


# ---- simplification by vertex clustering -------------------------------------------------------------------------

def _lexsort_rows(tri: torch.Tensor) -> torch.Tensor:
    """int64 [n]: the rows of an int [n,3] tensor in ascending (column 0, 1, 2) order, equal rows in input order (three stable sorts)."""
    order = torch.sort(tri[:, 2], stable=True).indices
    for col in (1, 0):
        order = order[torch.sort(tri[order, col], stable=True).indices]
    return order


def _canonical_face_order(faces: torch.Tensor) -> torch.Tensor:
    """int64 [Nt]: the faces ordered by their vertex triple rotated so that the smallest index comes first, then by the rotation that
    took them there: an order that does not know where a face stood in the array.  Faces that tie are the same triple in the same
    rotation, i.e. the same numbers to every kernel.  Nothing is read through an index."""
    a, b, c = faces.unbind(1)
    shift = torch.where((b < a) & (b < c), 1, torch.where((c < a) & (c < b), 2, 0))
    rot = torch.gather(faces, 1, (shift[:, None] + torch.arange(3, device=faces.device)) % 3)
    order = torch.sort(shift, stable=True).indices
    for col in (2, 1, 0):
        order = order[torch.sort(rot[order, col], stable=True).indices]
    return order


def simplify_clustering(vertices: torch.Tensor, faces: torch.Tensor, cell: float, colors: Optional[torch.Tensor] = None,
                        normals: Optional[torch.Tensor] = None, origin=None, placement: str = "quadric", stiffness: float = 1e-3,
                        return_map: bool = False, timings: Optional[dict] = None):
    """Quadric vertex clustering: (vertices, faces, colors, normals[, vertex_map]) of the mesh with one vertex per occupied cubic cell
    of side ``cell``.  The lattice's corner is min(vertices) - cell / 2 unless ``origin`` (three finite numbers, none above the
    minimum) is given; the cells, their key and the stable sort are voxel_downsample's, and clusters are numbered in ascending key
    order.  pmn_voxel_mean gives every cluster's mean position, colour (bytes as floats, back to bytes by floorf(c + 0.5f) clamped) and
    normal (renormalised in float64; a mean of zero or non-finite length gives a zero normal).  ``placement="quadric"``: the
    representative is the point of pmn_mesh_cluster_place -- the minimiser of the area-weighted squared distances to the planes of the
    faces at the cluster's corners plus ``stiffness`` * (their total weight) * the squared distance to the mean, clamped to the cell
    (the kernel is handed the faces sorted by their rotated vertex triple, so the order of the input faces changes no bit of it);
    the system's condition number is at most (1 + stiffness) / stiffness.  ``placement="mean"``: the mean itself.  Either way every
    input vertex lies in its representative's cell, hence within sqrt(3) * cell of it.
    Faces are mapped through the clusters (pmn_mesh_remap_faces); a face with two corners in one cluster is dropped, among faces with
    the same rotated triple the one with the lowest input index stays (opposite orientations are different faces), kept faces keep
    their input order and start with their smallest index, clusters that no kept face names are dropped.  ``vertex_map`` [Nv] int32 is
    the output index of every input vertex, or -1.  A mesh that collapses to nothing returns empty tensors.  Everything is a function
    of the mesh and the parameters alone, bit for bit.  PmnError for a host tensor, non-finite vertices, a cell or stiffness that is
    not positive and finite, a lattice beyond a 63-bit key, and faces that name a vertex outside the array (counted, never
    dereferenced).  ``timings``, if a dict, receives the seconds of each stage (it adds synchronisations)."""
    what = "simplify_clustering"
    cell, stiffness = float(cell), float(stiffness)
    if not (cell > 0.0 and math.isfinite(cell)):
        raise PmnError(f"{what}: cell must be positive and finite, got {cell}")
    if not (stiffness > 0.0 and math.isfinite(stiffness)):
        raise PmnError(f"{what}: stiffness must be positive and finite, got {stiffness}")
    if placement not in ("quadric", "mean"):
        raise PmnError(f"{what}: placement must be 'quadric' or 'mean', got {placement!r}")
    faces = _faces(faces, what)
    vertices = _dev_as(vertices, f"{what}: vertices", torch.float32)
    dev, nv, nt = faces.device, vertices.shape[0], faces.shape[0]
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.device != dev:
        raise PmnError(f"{what}: vertices must be [Nv,3] on {dev}")
    if nv > INT32_MAX - 255 or nt > _lib.MESH_SIMPLIFY_MAX_FACES:
        raise PmnError(f"{what}: at most 2^31 - 256 vertices and {_lib.MESH_SIMPLIFY_MAX_FACES} faces, got {nv} and {nt}")
    colors = _per_vertex(colors, "colors", torch.uint8, nv, dev, what)
    normals = _per_vertex(normals, "normals", torch.float32, nv, dev, what)
    if nt and not nv:
        _raise_invalid(what, nt, 0)

    def result(v, f, c, n, vmap):
        return (v, f, c, n) + ((vmap,) if return_map else ())

    def empty():
        return result(vertices.new_zeros((0, 3)), faces.new_zeros((0, 3)), None if colors is None else colors.new_zeros((0, 3)),
                      None if normals is None else normals.new_zeros((0, 3)), torch.full((nv,), -1, dtype=torch.int32, device=dev))

    if nv == 0:
        return empty()
    bad = int((~torch.isfinite(vertices)).any(1).sum())
    if bad:
        raise PmnError(f"{what}: {bad} vertices have non-finite coordinates")

    clock = [time.perf_counter()]

    def lap(stage):
        if timings is not None:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            timings[stage] = timings.get(stage, 0.0) + now - clock[0]
            clock[0] = now

    # clusters: the cells, the key and the stable sort of registration.voxel_downsample
    lo = vertices.min(0).values.double().cpu().numpy()
    if origin is None:
        org = lo - cell / 2
    else:
        org = np.asarray(origin, np.float64).reshape(-1)
        if org.shape != (3,) or not np.isfinite(org).all() or (org > lo).any():
            raise PmnError(f"{what}: origin must be three finite numbers, none above the vertices' minimum {lo.tolist()}")
    c = _cells(vertices, org.tolist(), cell)
    dims = (c.max(0).values + 1).cpu().tolist()
    if max(dims) > 2 ** 30 or dims[0] * dims[1] * dims[2] >= 2 ** 62:
        raise PmnError(f"{what}: a lattice of {dims} cells does not fit a 63-bit key; use a larger cell")
    keys = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    keys, perm = torch.sort(keys, stable=True)
    head = torch.ones(nv, dtype=torch.bool, device=dev)
    head[1:] = keys[1:] != keys[:-1]
    run = torch.cumsum(head, 0) - 1                        # the cluster of every sorted vertex
    m = int(run[-1]) + 1
    starts = torch.cat([torch.nonzero(head).reshape(-1), head.new_full((1,), nv, dtype=torch.int64)]).contiguous()
    cluster = torch.empty(nv, dtype=torch.int32, device=dev)
    cluster[perm] = run.to(torch.int32)
    lap("sort")

    # means: pmn_voxel_mean over the sorted vertices, colours and normals as further columns
    cols = [t.float() for t in (colors, normals) if t is not None]
    attr = torch.cat(cols, 1)[perm].contiguous() if cols else None
    mean = voxel_mean(vertices[perm].contiguous(), starts, attr)
    mean, mean_attr = mean if attr is not None else (mean, None)
    out_colors = out_normals = None
    if colors is not None:
        out_colors = torch.floor(mean_attr[:, :3] + 0.5).clamp_(0.0, 255.0).to(torch.uint8)
    if normals is not None:
        n64 = mean_attr[:, -3:].double()
        length = torch.sqrt((n64[:, 0] * n64[:, 0] + n64[:, 1] * n64[:, 1]) + n64[:, 2] * n64[:, 2])
        ok = (length > 0) & torch.isfinite(length)
        out_normals = torch.where(ok[:, None], n64 / torch.where(ok, length, torch.ones_like(length))[:, None],
                                  torch.zeros_like(n64)).float()
    lap("means")
    if nt == 0:
        return empty()

    # faces through the clusters, and the corner list of every cluster
    L = _lib.lib()
    corner_cluster = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    tri = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    flag = torch.empty(nt, dtype=torch.uint8, device=dev)
    invalid = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(L.pmn_mesh_remap_faces(faces.data_ptr(), nt, nv, cluster.data_ptr(), m, corner_cluster.data_ptr(), tri.data_ptr(),
                                     flag.data_ptr(), invalid.data_ptr(), _stream(faces)), "pmn_mesh_remap_faces")
    lap("remap")
    if placement == "quadric":
        # the kernel sums a run in (face, corner) order: it gets the faces in an order of their own, not the array's, so that
        # permuting the input faces changes no bit of a representative
        canon = _canonical_face_order(faces)
        faces_canon = faces[canon].contiguous()
        by_cluster = torch.sort(corner_cluster[canon].reshape(-1), stable=True)
        corners = by_cluster.indices.to(torch.int32)
        corner_starts = torch.searchsorted(by_cluster.values, torch.arange(m + 1, dtype=torch.int32, device=dev)).contiguous()
        cluster_keys = keys[starts[:-1]].contiguous()
        rep = torch.empty((m, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(L.pmn_mesh_cluster_place(vertices.data_ptr(), nv, faces_canon.data_ptr(), nt, corners.data_ptr(), corner_starts.data_ptr(),
                                           cluster_keys.data_ptr(), m, mean.data_ptr(), (ctypes.c_double * 3)(*org.tolist()), cell,
                                           (ctypes.c_int * 3)(*dims), stiffness, rep.data_ptr(), _stream(faces)),
                  "pmn_mesh_cluster_place")
    else:
        rep = mean
    lap("placement")

    # compaction (integer torch, as remove_components): one face per rotated triple, the clusters the kept faces name
    order = _lexsort_rows(tri)
    st = tri[order]
    first = torch.ones(nt, dtype=torch.bool, device=dev)
    first[1:] = (st[1:] != st[:-1]).any(1)
    fkeep = torch.zeros(nt, dtype=torch.bool, device=dev)
    fkeep[order] = first & (flag[order] == 0)
    named = torch.zeros(m + 1, dtype=torch.bool, device=dev)
    named[torch.where(fkeep[:, None], tri, torch.full_like(tri, m)).reshape(-1).long()] = True  # slot m takes the dropped faces
    named = named[:m]
    vscan = torch.cumsum(named, 0, dtype=torch.int64)
    fscan = torch.cumsum(fkeep, 0, dtype=torch.int64)
    nkv, nkf, bad = torch.stack((vscan[-1], fscan[-1], invalid[0].long())).tolist()  # the host read that sizes the outputs
    if bad:
        _raise_invalid(what, bad, nv)
    vidx = torch.searchsorted(vscan, torch.arange(1, nkv + 1, dtype=torch.int64, device=dev))
    fidx = torch.searchsorted(fscan, torch.arange(1, nkf + 1, dtype=torch.int64, device=dev))
    new_faces = (vscan[tri[fidx].long()] - 1).to(torch.int32)
    cl = cluster.long()
    vmap = torch.where(named[cl], vscan[cl] - 1, torch.full_like(cl, -1)).to(torch.int32)
    out = result(rep[vidx], new_faces, None if out_colors is None else out_colors[vidx],
                 None if out_normals is None else out_normals[vidx], vmap)
    lap("compaction")
    return out


# ---- smoothing and vertex normals from the faces --------------------------------------------------------------

class VertexAdjacency(NamedTuple):
    """The neighbours of every vertex in CSR form (vertex_adjacency)."""
    starts: torch.Tensor      # [Nv + 1] int64: row i is neighbours[starts[i]:starts[i + 1]]
    neighbours: torch.Tensor  # [E] int32: the distinct neighbours of every vertex, ascending within a row
    boundary: torch.Tensor    # [Nv] bool: the vertex lies on an edge that exactly one face corner-pair names


def _mesh_on_device(vertices: torch.Tensor, faces: torch.Tensor, what: str):
    faces = _faces(faces, what)
    vertices = _dev_as(vertices, f"{what}: vertices", torch.float32)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.device != faces.device:
        raise PmnError(f"{what}: vertices must be [Nv,3] on {faces.device}")
    if vertices.shape[0] > INT32_MAX - 255 or faces.shape[0] > _lib.MESH_SIMPLIFY_MAX_FACES:
        raise PmnError(f"{what}: at most 2^31 - 256 vertices and {_lib.MESH_SIMPLIFY_MAX_FACES} faces, got {vertices.shape[0]} and "
                       f"{faces.shape[0]}")
    return vertices, faces


def vertex_adjacency(faces: torch.Tensor, n_vertices: int) -> VertexAdjacency:
    """The vertex-to-vertex incidence of a mesh.  Every face (a, b, c) contributes its six directed pairs; a pair with equal ends is
    dropped; duplicates are merged (the 63-bit key a * Nv + b, a stable sort, the first of every run), so row i holds the distinct
    neighbours of i in ascending order.  An undirected edge is a boundary edge when exactly one face corner-pair names it, where faces
    that repeat a vertex name none; a vertex is a boundary vertex when it lies on one.  A function of the SET of faces, not of their
    order.  Integer torch, nothing is read through a face index; one host read.  PmnError, with their number, for faces that name a
    vertex outside 0..Nv-1."""
    what = "vertex_adjacency"
    faces = _faces(faces, what)
    nv, nt, dev = int(n_vertices), int(faces.shape[0]), faces.device
    if not 0 <= nv <= INT32_MAX - 255 or nt > _lib.MESH_SIMPLIFY_MAX_FACES:
        raise PmnError(f"{what}: n_vertices must be 0 .. 2^31 - 256 and at most {_lib.MESH_SIMPLIFY_MAX_FACES} faces, got {nv} / {nt}")
    f = faces.long()
    bad = int(((f < 0) | (f >= nv)).any(1).sum()) if nt else 0  # the host read
    if bad:
        _raise_invalid(what, bad, nv)
    a, b, c = f.unbind(1)
    src, dst = torch.cat((a, b, b, c, c, a)), torch.cat((b, a, c, b, a, c))
    keys = torch.sort((src * nv + dst)[src != dst], stable=True).values
    head = torch.ones(keys.shape[0], dtype=torch.bool, device=dev)
    head[1:] = keys[1:] != keys[:-1]
    keys = keys[head]
    rows = torch.div(keys, max(nv, 1), rounding_mode="floor")
    starts = torch.searchsorted(rows, torch.arange(nv + 1, dtype=torch.int64, device=dev)).contiguous()
    neighbours = (keys - rows * nv).to(torch.int32).contiguous()
    # the corner-pairs (a, b), (b, c), (c, a) of the faces with three different vertices, as undirected edges, counted
    proper = (a != b) & (b != c) & (a != c)
    p, q = torch.cat((a, b, c))[proper.repeat(3)], torch.cat((b, c, a))[proper.repeat(3)]
    edge, count = torch.unique(torch.minimum(p, q) * nv + torch.maximum(p, q), return_counts=True)
    edge = edge[count == 1]
    boundary = torch.zeros(nv, dtype=torch.bool, device=dev)
    boundary[torch.div(edge, max(nv, 1), rounding_mode="floor")] = True
    boundary[edge % max(nv, 1)] = True
    return VertexAdjacency(starts, neighbours, boundary)


def _check_adjacency(adjacency, nv: int, dev, what: str) -> VertexAdjacency:
    if not isinstance(adjacency, VertexAdjacency):
        raise PmnError(f"{what}: adjacency must come from vertex_adjacency")
    for t, name, dtype, shape in ((adjacency.starts, "starts", torch.int64, (nv + 1,)),
                                  (adjacency.neighbours, "neighbours", torch.int32, None),
                                  (adjacency.boundary, "boundary", torch.bool, (nv,))):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or t.device != dev or \
                (shape is not None and tuple(t.shape) != shape):
            raise PmnError(f"{what}: the adjacency's {name} must be a contiguous {dtype} tensor{'' if shape is None else ' ' + str(list(shape))} "
                           f"on {dev}")
    return adjacency


def smooth_steps(vertices: torch.Tensor, faces: torch.Tensor, factors, boundary: str = "fixed", pinned: Optional[torch.Tensor] = None,
                 adjacency: Optional[VertexAdjacency] = None) -> torch.Tensor:
    """pmn_mesh_smooth: new float32 [Nv,3] vertices after one umbrella step per entry of ``factors`` (finite numbers): a vertex with
    neighbours moves by factor * (the mean over its neighbours j of p_j - p_i), in float64 with one rounding to float32 per step
    (include/pmn_hip.h); a vertex without neighbours, or a pinned one, keeps its bits.  ``boundary="fixed"`` pins the boundary vertices
    of vertex_adjacency (they still feed their neighbours), ``"free"`` treats them like any other; ``pinned`` (bool [Nv]) is or-ed in.
    No factors: a bit-equal copy.  ``adjacency``: what vertex_adjacency(faces, Nv) returned, to spare building it again.  The caller's
    tensors are not written.  A function of the mesh and the factors alone, bit for bit, whatever the order of the faces.  An empty
    mesh returns without a launch.  PmnError for a host tensor, non-finite vertices or factors, an unknown boundary mode and faces that
    name a vertex outside the array (counted, never dereferenced)."""
    what = "smooth_steps"
    factors = [float(x) for x in factors]
    if not all(math.isfinite(x) for x in factors):
        raise PmnError(f"{what}: every factor must be finite")
    if len(factors) > _lib.MESH_SMOOTH_MAX_STEPS:
        raise PmnError(f"{what}: at most {_lib.MESH_SMOOTH_MAX_STEPS} steps, got {len(factors)}")
    if boundary not in ("fixed", "free"):
        raise PmnError(f"{what}: boundary must be 'fixed' or 'free', got {boundary!r}")
    vertices, faces = _mesh_on_device(vertices, faces, what)
    dev, nv, nt = faces.device, int(vertices.shape[0]), int(faces.shape[0])
    if pinned is not None:
        pinned = _dev_as(pinned, f"{what}: pinned", torch.bool)
        if tuple(pinned.shape) != (nv,) or pinned.device != dev:
            raise PmnError(f"{what}: pinned must be [{nv}] on {dev}, got {tuple(pinned.shape)} on {pinned.device}")
    if nt and not nv:
        _raise_invalid(what, nt, 0)
    if nv == 0:
        return vertices.clone()
    bad = int((~torch.isfinite(vertices)).any(1).sum())
    if bad:
        raise PmnError(f"{what}: {bad} vertices have non-finite coordinates")
    adj = vertex_adjacency(faces, nv) if adjacency is None else _check_adjacency(adjacency, nv, dev, what)
    if nt == 0:
        return vertices.clone()
    pin = adj.boundary if boundary == "fixed" else None
    if pinned is not None:
        pin = pinned if pin is None else pin | pinned
    out = torch.empty_like(vertices)
    scratch = torch.empty_like(vertices) if len(factors) > 1 else None
    invalid = torch.zeros(1, dtype=torch.int32, device=dev)
    n_entries = int(adj.neighbours.shape[0])
    with torch.cuda.device(dev):
        check(_lib.lib().pmn_mesh_smooth(vertices.data_ptr(), nv, adj.starts.data_ptr(), adj.neighbours.data_ptr() if n_entries else None,
                                         n_entries, _ptr(pin), (ctypes.c_double * max(len(factors), 1))(*factors), len(factors),
                                         out.data_ptr(), _ptr(scratch), invalid.data_ptr(), _stream(vertices)), "pmn_mesh_smooth")
    if adjacency is not None and factors:  # a CSR someone handed in is not trusted: the kernel skipped and counted what it could not use
        bad = int(invalid.item())
        if bad:
            raise PmnError(f"{what}: {bad} entries of the adjacency name a vertex outside 0..{nv - 1}")
    return out


def _check_lam(what: str, lam: float, iterations: int):
    lam, iterations = float(lam), int(iterations)
    if not (lam > 0.0 and lam <= 1.0):
        raise PmnError(f"{what}: lam must be in (0, 1], got {lam}")
    if iterations < 0:
        raise PmnError(f"{what}: iterations must be >= 0, got {iterations}")
    return lam, iterations


def smooth_taubin(vertices: torch.Tensor, faces: torch.Tensor, iterations: int = 10, lam: float = 0.5, mu: float = -0.53,
                  boundary: str = "fixed", pinned: Optional[torch.Tensor] = None,
                  adjacency: Optional[VertexAdjacency] = None) -> torch.Tensor:
    """Taubin's low-pass filter: ``iterations`` times a shrinking umbrella step with ``lam`` and an inflating one with ``mu``, i.e.
    smooth_steps with the factors lam, mu, lam, mu, ...; the pair removes ripple without the shrinkage of smooth_laplacian.  New float32
    [Nv,3] vertices; faces, colours and the number of vertices are the caller's and unchanged; ``iterations=0`` is a bit-equal copy.
    PmnError, beyond smooth_steps's, for ``lam`` outside (0, 1], ``mu`` not finite or not < -lam (Taubin's condition for a low-pass
    filter) and negative iterations."""
    what = "smooth_taubin"
    lam, iterations = _check_lam(what, lam, iterations)
    mu = float(mu)
    if not (math.isfinite(mu) and mu < -lam):
        raise PmnError(f"{what}: mu must be finite and < -lam = {-lam}, got {mu}")
    if 2 * iterations > _lib.MESH_SMOOTH_MAX_STEPS:
        raise PmnError(f"{what}: at most {_lib.MESH_SMOOTH_MAX_STEPS // 2} iterations, got {iterations}")
    return smooth_steps(vertices, faces, [lam, mu] * iterations, boundary=boundary, pinned=pinned, adjacency=adjacency)


def smooth_laplacian(vertices: torch.Tensor, faces: torch.Tensor, iterations: int = 1, lam: float = 0.5, boundary: str = "fixed",
                     pinned: Optional[torch.Tensor] = None, adjacency: Optional[VertexAdjacency] = None) -> torch.Tensor:
    """``iterations`` umbrella steps with ``lam`` in (0, 1] (smooth_steps with the factors lam, lam, ...): smooths and shrinks."""
    what = "smooth_laplacian"
    lam, iterations = _check_lam(what, lam, iterations)
    if iterations > _lib.MESH_SMOOTH_MAX_STEPS:
        raise PmnError(f"{what}: at most {_lib.MESH_SMOOTH_MAX_STEPS} iterations, got {iterations}")
    return smooth_steps(vertices, faces, [lam] * iterations, boundary=boundary, pinned=pinned, adjacency=adjacency)


def vertex_normals(vertices: torch.Tensor, faces: torch.Tensor, flip: bool = False) -> torch.Tensor:
    """pmn_mesh_vertex_normals: float32 [Nv,3], for every vertex the normalised sum of (B - A) x (C - A) over the faces (A, B, C) at
    its corners -- area-weighted, float64, one rounding -- by the right-hand rule of the faces' stored winding; ``flip`` negates it
    exactly.  A vertex with no face, or only faces without area, gets zero.  The kernel is handed the faces in _canonical_face_order,
    so the order of the caller's faces changes no bit.  An empty mesh returns without a launch.  PmnError for a host tensor and for
    faces that name a vertex outside the array (counted, never dereferenced); one host read."""
    what = "vertex_normals"
    vertices, faces = _mesh_on_device(vertices, faces, what)
    dev, nv, nt = faces.device, int(vertices.shape[0]), int(faces.shape[0])
    if nt and not nv:
        _raise_invalid(what, nt, 0)
    out = torch.zeros_like(vertices)
    if nv == 0 or nt == 0:
        return out
    faces_canon = faces[_canonical_face_order(faces)].contiguous()
    by_vertex = torch.sort(faces_canon.reshape(-1), stable=True)
    corners = by_vertex.indices.to(torch.int32)
    corner_starts = torch.searchsorted(by_vertex.values, torch.arange(nv + 1, dtype=torch.int32, device=dev)).contiguous()
    invalid = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().pmn_mesh_vertex_normals(vertices.data_ptr(), nv, faces_canon.data_ptr(), nt, corners.data_ptr(),
                                                 corner_starts.data_ptr(), 1 if flip else 0, out.data_ptr(), invalid.data_ptr(),
                                                 _stream(vertices)), "pmn_mesh_vertex_normals")
    bad = int(invalid.item())
    if bad:
        _raise_invalid(what, bad, nv)
    return out
