"""Operations on an indexed triangle mesh: the connected components of its vertices (pmn_mesh_components), the
removal of small components -- the floaters of a TSDF mesh -- and points drawn on the triangles at a fixed density per unit area
(pmn_mesh_face_samples / pmn_mesh_sample), which is what a surface is scored by.  A mesh is ``vertices`` [Nv,3] float32 and ``faces``
[Nt,3] int32 on a ROCm GPU, as ops.mt_extract returns them.  There is no CPU path: everything that launches refuses a host tensor.
tests/meshops_ref.py restates all of it in numpy."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import PmnError, check
from .ops import _dev_as, _ptr, _stream

INT32_MAX = 2 ** 31 - 1


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
