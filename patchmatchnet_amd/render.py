"""A mesh or a point cloud drawn into a scan's cameras on the device: the z-buffered projection the rest of the
pipeline lacks (pmn_raster_triangles / pmn_splat_points / pmn_raster_resolve), orbit cameras for a model without scan cameras; the PLY
reader for models this library did not write is ply.read_ply_model.  There is no CPU path: the renderer refuses a host device."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from ._lib import PmnError
from .ply import read_ply_model  # noqa: F401  (the models that are drawn)
from .tsdf import camera21


class Renderer:
    """Holds the z-buffer keys and the output planes for the largest view drawn so far.  The tensors a render call returns are views
    of these buffers: they are valid until the next call (copy what must outlive it)."""

    def __init__(self, device) -> None:
        device = torch.device(device)
        if device.type != "cuda":
            raise PmnError(f"Renderer: device {device} is not a ROCm GPU (no CPU fallback)")
        if device.index is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self._pixels = 0
        self._keys = self._depth = self._index = self._rgb = self._normal = self._worklist = None

    def _planes(self, h: int, w: int):
        h, w = int(h), int(w)
        if not (1 <= h <= _lib.RASTER_MAX_DIM and 1 <= w <= _lib.RASTER_MAX_DIM):
            raise PmnError(f"Renderer: a view is 1 .. {_lib.RASTER_MAX_DIM} pixels per side, got {h} x {w}")
        if h * w > self._pixels:
            self._pixels = h * w
            self._keys = torch.empty(h * w, dtype=torch.int64, device=self.device)
            self._depth = torch.empty(h * w, dtype=torch.float32, device=self.device)
            self._index = torch.empty(h * w, dtype=torch.int32, device=self.device)
            self._rgb = torch.empty(h * w * 3, dtype=torch.uint8, device=self.device)
            self._normal = torch.empty(h * w * 3, dtype=torch.float32, device=self.device)
        n = h * w
        keys = self._keys[:n].view(h, w)
        keys.fill_(-1)  # all ones: nothing drawn
        return (keys, self._depth[:n].view(h, w), self._index[:n].view(h, w), self._rgb[:3 * n].view(h, w, 3),
                self._normal[:3 * n].view(h, w, 3))

    def _attributes(self, n: int, colors, normals, what: str):
        for name, a, dtype in (("colors", colors, torch.uint8), ("normals", normals, torch.float32)):
            if a is not None and (not isinstance(a, torch.Tensor) or a.device != self.device or a.dtype != dtype or
                                  tuple(a.shape) != (n, 3) or not a.is_contiguous()):
                raise PmnError(f"{what}: {name} must be a contiguous [{n},3] {dtype} tensor on {self.device}")

    def render_mesh(self, vertices: torch.Tensor, faces: torch.Tensor, K, E, h: int, w: int, colors: Optional[torch.Tensor] = None,
                    normals: Optional[torch.Tensor] = None, shade: bool = True, rgb: bool = True, normal: bool = False,
                    max_box: int = 0):
        """(depth [h,w] float32 with 0 = nothing, index [h,w] int32 with -1, rgb [h,w,3] uint8 | None, normal [h,w,3] float32 | None,
        counters int32[4] on the device: read them after the loop over views, not inside it).  vertices [Nv,3] float32 world, faces
        [Nt,3] int32, colors [Nv,3] uint8 | None (mid-grey), normals [Nv,3] float32 world | None (then a face's own normal shades
        it); K [3,3] at h x w, E the world-to-camera extrinsic."""
        cam = camera21(K, E)
        keys, depth, index, rgb_out, normal_out = self._planes(h, w)
        if not isinstance(vertices, torch.Tensor) or vertices.device != self.device or not isinstance(faces, torch.Tensor) or \
                faces.device != self.device:
            raise PmnError(f"render_mesh: vertices and faces must be tensors on {self.device} (no CPU fallback)")
        self._attributes(vertices.shape[0], colors, normals, "render_mesh")
        if self._worklist is None or self._worklist.numel() < faces.shape[0]:
            self._worklist = torch.empty(faces.shape[0], dtype=torch.int32, device=self.device)
        counters = torch.zeros(4, dtype=torch.int32, device=self.device)
        ops.raster_triangles(vertices, faces, cam, keys, counters, self._worklist, max_box)
        ops.raster_resolve(keys, cam, vertices, faces, depth, index, colors, normals, shade, rgb_out if rgb else None,
                           normal_out if normal else None)
        return depth, index, rgb_out if rgb else None, normal_out if normal else None, counters

    def render_points(self, points: torch.Tensor, K, E, h: int, w: int, colors: Optional[torch.Tensor] = None,
                      normals: Optional[torch.Tensor] = None, radius_px: float = 0.0, radius_world: float = 0.0, shade: bool = True,
                      rgb: bool = True, normal: bool = False):
        """The same for a cloud: points [N,3] float32 world, a footprint of ``radius_px`` pixels (0 = the nearest pixel only) or of
        ``radius_world`` world units (radius_world * fx / z pixels, at most _lib.SPLAT_MAX_RADIUS).  Where the cloud is sparser than
        the footprint it is see-through.  counters: [0] behind the camera / not finite, [1] outside the guard band."""
        cam = camera21(K, E)
        keys, depth, index, rgb_out, normal_out = self._planes(h, w)
        if not isinstance(points, torch.Tensor) or points.device != self.device:
            raise PmnError(f"render_points: points must be a tensor on {self.device} (no CPU fallback)")
        self._attributes(points.shape[0], colors, normals, "render_points")
        counters = torch.zeros(4, dtype=torch.int32, device=self.device)
        ops.splat_points(points, cam, keys, counters, radius_px, radius_world)
        ops.raster_resolve(keys, cam, points, None, depth, index, colors, normals, shade, rgb_out if rgb else None,
                           normal_out if normal else None)
        return depth, index, rgb_out if rgb else None, normal_out if normal else None, counters


def orbit_cameras(bounds: Sequence[float], n: int, h: int, w: int, fov: float = 50.0):
    """n cameras on a circle about the vertical (y) axis through the centre of ``bounds`` = xmin ymin zmin xmax ymax zmax, looking at
    the centre, y down, the first one looking along +z: (K [n,3,3], E [n,4,4]) float32.  ``fov`` is the vertical field of view in
    degrees; the distance is chosen so that the sphere around the box (with a 5 % margin) lies inside every frame.  Host numpy."""
    b = np.asarray(bounds, np.float64).reshape(-1)
    if b.size != 6 or not np.isfinite(b).all() or (b[3:] < b[:3]).any():
        raise PmnError("orbit_cameras: bounds must be xmin ymin zmin xmax ymax zmax with max >= min")
    if int(n) < 1 or int(h) < 1 or int(w) < 1 or not 1.0 <= float(fov) <= 170.0:
        raise PmnError("orbit_cameras: n, h, w must be >= 1 and fov 1 .. 170 degrees")
    centre, radius = (b[:3] + b[3:]) / 2, max(float(np.linalg.norm(b[3:] - b[:3])) / 2, 1e-6)
    f = (h / 2.0) / np.tan(np.radians(fov) / 2.0)
    half = min(np.arctan((h - 1) / 2.0 / f), np.arctan((w - 1) / 2.0 / f))  # the narrower half-angle, to the outermost pixel CENTRES
    dist = 1.05 * radius / np.sin(half)
    K = np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]])
    Ks, Es = [], []
    for i in range(int(n)):
        a = 2.0 * np.pi * i / int(n)
        C = centre + dist * np.array([np.sin(a), 0.0, -np.cos(a)])
        z = (centre - C) / dist
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        E = np.eye(4)
        E[:3, :3] = np.stack((x, y, z))
        E[:3, 3] = -E[:3, :3] @ C
        Ks.append(K)
        Es.append(E)
    return np.stack(Ks).astype(np.float32), np.stack(Es).astype(np.float32)


# ---- models -------------------------------------------------------------------------------------------------------------------------

def upload_model(model: dict, device) -> dict:
    """The arrays of read_ply_model as contiguous device tensors (None stays None)."""
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(device)
    return {"vertices": up(model["vertices"], np.float32), "faces": up(model["faces"], np.int32),
            "colors": up(model["colors"], np.uint8), "normals": up(model["normals"], np.float32)}
