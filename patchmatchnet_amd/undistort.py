"""Host geometry of the image undistortion (colmap_input.py --undistort), numpy float64.

    distort(camera, u, v)             normalised (u, v) -> the distorted normalised point, every COLMAP model but FOV / THIN_PRISM_FISHEYE
    world_to_pixel / pixel_to_world   the forward model and its Newton inverse
    undistorted_camera(camera, ...)   the ideal PINHOLE camera every image of ``camera`` is resampled into

The per-pixel resampling itself runs on the GPU (pmn_undistort_image through ops.undistort_image, the same formulas in the same
operation order); the inverse is needed only at the 2 (W + H) border pixels of a camera and stays on the host.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from .colmap import CAMERA_MODEL_IDS, CAMERA_MODELS, Camera

PINHOLE_MODELS = ("SIMPLE_PINHOLE", "PINHOLE")
REFUSED_MODELS = ("FOV", "THIN_PRISM_FISHEYE")
NEWTON_STEPS = 100
NEWTON_TOL = 1e-12
_JAC_EPS = 1e-6  # central differences: the Jacobian only steers the iteration, the residual decides where it ends


class UndistortError(ValueError):
    """A camera that cannot be undistorted: the message names the camera id and the model."""


def check_model(camera: Camera) -> None:
    if camera.model in REFUSED_MODELS or camera.model not in CAMERA_MODEL_IDS:
        raise UndistortError(f"camera {camera.id}: model {camera.model} is not supported by --undistort (supported: every COLMAP "
                             f"model but {' and '.join(REFUSED_MODELS)})")


def focal_and_center(camera: Camera) -> Tuple[float, float, float, float]:
    p = dict(zip(CAMERA_MODELS[CAMERA_MODEL_IDS[camera.model]][1], camera.params))
    fx, fy = (p["f"], p["f"]) if "f" in p else (p["fx"], p["fy"])
    return float(fx), float(fy), float(p["cx"]), float(p["cy"])


def distortion_params(camera: Camera) -> Tuple[float, ...]:
    """The parameters after the intrinsics, in COLMAP's order."""
    names = CAMERA_MODELS[CAMERA_MODEL_IDS[camera.model]][1]
    return tuple(float(v) for v in camera.params[names.index("cy") + 1:])


def has_distortion(camera: Camera) -> bool:
    return any(v != 0 for v in distortion_params(camera))


def distort(camera: Camera, u, v):
    """(u, v) -> (ud, vd), arrays or scalars, in the operation order of pmn_undistort_image."""
    check_model(camera)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    k = distortion_params(camera)
    m = camera.model
    with np.errstate(all="ignore"):
        if m in PINHOLE_MODELS:
            return u, v
        if m in ("SIMPLE_RADIAL", "RADIAL"):
            r2 = u * u + v * v
            rad = k[0] * r2
            if m == "RADIAL":
                rad = rad + k[1] * (r2 * r2)
            return u + u * rad, v + v * rad
        if m in ("OPENCV", "FULL_OPENCV"):
            uu, vv, uv = u * u, v * v, u * v
            r2 = uu + vv
            r4 = r2 * r2
            if m == "OPENCV":
                k1, k2, p1, p2 = k
                rad = k1 * r2 + k2 * r4
                du = (u * rad + (2.0 * p1) * uv) + p2 * (r2 + 2.0 * uu)
                dv = (v * rad + (2.0 * p2) * uv) + p1 * (r2 + 2.0 * vv)
            else:
                k1, k2, p1, p2, k3, k4, k5, k6 = k
                r6 = r4 * r2
                rad = (((1.0 + k1 * r2) + k2 * r4) + k3 * r6) / (((1.0 + k4 * r2) + k5 * r4) + k6 * r6)
                du = ((u * rad + (2.0 * p1) * uv) + p2 * (r2 + 2.0 * uu)) - u
                dv = ((v * rad + (2.0 * p2) * uv) + p1 * (r2 + 2.0 * vv)) - v
            return u + du, v + dv
        r = np.sqrt(u * u + v * v)
        small = r < 1e-12
        rs = np.where(small, 1.0, r)
        th = np.arctan(r)
        t2 = th * th
        if m == "OPENCV_FISHEYE":
            t4 = t2 * t2
            thd = th * ((((1.0 + k[0] * t2) + k[1] * t4) + k[2] * (t4 * t2)) + k[3] * (t4 * t4))
            du = np.where(small, 0.0, (u * thd) / rs - u)
            dv = np.where(small, 0.0, (v * thd) / rs - v)
            return u + du, v + dv
        uf = np.where(small, u, (u * th) / rs)
        vf = np.where(small, v, (v * th) / rs)
        rad = k[0] * t2
        if m == "RADIAL_FISHEYE":
            rad = rad + k[1] * (t2 * t2)
        return uf + uf * rad, vf + vf * rad


def world_to_pixel(camera: Camera, u, v):
    """Normalised (u, v) -> pixel (px, py) of the distorted picture (pixel centres at +0.5)."""
    fx, fy, cx, cy = focal_and_center(camera)
    ud, vd = distort(camera, u, v)
    return fx * ud + cx, fy * vd + cy


def undistort_normalised(camera: Camera, ud, vd):
    """Newton's method on x + d(x) = x_d from x = x_d: at most NEWTON_STEPS steps, until the step is below NEWTON_TOL.  Returns
    (u, v, converged); a point that did not converge (or left the finite numbers) is flagged, never silently kept."""
    xd = np.stack([np.asarray(ud, np.float64).ravel(), np.asarray(vd, np.float64).ravel()], axis=1)
    x = xd.copy()
    done = np.zeros(len(x), bool)
    with np.errstate(all="ignore"):
        for _ in range(NEWTON_STEPS):
            act = ~done
            if not act.any():
                break
            p = x[act]
            f = np.stack(distort(camera, p[:, 0], p[:, 1]), axis=1) - xd[act]
            hu = _JAC_EPS * np.maximum(1.0, np.abs(p[:, 0]))
            hv = _JAC_EPS * np.maximum(1.0, np.abs(p[:, 1]))
            fu = (np.stack(distort(camera, p[:, 0] + hu, p[:, 1]), 1) - np.stack(distort(camera, p[:, 0] - hu, p[:, 1]), 1)) / (2 * hu)[:, None]
            fv = (np.stack(distort(camera, p[:, 0], p[:, 1] + hv), 1) - np.stack(distort(camera, p[:, 0], p[:, 1] - hv), 1)) / (2 * hv)[:, None]
            det = fu[:, 0] * fv[:, 1] - fv[:, 0] * fu[:, 1]
            su = (fv[:, 1] * f[:, 0] - fv[:, 0] * f[:, 1]) / det
            sv = (fu[:, 0] * f[:, 1] - fu[:, 1] * f[:, 0]) / det
            step = np.stack([su, sv], axis=1)
            bad = ~np.isfinite(step).all(axis=1)
            step[bad] = 0.0
            x[act] = p - step
            conv = (np.abs(step).max(axis=1) < NEWTON_TOL) & ~bad
            idx = np.flatnonzero(act)
            done[idx[conv]] = True
            dead = idx[bad]  # a singular or non-finite step: this point cannot converge; stop iterating it
            x[dead] = np.nan
            done[dead] = True
    ok = done & np.isfinite(x).all(axis=1)
    shape = np.asarray(ud).shape
    return x[:, 0].reshape(shape), x[:, 1].reshape(shape), ok.reshape(shape)


def pixel_to_world(camera: Camera, px, py):
    """Pixel of the distorted picture -> normalised (u, v, converged)."""
    fx, fy, cx, cy = focal_and_center(camera)
    return undistort_normalised(camera, (np.asarray(px, np.float64) - cx) / fx, (np.asarray(py, np.float64) - cy) / fy)


def _side(camera: Camera, px, py, axis: int, what: str) -> Tuple[float, float]:
    """min / max pinhole coordinate (x for axis 0, y for axis 1) of one image side's undistorted border pixels."""
    fx, fy, cx, cy = focal_and_center(camera)
    u, v, ok = pixel_to_world(camera, px, py)
    if not ok.any():
        raise UndistortError(f"camera {camera.id} ({camera.model}): no pixel of the {what} border could be undistorted (Newton's "
                             "method did not converge): the distortion is not invertible there")
    c = (fx * u + cx) if axis == 0 else (fy * v + cy)
    c = c[ok]
    return float(c.min()), float(c.max())


def undistorted_camera(camera: Camera, blank_pixels: float = 0.0, min_scale: float = 0.2, max_scale: float = 2.0,
                       max_image_size: int = -1) -> Camera:
    """The PINHOLE camera (same fx, fy) the pictures of ``camera`` are resampled into: DESIGN.md section 21.  blank_pixels 0 keeps
    only output pixels that see the source everywhere, 1 keeps every source pixel.  A pinhole camera is returned as it is (and is
    only ever resized by max_image_size)."""
    check_model(camera)
    fx, fy, cx, cy = focal_and_center(camera)
    W, H = int(camera.width), int(camera.height)
    if camera.model in PINHOLE_MODELS:
        out = camera
    else:
        ys, xs = np.arange(H) + 0.5, np.arange(W) + 0.5
        left_min_x, left_max_x = _side(camera, np.full(H, 0.5), ys, 0, "left")
        right_min_x, right_max_x = _side(camera, np.full(H, W - 0.5), ys, 0, "right")
        top_min_y, top_max_y = _side(camera, xs, np.full(W, 0.5), 1, "top")
        bottom_min_y, bottom_max_y = _side(camera, xs, np.full(W, H - 0.5), 1, "bottom")
        with np.errstate(all="ignore"):
            min_scale_x = min(np.float64(cx) / (cx - left_min_x), np.float64(W - 0.5 - cx) / (right_max_x - cx))
            max_scale_x = max(np.float64(cx) / (cx - left_max_x), np.float64(W - 0.5 - cx) / (right_min_x - cx))
            min_scale_y = min(np.float64(cy) / (cy - top_min_y), np.float64(H - 0.5 - cy) / (bottom_max_y - cy))
            max_scale_y = max(np.float64(cy) / (cy - top_max_y), np.float64(H - 0.5 - cy) / (bottom_min_y - cy))
            scale_x = 1.0 / (min_scale_x * blank_pixels + max_scale_x * (1.0 - blank_pixels))
            scale_y = 1.0 / (min_scale_y * blank_pixels + max_scale_y * (1.0 - blank_pixels))
        if not (np.isfinite(scale_x) and np.isfinite(scale_y)):
            raise UndistortError(f"camera {camera.id} ({camera.model}): the undistorted image bounds are degenerate")
        scale_x = min(max(float(scale_x), min_scale), max_scale)
        scale_y = min(max(float(scale_y), min_scale), max_scale)
        Wn, Hn = max(1, int(scale_x * W)), max(1, int(scale_y * H))
        out = Camera(camera.id, "PINHOLE", Wn, Hn, (fx, fy, cx * Wn / W, cy * Hn / H))
    if max_image_size > 0 and max(out.width, out.height) > max_image_size:
        ofx, ofy, ocx, ocy = focal_and_center(out)
        s = max_image_size / max(out.width, out.height)
        Wn, Hn = int(out.width * s), int(out.height * s)
        if Wn < 1 or Hn < 1:
            raise UndistortError(f"camera {camera.id}: max_image_size {max_image_size} leaves no pixel of a {out.width} x {out.height} image")
        rx, ry = Wn / out.width, Hn / out.height
        out = Camera(camera.id, "PINHOLE", Wn, Hn, (ofx * rx, ofy * ry, ocx * rx, ocy * ry))
    return out
