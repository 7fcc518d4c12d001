"""Float64 numpy oracle of the image undistortion, written from the definition and independent of
patchmatchnet_amd/undistort.py: the camera models, the Newton inverse (plain Python floats, one point at a time), the undistorted
camera, and the warp -- which returns the uint8 image, the valid mask, the sampling coordinates and the float64 values before
rounding.  ``write_case`` puts a synthetic COLMAP model whose pictures have their cameras' sizes on disk (colmap_synth.write_images
writes 24 x 32 pictures for 64 x 48 cameras: fine for the plain import, useless for undistortion).

Cameras are plain tuples here: (model name, width, height, params in COLMAP's order).
"""
from __future__ import annotations

import math
import os

import numpy as np

SINGLE_FOCAL = ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE")
SUPPORTED = SINGLE_FOCAL + ("PINHOLE", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV")


def load_cli():
    """This repository's colmap_input.py as a module, by path (other trees on sys.path have a script of the same name)."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap_input.py")
    spec = importlib.util.spec_from_file_location("pmn_colmap_input_cli", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def split(cam):
    """(fx, fy, cx, cy, distortion parameters)"""
    model, _, _, p = cam
    if model not in SUPPORTED:
        raise ValueError(f"oracle: model {model} is not supported")
    if model in SINGLE_FOCAL:
        return p[0], p[0], p[1], p[2], tuple(p[3:])
    return p[0], p[1], p[2], p[3], tuple(p[4:])


def distort(model, k, u, v):
    """The table of section 21 on numpy arrays (or numpy scalars): (u, v) -> (u + du, v + dv)."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        if model in ("SIMPLE_PINHOLE", "PINHOLE"):
            return u, v
        if model == "SIMPLE_RADIAL":
            rad = k[0] * (u * u + v * v)
            return u + u * rad, v + v * rad
        if model == "RADIAL":
            r2 = u * u + v * v
            rad = k[0] * r2 + k[1] * (r2 * r2)
            return u + u * rad, v + v * rad
        if model == "OPENCV":
            k1, k2, p1, p2 = k
            r2 = u * u + v * v
            rad = k1 * r2 + k2 * (r2 * r2)
            du = (u * rad + (2.0 * p1) * (u * v)) + p2 * (r2 + 2.0 * (u * u))
            dv = (v * rad + (2.0 * p2) * (u * v)) + p1 * (r2 + 2.0 * (v * v))
            return u + du, v + dv
        if model == "FULL_OPENCV":
            k1, k2, p1, p2, k3, k4, k5, k6 = k
            r2 = u * u + v * v
            r4 = r2 * r2
            r6 = r4 * r2
            rad = (((1.0 + k1 * r2) + k2 * r4) + k3 * r6) / (((1.0 + k4 * r2) + k5 * r4) + k6 * r6)
            du = ((u * rad + (2.0 * p1) * (u * v)) + p2 * (r2 + 2.0 * (u * u))) - u
            dv = ((v * rad + (2.0 * p2) * (u * v)) + p1 * (r2 + 2.0 * (v * v))) - v
            return u + du, v + dv
        r = np.sqrt(u * u + v * v)
        tiny = r < 1e-12
        safe = np.where(tiny, 1.0, r)
        theta = np.arctan(r)
        t2 = theta * theta
        if model == "OPENCV_FISHEYE":
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            thd = theta * ((((1.0 + k[0] * t2) + k[1] * t4) + k[2] * t6) + k[3] * t8)
            du = np.where(tiny, 0.0, (u * thd) / safe - u)
            dv = np.where(tiny, 0.0, (v * thd) / safe - v)
            return u + du, v + dv
        uf = np.where(tiny, u, (u * theta) / safe)
        vf = np.where(tiny, v, (v * theta) / safe)
        rad = k[0] * t2
        if model == "RADIAL_FISHEYE":
            rad = rad + k[1] * (t2 * t2)
        return uf + uf * rad, vf + vf * rad


def project(cam, u, v):
    """normalised -> pixel of the distorted picture"""
    fx, fy, cx, cy, k = split(cam)
    ud, vd = distort(cam[0], k, u, v)
    return fx * ud + cx, fy * vd + cy


def _distort1(model, k, u, v):
    a, b = distort(model, k, np.float64(u), np.float64(v))
    return float(a), float(b)


def unproject1(cam, px, py):
    """One pixel -> normalised (u, v), or None when Newton's method (at most 100 steps, until the step is below 1e-12) fails."""
    fx, fy, cx, cy, k = split(cam)
    xd, yd = (px - cx) / fx, (py - cy) / fy
    u, v = xd, yd
    h = 1e-7
    for _ in range(100):
        a, b = _distort1(cam[0], k, u, v)
        a1, b1 = _distort1(cam[0], k, u + h, v)
        a0, b0 = _distort1(cam[0], k, u - h, v)
        c1, d1 = _distort1(cam[0], k, u, v + h)
        c0, d0 = _distort1(cam[0], k, u, v - h)
        jaa, jba = (a1 - a0) / (2 * h), (b1 - b0) / (2 * h)   # d(a, b) / du
        jab, jbb = (c1 - c0) / (2 * h), (d1 - d0) / (2 * h)   # d(a, b) / dv
        det = jaa * jbb - jab * jba
        ra, rb = a - xd, b - yd
        if not (math.isfinite(det) and det != 0 and math.isfinite(ra) and math.isfinite(rb)):
            return None
        su, sv = (jbb * ra - jab * rb) / det, (jaa * rb - jba * ra) / det
        u, v = u - su, v - sv
        if max(abs(su), abs(sv)) < 1e-12:
            return u, v
    return None


def undistorted_camera(cam, blank_pixels=0.0, min_scale=0.2, max_scale=2.0, max_image_size=-1):
    """('PINHOLE', W', H', (fx, fy, cx', cy')) by the bounds / scales rule of section 21; a pinhole input is returned as it is unless
    max_image_size shrinks it."""
    model, W, H, _ = cam
    fx, fy, cx, cy, _ = split(cam)
    out = cam
    if model not in ("SIMPLE_PINHOLE", "PINHOLE"):
        def side(points, axis):
            got = [unproject1(cam, x, y) for x, y in points]
            vals = [(fx * g[0] + cx, fy * g[1] + cy)[axis] for g in got if g is not None]
            if not vals:
                raise ValueError("oracle: a whole side of the border failed to undistort")
            return min(vals), max(vals)
        left = side([(0.5, y + 0.5) for y in range(H)], 0)
        right = side([(W - 0.5, y + 0.5) for y in range(H)], 0)
        top = side([(x + 0.5, 0.5) for x in range(W)], 1)
        bottom = side([(x + 0.5, H - 0.5) for x in range(W)], 1)

        def scale(c, size, lo, hi):
            smin = min(c / (c - lo[0]), (size - 0.5 - c) / (hi[1] - c))
            smax = max(c / (c - lo[1]), (size - 0.5 - c) / (hi[0] - c))
            s = 1.0 / (smin * blank_pixels + smax * (1.0 - blank_pixels))
            return min(max(s, min_scale), max_scale)
        Wn = max(1, int(scale(cx, W, left, right) * W))
        Hn = max(1, int(scale(cy, H, top, bottom) * H))
        out = ("PINHOLE", Wn, Hn, (fx, fy, cx * Wn / W, cy * Hn / H))
    if max_image_size > 0 and max(out[1], out[2]) > max_image_size:
        ofx, ofy, ocx, ocy, _ = split(out)
        s = max_image_size / max(out[1], out[2])
        Wn, Hn = int(out[1] * s), int(out[2] * s)
        out = ("PINHOLE", Wn, Hn, (ofx * (Wn / out[1]), ofy * (Hn / out[2]), ocx * (Wn / out[1]), ocy * (Hn / out[2])))
    return out


def warp(image, cam, dst):
    """image uint8 [Hs, Ws] or [Hs, Ws, C] seen through ``cam`` -> (uint8 image [Hd, Wd(, C)], valid bool [Hd, Wd], coords float64
    [Hd, Wd, 2] = (sx, sy), values float64 before rounding, zero where invalid).  The per-pixel rule of section 21, step by step."""
    img = image if image.ndim == 3 else image[..., None]
    Hs, Ws, C = img.shape
    fx, fy, cx, cy, k = split(cam)
    dfx, dfy, dcx, dcy, _ = split(dst)
    Wd, Hd = dst[1], dst[2]
    x, y = np.meshgrid(np.arange(Wd, dtype=np.float64), np.arange(Hd, dtype=np.float64))
    with np.errstate(all="ignore"):
        u = ((x + 0.5) - dcx) / dfx
        v = ((y + 0.5) - dcy) / dfy
        ud, vd = distort(cam[0], k, u, v)
        sx = (fx * ud + cx) - 0.5
        sy = (fy * vd + cy) - 0.5
        x0, y0 = np.floor(sx), np.floor(sy)
        valid = (x0 >= 0) & (y0 >= 0) & (x0 + 1 <= Ws - 1) & (y0 + 1 <= Hs - 1)   # NaN and infinity compare false
    xi = np.where(valid, x0, 0).astype(np.int64)
    yi = np.where(valid, y0, 0).astype(np.int64)
    xi1, yi1 = np.minimum(xi + 1, Ws - 1), np.minimum(yi + 1, Hs - 1)
    with np.errstate(invalid="ignore"):
        ax = np.where(valid, sx - x0, 0.0)[..., None]
        ay = np.where(valid, sy - y0, 0.0)[..., None]
    f = img.astype(np.float64)
    s00, s01, s10, s11 = f[yi, xi], f[yi, xi1], f[yi1, xi], f[yi1, xi1]
    val = (1 - ay) * ((1 - ax) * s00 + ax * s01) + ay * ((1 - ax) * s10 + ax * s11)
    val = np.where(valid[..., None], val, 0.0)
    out = np.floor(val + 0.5).astype(np.uint8)
    if image.ndim == 2:
        out, val = out[..., 0], val[..., 0]
    return out, valid, np.stack([sx, sy], axis=-1), val


def near_tie(values, band=1e-6):
    """Samples whose value before rounding lies within ``band`` of a .5 tie."""
    return np.abs((values - np.floor(values)) - 0.5) <= band


def write_case(root, camera_models=("SIMPLE_RADIAL", "OPENCV", "SIMPLE_PINHOLE"), seed=21, n_images=6, width=64, height=48,
               distortion=0.08):
    """A colmap_synth model with its distortion parameters scaled up to something visible (the picture corners move by a pixel or
    two), and one seeded JPEG per image AT ITS
    CAMERA'S SIZE under <root>/images.  Returns (cameras as oracle tuples by id, image tuples of colmap_synth)."""
    import colmap_synth as CS
    from PIL import Image as PilImage
    cams, imgs, pts = CS.make_model(seed=seed, n_images=n_images, n_points=240, keypoints=150, mean_track=3.5,
                                    camera_models=camera_models, width=width, height=height)
    rng = np.random.default_rng(seed)
    scaled = []
    for cid, model, w, h, params in cams:
        n_intr = 3 if model in SINGLE_FOCAL else 4
        # colmap_synth draws every distortion parameter from +-0.01: the radial ones are scaled to +-distortion, the tangential
        # ones (OPENCV's p1, p2) to a quarter of that
        gain = [distortion / 0.01] * (len(params) - n_intr)
        if model == "OPENCV":
            gain[2] = gain[3] = distortion / 0.04
        params = list(params[:n_intr]) + [float(p) * g for p, g in zip(params[n_intr:], gain)]
        scaled.append((cid, model, w, h, params))
    CS.write_model(os.path.join(root, "sparse"), scaled, imgs, pts)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    for im in imgs:
        # smooth-ish content (a coarse random field blown up) so that JPEG keeps it recognisable; the tests compare exact bytes anyway
        coarse = rng.integers(0, 256, (height // 4, width // 4, 3), dtype=np.uint8)
        arr = np.repeat(np.repeat(coarse, 4, axis=0), 4, axis=1)
        PilImage.fromarray(arr).save(os.path.join(root, "images", im[4]), quality=92)
    return {c[0]: (c[1], c[2], c[3], tuple(c[4])) for c in scaled}, imgs


# ---- the cases of tests/test_undistort.py and tests/test_undistort_gpu.py --------------------------------------------------------
# name -> dict(cam = oracle camera tuple, channels, seed, and either dst = an explicit output camera or kw = the arguments of
# undistorted_camera).  Sizes are odd on purpose (53 x 37: the 4-pixel tail and partial 128 x 8 tiles run); 64 x 48 has full groups.
def _same_size_pinhole(cam):
    fx, fy, cx, cy, _ = split(cam)
    return ("PINHOLE", cam[1], cam[2], (fx, fy, cx, cy))


CASES = {
    # strong barrel distortion
    "radial_barrel": dict(cam=("RADIAL", 64, 48, (60.0, 31.3, 24.4, -0.15, 0.02)), channels=3, seed=1, kw={}),
    # k = +0.2 and -0.2 at f = 45 with every source pixel kept (blank_pixels = 1): 1.7 % and 13 % of the output lie outside the source
    "simple_radial_pincushion": dict(cam=("SIMPLE_RADIAL", 53, 37, (45.0, 26.2, 18.9, 0.2)), channels=3, seed=2, kw=dict(blank_pixels=1.0)),
    "simple_radial_blank": dict(cam=("SIMPLE_RADIAL", 53, 37, (45.0, 26.2, 18.9, -0.2)), channels=3, seed=17, kw=dict(blank_pixels=1.0)),
    "simple_radial_barrel_grey": dict(cam=("SIMPLE_RADIAL", 53, 37, (50.0, 27.0, 18.0, -0.12)), channels=1, seed=3, kw={}),
    # tangential terms
    "opencv_tangential": dict(cam=("OPENCV", 64, 48, (58.0, 59.0, 32.4, 23.7, -0.1, 0.01, 0.01, -0.008)), channels=3, seed=4, kw={}),
    "opencv_odd": dict(cam=("OPENCV", 53, 37, (47.0, 46.0, 26.0, 19.0, 0.08, -0.01, -0.004, 0.006)), channels=3, seed=5,
                       kw=dict(blank_pixels=0.5)),
    "full_opencv": dict(cam=("FULL_OPENCV", 53, 37, (48.0, 48.5, 26.4, 18.2, -0.1, 0.02, 0.003, -0.002, 0.001, 0.05, -0.01, 0.002)),
                        channels=3, seed=6, kw={}),
    # the denominator 1 + k4 r2 is EXACTLY zero on the four pixels 4 to the side and 4 up / down of the principal point (f = 32, so
    # r2 = 32 / 1024 there and k4 = -32), changes sign around them, and: "inf" has a non-zero numerator there, "nan" a zero one
    "full_opencv_inf": dict(cam=("FULL_OPENCV", 53, 37, (32.0, 32.0, 26.5, 18.5, -30.0, 1.0, 0.002, -0.001, 0.0, -32.0, 0.0, 0.0)),
                            channels=3, seed=7, dst="same"),
    "full_opencv_nan": dict(cam=("FULL_OPENCV", 53, 37, (32.0, 32.0, 26.5, 18.5, -32.0, 0.0, 0.002, -0.001, 0.0, -32.0, 0.0, 0.0)),
                            channels=1, seed=8, dst="same"),
    # fisheye with the principal point on a pixel centre of source and output: pixel (26, 18) has r = 0 exactly
    "fisheye_centre": dict(cam=("OPENCV_FISHEYE", 53, 37, (30.0, 30.0, 26.5, 18.5, 0.02, -0.005, 0.001, 0.0002)), channels=3, seed=9,
                           dst="same"),
    "fisheye_grey": dict(cam=("OPENCV_FISHEYE", 53, 37, (40.0, 41.0, 26.1, 18.3, -0.01, 0.004, 0.0, 0.0)), channels=1, seed=10, kw={}),
    # wide fisheye, every source pixel kept: the scale clamps at max_scale = 2 and the output (128 x 96) is larger than the source
    "fisheye_max_scale": dict(cam=("OPENCV_FISHEYE", 64, 48, (26.0, 26.0, 32.5, 24.5, 0.0, 0.0, 0.0, 0.0)), channels=3, seed=11,
                              kw=dict(blank_pixels=1.0)),
    "simple_radial_fisheye": dict(cam=("SIMPLE_RADIAL_FISHEYE", 53, 37, (36.0, 26.5, 18.5, 0.03)), channels=1, seed=12, dst="same"),
    "radial_fisheye": dict(cam=("RADIAL_FISHEYE", 64, 48, (40.0, 31.8, 24.1, -0.02, 0.004)), channels=3, seed=13, kw={}),
    # an output smaller than the source
    "radial_max_image_size": dict(cam=("RADIAL", 64, 48, (60.0, 31.3, 24.4, -0.15, 0.02)), channels=3, seed=14,
                                  kw=dict(blank_pixels=1.0, max_image_size=40)),
    "pinhole_max_image_size": dict(cam=("PINHOLE", 53, 37, (50.0, 51.0, 26.3, 18.6)), channels=3, seed=15, kw=dict(max_image_size=31)),
    "simple_pinhole_resized_grey": dict(cam=("SIMPLE_PINHOLE", 53, 37, (50.0, 26.3, 18.6)), channels=1, seed=16, kw=dict(max_image_size=30)),
}


def case_dst(case):
    return _same_size_pinhole(case["cam"]) if case.get("dst") == "same" else undistorted_camera(case["cam"], **case["kw"])


def case_image(case):
    _, W, H, _ = case["cam"]
    shape = (H, W, 3) if case["channels"] == 3 else (H, W)
    return np.random.default_rng(case["seed"]).integers(0, 256, shape, dtype=np.uint8)
