"""The depth-to-normal estimator of DESIGN.md section 14 (pmn_depth_normals, csrc/normals.hip) restated in numpy, and the analytic
scenes its tests use.  Written from the estimator's definition, not from the kernel: which neighbours are accepted and whether the
normal equations are singular are decided exactly as defined (float32 comparison, integer moments and determinant); the fit and the
normal are evaluated in float64 (``fit_dtype=np.float64``, the oracle) or in float32 (``np.float32``: the yardstick of what float32
evaluation alone costs -- the tolerance of the GPU tests is a multiple of the distance between the two, never of the kernel's output).
The reference project has no normal estimation, so the truth is analytic: planes, a sphere, a depth step."""
import numpy as np


def depth_normals_ref(depth, K, radius=2, rel_thres=0.01, fit_dtype=np.float64):
    """depth [H,W], K [3,3] -> normals [3,H,W] of dtype ``fit_dtype``: unit, facing the camera, or exactly zero."""
    z = np.ascontiguousarray(depth, np.float32)
    K = np.asarray(K, np.float32)  # the kernel receives float32 intrinsics
    H, W = z.shape
    r, T = int(radius), fit_dtype
    assert r in (1, 2, 3)
    with np.errstate(all="ignore"):
        valid = np.isfinite(z) & (z > 0)
        bound = np.float32(rel_thres) * z  # float32, one rounding
        pad = np.zeros((H + 2 * r, W + 2 * r), np.float32)  # outside the image: 0 = invalid
        pad[r:r + H, r:r + W] = z
        zp = z.astype(T)
        N, Sx, Sy, Sxx, Sxy, Syy = (np.zeros((H, W), np.int64) for _ in range(6))
        b0, b1, b2 = (np.zeros((H, W), T) for _ in range(3))
        for dy in range(-r, r + 1):  # row-major over the window: the order the float32 sums are taken in
            for dx in range(-r, r + 1):
                zq = pad[r + dy:r + dy + H, r + dx:r + dx + W]
                acc = valid & np.isfinite(zq) & (zq > 0) & (np.abs(zq - z) <= bound)  # float32 on both sides
                zqT = zq.astype(T)
                t = np.where(acc, (zp - zqT) / (zp * zqT), T(0))
                N += acc
                Sx += acc * dx
                Sy += acc * dy
                Sxx += acc * (dx * dx)
                Sxy += acc * (dx * dy)
                Syy += acc * (dy * dy)
                b0 = b0 + T(dx) * t
                b1 = b1 + T(dy) * t
                b2 = b2 + t
        A00, A01, A02 = Syy * N - Sy * Sy, Sx * Sy - Sxy * N, Sxy * Sy - Syy * Sx
        A11, A12, A22 = Sxx * N - Sx * Sx, Sxy * Sx - Sxx * Sy, Sxx * Syy - Sxy * Sxy
        D = Sxx * A00 + Sxy * A01 + Sx * A02
        assert np.abs(D).max(initial=0) < 2 ** 24  # exact in float32 too
        ok = valid & (D != 0)
        Dv = np.where(ok, D, 1).astype(T)
        f = lambda a: a.astype(T)
        a = ((f(A00) * b0 + f(A01) * b1) + f(A02) * b2) / Dv
        b = ((f(A01) * b0 + f(A11) * b1) + f(A12) * b2) / Dv
        c = ((f(A02) * b0 + f(A12) * b1) + f(A22) * b2) / Dv
        fx, sk, cx, fy, cy = T(K[0, 0]), T(K[0, 1]), T(K[0, 2]), T(K[1, 1]), T(K[1, 2])
        xs, ys = np.arange(W).astype(T)[None, :], np.arange(H).astype(T)[:, None]
        mx = fx * a
        my = sk * a + fy * b
        mz = ((T(1) / zp + c) + a * (cx - xs)) + b * (cy - ys)
        big = np.fmax(np.fmax(np.abs(mx), np.abs(my)), np.abs(mz))
        ok &= np.isfinite(big) & (big > 0)
        e = np.frexp(np.where(ok, big, T(1)))[1]  # exact power-of-two scaling before the norm
        mx, my, mz = (np.ldexp(np.where(ok, v, T(0)), -e).astype(T) for v in (mx, my, mz))
        length = np.sqrt((mx * mx + my * my) + mz * mz)
        ok &= np.isfinite(length) & (length > 0)
        length = np.where(ok, length, T(1))
        out = np.stack([np.where(ok, -v / length, T(0)) for v in (mx, my, mz)]).astype(T)
    return out


def rays(K, H, W):
    """inverse(K) (x, y, 1)^T at integer pixel coordinates, float64 [3,H,W]."""
    Ki = np.linalg.inv(np.asarray(K, np.float32).astype(np.float64))
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    return np.einsum("ij,jhw->ihw", Ki, np.stack((xs, ys, np.ones_like(xs))))


def angle(n, truth):
    """Angle in radians between unit vectors [3,...] (atan2 form: accurate near 0), float64."""
    n, truth = np.asarray(n, np.float64), np.asarray(truth, np.float64)
    if truth.ndim == 1:
        truth = truth.reshape(3, *([1] * (n.ndim - 1))) * np.ones_like(n)
    cr = np.stack((n[1] * truth[2] - n[2] * truth[1], n[2] * truth[0] - n[0] * truth[2], n[0] * truth[1] - n[1] * truth[0]))
    return np.arctan2(np.sqrt((cr * cr).sum(0)), (n * truth).sum(0))


# ---- cameras and scenes ------------------------------------------------------------------------------------------------------------

def camera(kind, H, W):
    """float32 K for an H x W image: "dtu" (f ~ 2900 at 1600 x 1200, scaled to the image) or "small" (f ~ 200 at 64 px); both with
    fx != fy, non-zero skew and an off-centre principal point."""
    if kind == "dtu":
        s = W / 1600.0
        return np.array([[2892.3 * s, 0.7 * s, 823.2 * s], [0, 2883.2 * (H / 1200.0), 619.1 * (H / 1200.0)], [0, 0, 1]], np.float32)
    s = W / 64.0
    return np.array([[201.5 * s, -0.4 * s, 30.2 * s], [0, 188.7 * (H / 64.0), 35.6 * (H / 64.0)], [0, 0, 1]], np.float32)


def plane_depth(K, H, W, nu, d):
    """Depth of the plane nu . X = d (nu unit, towards +z side so that depth > 0), rendered in float64, rounded to float32."""
    nu = np.asarray(nu, np.float64)
    nu = nu / np.linalg.norm(nu)
    den = np.einsum("i,ihw->hw", nu, rays(K, H, W))
    assert (den > 0).all()
    return (d / den).astype(np.float32), -nu  # truth: the unit normal facing the camera


PLANES = {  # name -> (camera kind, nu, d): DTU-like depths 400-900 and a small scene at z ~ 2
    "dtu_fronto": ("dtu", (0.0, 0.0, 1.0), 650.0),
    "dtu_tilt_x": ("dtu", (0.35, 0.0, 1.0), 600.0),
    "dtu_tilt_xy": ("dtu", (-0.30, 0.45, 1.0), 560.0),
    "small_fronto": ("small", (0.0, 0.0, 1.0), 2.0),
    "small_tilt": ("small", (0.5, -0.35, 1.0), 1.8),
}


def plane_scene(name, H, W):
    kind, nu, d = PLANES[name]
    K = camera(kind, H, W)
    z, truth = plane_depth(K, H, W, nu, d)
    return z, K, truth


def sphere_scene(H, W, kind="small"):
    """A sphere in front of the camera, background invalid (0).  Returns depth, K, truth normals [3,H,W] (zero on the background)."""
    K = camera(kind, H, W)
    ry = rays(K, H, W)
    zc = 2.0 if kind == "small" else 650.0
    c = np.array([0.02 * zc, -0.03 * zc, zc])
    R = 0.12 * zc
    dd = (ry * ry).sum(0)
    dc = np.einsum("i,ihw->hw", c, ry)
    disc = dc * dc - dd * (c @ c - R * R)
    hit = disc > 0
    tt = np.where(hit, (dc - np.sqrt(np.where(hit, disc, 0))) / dd, 0.0)  # ray parameter = depth (rays have z = 1)
    X = ry * tt
    nrm = np.where(hit, (X - c[:, None, None]) / R, 0.0)
    return tt.astype(np.float32), K, nrm


def step_scene(H, W, kind="dtu"):
    """Two planes meeting at the middle column, depths more than rel_thres = 1 % apart.  Returns depth, K, left-side mask."""
    K = camera(kind, H, W)
    s = 650.0 if kind == "dtu" else 2.0
    za, _ = plane_depth(K, H, W, (0.2, 0.1, 1.0), 0.9 * s)
    zb, _ = plane_depth(K, H, W, (-0.15, 0.05, 1.0), 1.1 * s)
    left = np.zeros((H, W), bool)
    left[:, :W // 2] = True
    return np.where(left, za, zb).astype(np.float32), K, left


def random_scene(H, W, seed, kind="dtu"):
    """A tilted plane with 0.3 % multiplicative depth noise (so that the 1 % test accepts most, not all, neighbours) and 10 % of the
    pixels invalidated with every kind of invalid value."""
    rng = np.random.default_rng(seed)
    K = camera(kind, H, W)
    z, _ = plane_depth(K, H, W, (0.25, -0.2, 1.0), 600.0 if kind == "dtu" else 2.0)
    z = (z * (1.0 + 0.003 * rng.standard_normal((H, W)))).astype(np.float32)
    bad = rng.random((H, W)) < 0.10
    z[bad] = rng.choice(np.array([0.0, -1.0, np.nan, np.inf, -np.inf], np.float32), size=int(bad.sum()))
    return z, K
