"""Numpy brute force of plane segmentation (pmn_plane_score, pmn_plane_inliers, pointcloud.segment_plane /
segment_planes, segment_cloud.py).  Nothing is shared with the product: the host expressions of pointcloud.py (hypotheses, refit, sign
rule, rmse) are restated here term by term, the sums are math.fsum over the float64 terms, and every count is a plain comparison of
float64 arrays that numpy evaluates in the written order, one rounding per operation, as the kernels do without contraction.

Also the case builders; tests/test_plane_ref.py asserts on this file alone that the cases contain what they are meant to."""
import math

import numpy as np

SUMS = 10
MAX_HYPOTHESES = 4096


# ---- definition -------------------------------------------------------------------------------------------------------------------
def _inlier_mask(points, plane, threshold, normals=None, active=None, min_cos=0.0):
    p = np.asarray(points, np.float32).astype(np.float64)
    a, b, c, d = (float(v) for v in plane)
    if not all(math.isfinite(v) for v in (a, b, c, d)):
        return np.zeros(len(p), bool)
    r = a * p[:, 0] + b * p[:, 1] + c * p[:, 2] + d
    m = np.abs(r) <= threshold
    if normals is not None and min_cos > 0.0:
        q = np.asarray(normals, np.float32).astype(np.float64)
        m &= np.abs(a * q[:, 0] + b * q[:, 1] + c * q[:, 2]) >= min_cos
    if active is not None:
        m &= np.asarray(active) != 0
    return m


def score(points, planes, threshold, normals=None, active=None, min_cos=0.0):
    """int32 [H]: the inliers of every plane row."""
    return np.array([int(_inlier_mask(points, pl, threshold, normals, active, min_cos).sum()) for pl in np.asarray(planes, np.float64)],
                    np.int32)


def frame(points, active=None):
    """(centre, extent): the centre (lo + hi) * 0.5 of the active bounding box and the bound of |p - centre|."""
    p = np.asarray(points, np.float32).astype(np.float64)
    if active is not None:
        p = p[np.asarray(active) != 0]
    lo, hi = p.min(0), p.max(0)
    centre = (lo + hi) * 0.5
    return centre, np.maximum(hi - centre, centre - lo)


def _terms(points, mask, centre):
    a = np.asarray(points, np.float32).astype(np.float64)[mask] - np.asarray(centre, np.float64)
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    return [np.ones(len(a)), ax, ay, az, ax * ax, ax * ay, ax * az, ay * ay, ay * az, az * az]


def inliers_and_sums(points, plane, threshold, normals=None, active=None, min_cos=0.0, centre=None):
    """(mask bool [n], sums float64 [10] by math.fsum, mags float64 [10] = sum |term|)."""
    if centre is None:
        centre = frame(points, active)[0]
    mask = _inlier_mask(points, plane, threshold, normals, active, min_cos)
    terms = _terms(points, mask, centre)
    return mask, np.array([math.fsum(t) for t in terms]), np.array([math.fsum(np.abs(t)) for t in terms])


def sum_bounds(extent):
    E = np.asarray(extent, np.float64)
    return np.array([1.0, E[0], E[1], E[2], E[0] * E[0], E[0] * E[1], E[0] * E[2], E[1] * E[1], E[1] * E[2], E[2] * E[2]])


def qualifies(points, mask, centre, extent):
    """True when every non-zero term of every sum is at least 2^-80 of its sum's bound: the digit sum then loses nothing (a term's 53 bits
    lie above 2^-133 of the bound, the digits reach down to 2^-157) and equals math.fsum."""
    for t, b in zip(_terms(points, mask, centre), sum_bounds(extent)):
        nz = np.abs(t[t != 0.0])
        if len(nz) and nz.min() < b * 2.0 ** -80:
            return False
    return True


def sign_rule(nrm):
    nrm = np.asarray(nrm, np.float64)
    k = int(np.argmax(np.abs(nrm)))  # the first of equal magnitudes: the lowest axis
    return -nrm if nrm[k] < 0.0 else nrm


def hypotheses(points, triplets):
    """float64 [H,4]: the plane through the three points points[triplets[h]], a NaN row where it is invalid."""
    p = np.asarray(points, np.float32).astype(np.float64)
    out = np.full((len(triplets), 4), np.nan)
    for h, (i, j, k) in enumerate(np.asarray(triplets)):
        if i == j or i == k or j == k:
            continue
        p0, p1, p2 = p[i], p[j], p[k]
        u, v = p1 - p0, p2 - p0
        w = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
        l2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
        if not l2 > 0.0:
            continue
        nrm = sign_rule(w / np.sqrt(l2))
        d = -(nrm[0] * p0[0] + nrm[1] * p0[1] + nrm[2] * p0[2])
        row = np.array([nrm[0], nrm[1], nrm[2], d])
        if np.isfinite(row).all():
            out[h] = row
    return out


def refit(sums, centre):
    cnt = sums[0]
    if cnt < 3.0:
        return None
    m = sums[1:4] / cnt
    C = np.empty((3, 3))
    for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[i, j] = C[j, i] = sums[4 + k] / cnt - m[i] * m[j]
    if not np.isfinite(C).all():
        return None
    nrm = sign_rule(np.linalg.eigh(C)[1][:, 0])
    d = -(nrm[0] * (centre[0] + m[0]) + nrm[1] * (centre[1] + m[1]) + nrm[2] * (centre[2] + m[2]))
    plane = np.array([nrm[0], nrm[1], nrm[2], d])
    return plane if np.isfinite(plane).all() else None


def rmse_from_sums(s, c, p):
    if s[0] < 1.0:
        return 0.0
    e = p[0] * c[0] + p[1] * c[1] + p[2] * c[2] + p[3]
    q = (p[0] * p[0] * s[4] + p[1] * p[1] * s[7] + p[2] * p[2] * s[9]
         + 2.0 * (p[0] * p[1] * s[5] + p[0] * p[2] * s[6] + p[1] * p[2] * s[8]))
    total = q + 2.0 * e * (p[0] * s[1] + p[1] * s[2] + p[2] * s[3]) + s[0] * e * e
    return float(np.sqrt(max(total, 0.0) / s[0]))


def _one(points, normals, active, threshold, min_cos, H, refine, rng):
    idx = np.flatnonzero(np.ones(len(points), bool) if active is None else np.asarray(active) != 0)
    if len(idx) < 3:
        raise ValueError("fewer than 3 active points")
    trip = rng.integers(0, len(idx), size=(H, 3))
    planes = hypotheses(points, idx[trip])
    if np.isnan(planes).any(1).all():
        raise ValueError("every hypothesis is invalid")
    counts = score(points, planes, threshold, normals, active, min_cos)
    best = int(np.argmax(counts))
    centre, _ = frame(points, active)
    plane = planes[best]
    mask, sums, _ = inliers_and_sums(points, plane, threshold, normals, active, min_cos, centre)
    refits, rejected = 0, False
    for _ in range(refine):
        new = refit(sums, centre)
        if new is None:
            break
        mask2, sums2, _ = inliers_and_sums(points, new, threshold, normals, active, min_cos, centre)
        if sums2[0] < sums[0]:
            rejected = True
            break
        same = np.array_equal(mask2, mask)
        plane, mask, sums, refits = new, mask2, sums2, refits + 1
        if same:
            break
    return {"plane": plane, "inliers": mask, "count": int(sums[0]), "rmse": rmse_from_sums(sums, centre, plane), "hypothesis": best,
            "refits": refits, "rejected": rejected, "counts": counts}


def _cos(normal_angle):
    return 0.0 if normal_angle is None else min(1.0, max(0.0, float(np.cos(np.radians(float(normal_angle))))))


def segment_plane(points, threshold, hypotheses=1024, seed=0, refine=3, normals=None, normal_angle=None, active=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    return _one(points, normals, active, threshold, _cos(normal_angle), hypotheses, refine, rng)


def segment_planes(points, threshold, max_planes=1, min_inliers=3, hypotheses=1024, seed=0, refine=3, normals=None, normal_angle=None,
                   active=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    left = np.ones(len(points), bool) if active is None else np.asarray(active) != 0
    labels = np.full(len(points), -1, np.int64)
    results = []
    while len(results) < max_planes and left.sum() >= 3:
        one = _one(points, normals, left, threshold, _cos(normal_angle), hypotheses, refine, rng)
        if one["count"] < min_inliers:
            break
        labels[one["inliers"]] = len(results)
        left = left & ~one["inliers"]
        results.append(one)
    return {"labels": labels, "planes": np.array([r["plane"] for r in results]).reshape(-1, 4), "counts": [r["count"] for r in results],
            "results": results}


# ---- cases ------------------------------------------------------------------------------------------------------------------------
PLANTED_S = 0.01  # half-width of the planted plane's noise


def planted_scene(seed=0):
    """About 4000 points: a tilted plane patch with uniform noise of half-width PLANTED_S along its normal (`planted`), a sphere that
    stands on it and uniform clutter on both sides.  Returns (points float32, planted bool, plane float64 [4] as planted, normals
    float32: the patch's normal on the patch, outward on the sphere, random on the clutter)."""
    rng = np.random.default_rng(seed)
    nrm = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0])
    e1 = np.cross(nrm, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    origin = np.array([0.1, -0.2, 0.3])
    uv = rng.uniform(-1.0, 1.0, (2200, 2))
    # float32 rounding moves a point by less than 2^-24 * 2: the residuals stay far inside 2 * PLANTED_S
    patch = origin + uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.uniform(-PLANTED_S, PLANTED_S, (2200, 1)) * nrm
    d = rng.standard_normal((1100, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sphere = origin + 0.5 * nrm + 0.4 * d
    clutter = origin + rng.uniform(-1.5, 1.5, (700, 3))
    cn = rng.standard_normal((700, 3))
    cn /= np.linalg.norm(cn, axis=1, keepdims=True)
    pts = np.concatenate([patch, sphere, clutter]).astype(np.float32)
    normals = np.concatenate([np.tile(nrm, (2200, 1)), d, cn]).astype(np.float32)
    perm = rng.permutation(len(pts))
    planted = np.zeros(len(pts), bool)
    planted[:2200] = True
    plane = np.array([nrm[0], nrm[1], nrm[2], -float(nrm @ origin)])
    return np.ascontiguousarray(pts[perm]), planted[perm], plane, np.ascontiguousarray(normals[perm])


def planted_cameras():
    """Five camera centres on the sphere's side of the planted plane."""
    return np.array([[0.1, -0.2, 2.5], [1.5, -0.2, 2.0], [-1.3, 0.3, 2.2], [0.2, 1.2, 2.4], [0.4, -1.6, 1.9]], np.float64)


def two_planes(seed=1):
    """(points, which): a floor z = 0 (which 0, 1500 points), a wall x = 0 (which 1, 1000 points), both with noise of half-width
    PLANTED_S, and 300 clutter points (which -1)."""
    rng = np.random.default_rng(seed)
    floor = np.stack([rng.uniform(0.05, 2.0, 1500), rng.uniform(-1.0, 1.0, 1500), rng.uniform(-PLANTED_S, PLANTED_S, 1500)], 1)
    wall = np.stack([rng.uniform(-PLANTED_S, PLANTED_S, 1000), rng.uniform(-1.0, 1.0, 1000), rng.uniform(0.05, 1.5, 1000)], 1)
    clutter = rng.uniform(-0.5, 2.0, (300, 3))
    pts = np.concatenate([floor, wall, clutter]).astype(np.float32)
    which = np.concatenate([np.zeros(1500, int), np.ones(1000, int), -np.ones(300, int)])
    perm = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), which[perm]


def tie_case():
    """12 points with small integer coordinates: 8 on z = 0, 4 off it.  Every triplet of the 8 gives the plane z = 0 exactly, so with 64
    draws several hypotheses share the best count 8."""
    on = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 1, 0], [1, 3, 0], [4, 4, 0], [2, 5, 0], [5, 2, 0]]
    off = [[1, 1, 3], [2, 2, 7], [3, 0, -5], [0, 4, 11]]
    return np.array(on + off, np.float32)


def rejected_refit_case(seed=2):
    """42 points on integer x, y: 10 on z = 0, 24 on z = +0.5 and 8 on z = -0.5, threshold 0.5.  A triplet of the 10 gives z = 0 with all
    42 as inliers (32 of them exactly ON the threshold); their least-squares plane lies near z = +0.19 and loses the 8 lower points."""
    rng = np.random.default_rng(seed)
    xy = rng.integers(-6, 7, (42, 2)).astype(np.float64)
    z = np.concatenate([np.zeros(10), np.full(24, 0.5), np.full(8, -0.5)])
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32), 0.5


def score_case(n, H, seed=0):
    """(points [n,3], planes [H,4], normals [n,3], active [n], threshold, min_cos) for the count tests.  Coordinates are multiples of
    1/8 in [-4, 4], so the axis-aligned rows (0, 0, 1, -k/8) meet points with r == threshold == 0.25 EXACTLY; the other rows are planes
    through random triplets; every 7th row holds a NaN or an infinity; a tenth of the normals are 0 0 0."""
    rng = np.random.default_rng(1000 * seed + n + 7 * H)
    pts = (rng.integers(-32, 33, (n, 3)) / 8.0).astype(np.float32)
    normals = rng.standard_normal((n, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    normals[rng.random(n) < 0.1] = 0.0
    planes = hypotheses(pts, rng.integers(0, n, (H, 3)))  # with n < 3 or repeats: NaN rows
    for h in range(0, H, 3):
        planes[h] = [0.0, 0.0, 1.0, -rng.integers(-32, 33) / 8.0]
    for h in range(1, H, 7):
        planes[h] = [1.0, 0.0, 0.0, 0.5]
        planes[h, rng.integers(0, 4)] = (np.nan, np.inf, -np.inf)[h % 3]
    active = (rng.random(n) < 0.7).astype(np.uint8)
    return pts, planes, normals.astype(np.float32), active, 0.25, 0.5
