"""Extended-precision restatement of fuse_view_kernel (csrc/fusion.hip: pmn_fuse_view, pmn_fuse_view_merged) -- TEST INFRASTRUCTURE, a
helper of tests/test_fusion_space.py (CPU) and tests/test_fusion_space_gpu.py, not a test module.

``fuse_view_ref`` takes what the kernel takes -- the flat map slots, their sizes, the slot numbers, the ``mats`` float block (48 + 64 n
floats, layout in include/pmn_hip.h) and the thresholds -- so camera algebra is not part of what is compared.  It keeps the kernel's
dtype flow (float32 inputs, float64 products, float32 casts of the map coordinates, the re-projected depth and position), but every
float64 step is evaluated in np.longdouble (x87 extended: 64-bit significand) and rounded only where the kernel casts to float32:
(float)xs, (float)ys, depth_rep = (float)wz, x_rep, y_rep, (float)sz of the merged kernel, (float) of the world point.  cv2.remap is
oracle.fusion_oracle.remap_linear_cv2 (pinned by tests/golden/cv2_reference.npz); ``rel``, the ``acc`` sum in source order and
``total`` are numpy float32, ``depth_avg`` is one correctly rounded float64 division: all exact restatements.

What is left between the kernel (float64, fused multiply-adds) and this file (or numpy on any BLAS) is the float64 rounding of the
products.  It can change a result only by moving a value across a float32 rounding boundary at one of the casts, or ``dist`` across
geo_pixel_thres.  A (pixel, source) entry where that could happen is FRAGILE; a pixel none of whose sources is fragile is DECIDED, and
on decided pixels the kernel has to give this file's masks, counts and averaged depth bit for bit.

THE WINDOW.  Derivation (u = 2^-53, the float64 unit roundoff).  Every value is carried with a magnitude ``mag``: the sum of the
absolute values of the terms it was formed from, carried through the chain (a dot product sum m_i v_i has mag = sum |m_i| mag_i; a
quotient a / b has (mag_a + |a / b| mag_b) / |b|; an exactly representable leaf has mag = |v|) -- "the largest intermediate", which
under cancellation is far above |v| (ys in image row 0: |v| ~ 1e-6, mag ~ 20).  By the standard running error bound a float64
evaluation of such a chain, fused or not, in any summation order, differs from the exact value by at most k u mag (1 + O(u)), k = the
number of roundings on the longest path to the value.  The longest path ends at x_rep:
    inverse(K_ref) (3 terms: 5 roundings unfused), T (4 terms: 7), K_src (5), the quotient (1), the product with the sample (1),
    inverse(K_src) (5), T2 (7), K_ref (5), the quotient (1)                                                        k <= 37,
six chained 3- and 4-term dot products and two quotients.  The longdouble evaluation here has the same k with u' = 2^-64.  The two
sides differ by < 40 u mag, and the window is
    W_MAG = 256 u = 2^-45 of the carried magnitude:  a few hundred float64 ulps of the largest intermediate, 6 times the bound.
Relative to the value itself that is 2^-45 mag / |v|; mag / |v| has a median of 1.5 .. 11 (by cast) on the rows of tests/fusion_space.py and is
unbounded towards the image's first row and column, so in the relative terms it was expected in the window is of the order 2^-42 ..
2^-40 and wider where values cancel.  Where a window relative to the value is what applies (below), W_REL = 2^-40.  Both were fixed
from this derivation before the kernel ran against them and have not been tuned.

THE RULE.  An entry is fragile when one of
  * the longdouble wz (and, for a claim, sz) lies within W_MAG mag of the midpoint between two neighbouring float32 values;
  * the float32 casts of the two ends of [v - W_MAG mag, v + W_MAG mag], v = xs or ys, differ AND give another cvRound(32 f), another
    verdict of the remap's |32 f| < 2^30, or another rintf(f): the kernel reads (float)xs and (float)ys through these three monotone
    functions only (the fixed-point coordinate of the remap, the claim's address) -- a cast that falls the other way between two
    float32 values 1e-13 apart at ys ~ 1e-6 changes nothing downstream;
  * the longdouble px / pz or py / pz lies within W_REL |v| of such a midpoint;
  * dist lies within W_REL max(1, thr) + slack of geo_pixel_thres, where slack is 0 unless the cast of x_rep (y_rep) is not stable
    under the magnitude window -- cancellation in column or row 0, where |v| << mag -- and then one float32 ulp of x_rep (y_rep) plus
    W_MAG mag: the most dist can move when that cast falls the other way.
Non-finite values are never fragile (comparisons with NaN are false on both sides, infinities stay infinities).  The world point's
cast is not under the rule: a decided, final pixel's xyz may differ by one float32 ulp plus W_MAG mag of the component (far below one
ulp except where the component cancels to nearly zero: world x in the column of the principal point is ~1e-7 with mag ~ 200).

MEASURED fragile share, from this file alone (``python tests/fusion_space.py``; tests/test_fusion_space.py asserts <= 1e-3 per row and
over the table and prints it): 8 of 207339 (pixel, source) entries over the table, 3.9e-5.  One entry each in the rows mixed-sizes
(1.5e-4 of the row), reordered (2.9e-4), nsrc32 (3.3e-5), nsrc32-thres32 (1.1e-4), camera-away, bad-ref, bad-src and spikes (6.9e-5
each); none in the other 22 rows.  On the device (MI355X) every decided pixel of every row matched bit for bit, and no world point
component of a decided, final pixel was further than its bound; nearly all were equal.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from oracle import fusion_oracle as FO

L = np.longdouble
assert np.finfo(L).nmant >= 63, "fusion_ref64 needs an extended-precision np.longdouble (x86-64: 64-bit significand)"

W_REL = 2.0 ** -40          # relative window (of the value itself)
W_MAG = 256 * 2.0 ** -53    # 256 float64 ulps of the carried magnitude
REF_FLOATS, SRC_FLOATS = 48, 64


def _leaf(v) -> Tuple[np.ndarray, np.ndarray]:
    v = np.asarray(v, L)
    return v, np.abs(v)


def _dot(m: np.ndarray, vs: Sequence[Tuple[np.ndarray, np.ndarray]]):
    """sum m[i] * v_i over (value, magnitude) pairs, in longdouble; a missing last pair is the constant 1."""
    val, mag = L(0), L(0)
    for i, (v, g) in enumerate(vs):
        val = val + L(m[i]) * v
        mag = mag + abs(L(m[i])) * g
    if len(vs) < len(m):
        val, mag = val + L(m[len(vs)]), mag + abs(L(m[len(vs)]))
    return val, mag


def _div(a, b):
    q = a[0] / b[0]
    return q, (a[1] + np.abs(q) * b[1]) / np.abs(b[0])


def ulp32(f: np.ndarray) -> np.ndarray:
    """Spacing of float32 at |f| (the larger neighbour's distance); non-finite -> NaN."""
    f = np.abs(np.asarray(f, np.float32))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isfinite(f), np.nextafter(f, np.float32(np.inf)).astype(np.float64) - f.astype(np.float64), np.nan)


def _near_f32_boundary(v: np.ndarray, window: np.ndarray) -> np.ndarray:
    """True where the finite longdouble ``v`` lies within ``window`` (absolute) of a midpoint between neighbouring float32 values."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = v.astype(np.float32)
        lo = (f.astype(L) + np.nextafter(f, np.float32(-np.inf)).astype(L)) / 2
        hi = (f.astype(L) + np.nextafter(f, np.float32(np.inf)).astype(L)) / 2
        d = np.minimum(np.abs(v - lo), np.abs(v - hi))
        return np.isfinite(v) & np.isfinite(window) & (d <= window)


def _coordinate_unstable(v: np.ndarray, window: np.ndarray) -> np.ndarray:
    """(float)xs and (float)ys are read only as cvRound(32 f) behind the test |32 f| < 2^30 (the remap) and as rintf(f) (the claim's
    address), all monotone in f: the cast matters only if the float32 values of the two ends of [v - window, v + window] differ in
    one of the three."""
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = (v - window).astype(np.float32), (v + window).astype(np.float32)
        m_lo, m_hi = lo * np.float32(32.0), hi * np.float32(32.0)
        g_lo, g_hi = np.abs(m_lo) < np.float32(2.0 ** 30), np.abs(m_hi) < np.float32(2.0 ** 30)
        differ = (g_lo != g_hi) | (g_lo & g_hi & (np.rint(m_lo) != np.rint(m_hi))) | (np.rint(lo) != np.rint(hi))
        return np.isfinite(v) & np.isfinite(window) & (lo != hi) & differ


def _slot(maps: np.ndarray, sizes, slot: int):
    h, w = sizes[slot]
    flat = np.asarray(maps[slot], np.float32)
    return flat[:h * w].reshape(h, w), flat[h * w:2 * h * w].reshape(h, w)


def fuse_view_ref(maps: np.ndarray, sizes: Sequence[Tuple[int, int]], ref_slot: int, src_slots: Sequence[int], mats: np.ndarray,
                  thresholds) -> Dict[str, np.ndarray]:
    """One reference view.  maps float32 [V,F] flat slots (depth [h_v,w_v] then confidence [h_v,w_v] at the start of slot v), sizes
    [(h_v, w_v)] per slot, thresholds = (geo_pixel_thres, geo_depth_thres, geo_mask_thres, photo_thres).  Returns photo / geo / final
    bool [H,W], geo_sum int32, depth_avg float64, xyz float32 [H,W,3] with xyz_slack float64 [H,W,3] (= W_MAG mag), and per source [n,H,W]:
    verdict, depth_rep float32, rel float32, fragile, xs / ys float32 (the coordinates that feed the remap), kz_negative, sz float32 with
    sz_fragile; decided bool [H,W] and n_fragile int [H,W]."""
    thr_px, thr_d, thr_n, thr_p = thresholds
    thr_px, thr_d, thr_p = np.float32(thr_px), np.float32(thr_d), np.float32(thr_p)
    mats = np.asarray(mats, np.float32).reshape(-1)
    n = len(src_slots)
    assert mats.size == REF_FLOATS + SRC_FLOATS * n
    d_ref, conf = _slot(maps, sizes, ref_slot)
    H, W = d_ref.shape
    Kri, Kr, Eri = mats[0:9], mats[9:18], mats[18:34]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x, y = xx.astype(L), yy.astype(L)
    out = dict(verdict=np.zeros((n, H, W), bool), depth_rep=np.zeros((n, H, W), np.float32), fragile=np.zeros((n, H, W), bool),
               xs=np.zeros((n, H, W), np.float32), ys=np.zeros((n, H, W), np.float32), kz_negative=np.zeros((n, H, W), bool),
               sz=np.zeros((n, H, W), np.float32), sz_fragile=np.zeros((n, H, W), bool), rel=np.zeros((n, H, W), np.float32))
    with np.errstate(all="ignore"):
        d = d_ref.astype(L)
        pt = [_leaf(x * d), _leaf(y * d), _leaf(d)]  # int * float32: exact in float64
        r = [_dot(Kri[3 * k:3 * k + 3], pt) for k in range(3)]
        geo_sum = np.zeros((H, W), np.int32)
        acc = np.zeros((H, W), np.float32)
        for s in range(n):
            M = mats[REF_FLOATS + s * SRC_FLOATS:REF_FLOATS + (s + 1) * SRC_FLOATS]
            T, Ks, Ksi, T2 = M[0:16], M[16:25], M[25:34], M[34:50]
            src, _ = _slot(maps, sizes, src_slots[s])
            sc = [_dot(T[4 * k:4 * k + 4], r) for k in range(3)]
            kk = [_dot(Ks[3 * k:3 * k + 3], sc) for k in range(3)]
            xs, ys = _div(kk[0], kk[2]), _div(kk[1], kk[2])
            xs32, ys32 = xs[0].astype(np.float32), ys[0].astype(np.float32)
            sampled = FO.remap_linear_cv2(src, xs32, ys32)
            sm = sampled.astype(L)
            b = [(xs[0] * sm, xs[1] * np.abs(sm)), (ys[0] * sm, ys[1] * np.abs(sm)), _leaf(sm)]
            q = [_dot(Ksi[3 * k:3 * k + 3], b) for k in range(3)]
            wv = [_dot(T2[4 * k:4 * k + 4], q) for k in range(3)]
            depth_rep = wv[2][0].astype(np.float32)
            p = [_dot(Kr[3 * k:3 * k + 3], wv) for k in range(3)]
            xr, yr = _div(p[0], p[2]), _div(p[1], p[2])
            x_rep, y_rep = xr[0].astype(np.float32), yr[0].astype(np.float32)
            ex, ey = x_rep.astype(L) - x, y_rep.astype(L) - y
            dist = np.sqrt(ex * ex + ey * ey)
            rel = np.abs(depth_rep - d_ref) / d_ref  # float32 throughout
            m = (dist < L(thr_px)) & (rel < thr_d)
            # -- the fragile rule (module docstring)
            frag = _coordinate_unstable(xs[0], W_MAG * xs[1]) | _coordinate_unstable(ys[0], W_MAG * ys[1])
            frag |= _near_f32_boundary(wv[2][0], W_MAG * wv[2][1])
            frag |= _near_f32_boundary(xr[0], W_REL * np.abs(xr[0])) | _near_f32_boundary(yr[0], W_REL * np.abs(yr[0]))
            slack = L(W_REL) * max(L(1), L(thr_px))
            for v, f32 in ((xr, x_rep), (yr, y_rep)):
                loose = _near_f32_boundary(v[0], W_MAG * v[1])
                slack = slack + np.where(loose, ulp32(f32).astype(L) + W_MAG * v[1], L(0))
            frag |= np.isfinite(dist) & (np.abs(dist - L(thr_px)) <= slack)
            out["verdict"][s], out["depth_rep"][s], out["fragile"][s], out["rel"][s] = m, depth_rep, frag, rel
            out["xs"][s], out["ys"][s], out["kz_negative"][s] = xs32, ys32, kk[2][0] < 0
            out["sz"][s], out["sz_fragile"][s] = sc[2][0].astype(np.float32), _near_f32_boundary(sc[2][0], W_MAG * sc[2][1])
            geo_sum += m.astype(np.int32)
            acc = acc + np.where(m, depth_rep, np.float32(0.0)).astype(np.float32)
        total = acc + d_ref
        avg = total.astype(np.float64) / (geo_sum + 1).astype(np.float64)
        a = avg.astype(L)
        apt = [_leaf(x * a), _leaf(y * a), _leaf(a)]
        c = [_dot(Kri[3 * k:3 * k + 3], apt) for k in range(3)]
        world = [_dot(Eri[4 * k:4 * k + 4], c) for k in range(3)]
        out["xyz"] = np.stack([wd[0].astype(np.float32) for wd in world], -1)
        out["xyz_slack"] = np.stack([(W_MAG * wd[1]).astype(np.float64) for wd in world], -1)
    photo = conf > thr_p
    geo = geo_sum >= int(thr_n)
    out.update(photo=photo, geo=geo, final=photo & geo, geo_sum=geo_sum, depth_avg=avg, n_fragile=out["fragile"].sum(0).astype(np.int32))
    out["decided"] = out["n_fragile"] == 0
    return out


def _claim_pixels(x32, y32, h: int, w: int):
    """The kernel's claim address for float32 coordinates: rintf, the inside test made in float, -> (inside, iy, ix)."""
    with np.errstate(invalid="ignore"):
        fx, fy = np.rint(x32), np.rint(y32)
        inside = (fx >= 0) & (fx < np.float32(w)) & (fy >= 0) & (fy < np.float32(h))
    return inside, np.where(inside, fy, 0).astype(np.int64), np.where(inside, fx, 0).astype(np.int64)


def merge_ref(view: Dict[str, np.ndarray], maps: np.ndarray, sizes: Sequence[Tuple[int, int]], ref_slot: int, src_slots: Sequence[int],
              thresholds, claimed: np.ndarray) -> Dict[str, np.ndarray]:
    """The merged kernel's extra outputs on top of ``view`` = fuse_view_ref(...) and the claim bytes ``claimed`` uint8 [V,S] as they
    stand before the launch.  Returns emit bool [H,W] (= final && !claimed[ref_slot]); claimed_after uint8 [V,S]: ``claimed`` plus
    the claims of the pixels whose claims are certain (decided, and the cast of sz not fragile); maybe bool [V,S]: bytes that an
    uncertain pixel could set (every source it agrees with or is fragile on, at the address of its float32 coordinates and of their
    float32 neighbours, whatever the depth guard says); rejected: certain claims that the guard |d_s - z| / z < thr turned down."""
    thr_d = np.float32(thresholds[1])
    H, W = view["final"].shape
    emit = view["final"] & (np.asarray(claimed[ref_slot][:H * W]).reshape(H, W) == 0)
    after = np.array(claimed, np.uint8, copy=True)
    maybe = np.zeros(after.shape, bool)
    rejected = 0
    for s, slot in enumerate(src_slots):
        h, w = sizes[slot]
        d_s, _ = _slot(maps, sizes, slot)
        z = view["sz"][s]
        inside, iy, ix = _claim_pixels(view["xs"][s], view["ys"][s], h, w)
        with np.errstate(all="ignore"):
            guard = np.abs(d_s[iy, ix] - z) / z < thr_d  # float32 throughout
        certain = view["decided"] & ~view["sz_fragile"][s]
        lay = view["final"] & view["verdict"][s] & inside & certain
        rejected += int(np.count_nonzero(lay & ~guard))
        after[slot][(iy * w + ix)[lay & guard]] = 1
        # an uncertain pixel: its final flag, this source's verdict, the guard and (when a coordinate cast is fragile) the address
        # may all fall the other way
        unsure = ~certain & view["photo"] & (view["verdict"][s] | view["fragile"][s])
        for py, px in zip(*np.nonzero(unsure)):
            x0, y0 = view["xs"][s][py, px], view["ys"][s][py, px]
            for xc in (np.nextafter(x0, np.float32(-np.inf)), x0, np.nextafter(x0, np.float32(np.inf))):
                for yc in (np.nextafter(y0, np.float32(-np.inf)), y0, np.nextafter(y0, np.float32(np.inf))):
                    ok, cy, cx = _claim_pixels(np.float32(xc), np.float32(yc), h, w)
                    if ok:
                        maybe[slot][int(cy) * w + int(cx)] = True
    return dict(emit=emit, claimed_after=after, maybe=maybe, rejected=rejected)
