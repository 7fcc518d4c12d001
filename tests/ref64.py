"""Float64 restatement of the PatchMatch hot path: the operations behind pmn_init_hypotheses, pmn_warp_correlate(_views),
pmn_feature_weight, pmn_aggregate_regress, pmn_confidence and pmn_normalize_depth, written from the reference's semantics
(models/patchmatch.py, models/module.py, models/net.py; ATen's grid_sample) in plain vectorised numpy.

Every function takes the fp32 arrays the kernel takes and evaluates in float64, so what it returns is the operation itself up to
float64 rounding: an independent yardstick for the HIP kernels (tests/test_kernel_space_gpu.py) that shares no code with the fp32
oracle (oracle/oracle.py, oracle/pmn_oracle.c).  Layouts are planar: features [B,C,h,w], hypotheses [B,D,h,w], offsets [B,2K,h,w]
(channel 2k = x, 2k+1 = y), neighbour tables [K,2] of (dy, dx).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

BN_EPS = 1e-5


def f64(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64)


# ---- bilinear sampling (ATen grid_sampler_2d: corners nw, ne, sw, se; an out-of-range corner contributes nothing) ------------------

def bilinear(src: np.ndarray, ix: np.ndarray, iy: np.ndarray, dtype=np.float64) -> np.ndarray:
    """src [C,H,W]; ix, iy un-normalised positions of any shape S -> [C, *S] (zero padding outside the map).  ``dtype``: the type
    every operation runs in (float64: the yardstick; float32: ATen's own arithmetic, tests/camera_space.py)."""
    C, H, W = src.shape
    T = np.dtype(dtype).type
    ix, iy = np.asarray(ix, dtype), np.asarray(iy, dtype)
    # positions far outside (or not a number) cannot reach a texel: clamp them before the integer conversion
    ix = np.where(np.isnan(ix), T(-4.0), np.clip(ix, T(-4.0), T(W + 4.0)))
    iy = np.where(np.isnan(iy), T(-4.0), np.clip(iy, T(-4.0), T(H + 4.0)))
    x0, y0 = np.floor(ix), np.floor(iy)
    out = np.zeros((C,) + ix.shape, dtype)
    flat = np.asarray(src, dtype).reshape(C, H * W)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + T(dx), y0 + T(dy)
            wgt = (T(1.0) - np.abs(ix - xx)) * (T(1.0) - np.abs(iy - yy))
            ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            idx = (np.clip(yy, 0, H - 1) * W + np.clip(xx, 0, W - 1)).astype(np.int64)
            out += flat[:, idx] * np.where(ok, wgt, T(0.0))
    return out


# ---- neighbour positions (get_grid, patchmatch.py:396-426) sampled with grid_sample(align_corners=False, padding="border") --------

def neighbor_positions(offsets: np.ndarray, table: np.ndarray, h: int, w: int):
    """offsets [B,2K,h,w], table [K,2] (dy, dx) -> (ix, iy) [B,K,h,w], already clipped to the border."""
    off = f64(offsets)
    tab = np.asarray(table, np.int64).reshape(-1, 2)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    X = x + (tab[:, 1].reshape(1, -1, 1, 1) + off[:, 0::2])
    Y = y + (tab[:, 0].reshape(1, -1, 1, 1) + off[:, 1::2])
    xn = X / ((w - 1) / 2.0) - 1.0
    yn = Y / ((h - 1) / 2.0) - 1.0
    ix = np.clip(((xn + 1.0) * w - 1.0) / 2.0, 0.0, w - 1.0)
    iy = np.clip(((yn + 1.0) * h - 1.0) / 2.0, 0.0, h - 1.0)
    return ix, iy


def neighbor_gather(inp: np.ndarray, offsets: np.ndarray, table: np.ndarray) -> np.ndarray:
    """inp [B,Cn,h,w] -> [B,Cn,K,h,w]."""
    B, Cn, h, w = inp.shape
    ix, iy = neighbor_positions(offsets, table, h, w)
    return np.stack([bilinear(f64(inp[b]), ix[b], iy[b]) for b in range(B)])


# ---- DepthInitialization + Propagation (patchmatch.py:53-94, 115-124) ---------------------------------------------------------------

def depth_initialization(noise: Optional[np.ndarray], depth: Optional[np.ndarray], depth_shift: int, depth_min, depth_max,
                         num_sample: int, interval_scale: float, h: int, w: int) -> np.ndarray:
    """-> [B,D0,h,w]: 48 inverse-depth bins jittered by ``noise`` [B,48,h,w], or ``num_sample`` local samples around ``depth``
    [B,1,h>>s,w>>s] (nearest up-sampled by 2**depth_shift, net.py:274) spaced interval_scale * (1/dmin - 1/dmax) in inverse depth."""
    inv_min = (1.0 / f64(depth_min)).reshape(-1, 1, 1, 1)
    inv_max = (1.0 / f64(depth_max)).reshape(-1, 1, 1, 1)
    if noise is not None:
        u = f64(noise) + np.arange(48, dtype=np.float64).reshape(1, 48, 1, 1)
        return 1.0 / (inv_max + u / 48.0 * (inv_min - inv_max))
    d = f64(depth)
    if depth_shift:
        d = np.repeat(np.repeat(d, 1 << depth_shift, axis=2), 1 << depth_shift, axis=3)
    assert d.shape[2:] == (h, w)
    if num_sample == 1:
        return d.copy()
    k = np.arange(-num_sample // 2, num_sample // 2, dtype=np.float64).reshape(1, num_sample, 1, 1)
    inv = np.clip(1.0 / d + (inv_min - inv_max) * float(np.float32(interval_scale)) * k, inv_max, inv_min)
    return 1.0 / inv


def xnorm_of(depth_sample: np.ndarray, depth_min, depth_max) -> np.ndarray:
    """Normalised inverse depth (patchmatch.py:650-657): (1/d - 1/dmax) / (1/dmin - 1/dmax)."""
    inv_min = (1.0 / f64(depth_min)).reshape(-1, 1, 1, 1)
    inv_max = (1.0 / f64(depth_max)).reshape(-1, 1, 1, 1)
    return (1.0 / f64(depth_sample) - inv_max) / (inv_min - inv_max)


def init_hypotheses(noise, depth, depth_shift, depth_min, depth_max, num_sample, interval_scale, propa_offsets, table, h, w):
    """-> (depth_sample [B,D,h,w] sorted ascending when propagated, xnorm [B,D,h,w])."""
    ds = depth_initialization(noise, depth, depth_shift, depth_min, depth_max, num_sample, interval_scale, h, w)
    if propa_offsets is not None:
        D0 = ds.shape[1]
        nb = neighbor_gather(ds[:, D0 // 2:D0 // 2 + 1], propa_offsets, table)[:, 0]
        ds = np.sort(np.concatenate([ds, nb], axis=1), axis=1)
    return ds, xnorm_of(ds, depth_min, depth_max)


# ---- pointwise MLPs (ConvBnReLU3D x2 + Conv3d, module.py:43-72; BatchNorm in eval mode) ----------------------------------------------

def _t(x) -> np.ndarray:
    return x.detach().cpu().double().numpy()


def mlp(x: np.ndarray, net, sigmoid: bool) -> np.ndarray:
    """x [B,G,...] -> [B,...] through a SimilarityNet / PixelwiseNet / FeatureWeightNet module's own parameters."""
    x = f64(x)
    G = x.shape[1]
    last = getattr(net, net._last)

    def layer(v, conv, bn):
        wgt = _t(conv.weight).reshape(conv.weight.shape[0], -1)
        y = np.tensordot(wgt, v, axes=([1], [1]))  # [O,B,...]
        y = np.moveaxis(y, 0, 1)
        sh = (1, -1) + (1,) * (y.ndim - 2)
        y = (y - _t(bn.running_mean).reshape(sh)) / np.sqrt(_t(bn.running_var).reshape(sh) + BN_EPS) * _t(bn.weight).reshape(sh) \
            + _t(bn.bias).reshape(sh)
        return np.maximum(y, 0.0)

    assert _t(net.conv0.conv.weight).reshape(16, -1).shape[1] == G
    h0 = layer(x, net.conv0.conv, net.conv0.bn)
    h1 = layer(h0, net.conv1.conv, net.conv1.bn)
    out = np.tensordot(_t(last.weight).reshape(8), h1, axes=([0], [1])) + float(_t(last.bias).reshape(-1)[0])
    return 1.0 / (1.0 + np.exp(-out)) if sigmoid else out


# ---- warping (module.py:130-181) + group-wise correlation (patchmatch.py:193-203) ----------------------------------------------------

def warp_positions(P: np.ndarray, depth: np.ndarray, h: int, w: int, hs: int, ws: int, dtype=np.float64, front_eps: float = 1e-3,
                   sentinel=None, details: bool = False, xy=None):
    """P = relative projection src_proj @ inv(ref_proj) [4,4]; depth [D,h,w] -> (ix, iy) [D,h,w] in the source map.  A point on or
    behind the source camera (z <= 1e-3) samples NOTHING: the reference replaces it by (w, h, 1), which its chain carries to
    (w (ws-1)/(w-1), h (hs-1)/(h-1)) -- outside every tap of a source map as large as the reference's, but on the last texel of a
    smaller one (its recorded output has that: tests/golden ops_small.npz, case B); here its position is (ws, hs), outside every
    tap of any map (pmn_pose_position replaces the point by (2w, 2h, 1), which lands outside any map as well).

    ``dtype``: the type every operation runs in, in the reference's order (module.py:161-173 and grid_sample's un-normalisation):
    float64 is the yardstick, float32 the reference's own arithmetic.  ``front_eps`` / ``sentinel`` (the position (ix, iy) given to
    a point behind the camera) restate mistakes (tests/kernel_space.py).  ``details``: also returns {"front", "pz"}, pz before the
    sentinel replaces it.  ``xy``: reference pixels (x, y) of depth's shape instead of the h x w grid."""
    T = np.dtype(dtype).type
    P = np.asarray(P, dtype)
    if xy is None:
        y, x = np.meshgrid(np.arange(h, dtype=dtype), np.arange(w, dtype=dtype), indexing="ij")
    else:
        x, y = np.asarray(xy[0], dtype), np.asarray(xy[1], dtype)
    d = np.asarray(depth, dtype)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        r = [(P[i, 0] * x + P[i, 1] * y) + P[i, 2] for i in range(3)]
        px, py, pz0 = (r[i] * d + P[i, 3] for i in range(3))
        front = pz0 > T(front_eps)  # (a NaN depth is not in front: `pz <= 1e-3` is false for it, but so is every later comparison)
        px, py, pz = np.where(front, px, T(w)), np.where(front, py, T(h)), np.where(front, pz0, T(1.0))
        xn = (px / pz) / (T(w - 1) / T(2.0)) - T(1.0)
        yn = (py / pz) / (T(h - 1) / T(2.0)) - T(1.0)
        ix, iy = (xn + T(1.0)) / T(2.0) * T(ws - 1), (yn + T(1.0)) / T(2.0) * T(hs - 1)
    sx, sy = (ws, hs) if sentinel is None else sentinel
    ix, iy = np.where(front, ix, T(sx)), np.where(front, iy, T(sy))
    return (ix, iy, {"front": front, "pz": pz0}) if details else (ix, iy)


def view_similarity(ref: np.ndarray, src: np.ndarray, rel_proj: np.ndarray, depth: np.ndarray, G: int, warp_kw=None) -> np.ndarray:
    """ref [B,C,h,w], src [B,C,hs,ws] (one source view), rel_proj [B,4,4], depth [B,D,h,w] -> [B,G,D,h,w]:
    mean over the C/G channels of a group of warped source * reference.  ``warp_kw``: keyword arguments of warp_positions."""
    B, C, h, w = ref.shape
    hs, ws = src.shape[2:]
    out = []
    for b in range(B):
        ix, iy = warp_positions(rel_proj[b], depth[b], h, w, hs, ws, **(warp_kw or {}))
        warped = bilinear(f64(src[b]), ix, iy)  # [C,D,h,w]
        prod = warped * f64(ref[b])[:, None]
        out.append(prod.reshape(G, C // G, *prod.shape[1:]).mean(axis=1))
    return np.stack(out)


def warp_correlate(ref: np.ndarray, srcs: Sequence[np.ndarray], rel_proj: np.ndarray, depth: np.ndarray,
                   view_weights: Optional[np.ndarray], vw_shift: int, similarity_net, pixelwise_net, G: int,
                   warp_kw=None) -> Dict[str, np.ndarray]:
    """Evaluation up to the SimilarityNet MLP (patchmatch.py:179-224, 565-566).  srcs: N maps [B,C,hs,ws]; view_weights [B,N,h>>s,
    w>>s] (read at (y>>s, x>>s)) or None: then PixelwiseNet computes them (max over D of its sigmoid response, patchmatch.py:695-702).
    -> similarity [B,G,D,h,w], cost [B,D,h,w], view_weights [B,N,h,w], responses [B,N,D,h,w] (None when weights were given)."""
    B, C, h, w = ref.shape
    sim_sum = 0.0
    wsum = 1e-5
    vws, resps = [], []
    for v, src in enumerate(srcs):
        sim = view_similarity(ref, src, rel_proj[:, v], depth, G, warp_kw)
        if view_weights is None:
            resp = mlp(sim, pixelwise_net, sigmoid=True)  # [B,D,h,w]
            resps.append(resp)
            vw = resp.max(axis=1)
        else:
            s = vw_shift
            vw = f64(view_weights[:, v])[:, (np.arange(h) >> s)][:, :, (np.arange(w) >> s)]
        vws.append(vw)
        sim_sum = sim_sum + sim * vw[:, None, None]
        wsum = wsum + vw
    similarity = sim_sum / wsum[:, None, None]
    return {"similarity": similarity, "cost": mlp(similarity, similarity_net, sigmoid=False), "view_weights": np.stack(vws, 1),
            "responses": np.stack(resps, 1) if resps else None}


def feature_weight(ref: np.ndarray, offsets: np.ndarray, table: np.ndarray, net, G: int) -> np.ndarray:
    """FeatureWeightNet (patchmatch.py:613-624): sigmoid(MLP(group-mean of ref(neighbour) * ref)) -> [B,K,h,w]."""
    B, C, h, w = ref.shape
    nb = neighbor_gather(ref, offsets, table)  # [B,C,K,h,w]
    prod = nb * f64(ref)[:, :, None]
    corr = prod.reshape(B, G, C // G, *prod.shape[2:]).mean(axis=2)
    return mlp(corr, net, sigmoid=True)


def depth_weight(xnorm: np.ndarray, offsets: np.ndarray, table: np.ndarray, interval_scale: float) -> np.ndarray:
    """patchmatch.py:650-669 from the normalised inverse depth -> [B,D,K,h,w]."""
    x1 = neighbor_gather(xnorm, offsets, table)
    v = np.clip(np.abs(x1 - f64(xnorm)[:, :, None]) / float(np.float32(interval_scale)), 0.0, 4.0)
    return 1.0 / (1.0 + np.exp(-(4.0 - 2.0 * v)))


def softmax(score: np.ndarray) -> np.ndarray:
    z = score - score.max(axis=1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=1, keepdims=True)


def regress(depth_sample: np.ndarray, prob: np.ndarray, is_inverse: bool) -> np.ndarray:
    """patchmatch.py:226-237 -> [B,h,w]; the inverse form interpolates in inverse depth between the first and last hypothesis."""
    ds = f64(depth_sample)
    D = ds.shape[1]
    if not is_inverse:
        return (ds * prob).sum(axis=1)
    idx = (np.arange(D, dtype=np.float64).reshape(1, D, 1, 1) * prob).sum(axis=1)
    inv_min, inv_max = 1.0 / ds[:, -1], 1.0 / ds[:, 0]
    return 1.0 / (inv_max + idx / (D - 1) * (inv_min - inv_max))


def aggregate_regress(cost, depth_sample, xnorm, fweight, offsets, table, interval_scale, is_inverse):
    """Adaptive spatial aggregation (patchmatch.py:502-510, 565-577), softmax over D and regression -> (score [B,D,h,w],
    depth [B,h,w], pre-softmax score [B,D,h,w])."""
    wgt = depth_weight(xnorm, offsets, table, interval_scale) * f64(fweight)[:, None]
    wgt = wgt / wgt.sum(axis=2, keepdims=True)
    pre = (neighbor_gather(cost, offsets, table) * wgt).sum(axis=2)
    prob = softmax(pre)
    return prob, regress(depth_sample, prob, is_inverse), pre


# ---- epilogue (net.py:288-299, module.py:184-196) -------------------------------------------------------------------------------------

def confidence(score: np.ndarray, H: int, W: int):
    """-> (confidence [B,H,W], depth_index [B,h,w], the regressed index before truncation [B,h,w]): the sum of the probabilities
    at index-1 .. index+2 (4 * avg_pool3d over the zero-padded volume), nearest-resized to H x W."""
    s = f64(score)
    B, D, h, w = s.shape
    idxf = (s * np.arange(D, dtype=np.float64).reshape(1, D, 1, 1)).sum(axis=1)
    idx = np.clip(np.trunc(idxf).astype(np.int64), 0, D - 1)
    pad = np.concatenate([np.zeros((B, 1, h, w)), s, np.zeros((B, 2, h, w))], axis=1)
    win = sum(np.take_along_axis(pad, (idx + j)[:, None], axis=1)[:, 0] for j in range(4))
    ys = np.minimum(np.floor(np.arange(H) * (h / H)).astype(np.int64), h - 1)
    xs = np.minimum(np.floor(np.arange(W) * (w / W)).astype(np.int64), w - 1)
    return win[:, ys][:, :, xs], idx, idxf


def normalize_depth(depth: np.ndarray, depth_min, depth_max) -> np.ndarray:
    """net.py:104-106: (depth - dmin[b]) / (dmax[b] - dmin[b])."""
    d = f64(depth)
    sh = (-1,) + (1,) * (d.ndim - 1)
    lo, hi = f64(depth_min).reshape(sh), f64(depth_max).reshape(sh)
    return (d - lo) / (hi - lo)
