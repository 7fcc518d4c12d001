"""Plain numpy float64 reference of the convolution side of the hot path (csrc/conv.hip, conv_mfma.hip, conv_f16s.hip, refine.hip):
direct and transposed convolution, BatchNorm, the two x2 up-samplings and the fused chains, evaluated from the UNPACKED weights and
BatchNorm tensors (never from the packed device buffers).  Planar [N,C,H,W] arrays throughout.  Every convolution also returns its
magnitude bound A = sum |x . w| + |shift| in float64: the scale rounding errors of any evaluation order are proportional to.

Helper module (no tests here): tests/test_conv_space.py checks it against torch.nn.functional in float64, tests/test_conv_space_gpu.py
compares the kernels with it.  ``f16s_conv`` is not a reference: it is the split-fp16 arithmetic of conv_f16s.hip restated (vectorised
form of tests/test_f16s_emulation.py::emulate), used to measure what that arithmetic costs against the reference."""
from __future__ import annotations

import numpy as np

BN_EPS = 1e-5


def f64(a) -> np.ndarray:
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, np.float64)


def fold(w, bn=None, bias=None, transposed: bool = False):
    """(weights with the BatchNorm scale folded in, shift) in float64; ``bn`` = (weight, bias, running_mean, running_var)."""
    w = f64(w)
    cout = w.shape[1] if transposed else w.shape[0]
    if bn is not None:
        g, b, m, v = (f64(t) for t in bn)
        s = g / np.sqrt(v + BN_EPS)
        w = w * (s[None, :, None, None] if transposed else s[:, None, None, None])
        return w, b - m * s
    return w, (f64(bias) if bias is not None else np.zeros(cout))


def _taps(x, K, stride, pad, dil, border):
    N, C, H, W = x.shape
    Ho = (H + 2 * pad - dil * (K - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (K - 1) - 1) // stride + 1
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)), mode="edge" if border == "clamp" else "constant")
    for ky in range(K):
        for kx in range(K):
            yield ky, kx, xp[:, :, ky * dil:ky * dil + (Ho - 1) * stride + 1:stride, kx * dil:kx * dil + (Wo - 1) * stride + 1:stride]


def conv2d(x, w, shift=None, stride=1, pad=0, dil=1, border="zero", drop=None):
    """x [N,C,H,W], w [O,C,K,K] -> (y, A) [N,O,Ho,Wo].  ``border`` "clamp" replicates the edge instead of zero padding and ``drop`` =
    (kx, period) leaves tap column kx out of every output column ox > 0 with ox % period == 0 (two kernel mistakes, for
    conv_space.mistakes)."""
    x, w = f64(x), f64(w)
    y = A = None
    for ky, kx, p in _taps(x, w.shape[2], stride, pad, dil, border):
        t = np.einsum("nchw,oc->nohw", p, w[:, :, ky, kx])
        if drop is not None and kx == drop[0]:
            ox = np.arange(t.shape[3])
            t = t * ~((ox > 0) & (ox % drop[1] == 0))
        a = np.einsum("nchw,oc->nohw", np.abs(p), np.abs(w[:, :, ky, kx]))
        y, A = (t, a) if y is None else (y + t, A + a)
    if shift is not None:
        s = f64(shift).reshape(1, -1, 1, 1)
        y, A = y + s, A + np.abs(s)
    return y, A


def conv_bn(x, w, bn=None, bias=None, relu=False, **kw):
    """conv2d + BatchNorm (eval) or bias + optional ReLU -> (y, A)."""
    wf, sh = fold(w, bn, bias)
    y, A = conv2d(x, wf, sh, **kw)
    return (np.maximum(y, 0.0) if relu else y), A


def deconv3x3s2(x, w, shift=None, short=False, swap=False):
    """ConvTranspose2d(k 3, stride 2, padding 1, output_padding 1): x [N,C,H,W], w [C,O,3,3] -> (y, A) [N,O,2H,2W].  ``short``: the
    last output row and column get no contribution (output_padding forgotten); ``swap``: even and odd output coordinates take each
    other's tap sets (two kernel mistakes)."""
    x, w = f64(x), f64(w)
    N, C, H, W = x.shape
    O = w.shape[1]
    buf = np.zeros((N, O, 2 * H + 2, 2 * W + 2))
    ab = np.zeros_like(buf)
    for ky in range(3):
        for kx in range(3):
            buf[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += np.einsum("nchw,co->nohw", x, w[:, :, ky, kx])
            ab[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += np.einsum("nchw,co->nohw", np.abs(x), np.abs(w[:, :, ky, kx]))
    y, A = buf[:, :, 1:2 * H + 1, 1:2 * W + 1].copy(), ab[:, :, 1:2 * H + 1, 1:2 * W + 1].copy()
    if swap:  # pixel (oy, ox) computed with the tap set of (oy ^ 1, ox ^ 1)
        y = y[:, :, np.arange(2 * H) ^ 1][:, :, :, np.arange(2 * W) ^ 1]
    if short:
        y[:, :, -1, :] = 0.0
        y[:, :, :, -1] = 0.0
    if shift is not None:
        s = f64(shift).reshape(1, -1, 1, 1)
        y, A = y + s, A + np.abs(s)
    return y, A


def deconv_bn(x, w, bn=None, relu=False, **kw):
    wf, sh = fold(w, bn, None, transposed=True)
    y, A = deconv3x3s2(x, wf, sh, **kw)
    return (np.maximum(y, 0.0) if relu else y), A


def _axis2(n_in, align_corners=False):
    o = np.arange(2 * n_in, dtype=np.float64)
    src = o * ((n_in - 1) / max(2 * n_in - 1, 1)) if align_corners else np.maximum((o + 0.5) * 0.5 - 0.5, 0.0)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def bilinear2(u, align_corners=False):
    """x2 bilinear up-sampling of [N,C,h,w] (align_corners=False: the FPN add of reference models/net.py:60,65)."""
    u = f64(u)
    y0, y1, ly = _axis2(u.shape[2], align_corners)
    x0, x1, lx = _axis2(u.shape[3], align_corners)
    ly, lx = ly[:, None], lx[None, :]
    top = u[:, :, y0][:, :, :, x0] * (1 - lx) + u[:, :, y0][:, :, :, x1] * lx
    bot = u[:, :, y1][:, :, :, x0] * (1 - lx) + u[:, :, y1][:, :, :, x1] * lx
    return top * (1 - ly) + bot * ly


def nearest2(d, shift=0):
    """x2 nearest up-sampling of [N,C,h,w]: out[y, x] = d[y >> 1, x >> 1]; ``shift`` 1 indexes one output pixel off (a mistake)."""
    d = f64(d)
    ys = np.minimum((np.arange(2 * d.shape[2]) + shift) >> 1, d.shape[2] - 1)
    xs = np.minimum((np.arange(2 * d.shape[3]) + shift) >> 1, d.shape[3] - 1)
    return d[:, :, ys][:, :, :, xs]


# ---- fused chains: zero padding applies to the INTERMEDIATE map (conv_bn pads its own input) -----------------------------------------

def chain2(x, la, lb, relu=True, pad_input=False):
    """Two 3x3 / padding 1 layers (the stem: conv0, conv1; the pair kernel: conv3, conv4); l = dict(w=, bn=).  ``pad_input``: the
    mistake of zero-padding the input by 2 and evaluating both layers without padding (the intermediate map is then NOT zero
    outside the image)."""
    if pad_input:
        xp = np.pad(f64(x), ((0, 0), (0, 0), (2, 2), (2, 2)))
        m, _ = conv_bn(xp, la["w"], la.get("bn"), la.get("bias"), relu=relu, pad=0)
        return conv_bn(m, lb["w"], lb.get("bn"), lb.get("bias"), relu=relu, pad=0)
    m, _ = conv_bn(x, la["w"], la.get("bn"), la.get("bias"), relu=relu, pad=1)
    return conv_bn(m, lb["w"], lb.get("bn"), lb.get("bias"), relu=relu, pad=1)


def chain3(x, l0, l1, l2, conv1_off_image=False, conv0_off_image=False, origin=0, tile_roll=0, relu1=True):
    """FeatureNet's front (reference models/net.py:17-20, 51-52): conv0 3 -> 8 and conv1 8 -> 8 (3x3, padding 1), conv2 8 -> 16 (5x5,
    stride 2, padding 2), BatchNorm or bias and ReLU after each; every layer zero-pads ITS OWN input map -> (y, A) of conv2,
    [N,16,(H-1)//2+1,(W-1)//2+1].  Keyword arguments: mistakes of a kernel that fuses the three layers over patches.
    ``conv1_off_image``: conv1's map is not zeroed outside the image before conv2 -- conv1 is evaluated there, from the zero-padded
    conv0 map, and conv2 reads ReLU(shift + ...) where it should read 0.  ``conv0_off_image``: the same one layer down (conv0 is
    evaluated one pixel outside the image from the zero-padded image, and conv1 reads that).  ``origin`` = +-1: conv2 samples conv1
    around 2 o + origin instead of 2 o.  ``tile_roll`` = t: outputs with o % 16 == 15 along an axis are computed from conv1's map
    rolled by t pixels along that axis (a tile's last row / column taken from the neighbouring tile's patch).  ``relu1`` False: no
    ReLU after conv1."""
    def cb(m, l, **kw):
        return conv_bn(m, l["w"], l.get("bn"), l.get("bias"), **kw)

    def margin(m, before, after):
        return np.pad(m, ((0, 0), (0, 0), (before, after), (before, after)))

    def conv2(m1):  # m1 [N,8,H,W]: taps 2 o + origin - 2 .. 2 o + origin + 2
        return cb(margin(m1, 2 - origin, 2 + origin), l2, relu=True, stride=2, pad=0)

    x = f64(x)
    if conv0_off_image:
        m0, _ = cb(margin(x, 2, 2), l0, relu=True, pad=0)    # [H+2, W+2]: not zero in the one-pixel rim conv1 reads
        m1, _ = cb(m0, l1, relu=relu1, pad=0)
        return conv2(m1)
    m0, _ = cb(x, l0, relu=True, pad=1)
    if conv1_off_image:
        m1, _ = cb(margin(m0, 3, 3), l1, relu=relu1, pad=0)  # [H+4, W+4]: not zero in the two-pixel rim conv2 reads
        return cb(m1, l2, relu=True, stride=2, pad=0)
    m1, _ = cb(m0, l1, relu=relu1, pad=1)
    y, A = conv2(m1)
    if tile_roll:
        y = y.copy()
        for ax in (2, 3):
            rim = np.arange(y.shape[ax]) % 16 == 15
            other = conv2(np.roll(m1, -tile_roll, axis=ax))[0]
            if ax == 2:
                y[:, :, rim, :] = other[:, :, rim, :]
            else:
                y[:, :, :, rim] = other[:, :, :, rim]
    return y, A


def fpn_tail(x, up, w_in, b_in, w_out, align_corners=False):
    """output3(bilinear_x2(up) + inner2(x)) (reference models/net.py:64-67) -> (y, A)."""
    inner, Ai = conv2d(x, w_in, b_in)
    u = bilinear2(up, align_corners)
    y, _ = conv2d(u + inner, w_out)
    A = np.einsum("nchw,oc->nohw", np.abs(u) + Ai, np.abs(f64(w_out)[:, :, 0, 0]))
    return y, A


def fpn_level(x, u, w, b, align_corners=False):
    """bilinear_x2(u) + b + x @ w with w [cin,cout] (params.fold_fpn) -> (y, A)."""
    y, A = conv2d(x, f64(w).T[:, :, None, None], b)
    if u is not None:
        up = bilinear2(u, align_corners)
        y, A = y + up, A + np.abs(up)
    return y, A


def refine_front(img, t2, c0, dc, **kw):
    """cat(relu(bn(deconv(t2))), relu(bn(conv0(img)))) (reference models/net.py:110-117) -> (x16, A)."""
    a, Aa = deconv_bn(t2, dc["w"], dc["bn"], relu=True, **kw)
    b, Ab = conv_bn(img, c0["w"], c0["bn"], relu=True, pad=1)
    return np.concatenate([a, b], 1), np.concatenate([Aa, Ab], 1)


def refine_tail(x16, c3, wr, dnorm, dmin, dmax, pad_input=False, near_shift=0, swap_halves=False, roll_range=False):
    """(nearest_x2(dnorm) + res(relu(bn(conv3(x16))))) * (dmax - dmin) + dmin (reference models/net.py:117-122)
    -> dict(depth, norm, res).  Keyword arguments: kernel mistakes."""
    if pad_input:
        m, _ = conv_bn(np.pad(f64(x16), ((0, 0), (0, 0), (2, 2), (2, 2))), c3["w"], c3["bn"], relu=True, pad=0)
        res, _ = conv2d(m, wr, pad=0)
    else:
        m, _ = conv_bn(x16, c3["w"], c3["bn"], relu=True, pad=1)
        if swap_halves:
            m = np.concatenate([m[:, 4:], m[:, :4]], 1)
        res, _ = conv2d(m, wr, pad=1)
    lo, hi = f64(dmin).reshape(-1, 1, 1, 1), f64(dmax).reshape(-1, 1, 1, 1)
    if roll_range:
        lo, hi = np.roll(lo, 1, 0), np.roll(hi, 1, 0)
    norm = nearest2(dnorm, near_shift) + res
    return {"depth": norm * (hi - lo) + lo, "norm": norm, "res": res}


def refine_fused(img, t2, c0, dc, c3, wr, dnorm, dmin, dmax, front_kw=None, **kw):
    x16, _ = refine_front(img, t2, c0, dc, **(front_kw or {}))
    return refine_tail(x16, c3, wr, dnorm, dmin, dmax, **kw)


# ---- the split-fp16 arithmetic of conv_f16s.hip ---------------------------------------------------------------------------------------

def f16s_conv(x, w, shift, K, stride, dil, CC, relu, drop_lo=False, acc64=False):
    """x [N,C,H,W] float32, w [O,C,K,K] float64 (BatchNorm folded), padding dil * (K // 2): every operand split into
    hi = fp16(v), lo = fp16((v - hi) * 2048) (params.split_f16); main += hi.hi, low += hi.lo then lo.hi, one v_mfma_f32_16x16x32_f16 =
    four k-blocks of 8 channels each (k order: chunk of CC channels, tap, block of 8), products exact, the sum of one MFMA formed
    exactly and rounded into the fp32 accumulator; epilogue main + low / 2048 + shift in fp32.  -> float32 [N,O,Ho,Wo].
    ``acc64``: accumulators and epilogue in float64 and a float64 result, which is the arithmetic of
    tests/test_f16s_emulation.py::emulate before its final rounding (the cross-check of the split products and their order)."""
    at = np.float64 if acc64 else np.float32
    from patchmatchnet_amd import params
    x = np.asarray(x, np.float32)
    N, C, H, W = x.shape
    O = w.shape[0]
    pad = dil * (K // 2)
    xh, xl = (a.astype(np.float64) for a in params.split_f16(x))
    wh, wl = (a.astype(np.float64) for a in params.split_f16(w))
    blocks = [(ch, ky, kx, cb) for ch in range(C // CC) for ky in range(K) for kx in range(K) for cb in range(CC // 8)]
    per_chunk = K * K * (CC // 8)
    taps_h = {(ky, kx): p for ky, kx, p in _taps(xh, K, stride, pad, dil, "zero")}
    taps_l = {(ky, kx): p for ky, kx, p in _taps(xl, K, stride, pad, dil, "zero")}
    shp = (N, O) + next(iter(taps_h.values())).shape[2:]
    accM, accL = np.zeros(shp, at), np.zeros(shp, at)
    for ch in range(C // CC):
        chunk = blocks[ch * per_chunk:(ch + 1) * per_chunk]
        for s0 in range(0, per_chunk, 4):
            m = hl = lh = 0.0
            for _, ky, kx, cb in chunk[s0:s0 + 4]:
                c = slice(ch * CC + 8 * cb, ch * CC + 8 * cb + 8)
                m = m + np.einsum("nchw,oc->nohw", taps_h[ky, kx][:, c], wh[:, c, ky, kx])
                hl = hl + np.einsum("nchw,oc->nohw", taps_h[ky, kx][:, c], wl[:, c, ky, kx])
                lh = lh + np.einsum("nchw,oc->nohw", taps_l[ky, kx][:, c], wh[:, c, ky, kx])
            accM = (accM.astype(np.float64) + m).astype(at)
            if not drop_lo:
                accL = (accL.astype(np.float64) + hl).astype(at)
                accL = (accL.astype(np.float64) + lh).astype(at)
    v = accM + accL * at(1.0 / 2048.0) + np.asarray(shift, np.float32).astype(at).reshape(1, -1, 1, 1)
    return np.maximum(v, at(0)) if relu else v
