"""The camera space (tests/camera_space.py) on the device: pmn_stage_projections and pmn_differentiable_warping on rigs that are not
DTU, against the reference's own operations in float64.  The gates are the project's 4 x rule (DESIGN.md sections 14-16): a kernel
may be 4 x as far from float64 as the float32 restatement of the reference is on the same inputs; tests/test_camera_space.py shows on
the CPU that the restatement meets every condition these tests lean on.

(a) pmn_stage_projections by what it is for: where a reference pixel lands in the source image, every rig, every stage.
(b) the six pivot orders of its 4 x 4 inverse, entry by entry (rig `turned`).
(c) pmn_differentiable_warping on the ramps (x index, y index, ones): sampling position and surviving tap weight, every rig, source
    view and stage; behind-camera hypotheses exactly zero on source maps of any size.
(d) one call with NaN, infinite and negative depths and a translation of 1e30.

MEASURED on MI355X: see DESIGN.md section 27 (kernel and reference-float32 position errors per rig)."""
import numpy as np
import pytest
import torch

import camera_space as CS
import ref64 as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gpu():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    import patchmatchnet_amd as P
    P.lib()
    return P


def _library():
    _gpu()
    from patchmatchnet_amd import _lib
    return _lib.lib()


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _stage_projections(intr, extr, nstages, scale0):
    """pmn_stage_projections into a buffer of NaNs -> (return code, rel [nstages,B,V-1,4,4])."""
    B, V = intr.shape[:2]
    K, E = t(intr), t(extr)
    rel = torch.full((nstages, B, V - 1, 4, 4), float("nan"), dtype=torch.float32, device=DEV)
    with torch.cuda.device(rel.device):
        rc = _library().pmn_stage_projections(K.data_ptr(), E.data_ptr(), B, V, nstages, float(scale0), rel.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, n(rel)


def _warp(src, proj, depth, poison=float("nan")):
    """pmn_differentiable_warping (the C entry point: the projection is given, not computed) into a poisoned buffer ->
    (return code, warped [B,C,D,h,w]).  src [B,C,hs,ws], proj [B,4,4], depth [B,D,h,w]."""
    B, C, hs, ws = src.shape
    _, D, h, w = depth.shape
    assert proj.shape == (B, 4, 4) and hs >= 2 and ws >= 2 and h >= 2 and w >= 2
    s, p, d = t(src.astype(np.float32)), t(proj.astype(np.float32)), t(depth.astype(np.float32))
    out = torch.full((B, C, D, h, w), poison, dtype=torch.float32, device=DEV)
    with torch.cuda.device(out.device):
        rc = _library().pmn_differentiable_warping(s.data_ptr(), p.data_ptr(), d.data_ptr(), B, C, D, h, w, hs, ws, out.data_ptr(),
                                                     _stream())
    torch.cuda.synchronize()
    return rc, n(out)


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CS.RIG_NAMES)
def test_stage_projections_land_pixels_where_float64_does(name):
    rig = CS.rigs()[name]
    rc, rel = _stage_projections(rig.intrinsics, rig.extrinsics, rig.nstages, rig.scale0)
    assert rc == 0
    assert rel.shape == (rig.nstages, rig.B, rig.V - 1, 4, 4)
    assert np.isfinite(rel).all(), "an element of the output was not written"
    P = _gpu()
    again = n(P.ops.stage_projections(t(rig.intrinsics), t(rig.extrinsics), rig.nstages, rig.scale0))
    assert again.shape == rel.shape and np.array_equal(again, rel)
    for s, scale in enumerate(rig.scales()):
        kernel = CS.projection_error(rel[s], rig, s)
        ref = CS.projection_error(CS.projections(rig, scale, np.float32), rig, s)
        print(f"MEASURED {name} stage {s} (scale {scale:g}): pmn_stage_projections {kernel:.3e} px, reference float32 {ref:.3e} px")
        assert ref > 0.0
        assert kernel <= 4.0 * ref, f"{name} stage {s}: {kernel:.3e} px > 4 x {ref:.3e} px"


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kernel_inverses():
    """inverse(P_ref) of every sample of `turned` as the kernel computes it: view 1 gets K = diag(1 / scale0, 1 / scale0, 1) and
    E = I, so its projection at the stage's scale is the identity and rel = inverse(P_ref), rounded once."""
    rig = CS.rigs()["turned"]
    assert rig.nstages == 1 and 1.0 / rig.scale0 == 4.0
    intr, extr = rig.intrinsics.copy(), rig.extrinsics.copy()
    intr[:, 1] = np.diag([1.0 / rig.scale0, 1.0 / rig.scale0, 1.0]).astype(np.float32)
    extr[:, 1] = np.eye(4, dtype=np.float32)
    rc, rel = _stage_projections(intr, extr, 1, rig.scale0)
    assert rc == 0 and rel.shape == (1, rig.B, 1, 4, 4)
    return rel[0, :, 0], CS.stage_proj(rig, rig.scale0, np.float32)[:, 0]


@pytest.mark.parametrize("pattern", CS.PATTERNS, ids=[f"col0-row{p[0]}-col1-row{p[1]}" for p in CS.PATTERNS])
def test_inverse_on_every_pivot_pattern(kernel_inverses, pattern):
    inv, P_ref = kernel_inverses
    cases = CS.pivot_cases()[pattern]
    assert cases
    for b in cases:
        assert CS.pivot_pattern(P_ref[b]) == pattern
        ratio, ok = CS.inverse_gate(inv[b], P_ref[b])
        port = CS.gauss_jordan_port(P_ref[b])
        print(f"MEASURED turned b={b} pattern {pattern[:2]}: kernel inverse at {ratio:.3f} of its per-entry bound; "
              f"{int((inv[b] != port).sum())} of 16 entries differ from the CPU port")
        assert ok, f"turned b={b}, pattern {pattern}: an entry of the kernel's inverse is {ratio:.3g} x its bound"


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------

def _check_warp_case(name, c):
    B = c.P.shape[0]
    src = np.broadcast_to(CS.ramps(c.hs, c.ws), (B, 3, c.hs, c.ws))
    rc, out = _warp(src, c.P, c.depth)
    assert rc == 0
    assert out.shape == (B, 3) + c.depth.shape[1:]
    assert np.isfinite(out).all(), "an element of the output was not written"
    rc2, out2 = _warp(src, c.P, c.depth, poison=float("inf"))
    assert rc2 == 0 and np.array_equal(out, out2), "a second call gives other bits"
    keep = ~c.near
    assert 1.0 - keep.mean() <= 0.01
    o = out.transpose(1, 0, 2, 3, 4).astype(np.float64)
    want, ref32 = c.want.transpose(1, 0, 2, 3, 4), c.ref32.transpose(1, 0, 2, 3, 4).astype(np.float64)
    k_err = [float(np.abs(o[ch] - want[ch])[keep].max()) for ch in range(3)]
    r_err = [float(np.abs(ref32[ch] - want[ch])[keep].max()) for ch in range(3)]
    behind = ~c.pos64[2] & ~c.pos32[2] & keep
    leak = float(np.abs(o[:, behind]).max()) if behind.any() else 0.0
    # the position the kernel sampled at, where all four taps are inside (channel 2, the tap weights, is one there)
    inside = CS.classify(c.pos64[0], c.pos64[1], c.pos64[2], c.hs, c.ws)["inside"] & keep
    k_pos = r_pos = 0.0
    if inside.any():
        k_pos = float(max(np.abs(o[0] - c.pos64[0])[inside].max(), np.abs(o[1] - c.pos64[1])[inside].max()))
        r_pos = float(max(np.abs(ref32[0] - c.pos64[0])[inside].max(), np.abs(ref32[1] - c.pos64[1])[inside].max()))
    for ch in range(3):
        assert k_err[ch] <= 4.0 * r_err[ch], (f"{name} stage {c.stage} view {c.view} channel {ch}: kernel {k_err[ch]:.3e} > 4 x reference "
                                              f"float32 {r_err[ch]:.3e}")
    return k_err, r_err, k_pos, r_pos, int(behind.sum()), leak


@pytest.mark.parametrize("name", CS.RIG_NAMES)
def test_warping_on_the_ramps(name):
    """A hypothesis behind the source camera is exactly zero in all three channels, also where hs < h or ws < w (`mixed`: source 1's
    map is 12 x 16 under a 24 x 32 reference).  The reference's sentinel (w, h, 1) is carried to (w (ws-1)/(w-1), h (hs-1)/(h-1)) =
    (15.48, 11.48) there: the last texel, with the weight (1 - 15/31) (1 - 11/23) = 0.269.  Measured on MI355X with that chain:
    behind-camera samples of `mixed` up to 4.039 (texel 15 x 0.269); `ring` (equal sizes) all zero.  pmn_pose_position now replaces
    such a point by (2w, 2h, 1), which the same chain carries outside every tap of any map."""
    worst = np.zeros((2, 3))
    pos = np.zeros(2)
    behind = 0
    for c in CS.warp_cases(name):
        k, r, kp, rp, nb, leak = _check_warp_case(name, c)
        assert leak == 0.0, f"{name} stage {c.stage} view {c.view}: a behind-camera hypothesis samples {leak:.3e} of the {c.hs}x{c.ws} map"
        worst = np.maximum(worst, [k, r])
        pos = np.maximum(pos, [kp, rp])
        behind += nb
    print(f"MEASURED {name} warp 24x32: kernel (x, y, 1) {worst[0][0]:.3e} {worst[0][1]:.3e} {worst[0][2]:.3e}, reference float32 "
          f"{worst[1][0]:.3e} {worst[1][1]:.3e} {worst[1][2]:.3e}; inside positions: kernel {pos[0]:.3e} px, reference float32 "
          f"{pos[1]:.3e} px; {behind} behind-camera samples, all exactly zero")
    if "behind" in CS.rigs()[name].shares:
        assert behind > 0


@pytest.mark.parametrize("name", CS.LARGE)
def test_warping_on_the_ramps_at_296x400(name):
    c = CS.large_case(name)
    assert (c.h, c.w, c.depth.shape[1]) == (296, 400, 4)
    k, r, kp, rp, _, _ = _check_warp_case(name, c)
    print(f"MEASURED {name} warp 296x400: kernel (x, y, 1) {k[0]:.3e} {k[1]:.3e} {k[2]:.3e}, reference float32 {r[0]:.3e} {r[1]:.3e} "
          f"{r[2]:.3e}; inside positions: kernel {kp:.3e} px, reference float32 {rp:.3e} px")


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------------

def test_warping_extremes():
    """One 8 x 8 call on the ring with the seven source views as the batch: hypothesis 2 is NaN, 4 is +inf, 6 is -3 everywhere, and
    view 4's projection has an x and y translation of 1e30.  The call succeeds; NaN and infinite depths, and every hypothesis under
    the 1e30 translation, give exact zeros; a negative depth gives zero wherever the point is behind the source camera (on a ring it
    is in FRONT of the cameras beside the reference: there it is sampled like any other point, and must agree with float64); all
    other hypotheses have the bits of a call without the poison.  Every address the kernel forms is legal by construction
    (pmn_axis clamps before the integer conversion): this checks the values that come out, it provokes nothing."""
    rig = CS.rigs()["ring"]
    h = w = D = 8
    P = CS.projections(rig, rig.scale0, np.float32, CS.cropped(rig, 0, h, w))[0]            # [7,4,4]
    depth = np.stack([CS.hypotheses(rig, 0, D, h, w, seed=9)] * 7)
    src = np.broadcast_to(CS.ramps(h, w), (7, 3, h, w))
    rc, clean = _warp(src, P, depth)
    assert rc == 0 and np.isfinite(clean).all() and (clean != 0).any()
    bad_d, bad_P = depth.copy(), P.copy()
    bad_d[:, 2], bad_d[:, 4], bad_d[:, 6] = np.nan, np.inf, -3.0
    bad_P[3, 0, 3] = bad_P[3, 1, 3] = 1e30
    rc, out = _warp(src, bad_P, bad_d)
    assert rc == 0, "PMN_OK expected"
    assert np.isfinite(out).all()
    assert (out[:, :, 2] == 0).all() and (out[:, :, 4] == 0).all() and (out[3] == 0).all()
    others = [b for b in range(7) if b != 3]
    for b in others:
        ix, iy, front = CS.positions(P[b], bad_d[b, 6:7], h, w, h, w, np.float64)
        assert (out[b, :, 6:7][:, ~front] == 0).all()
        want = R.bilinear(CS.ramps(h, w), ix, iy)
        jx, jy, _ = CS.positions(P[b], bad_d[b, 6:7], h, w, h, w, np.float32)
        ref = np.abs(R.bilinear(CS.ramps(h, w), jx, jy, dtype=np.float32) - want).max()
        assert np.abs(out[b, :, 6:7] - want).max() <= 4.0 * max(ref, float(np.spacing(np.float32(w))))
    for d in (0, 1, 3, 5, 7):
        assert np.array_equal(out[others][:, :, d], clean[others][:, :, d]), d
