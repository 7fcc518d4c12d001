"""GPU tests of pmn_depth_metrics (ops.depth_metrics) against a numpy statement -- fp32 per element, math.fsum sums -- and against
the reference's own torch formulas."""
import numpy as np
import pytest
import torch

import metrics_ref as MR

pytestmark = pytest.mark.gpu
THRESHOLDS = (1.0, 2.0, 4.0, 8.0)


def _case(B, H, W, iters, seed):
    """Ground truth around 600 with exact-threshold, both-sides-of-1, NaN / inf estimates; sample 1 (when B > 1) entirely below
    depth_min."""
    rng = np.random.default_rng(seed)
    gt = (550.0 + 100.0 * rng.random((B, H, W))).astype(np.float32)
    gt[:, ::7, ::5] = 500.0  # below depth_min: masked
    dmin = np.full(B, 520.0, np.float32)
    gt[0, 1, 1] = dmin[0] = 530.0  # a pixel exactly at depth_min is valid
    if B > 1:
        gt[1] = 510.0  # empty mask in every stage
    maps = []
    for s, n in enumerate(iters):
        g = gt[:, ::1 << s, ::1 << s][:, :H >> s, :W >> s]
        ms = []
        for k in range(n):
            noise = rng.choice(np.asarray([0.25, 0.999, 1.0, 1.001, 3.0, 12.0], np.float32), size=g.shape) * rng.choice([-1, 1], size=g.shape)
            ms.append((g + noise.astype(np.float32)).astype(np.float32))
        maps.append(ms)
    # stage 0's last map: differences exactly at every threshold (gt = 600 is exact with room for +-8)
    d0 = maps[0][-1]
    gt[0, 2, :8] = 600.0
    d0[0, 2, :8] = 600.0 + np.asarray([1, -1, 2, -2, 4, -4, 8, -8], np.float32)
    d0[0, 3, 0], d0[0, 3, 1], d0[0, 3, 2] = np.nan, np.inf, -np.inf
    if iters[1] > 1:
        maps[1][0][0, 5, 6] = np.nan  # a NaN in an earlier iteration only poisons that map's smooth-L1 sum
    return gt, dmin, maps


def _run(gt, dmin, maps, thresholds=THRESHOLDS):
    import patchmatchnet_amd as P
    dpm = {s: [torch.from_numpy(m).cuda()[:, None] for m in ms] for s, ms in enumerate(maps)}
    return P.ops.depth_metrics(torch.from_numpy(gt).cuda(), torch.from_numpy(dmin).cuda(), dpm, thresholds), dpm


@pytest.mark.parametrize("B,H,W,iters", [(1, 64, 80, (1, 1, 2, 2)), (2, 512, 640, (1, 2, 2, 2)), (3, 1200, 1600, (1, 1, 2, 2)),
                                         (3, 64, 80, (1, 2, 2, 2)), (2, 1200, 1600, (1, 2, 2, 2)), (1, 512, 640, (1, 1, 2, 2))])
def test_rows_match_numpy(B, H, W, iters):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    gt, dmin, maps = _case(B, H, W, iters, seed=B * 1000 + H)
    rows, _ = _run(gt, dmin, maps)
    got = rows.cpu().numpy()
    want = MR.rows_numpy(gt, dmin, maps, THRESHOLDS)
    counts = list(range(MR.COUNT, MR.COUNT + 4)) + list(range(MR.THR, MR.THR + 8))
    np.testing.assert_array_equal(got[:, counts], want[:, counts])
    sums = [i for i in range(MR.ROW) if i not in counts]
    g, w = got[:, sums], want[:, sums]
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w))
    fin = np.isfinite(w)
    np.testing.assert_array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)])
    rel = np.abs(g[fin] - w[fin]) / np.maximum(np.abs(w[fin]), 1e-300)
    assert rel.max(initial=0.0) <= 1e-10, rel.max()
    # the crafted cases really are in there
    assert np.isnan(got[0, MR.SL1]) and np.isnan(got[0, MR.ABS])  # NaN estimate at stage 0
    assert got[0, MR.COUNT] > 0 and np.isfinite(got[0, MR.ABS + 1]) and got[0, MR.THR + 3] >= 2  # +-8 not above 8; +-inf is
    if B > 1:
        assert got[1, :MR.ABS].sum() == 0 and not np.any(got[1])  # empty mask: all zero


def test_three_runs_are_bit_identical():
    gt, dmin, maps = _case(3, 512, 640, (1, 2, 2, 2), seed=5)
    runs = []
    for _ in range(3):
        rows, _ = _run(gt, dmin, maps)
        runs.append(rows.cpu().numpy().tobytes())
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rows, _ = _run(gt, dmin, maps)
    stream.synchronize()
    runs.append(rows.cpu().numpy().tobytes())
    assert len(set(runs)) == 1


def test_against_the_reference_formulas():
    from patchmatchnet_amd import validate as V
    gt, dmin, maps = _case(3, 512, 640, (1, 2, 2, 2), seed=11)
    gt[1] = 560.0 + gt[1] * 0  # every sample has valid pixels (the reference's mean of an empty tensor is NaN; covered on the CPU)
    maps[0][-1][0, 3, :3] = 600.0  # finite estimates
    maps[1][0][0, 5, 6] = gt[0, 10, 12] + np.float32(0.5)
    rows, dpm = _run(gt, dmin, maps)
    got = V.batch_scalars(rows.cpu().numpy(), [1, 2, 2, 2])
    gt_t = torch.from_numpy(gt).cuda()[:, None]
    want = MR.reference_scalars(dpm, gt_t, gt_t >= torch.from_numpy(dmin).cuda()[:, None, None, None])
    MR.assert_close_dict(got, want, 1e-5)


def test_bad_shapes_raise():
    import patchmatchnet_amd as P
    gt, dmin, maps = _case(2, 64, 80, (1, 1, 2, 2), seed=3)
    g, dm = torch.from_numpy(gt).cuda(), torch.from_numpy(dmin).cuda()
    dpm = {s: [torch.from_numpy(m).cuda()[:, None] for m in ms] for s, ms in enumerate(maps)}
    with pytest.raises(P.PmnError, match="nearest down-sampling"):  # H not a multiple of 8: the model's 13x... maps do not fit
        g2 = torch.zeros(2, 100, 80, device="cuda")
        P.ops.depth_metrics(g2, dm, {0: [torch.zeros(2, 1, 100, 80, device="cuda")], 1: [torch.zeros(2, 1, 52, 40, device="cuda")]})
    with pytest.raises(P.PmnError):  # batch mismatch
        P.ops.depth_metrics(g, dm[:1], dpm)
    with pytest.raises(P.PmnError):  # stage 0 of the wrong size
        P.ops.depth_metrics(g, dm, {0: [torch.zeros(2, 1, 64, 72, device="cuda")]})
    with pytest.raises(P.PmnError):  # iterations of one stage disagree
        P.ops.depth_metrics(g, dm, {0: dpm[0], 1: [dpm[1][0], torch.zeros(2, 1, 16, 20, device="cuda")]})
    with pytest.raises(P.PmnError):  # too many thresholds
        P.ops.depth_metrics(g, dm, dpm, thresholds=list(range(9)))
    with pytest.raises(P.PmnError):  # CPU tensor
        P.ops.depth_metrics(g.cpu(), dm, dpm)
    # and the C boundary itself refuses a stage size that is not floor(H / 2^s) with PMN_ERR_SHAPE, launching nothing
    import ctypes
    L = P._lib.lib()
    ptrs = (ctypes.c_void_p * 2)(dpm[0][0].data_ptr(), dpm[1][0].data_ptr())
    it = (ctypes.c_int * 2)(1, 1)
    hw = (ctypes.c_int * 4)(64, 80, 33, 40)
    scratch = torch.empty(P._lib.metrics_scratch(2, 64, 80), dtype=torch.float64, device="cuda")
    out = torch.empty(2, P._lib.METRICS_ROW, dtype=torch.float64, device="cuda")
    rc = L.pmn_depth_metrics(g.data_ptr(), dm.data_ptr(), ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(it, ctypes.c_void_p),
                             ctypes.cast(hw, ctypes.c_void_p), 2, None, 0, 2, 64, 80, scratch.data_ptr(), scratch.numel(),
                             out.data_ptr(), None)
    assert rc == -2
    hw[2] = 32
    rc = L.pmn_depth_metrics(g.data_ptr(), dm.data_ptr(), ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(it, ctypes.c_void_p),
                             ctypes.cast(hw, ctypes.c_void_p), 2, None, 0, 2, 64, 80, scratch.data_ptr(), scratch.numel() - 1,
                             out.data_ptr(), None)
    assert rc == -1  # scratch too small


def test_launch_plan_records_both_launches():
    import ctypes
    import patchmatchnet_amd as P
    gt, dmin, maps = _case(1, 64, 80, (1, 1, 2, 2), seed=4)
    L = P._lib.lib()
    plan = ctypes.c_void_p()
    P._lib.check(L.pmn_plan_create(ctypes.byref(plan)), "create")
    g, dm = torch.from_numpy(gt).cuda(), torch.from_numpy(dmin).cuda()
    dpm = {s: [torch.from_numpy(m).cuda()[:, None] for m in ms] for s, ms in enumerate(maps)}
    out = torch.full((1, P._lib.METRICS_ROW), -1.0, dtype=torch.float64, device="cuda")
    scratch = torch.empty(P._lib.metrics_scratch(1, 64, 80), dtype=torch.float64, device="cuda")  # alive as long as the plan
    P._lib.check(L.pmn_plan_begin(plan), "begin")
    P.ops.depth_metrics(g, dm, dpm, out=out, scratch=scratch)
    P._lib.check(L.pmn_plan_end(plan), "end")
    try:
        names = [L.pmn_plan_kernel_name(plan, i).decode() for i in range(L.pmn_plan_count(plan))]
        assert len(names) == 2 and "depth_metrics_kernel" in names[0] and "depth_metrics_finish_kernel" in names[1], names
        torch.cuda.synchronize()
        assert (out.cpu() == -1.0).all()  # recording launches nothing
        P._lib.check(L.pmn_plan_launch(plan, torch.cuda.current_stream().cuda_stream), "launch")
        want, _ = _run(gt, dmin, maps)
        assert out.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()  # bit for bit (the row holds a NaN)
    finally:
        L.pmn_plan_destroy(plan)
