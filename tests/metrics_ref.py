"""Independent statements of the validation metrics, for the tests of pmn_depth_metrics and train.py --mode test.

``rows_numpy``: the kernel's row layout (include/pmn_hip.h, PMN_METRICS_*) from numpy -- per element fp32 as torch computes it,
every sum by math.fsum (exact, then rounded once).
``reference_scalars``: the reference's own formulas on torch tensors (reference train.py:164-175 + 194-200 create_stage_images,
models/net.py:321-342 patchmatchnet_loss, utils.py:170-221 threshold_metrics / absolute_depth_error_metrics): boolean indexing,
F.smooth_l1_loss, per-image means then the batch mean."""
import math
from typing import Dict, List, Sequence

import numpy as np
import torch
import torch.nn.functional as F

ROW, COUNT, ABS, THR, SL1, MAX_ITERS = 36, 0, 4, 8, 16, 5


def _fsum(x):
    """math.fsum with a float sum's IEEE results: NaN if a NaN or both infinities occur, the infinity if one occurs."""
    x = np.asarray(x, np.float64)
    if np.isnan(x).any() or (np.isposinf(x).any() and np.isneginf(x).any()):
        return float("nan")
    if np.isinf(x).any():
        return float(x[np.isinf(x)][0])
    return math.fsum(x)


def rows_numpy(gt: np.ndarray, depth_min: np.ndarray, stage_maps: Sequence[Sequence[np.ndarray]],
               thresholds: Sequence[float]) -> np.ndarray:
    """gt [B,H,W] float32, depth_min [B] float32, stage_maps[s][k] [B,H>>s,W>>s] float32 -> rows [B,ROW] float64."""
    gt = np.asarray(gt, np.float32)
    B, H, W = gt.shape
    rows = np.zeros((B, ROW), np.float64)
    for b in range(B):
        for s, maps in enumerate(stage_maps):
            g = gt[b, ::1 << s, ::1 << s][:H >> s, :W >> s]
            mask = g >= np.float32(depth_min[b])
            gv = g[mask]
            rows[b, COUNT + s] = int(mask.sum())
            for k, m in enumerate(maps):
                d = np.asarray(m, np.float32)[b][mask]
                with np.errstate(invalid="ignore", over="ignore"):
                    z = np.abs(d - gv)
                    sl = np.where(z < np.float32(1.0), np.float32(0.5) * z * z, z - np.float32(0.5)).astype(np.float32)
                rows[b, SL1 + s * MAX_ITERS + k] = _fsum(sl)
                if k == len(maps) - 1:
                    rows[b, ABS + s] = _fsum(z)
                    if s == 0:
                        for t, th in enumerate(thresholds):
                            with np.errstate(invalid="ignore"):
                                rows[b, THR + t] = int((z > np.float32(th)).sum())
    return rows


def create_stage_images(image: torch.Tensor, stages: int = 4) -> List[torch.Tensor]:
    return [image] + [F.interpolate(image, scale_factor=0.5 ** s, mode="nearest") for s in range(1, stages)]


def reference_scalars(depth_patchmatch: Dict[int, List[torch.Tensor]], depth_gt: torch.Tensor, mask: torch.Tensor,
                      thresholds: Sequence[float] = (1, 2, 4, 8)) -> Dict[str, float]:
    """depth_gt [B,1,H,W] float32, mask [B,1,H,W] bool; the reference's scalar_outputs of one batch as floats."""
    stages = len(depth_patchmatch)
    gts = create_stage_images(depth_gt, stages)
    masks = [m.bool() for m in create_stage_images(mask.float(), stages)]
    loss = 0
    for i in range(stages):
        g = gts[i][masks[i]]
        for depth in depth_patchmatch[i]:
            loss = loss + F.smooth_l1_loss(depth[masks[i]], g, reduction="mean")
    out = {"loss": float(loss)}

    def per_image(fn, est, gt, m, *a):
        return torch.stack([fn(est[b], gt[b], m[b], *a) for b in range(gt.shape[0])]).mean()

    def abs_err(e, g, m):
        e, g = e[m], g[m]
        return torch.mean((e - g).abs())

    def thr_err(e, g, m, t):
        e, g = e[m], g[m]
        return torch.mean((torch.abs(e - g).float() > t).float())

    for i in range(stages):
        out[f"depth-error-stage-{i}"] = float(per_image(abs_err, depth_patchmatch[i][-1], gts[i], masks[i]))
    for t in thresholds:
        out[f"threshold-{t}mm-error"] = float(per_image(thr_err, depth_patchmatch[0][-1], gts[0], masks[0], float(t)))
    return out


def assert_close_dict(got: Dict[str, float], want: Dict[str, float], rtol: float) -> None:
    assert set(got) == set(want), set(got) ^ set(want)
    for k in want:
        g, w = got[k], want[k]
        if math.isnan(w):
            assert math.isnan(g), (k, g, w)
            continue
        assert abs(g - w) <= rtol * max(abs(w), 1e-30) or abs(g - w) <= 1e-12, (k, g, w, abs(g - w) / max(abs(w), 1e-30))
