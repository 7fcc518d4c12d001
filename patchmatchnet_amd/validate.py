"""Validation against ground-truth depth: the engine side of train.py --mode test (reference train.py:63-76, 127-181; metrics
utils.py:170-221; loss models/net.py:321-342).

The reference scores a batch through boolean indexing (``depth[mask]``), a device synchronisation per call and ten calls per batch.
Here pmn_depth_metrics (ops.depth_metrics) writes one row of raw float64 sums and exact counts per sample on the device, the rows of
a batch reach the host with ONE asynchronous copy into pinned memory, and the reference's scalars are formed from them on the host
(``batch_scalars``) once the copy has landed -- the batch loop never waits for the GPU; its print lines trail the GPU by at most
``depth`` batches, in order.
"""
from __future__ import annotations

import collections
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from ._lib import PmnError

THRESHOLDS = (1.0, 2.0, 4.0, 8.0)  # reference train.py:174


def threshold_name(t: float) -> str:
    """The reference's key, f"threshold-{t}mm-error" with its integer t (1, 2, 4, 8)."""
    t = float(t)
    return "threshold-{}mm-error".format(int(t) if t.is_integer() else t)


def stage_iterations(model) -> List[int]:
    """Maps per stage of the forward's depth_patchmatch: 1 for stage 0 (the refined map), then PatchMatch's iterations of stages
    1, 2, 3 (patchmatch_iteration[s - 1])."""
    return [1] + [int(getattr(model, f"patchmatch_{s}").patchmatch_iteration) for s in range(1, model.stages)]


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(a, np.float64) / np.asarray(b, np.float64)


def image_metrics(row: np.ndarray, iters: Sequence[int], thresholds: Sequence[float] = THRESHOLDS) -> Dict[str, float]:
    """One sample's metrics from its row: what the reference computes per image before it takes the batch mean -- the depth error
    per stage, the threshold error rates, and the masked smooth-L1 mean of every map ("smooth-l1-stage-s-iter-k").  An empty mask
    gives NaN, as torch's mean of an empty tensor does."""
    row = np.asarray(row, np.float64)
    out: Dict[str, float] = {}
    for s, n in enumerate(iters):
        out[f"valid-pixels-stage-{s}"] = float(row[_lib.METRICS_COUNT + s])
        out[f"depth-error-stage-{s}"] = float(_div(row[_lib.METRICS_ABS + s], row[_lib.METRICS_COUNT + s]))
        for k in range(n):
            out[f"smooth-l1-stage-{s}-iter-{k}"] = float(_div(row[_lib.METRICS_SL1 + s * _lib.METRICS_MAX_ITERS + k],
                                                              row[_lib.METRICS_COUNT + s]))
    for i, t in enumerate(thresholds):
        out[threshold_name(t)] = float(_div(row[_lib.METRICS_THR + i], row[_lib.METRICS_COUNT]))
    return out


def batch_scalars(rows: np.ndarray, iters: Sequence[int], thresholds: Sequence[float] = THRESHOLDS) -> Dict[str, float]:
    """The reference's scalar_outputs of one batch (train.py:164-175), restated on the rows [B, METRICS_ROW]:
      loss                  = sum over stages and iterations of (sum_b smooth-L1 sum) / (sum_b valid count of the stage)
                              -- F.smooth_l1_loss(reduction="mean") over the batch's masked pixels, patchmatchnet_loss;
      depth-error-stage-i   = mean over b of (sum |d_last - gt|) / count  -- per image, then the batch mean;
      threshold-{t}mm-error = mean over b of (count of |d0 - gt| > t) / count of stage 0.
    An empty mask gives NaN, as torch does."""
    rows = np.asarray(rows, np.float64).reshape(-1, _lib.METRICS_ROW)
    loss = 0.0
    for s, n in enumerate(iters):
        count = rows[:, _lib.METRICS_COUNT + s].sum()
        for k in range(n):
            loss += float(_div(rows[:, _lib.METRICS_SL1 + s * _lib.METRICS_MAX_ITERS + k].sum(), count))
    out = {"loss": loss}
    for s in range(len(iters)):
        out[f"depth-error-stage-{s}"] = float(_div(rows[:, _lib.METRICS_ABS + s], rows[:, _lib.METRICS_COUNT + s]).mean())
    for i, t in enumerate(thresholds):
        out[threshold_name(t)] = float(_div(rows[:, _lib.METRICS_THR + i], rows[:, _lib.METRICS_COUNT]).mean())
    return out


class DictAverage:
    """The reference's DictAverageMeter (utils.py:138-167): every update counts once, so each batch -- the last, partial one
    included -- weighs the same in ``mean()``."""

    def __init__(self) -> None:
        self.data: Dict[str, float] = {}
        self.count = 0

    def update(self, values: Dict[str, float]) -> None:
        self.count += 1
        for k, v in values.items():
            self.data[k] = self.data.get(k, 0.0) + float(v)

    def mean(self) -> Dict[str, float]:
        return {k: v / self.count for k, v in self.data.items()}


class Validator:
    """Runs the forward and the metrics of one collated batch after another on the current stream and hands back their results in
    order, without waiting for the GPU in ``submit`` / ``poll``.

    ``submit(batch)``: ``batch`` is what a DataLoader over MVSDataset(load_depth_gt=True) yields (pinned, so that the uploads are
    asynchronous); it is uploaded, the forward runs eagerly (``hip_graph=0``) or as one launch-plan replay that also holds the metrics
    launches (``hip_graph=1``, graph.PlannedValidationForward), and the rows are copied into a ring of ``depth`` pinned buffers.  Returns
    the results that are ready; when ``depth`` batches are in flight, it first waits for the oldest one (an event that has long
    completed in a steady pipeline).  ``drain()`` waits for the rest.  A result: {"batch", "scans", "views", "rows" [B,ROW] float64,
    "scalars", "time" = GPU seconds from the batch's upload to its rows}."""

    def __init__(self, model, iters: Sequence[int], thresholds: Sequence[float] = THRESHOLDS, hip_graph: int = 0, depth: int = 4,
                 device=None) -> None:
        if hip_graph not in (0, 1):
            raise PmnError("Validator: hip_graph must be 0 (eager) or 1 (launch plan)")
        self.model, self.iters, self.thresholds = model, list(iters), tuple(float(t) for t in thresholds)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.depth = max(int(depth), 1)
        self.planned = None
        if hip_graph:
            from .graph import PlannedValidationForward
            self.planned = PlannedValidationForward(model, self.thresholds)
        self.ring: List[Optional[torch.Tensor]] = [None] * self.depth
        self.queue: collections.deque = collections.deque()
        self.submitted = 0

    def _up(self, t: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        return t.to(self.device, non_blocking=True).to(dtype)

    def submit(self, batch: Dict) -> List[Dict]:
        ready = []
        if len(self.queue) >= self.depth:
            self.queue[0]["end"].synchronize()
            ready.append(self._finish(self.queue.popleft()))
        gt = batch.get("depth_gt")
        if not isinstance(gt, torch.Tensor) or gt.dim() != 4:
            raise PmnError("Validator: the batch carries no ground truth (MVSDataset(load_depth_gt=True) and a depth_gt file for "
                           "every sample are needed)")
        stream = torch.cuda.current_stream(self.device)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        images = [self._up(im) for im in batch["images"]]
        intrinsics, extrinsics = self._up(batch["intrinsics"]), self._up(batch["extrinsics"])
        depth_min, depth_max = self._up(batch["depth_min"]), self._up(batch["depth_max"])
        depth_gt = self._up(gt)
        with torch.no_grad():
            if self.planned is not None:
                _, _, rows = self.planned(images, intrinsics, extrinsics, depth_min, depth_max, depth_gt)
            else:
                _, _, maps = self.model(images, intrinsics, extrinsics, depth_min, depth_max)
                rows = ops.depth_metrics(depth_gt, depth_min, maps, self.thresholds)
        B = rows.shape[0]
        k = self.submitted % self.depth
        if self.ring[k] is None or self.ring[k].shape[0] < B:
            self.ring[k] = torch.empty((max(B, 1), _lib.METRICS_ROW), dtype=torch.float64).pin_memory()
        host = self.ring[k][:B]
        host.copy_(rows, non_blocking=True)
        end.record(stream)
        self.queue.append({"batch": self.submitted, "host": host, "start": start, "end": end, "B": B,
                           "scans": list(batch.get("scan", [""] * B)), "views": [int(v) for v in batch.get("ref_view", [-1] * B)]})
        self.submitted += 1
        return ready + self.poll()

    def poll(self) -> List[Dict]:
        out = []
        while self.queue and self.queue[0]["end"].query():
            out.append(self._finish(self.queue.popleft()))
        return out

    def drain(self) -> List[Dict]:
        out = []
        while self.queue:
            self.queue[0]["end"].synchronize()
            out.append(self._finish(self.queue.popleft()))
        return out

    def _finish(self, item: Dict) -> Dict:
        rows = item["host"].numpy().copy()
        return {"batch": item["batch"], "scans": item["scans"], "views": item["views"], "rows": rows,
                "scalars": batch_scalars(rows, self.iters, self.thresholds),
                "time": item["start"].elapsed_time(item["end"]) / 1000.0}


def finite_or_none(x: float):
    """JSON has no NaN / inf: such values are written as null."""
    return x if math.isfinite(x) else None
