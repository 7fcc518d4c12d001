"""Tensor-level entry points of the HIP path: thin, checked wrappers over the C ABI (include/pmn_hip.h).

PyTorch is used here only as the owner of device memory and of the current HIP stream.  Every function requires
float32, contiguous tensors on a ROCm device and raises otherwise -- there is no CPU or eager fallback.
"""
from __future__ import annotations

import ctypes
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import PmnError, check


# ---- optional per-launch timing of the hot kernel (bench.py's roofline leg) --------------------------------------
# When enabled, every pmn_warp_correlate launch is bracketed by HIP events recorded on the launch stream (torch's
# current stream) and tagged with its ALGORITHMIC byte count B_alg = 4*h*w*[(1+N)*C + D + N + G*D].
_TIMING = None
_TIMING_ON = True


def enable_kernel_timing() -> None:
    global _TIMING, _TIMING_ON
    _TIMING, _TIMING_ON = [], True


def pause_kernel_timing(paused: bool) -> None:
    """Suspends / resumes recording without dropping what was recorded (an event pair costs ~10 us of stream time on
    ROCm, so bench.py samples every few steps instead of bracketing every launch)."""
    global _TIMING_ON
    _TIMING_ON = not paused


def disable_kernel_timing():
    """Stops recording and returns [(milliseconds, algorithmic_bytes, tag), ...] (synchronises once)."""
    global _TIMING
    rec, _TIMING = _TIMING, None
    if not rec:
        return []
    torch.cuda.synchronize()
    return [(s.elapsed_time(e), nbytes, tag) for s, e, nbytes, tag in rec]


TUNE_WINDOW_BYTES, TUNE_FLAGS, TUNE_WINDOW_BYTES_PIXELWISE, TUNE_ABLATE = 0, 1, 2, 3
TUNE_LANE_WINDOW_BYTES, TUNE_LANE_ABLATE, TUNE_LANE_WAVES_PER_SIMD = 4, 5, 6
TUNE_TILE_WINDOW_BYTES = 10
FLAG_WINDOWED, FLAG_NO_ROTATION, FLAG_STREAM_PIXELWISE, FLAG_STREAM_VIEWS, FLAG_WIN_V1, FLAG_TILE, FLAG_MFMA = 1, 2, 4, 8, 16, 32, 64
DEFAULT_FLAGS = 0  # the library default: streaming kernels for every launch (the fastest measured, profiles/README.md)


def set_tuning(key: int, value: int) -> None:
    """pmn_set_tuning of the EXPERIMENTAL build only (include/pmn_hip_experimental.h; PMN_EXPERIMENTAL=1): selects one of the
    research kernel families of pmn_warp_correlate / their window sizes; all families give bit-identical results
    (tests/test_gather_win.py).  The product library has neither the kernels nor the symbol."""
    if not _lib.experimental():
        raise PmnError("pmn_set_tuning exists only in libpmn_hip_experimental.so: build with `make -C patchmatchnet_amd/csrc "
                       "EXPERIMENTAL=1` and run with PMN_EXPERIMENTAL=1")
    check(_lib.lib().pmn_set_tuning(int(key), int(value)), "pmn_set_tuning")


# ---- opt-in activation-range check of the fp16-split entry points (PMN_CHECK_F16_DOMAIN=1; include/pmn_hip.h) --------------------------
import os as _os

F16_DOMAIN_CHECK = _os.environ.get("PMN_CHECK_F16_DOMAIN", "") == "1"
_F16_FLAGS = {}


def _f16_domain_probe(*tensors: Optional[torch.Tensor]) -> None:
    """PMN_CHECK_F16_DOMAIN=1: one pmn_check_f16_domain launch per input of an _f16s entry point (a pass over the tensor: a debugging
    aid for checkpoints / inputs other than the ones this was built on, not a default)."""
    if not F16_DOMAIN_CHECK:
        return
    for t in tensors:
        if t is None or not t.is_cuda or t.numel() == 0:
            continue
        flag = _F16_FLAGS.get(t.device)
        if flag is None:
            flag = _F16_FLAGS[t.device] = torch.zeros(1, dtype=torch.int32, device=t.device)
        with torch.cuda.device(t.device):
            check(_lib.lib().pmn_check_f16_domain(t.data_ptr(), t.numel(), flag.data_ptr(), _stream(t)), "pmn_check_f16_domain")


def f16_domain_check(reset: bool = True) -> None:
    """Raises PmnError when an activation handed to an fp16-split kernel since the last call was not finite or >= 65504 in magnitude
    (synchronises; only meaningful with PMN_CHECK_F16_DOMAIN=1)."""
    bad = [str(d) for d, f in _F16_FLAGS.items() if int(f.item()) != 0]
    if reset:
        for f in _F16_FLAGS.values():
            f.zero_()
    if bad:
        raise PmnError("an activation outside the fp16-split kernels' domain (|x| >= 65504 or not finite) reached pmn_*_f16s on " +
                       ", ".join(bad) + ": the outputs contain inf / NaN where an fp32 convolution is finite -- set f16_split = False on "
                       "FeatureNet / Refinement / PatchMatch for this checkpoint or input range (include/pmn_hip.h)")


def _dev(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise PmnError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise PmnError(f"{name}: tensor is on {t.device}; patchmatchnet_amd runs only on a ROCm GPU (no CPU fallback)")
    if t.dtype != torch.float32:
        raise PmnError(f"{name}: expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise PmnError(f"{name}: tensor must be contiguous")
    return t


def _dlast(t: torch.Tensor, name: str) -> torch.Tensor:
    """[B,D,h,w] tensor whose STORAGE is hypothesis-last [B,h,w,D] (what pmn_init_hypotheses / pmn_warp_correlate write and
    pmn_aggregate_regress reads); a planar tensor (tests, oracle data) is re-laid-out here."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise PmnError(f"{name}: expected a float32 tensor on a ROCm GPU (no CPU fallback)")
    if t.permute(0, 2, 3, 1).is_contiguous():
        return t
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _dev_as(t: torch.Tensor, name: str, dtype: torch.dtype) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise PmnError(f"{name}: expected a tensor on a ROCm GPU (no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous():
        raise PmnError(f"{name}: expected a contiguous {dtype} tensor")
    return t


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


# ---- the fork / join region of a launch plan that is being recorded (include/pmn_hip.h: pmn_plan_fork; graph.PlannedForward) -------------
# PatchmatchNet.forward marks the stretch whose launches fall into two independent branches with plan_fork / plan_switch / plan_join.
# Outside a plan recording the three are no-ops: eager launches and HIP-graph capture stay on one stream, in the same order.  While
# a plan is recorded they tag its entries, and -- because the recording pass runs the branches one after the other while a replay
# runs them side by side -- guard the one thing sequential recording hides: the caching allocator handing a block that one branch
# freed to the other branch (DESIGN_LESSONS.md).  Every tensor allocated inside the region is held until the join, so no block is
# reused inside it, and what each branch's calls read and write is collected and checked for overlap at the join (host only).
_RECORDING = threading.local()


class PlanRegion:
    """Per-recording state: ``plan`` (the pmn_plan handle), the open region's branch, the tensors held until the join, and per branch
    the (address, bytes) ranges its calls read / wrote / allocated."""

    def __init__(self, plan) -> None:
        self.plan, self.open, self.branch, self.forked = plan, False, 0, False
        self.held: List[torch.Tensor] = []
        self.reads = {0: [], 1: []}
        self.writes = {0: [], 1: []}
        self.allocated = {0: [], 1: []}
        self.held_bytes = 0


def begin_plan_recording(plan) -> PlanRegion:
    """graph.PlannedForward: this thread records ``plan`` from now on (until end_plan_recording)."""
    _RECORDING.region = PlanRegion(plan)
    return _RECORDING.region


def end_plan_recording() -> None:
    _RECORDING.region = None


def _region() -> Optional[PlanRegion]:
    return getattr(_RECORDING, "region", None)


def plan_fork() -> None:
    r = _region()
    if r is not None:
        check(_lib.lib().pmn_plan_fork(r.plan), "pmn_plan_fork")
        r.open, r.branch, r.forked = True, 0, True


def plan_switch(branch: int) -> None:
    """0 = main, 1 = side: the branch of the launches that follow."""
    r = _region()
    if r is not None:
        check(_lib.lib().pmn_plan_switch(r.plan, int(branch)), "pmn_plan_switch")
        r.branch = int(branch)


def plan_join() -> None:
    r = _region()
    if r is not None:
        for b in (0, 1):  # every block the region allocated is the output of a call that declared it
            for rng in r.allocated[b]:
                if not any(_ranges_overlap(rng, w) for w in r.writes[b]):
                    raise PmnError("plan_join: a tensor allocated between fork and join is not among the outputs its branch's calls "
                                   "declared (ops._note): the overlap check would not see it")
        check_branch_overlap(r.reads[0], r.writes[0], r.reads[1], r.writes[1])
        check(_lib.lib().pmn_plan_join(r.plan), "pmn_plan_join")
        r.open, r.branch = False, 0
        r.held.clear()


def _range(t: torch.Tensor) -> Tuple[int, int]:
    return (t.data_ptr(), t.numel() * t.element_size())  # (every tensor the kernels see is dense, possibly permuted)


def _ranges_overlap(a: Tuple[int, int], b: Tuple[int, int]) -> bool:
    return a[1] > 0 and b[1] > 0 and a[0] < b[0] + b[1] and b[0] < a[0] + a[1]


def check_branch_overlap(main_reads, main_writes, side_reads, side_writes) -> None:
    """(address, bytes) ranges of what the two branches of a fork read and write: raises PmnError when one branch writes what the
    other reads or writes (on replay the branches run concurrently).  Host arithmetic only."""
    for who, writes, others in (("main", main_writes, list(side_reads) + list(side_writes)),
                                ("side", side_writes, list(main_reads) + list(main_writes))):
        for w in writes:
            for o in others:
                if _ranges_overlap(w, o):
                    raise PmnError(f"plan fork: the {who} branch writes [{w[0]:#x}, +{w[1]}) which the other branch touches at "
                                   f"[{o[0]:#x}, +{o[1]}): the branches run concurrently on replay and must not share a buffer")


def _hold(t, fresh: bool) -> None:
    """graph._LibraryLaunchesOnly: a tensor the recording pass just allocated (``fresh``) or derived."""
    r = _region()
    if r is not None and r.open and isinstance(t, torch.Tensor) and t.is_cuda:
        r.held.append(t)
        if fresh and t.numel():
            r.allocated[r.branch].append(_range(t))
            r.held_bytes += t.numel() * t.element_size()


def _note(reads, writes) -> None:
    """What the call being issued reads and writes (tensors; None entries are skipped), for the open region's overlap check."""
    r = _region()
    if r is not None and r.open:
        r.reads[r.branch] += [_range(t) for t in reads if t is not None]
        r.writes[r.branch] += [_range(t) for t in writes if t is not None]


def _host_f32(a: np.ndarray, n: int, name: str):
    a = np.ascontiguousarray(a, np.float32)
    if a.size != n:
        raise PmnError(f"{name}: expected {n} floats, got {a.size}")
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _host_i32(a: np.ndarray, n: int, name: str):
    a = np.ascontiguousarray(a, np.int32)
    if a.size != n:
        raise PmnError(f"{name}: expected {n} ints, got {a.size}")
    return a, a.ctypes.data_as(ctypes.c_void_p)


def nchw_to_nhwc(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B,C,h,w] -> [B,h,w,C] (fresh tensor, or into ``out`` which may be a slice of a stacked buffer).  An input that is
    already channels-last in memory (an NCHW-shaped view of NHWC storage) is returned as a view, without a copy."""
    if out is None and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and not x.is_contiguous():
        v = x.permute(0, 2, 3, 1)
        if v.is_contiguous():
            return v
        x = x.contiguous()
    _dev(x, "x")
    B, C, h, w = x.shape
    if out is None:
        out = torch.empty((B, h, w, C), dtype=torch.float32, device=x.device)
    else:
        _dev(out, "out")
        if tuple(out.shape) != (B, h, w, C):
            raise PmnError("nchw_to_nhwc: bad output shape")
    _note((x,), (out,))
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_nchw_to_nhwc(x.data_ptr(), out.data_ptr(), B, C, h, w, _stream(x)), "pmn_nchw_to_nhwc")
    return out


def stack_sources_nhwc(src_features: Sequence[torch.Tensor]) -> torch.Tensor:
    """List of N source feature maps [B,C,hs,ws] -> one channels-last buffer [N,B,hs,ws,C] (all maps one size; see
    ``stack_sources_padded`` for source views of different sizes)."""
    buf, sizes = stack_sources_padded(src_features)
    if any(sz != sizes[0] for sz in sizes):
        raise PmnError("all source feature maps of one stage must share a shape (stack_sources_padded handles mixed sizes)")
    return buf


def stack_sources_padded(src_features: Sequence[torch.Tensor]):
    """List of N source feature maps [B,C,hs_v,ws_v] -> (channels-last buffer [N,B,HS,WS,C] with HS x WS the LARGEST map and every
    smaller map in the top-left corner of its slice, zeros elsewhere; [(hs_v, ws_v)]).  The reference warps every source view at
    its own size (models/module.py:130-181: F.grid_sample un-normalises with the source map's size and pads with zeros), so a
    sample whose images differ in size is legal there; pmn_warp_correlate reads one size per launch, and zero padding IS
    grid_sample's padding -- the per-view scale is restored on the projection (``rescale_projection_rows``)."""
    if len(src_features) == 0:
        raise PmnError("at least one source view is required")
    B, C = src_features[0].shape[:2]
    sizes = [(int(f.shape[2]), int(f.shape[3])) for f in src_features]
    if any(tuple(f.shape[:2]) != (B, C) for f in src_features):
        raise PmnError("source feature maps of one stage must share batch size and channels")
    hs, ws = max(h for h, _ in sizes), max(w for _, w in sizes)
    mixed = any(sz != (hs, ws) for sz in sizes)
    alloc = torch.zeros if mixed else torch.empty
    buf = alloc((len(src_features), B, hs, ws, C), dtype=torch.float32, device=src_features[0].device)
    for i, f in enumerate(src_features):
        v = f.permute(0, 2, 3, 1)
        if sizes[i] != (hs, ws):
            _dev(f.contiguous(), "src_feature")
            buf[i][:, :sizes[i][0], :sizes[i][1], :].copy_(v)
        elif f.is_cuda and f.dtype == torch.float32 and v.is_contiguous():
            buf[i].copy_(v)  # an NCHW-shaped view of channels-last storage (the HIP FeatureNet's output): one plain copy, not a
            #                  transpose to NCHW and back (eval.py's encode-once path hands such views over, 5 per stage)
        else:
            nchw_to_nhwc(f.contiguous(), buf[i])
    return buf, sizes


def rescale_projection_rows(rel_proj: torch.Tensor, sizes, padded_hw) -> torch.Tensor:
    """Relative projections [B,N,4,4] for source maps that sit zero-padded in an HS x WS buffer: the kernel scales the projected
    position by (WS-1)/(w-1), the reference by (ws_v-1)/(w-1) (normalise with the reference map, un-normalise with the source map:
    models/module.py:170-181) -- rows 0 / 1 of view v are multiplied by (ws_v-1)/(WS-1) / (hs_v-1)/(HS-1).  Identity (same tensor)
    when every map has the padded size."""
    HS, WS = padded_hw
    if all(sz == (HS, WS) for sz in sizes):
        return rel_proj
    out = rel_proj.clone()
    for v, (h_v, w_v) in enumerate(sizes):
        if (h_v, w_v) != (HS, WS):
            out[:, v, 0, :] *= (w_v - 1) / (WS - 1)
            out[:, v, 1, :] *= (h_v - 1) / (HS - 1)
    return out.contiguous()


def _mlp_dev(t: torch.Tensor, name: str) -> torch.Tensor:
    _dev(t, name)
    if t.numel() != _lib.MLP_FLOATS:
        raise PmnError(f"{name}: expected a packed MLP block of {_lib.MLP_FLOATS} floats")
    return t


def feature_weight(ref_nhwc: torch.Tensor, eval_offsets: torch.Tensor, table: np.ndarray, mlp: torch.Tensor,
                   G: int) -> torch.Tensor:
    """FeatureWeightNet (reference models/patchmatch.py:603-624) -> [B,K,h,w]."""
    _dev(ref_nhwc, "ref_nhwc")
    _dev(eval_offsets, "eval_offsets")
    B, h, w, C = ref_nhwc.shape
    K = eval_offsets.shape[1] // 2
    if tuple(eval_offsets.shape) != (B, 2 * K, h, w):
        raise PmnError("feature_weight: eval_offsets must be [B,2K,h,w]")
    tab, tab_p = _host_i32(table, 2 * K, "table")
    _mlp_dev(mlp, "mlp")
    out = torch.empty((B, K, h, w), dtype=torch.float32, device=ref_nhwc.device)
    _note((ref_nhwc, eval_offsets, mlp), (out,))
    with torch.cuda.device(ref_nhwc.device):
        check(_lib.lib().pmn_feature_weight(ref_nhwc.data_ptr(), eval_offsets.data_ptr(), tab_p, mlp.data_ptr(), B, C, G,
                                            K, h, w,
                                            out.data_ptr(), _stream(out)), "pmn_feature_weight")
    return out


def init_hypotheses(noise: Optional[torch.Tensor], depth: Optional[torch.Tensor], depth_shift: int,
                    depth_min: torch.Tensor, depth_max: torch.Tensor, num_sample: int, interval_scale: float,
                    propa_offsets: Optional[torch.Tensor], table: Optional[np.ndarray], h: int, w: int
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """DepthInitialization + Propagation (reference models/patchmatch.py:53-94, 115-124).

    Returns (depth_sample [B,D,h,w], xnorm [B,D,h,w] -- a hypothesis-last view: storage [B,h,w,D])."""
    _dev(depth_min, "depth_min")
    _dev(depth_max, "depth_max")
    B = depth_min.shape[0]
    dev = depth_min.device
    if noise is not None:
        _dev(noise, "noise")
        if tuple(noise.shape) != (B, 48, h, w):
            raise PmnError("init_hypotheses: noise must be [B,48,h,w]")
        D0 = 48
    else:
        if depth is None:
            raise PmnError("init_hypotheses: need noise or depth")
        _dev(depth, "depth")
        if tuple(depth.shape) != (B, 1, h >> depth_shift, w >> depth_shift):
            raise PmnError(f"init_hypotheses: depth must be [B,1,{h >> depth_shift},{w >> depth_shift}], "
                           f"got {tuple(depth.shape)}")
        D0 = num_sample
    K = 0
    tab_p = None
    tab = None
    if propa_offsets is not None:
        _dev(propa_offsets, "propa_offsets")
        K = propa_offsets.shape[1] // 2
        if tuple(propa_offsets.shape) != (B, 2 * K, h, w):
            raise PmnError("init_hypotheses: propa_offsets must be [B,2K,h,w]")
        tab, tab_p = _host_i32(table, 2 * K, "table")
    D = D0 + K
    ds = torch.empty((B, D, h, w), dtype=torch.float32, device=dev)
    xn = torch.empty((B, h, w, D), dtype=torch.float32, device=dev).permute(0, 3, 1, 2)
    _note((noise, depth if noise is None else None, depth_min, depth_max, propa_offsets), (ds, xn))
    with torch.cuda.device(dev):
        check(_lib.lib().pmn_init_hypotheses(_ptr(noise), _ptr(depth) if noise is None else None, depth_shift,
                                             depth_min.data_ptr(), depth_max.data_ptr(), num_sample,
                                             float(interval_scale), _ptr(propa_offsets), tab_p, K, B, h, w,
                                             ds.data_ptr(), xn.data_ptr(), _stream(ds)), "pmn_init_hypotheses")
    del tab
    return ds, xn


class SourceTable:
    """The source views of a sample as a DEVICE table of per-view addresses (pmn_warp_correlate_views) instead of one stacked
    [N,B,hs,ws,C] tensor: ``table`` int64 [N] on the device, entry v = data_ptr of view v's channels-last [B,hs,ws,C] map.  Duck-types
    the stacked tensor where only its shape / device are read.  The maps themselves must outlive the launch (the caller holds them)."""

    def __init__(self, table: torch.Tensor, shape) -> None:
        if table.dtype != torch.int64 or not table.is_cuda or table.numel() != int(shape[0]):
            raise PmnError("SourceTable: int64 device tensor with one address per source view")
        self.table, self.shape, self.device = table, tuple(int(x) for x in shape), table.device

    @staticmethod
    def image_in_place(im: torch.Tensor) -> bool:
        """True when pmn_stem_f16s_views can read this [B,3,H,W] image where it is (dense float32, 16-byte aligned)."""
        return bool(im.is_cuda and im.dtype == torch.float32 and im.is_contiguous() and im.data_ptr() % 16 == 0)

    @staticmethod
    def addresses(maps) -> list:
        """data_ptr of every view's map after checking it is a dense channels-last [B,hs,ws,C] float32 device tensor."""
        out = []
        for m in maps:
            if not (m.is_cuda and m.dtype == torch.float32 and m.is_contiguous()):
                raise PmnError("SourceTable: dense float32 channels-last device maps")
            out.append(m.data_ptr())
        return out


def warp_correlate(ref_nhwc: torch.Tensor, src_nhwc, rel_proj: torch.Tensor, depth_sample: torch.Tensor,
                   view_weights: Optional[torch.Tensor], vw_shift: int, similarity_mlp: torch.Tensor,
                   pixelwise_mlp: Optional[torch.Tensor], G: int, want_similarity: bool = False,
                   want_argmax: bool = False):
    """The fused warp + gather + group-correlation + view aggregation + SimilarityNet-MLP kernel.

    Returns (cost [B,D,h,w] (a hypothesis-last view: storage [B,h,w,D]), view_weights [B,N,h,w] (input passed through, or computed), argmax or None,
    aggregated similarity [B,G,D,h,w] or None)."""
    _dev(ref_nhwc, "ref_nhwc")
    table = src_nhwc if isinstance(src_nhwc, SourceTable) else None
    if table is None:
        _dev(src_nhwc, "src_nhwc")
    _dev(rel_proj, "rel_proj")
    _dev(depth_sample, "depth_sample")
    B, h, w, C = ref_nhwc.shape
    N, Bs, hs, ws, Cs = src_nhwc.shape
    D = depth_sample.shape[1]
    if Bs != B or Cs != C or tuple(depth_sample.shape) != (B, D, h, w) or tuple(rel_proj.shape) != (B, N, 4, 4):
        raise PmnError("warp_correlate: inconsistent shapes")
    dev = ref_nhwc.device
    sim_p = _mlp_dev(similarity_mlp, "similarity_mlp").data_ptr()
    pix_p, vw_out, argmax = None, None, None
    if view_weights is not None:
        _dev(view_weights, "view_weights")
        if tuple(view_weights.shape) != (B, N, h >> vw_shift, w >> vw_shift):
            raise PmnError("Patchmatch Evaluation: Different number of images and view weights")
    else:
        if pixelwise_mlp is None:
            raise PmnError("warp_correlate: pixelwise_mlp required when view_weights is None")
        pix_p = _mlp_dev(pixelwise_mlp, "pixelwise_mlp").data_ptr()
        vw_out = torch.empty((B, N, h, w), dtype=torch.float32, device=dev)
        if want_argmax:
            argmax = torch.empty((B, N, h, w), dtype=torch.int32, device=dev)
    cost = torch.empty((B, h, w, D), dtype=torch.float32, device=dev).permute(0, 3, 1, 2)  # hypothesis-last storage
    sim = torch.empty((B, G, D, h, w), dtype=torch.float32, device=dev) if want_similarity else None
    _note((ref_nhwc, src_nhwc if table is None else table.table, rel_proj, depth_sample, view_weights, similarity_mlp, pixelwise_mlp),
          (cost, vw_out, argmax, sim))
    with torch.cuda.device(dev):
        if _TIMING is not None and _TIMING_ON:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        fn = _lib.lib().pmn_warp_correlate if table is None else _lib.lib().pmn_warp_correlate_views
        check(fn(ref_nhwc.data_ptr(), (src_nhwc if table is None else table.table).data_ptr(), rel_proj.data_ptr(),
                 depth_sample.data_ptr(), _ptr(view_weights), vw_shift, sim_p, pix_p, B, N, C,
                 G, D, h, w, hs, ws, cost.data_ptr(), _ptr(vw_out), _ptr(argmax), _ptr(sim),
                 _stream(cost)), "pmn_warp_correlate")
        if _TIMING is not None and _TIMING_ON:
            ev1.record()
            _TIMING.append((ev0, ev1, 4 * B * h * w * ((1 + N) * C + D + N + G * D),
                            f"C{C}_D{D}_{h}x{w}_N{N}_{'vw' if view_weights is not None else 'pixelwise'}"))
    return cost, (view_weights if view_weights is not None else vw_out), argmax, sim


def aggregate_regress(cost: torch.Tensor, depth_sample: torch.Tensor, xnorm: torch.Tensor, feature_weight_: torch.Tensor,
                      eval_offsets: torch.Tensor, table: np.ndarray, interval_scale: float, is_inverse: bool
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Adaptive spatial aggregation + softmax + regression -> (score [B,D,h,w], depth [B,h,w])."""
    for n, t in (("depth_sample", depth_sample), ("feature_weight", feature_weight_), ("eval_offsets", eval_offsets)):
        _dev(t, n)
    cost, xnorm = _dlast(cost, "cost"), _dlast(xnorm, "xnorm")
    B, D, h, w = cost.shape
    K = feature_weight_.shape[1]
    if tuple(depth_sample.shape) != (B, D, h, w) or tuple(xnorm.shape) != (B, D, h, w) or \
            tuple(feature_weight_.shape) != (B, K, h, w) or tuple(eval_offsets.shape) != (B, 2 * K, h, w):
        raise PmnError("aggregate_regress: inconsistent shapes")
    tab, tab_p = _host_i32(table, 2 * K, "table")
    score = torch.empty((B, D, h, w), dtype=torch.float32, device=cost.device)
    depth = torch.empty((B, h, w), dtype=torch.float32, device=cost.device)
    _note((cost, depth_sample, xnorm, feature_weight_, eval_offsets), (score, depth))
    with torch.cuda.device(cost.device):
        check(_lib.lib().pmn_aggregate_regress(cost.data_ptr(), depth_sample.data_ptr(), xnorm.data_ptr(),
                                               feature_weight_.data_ptr(), eval_offsets.data_ptr(), tab_p, K,
                                               float(interval_scale), 1 if is_inverse else 0, B, D, h, w,
                                               score.data_ptr(), depth.data_ptr(), _stream(cost)),
              "pmn_aggregate_regress")
    return score, depth


def confidence(score: torch.Tensor, H: int, W: int, want_index: bool = False):
    """Photometric confidence (reference models/net.py:288-299) -> ([B,H,W], depth_index [B,h,w] int32 or None)."""
    _dev(score, "score")
    B, D, h, w = score.shape
    conf = torch.empty((B, H, W), dtype=torch.float32, device=score.device)
    idx = torch.empty((B, h, w), dtype=torch.int32, device=score.device) if want_index else None
    with torch.cuda.device(score.device):
        check(_lib.lib().pmn_confidence(score.data_ptr(), B, D, h, w, H, W, conf.data_ptr(), _ptr(idx), _stream(score)),
              "pmn_confidence")
    return conf, idx


def relative_projection(src_projs: Sequence[torch.Tensor], ref_proj: torch.Tensor) -> torch.Tensor:
    """src_proj @ inverse(ref_proj) for every source view (reference models/module.py:148) -> [B,N,4,4]."""
    inv = torch.inverse(ref_proj)
    return torch.matmul(torch.stack(list(src_projs), dim=1), inv.unsqueeze(1)).contiguous()


def differentiable_warping(src_fea: torch.Tensor, src_proj: torch.Tensor, ref_proj: torch.Tensor,
                           depth_samples: torch.Tensor) -> torch.Tensor:
    """Drop-in for reference models/module.py:130-181 (inference): [B,C,Hs,Ws],[B,4,4],[B,4,4],[B,D,H,W] -> [B,C,D,H,W]."""
    src_fea = _dev(src_fea.contiguous(), "src_fea")
    depth_samples = _dev(depth_samples.contiguous(), "depth_samples")
    B, C, hs, ws = src_fea.shape
    _, D, h, w = depth_samples.shape
    proj = torch.matmul(src_proj, torch.inverse(ref_proj)).contiguous()
    _dev(proj, "proj")
    out = torch.empty((B, C, D, h, w), dtype=torch.float32, device=src_fea.device)
    with torch.cuda.device(src_fea.device):
        check(_lib.lib().pmn_differentiable_warping(src_fea.data_ptr(), proj.data_ptr(), depth_samples.data_ptr(), B, C,
                                                    D, h, w, hs, ws, out.data_ptr(), _stream(out)),
              "pmn_differentiable_warping")
    return out


def stage_projections(intrinsics: torch.Tensor, extrinsics: torch.Tensor, nstages: int = 3, scale0: float = 0.125
                      ) -> torch.Tensor:
    """pmn_stage_projections: intrinsics [B,V,3,3], extrinsics [B,V,4,4] -> relative projections [nstages,B,V-1,4,4]
    (stage index 0 = coarsest, scale0; reference models/net.py:221-232 + models/module.py:148)."""
    intrinsics = _dev(intrinsics.float().contiguous(), "intrinsics")
    extrinsics = _dev(extrinsics.float().contiguous(), "extrinsics")
    B, V = intrinsics.shape[:2]
    rel = torch.empty((nstages, B, V - 1, 4, 4), dtype=torch.float32, device=intrinsics.device)
    with torch.cuda.device(rel.device):
        check(_lib.lib().pmn_stage_projections(intrinsics.data_ptr(), extrinsics.data_ptr(), B, V, nstages, float(scale0),
                                               rel.data_ptr(), _stream(rel)), "pmn_stage_projections")
    return rel


def normalize_depth(depth: torch.Tensor, depth_min: torch.Tensor, depth_max: torch.Tensor) -> torch.Tensor:
    """pmn_normalize_depth: (depth - depth_min[b]) / (depth_max[b] - depth_min[b]) for depth [B, ...] (reference models/net.py:104-106),
    the bits of the torch expression; with it the forward launches nothing but this library's kernels (launch plans, plan.py)."""
    depth = _dev(depth.contiguous(), "depth")
    lo, hi = _dev(depth_min.float().contiguous(), "depth_min"), _dev(depth_max.float().contiguous(), "depth_max")
    B = depth.shape[0]
    if lo.numel() != B or hi.numel() != B:
        raise PmnError("normalize_depth: depth_min / depth_max must hold one value per batch element")
    out = torch.empty_like(depth)
    with torch.cuda.device(depth.device):
        check(_lib.lib().pmn_normalize_depth(depth.data_ptr(), lo.data_ptr(), hi.data_ptr(), B, depth.numel() // B, out.data_ptr(),
                                             _stream(out)), "pmn_normalize_depth")
    return out


def conv2d(x: torch.Tensor, weights: torch.Tensor, shift: torch.Tensor, cout: int, K: int, stride: int = 1, pad: int = 0,
           dil: int = 1, relu: bool = False, up: Optional[torch.Tensor] = None, in_nchw: bool = False,
           out_nchw: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pmn_conv2d: x [N,H,W,cin] (or [N,cin,H,W] with in_nchw) -> [N,Ho,Wo,cout] (or [N,cout,Ho,Wo] with out_nchw);
    ``weights`` / ``shift`` from params.pack_conv (device tensors); ``up`` [N,Ho/2,Wo/2,cout] is up-sampled x2 and added."""
    _dev(x, "x")
    _dev(weights, "weights")
    _dev(shift, "shift")
    if in_nchw:
        N, cin, H, W = x.shape
    else:
        N, H, W, cin = x.shape
    if tuple(weights.shape[:3]) != (K, K, cin) or shift.numel() != weights.shape[3]:
        raise PmnError("conv2d: packed weights do not match the input")
    Ho = (H + 2 * pad - dil * (K - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (K - 1) - 1) // stride + 1
    shape = (N, cout, Ho, Wo) if out_nchw else (N, Ho, Wo, cout)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        _dev(out, "out")
        if tuple(out.shape) != shape:
            raise PmnError("conv2d: bad `out` shape")
    up_h = up_w = 0
    if up is not None:
        _dev(up, "up")
        if tuple(up.shape) != (N, Ho // 2, Wo // 2, cout) or Ho % 2 or Wo % 2:
            raise PmnError("conv2d: `up` must be [N,Ho/2,Wo/2,cout]")
        up_h, up_w = up.shape[1], up.shape[2]
    _note((x, weights, shift, up), (out,))
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_conv2d(x.data_ptr(), weights.data_ptr(), shift.data_ptr(), _ptr(up), out.data_ptr(), N, H, W,
                                    cin, cout, K, stride, pad, dil, 1 if relu else 0, 1 if in_nchw else 0,
                                    1 if out_nchw else 0, up_h, up_w, _stream(x)), "pmn_conv2d")
    return out


def fpn_tail(x: torch.Tensor, up: torch.Tensor, w_in: torch.Tensor, b_in: torch.Tensor, w_out: torch.Tensor) -> torch.Tensor:
    """pmn_fpn_tail: output3(bilinear_x2(up) + inner2(x)) (reference models/net.py:64-67); x [N,H,W,16], up [N,H/2,W/2,64]
    -> [N,H,W,16]; weights in params.pack_conv layout."""
    for n_, t_ in (("x", x), ("up", up), ("w_in", w_in), ("b_in", b_in), ("w_out", w_out)):
        _dev(t_, n_)
    N, H, W, cin = x.shape
    cmid, cout = up.shape[3], w_out.shape[3]
    if tuple(up.shape) != (N, H // 2, W // 2, cmid) or tuple(w_in.shape) != (1, 1, cin, cmid) or \
            tuple(w_out.shape) != (1, 1, cmid, cout):
        raise PmnError("fpn_tail: inconsistent shapes")
    out = torch.empty((N, H, W, cout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_fpn_tail(x.data_ptr(), up.data_ptr(), w_in.data_ptr(), b_in.data_ptr(), w_out.data_ptr(),
                                      out.data_ptr(), N, H, W, cin, cmid, cout, _stream(x)), "pmn_fpn_tail")
    return out


MFMA_CONV_SHAPES = {(64, 64, 3, 1), (32, 32, 3, 1), (32, 64, 5, 2), (16, 32, 5, 2)}  # (cin, cout, K, stride)
MFMA_HEAD_SHAPES = {(64, 2), (32, 4), (16, 6)}  # (cin, dilation) of the planar offset-head form, cout <= 64


def conv2d_mfma(x: torch.Tensor, weights: torch.Tensor, shift: torch.Tensor, K: int, stride: int = 1, pad: int = 0,
                relu: bool = True) -> torch.Tensor:
    """pmn_conv2d_mfma (planar = 0): conv + folded-BN shift + ReLU as fp32 implicit GEMM on the matrix cores; x [N,H,W,cin]
    channels-last, weights from params.pack_conv_mfma ([K*K, cin/8, cout/32, 64, 4]) -> [N,Ho,Wo,cout]."""
    for n_, t_ in (("x", x), ("weights", weights), ("shift", shift)):
        _dev(t_, n_)
    N, H, W, cin = x.shape
    cout = shift.shape[0]
    if tuple(weights.shape) != (K * K, cin // 8, cout // 32, 64, 4):
        raise PmnError("conv2d_mfma: weights are not in pack_conv_mfma layout for this input")
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    out = torch.empty((N, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_conv2d_mfma(x.data_ptr(), weights.data_ptr(), shift.data_ptr(), out.data_ptr(), None, N, H, W,
                                         cin, cout, cout, K, stride, pad, 1, 1 if relu else 0, 0, _stream(x)),
              "pmn_conv2d_mfma")
    return out


def conv3x3_wino(x: torch.Tensor, weights: torch.Tensor, shift: torch.Tensor, relu: bool = True) -> torch.Tensor:
    """pmn_conv3x3_wino: 3x3 / stride 1 / padding 1 convolution with cin == cout in {16,32,64} + folded-BN shift + ReLU in
    Winograd F(2x2,3x3) form on the matrix cores; x [N,H,W,C] channels-last, weights from params.pack_conv_wino."""
    if not _lib.experimental():
        raise PmnError("conv3x3_wino: research build only (make -C patchmatchnet_amd/csrc EXPERIMENTAL=1, PMN_EXPERIMENTAL=1)")
    for n_, t_ in (("x", x), ("weights", weights), ("shift", shift)):
        _dev(t_, n_)
    N, H, W, C = x.shape
    if tuple(weights.shape) != (C // 16, 16, C // 16, 64, 4) or tuple(shift.shape) != (C,):
        raise PmnError("conv3x3_wino: weights are not in pack_conv_wino layout for this input")
    out = torch.empty((N, H, W, C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_conv3x3_wino(x.data_ptr(), weights.data_ptr(), shift.data_ptr(), out.data_ptr(), N, H, W, C,
                                          1 if relu else 0, _stream(x)), "pmn_conv3x3_wino")
    return out


def conv5x5s2_wino(x: torch.Tensor, weights: torch.Tensor, shift: torch.Tensor, relu: bool = True) -> torch.Tensor:
    """pmn_conv5x5s2_wino: 5x5 / stride 2 / padding 2 convolution + folded-BN shift + ReLU in phase-decomposed Winograd form on
    the matrix cores; x [N,H,W,cin] channels-last, weights from params.pack_conv5x5s2_wino -> [N,(H-1)//2+1,(W-1)//2+1,cout]."""
    if not _lib.experimental():
        raise PmnError("conv5x5s2_wino: research build only (make -C patchmatchnet_amd/csrc EXPERIMENTAL=1, PMN_EXPERIMENTAL=1)")
    for n_, t_ in (("x", x), ("weights", weights), ("shift", shift)):
        _dev(t_, n_)
    N, H, W, cin = x.shape
    cout = shift.shape[0]
    if tuple(weights.shape) != (cin // 8, 49, cout // 16, 64, 2):
        raise PmnError("conv5x5s2_wino: weights are not in pack_conv5x5s2_wino layout for this input")
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, cout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_conv5x5s2_wino(x.data_ptr(), weights.data_ptr(), shift.data_ptr(), out.data_ptr(), N, H, W, cin,
                                            cout, 1 if relu else 0, _stream(x)), "pmn_conv5x5s2_wino")
    return out


F16S_SHAPES = {(3, 1, 16, 16), (3, 1, 32, 32), (3, 1, 64, 64), (5, 2, 8, 16), (5, 2, 16, 32), (5, 2, 32, 64)}  # (k, stride, cin, cout)


def conv2d_f16s(x: torch.Tensor, weights: torch.Tensor, shift: torch.Tensor, k: int, stride: int, relu: bool = True) -> torch.Tensor:
    """pmn_conv2d_f16s: convolution (padding k // 2) + folded-BN shift + ReLU on the FP16 matrix cores with split (hi + lo/2048)
    operands -- fp32-convolution accuracy; x [N,H,W,cin] channels-last float32, weights float16 from params.pack_conv_f16s ->
    [N,(H-1)//stride+1,(W-1)//stride+1,cout] float32."""
    _dev(x, "x")
    _f16_domain_probe(x)
    _dev(shift, "shift")
    _dev_as(weights, "conv2d_f16s: weights (params.pack_conv_f16s)", torch.float16)
    N, H, W, cin = x.shape
    cout = shift.shape[0]
    if (k, stride, cin, cout) not in F16S_SHAPES:
        raise PmnError(f"conv2d_f16s: unsupported layer (k={k}, stride={stride}, cin={cin}, cout={cout})")
    from . import params as _params
    cc = _params.f16s_chunk(cin, k)
    if tuple(weights.shape) != (cin // cc, (k * k * (cc // 8) + 3) // 4, cout // 16, 2, 64, 8):
        raise PmnError("conv2d_f16s: weights are not in pack_conv_f16s layout for this input")
    out = torch.empty((N, (H - 1) // stride + 1, (W - 1) // stride + 1, cout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_conv2d_f16s(x.data_ptr(), weights.data_ptr(), shift.data_ptr(), out.data_ptr(), N, H, W, cin, cout, k,
                                         stride, 1 if relu else 0, _stream(x)), "pmn_conv2d_f16s")
    return out


def conv2d_f16s_pair(x: torch.Tensor, weights_a: torch.Tensor, shift_a: torch.Tensor, weights_b: torch.Tensor, shift_b: torch.Tensor,
                     relu: bool = True) -> torch.Tensor:
    """pmn_conv2d_f16s_pair: two consecutive 3x3 / stride-1 / 16 -> 16 ConvBnReLU layers in one launch (FeatureNet conv3 + conv4), the
    intermediate map kept in LDS; x [N,H,W,16] channels-last float32, (weights, shift) pairs from params.pack_conv_f16s.  Bit-identical
    to conv2d_f16s(conv2d_f16s(x, a...), b...)."""
    _dev(x, "x")
    _f16_domain_probe(x)
    N, H, W, C = x.shape
    for w_, s_ in ((weights_a, shift_a), (weights_b, shift_b)):
        _dev(s_, "shift")
        _dev_as(w_, "conv2d_f16s_pair: weights", torch.float16)
        if tuple(w_.shape) != (1, 5, 1, 2, 64, 8) or s_.numel() != 16:
            raise PmnError("conv2d_f16s_pair: weights must be params.pack_conv_f16s of a (3, 1, 16, 16) layer")
    if C != 16:
        raise PmnError("conv2d_f16s_pair: 16-channel layers only")
    out = torch.empty((N, H, W, 16), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_conv2d_f16s_pair(x.data_ptr(), weights_a.data_ptr(), shift_a.data_ptr(), weights_b.data_ptr(), shift_b.data_ptr(),
                                              out.data_ptr(), N, H, W, 16, 1 if relu else 0, _stream(x)), "pmn_conv2d_f16s_pair")
    return out


def pointwise_split_mfma(x: torch.Tensor, weights: torch.Tensor, shift: torch.Tensor, cout: int, ca: int):
    """pmn_conv2d_mfma, 1x1 form: out = x @ W + shift on the matrix cores with the output channels split between two
    channels-last tensors (the 1/8-resolution level of the folded FPN head); x [N,H,W,64], weights from
    params.pack_conv_mfma of the [cout,64,1,1] filter -> ([N,H,W,ca], [N,H,W,cout-ca])."""
    for n_, t_ in (("x", x), ("weights", weights), ("shift", shift)):
        _dev(t_, n_)
    N, H, W, cin = x.shape
    coutp = shift.shape[0]
    if tuple(weights.shape) != (1, cin // 8, coutp // 32, 64, 4) or not 0 < ca < cout <= coutp:
        raise PmnError("pointwise_split_mfma: weights are not in pack_conv_mfma layout for this input")
    out_a = torch.empty((N, H, W, ca), dtype=torch.float32, device=x.device)
    out_b = torch.empty((N, H, W, cout - ca), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_conv2d_mfma(x.data_ptr(), weights.data_ptr(), shift.data_ptr(), out_a.data_ptr(), out_b.data_ptr(),
                                         N, H, W, cin, cout, ca, 1, 1, 0, 1, 0, 0, _stream(x)), "pmn_conv2d_mfma")
    return out_a, out_b


def offset_heads_mfma(x: torch.Tensor, weights: torch.Tensor, shift: torch.Tensor, cout: int, ca: int, dil: int):
    """pmn_conv2d_mfma (planar = 1): the offset heads of one stage (propa_conv rows first, then eval_conv; reference
    models/patchmatch.py:288-311) as one dilated 3x3 convolution with bias; x [N,H,W,cin] channels-last, weights from
    params.pack_conv_mfma of the row-concatenated filters -> ([N,ca,H,W], [N,cout-ca,H,W] or None) planar."""
    for n_, t_ in (("x", x), ("weights", weights), ("shift", shift)):
        _dev(t_, n_)
    N, H, W, cin = x.shape
    coutp = shift.shape[0]
    if tuple(weights.shape) != (9, cin // 8, coutp // 32, 64, 4) or not 0 < ca <= cout <= coutp:
        raise PmnError("offset_heads_mfma: weights are not in pack_conv_mfma layout for this input")
    out_a = torch.empty((N, ca, H, W), dtype=torch.float32, device=x.device)
    out_b = torch.empty((N, cout - ca, H, W), dtype=torch.float32, device=x.device) if ca < cout else None
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_conv2d_mfma(x.data_ptr(), weights.data_ptr(), shift.data_ptr(), out_a.data_ptr(), _ptr(out_b), N,
                                         H, W, cin, cout, ca, 3, 1, dil, dil, 0, 1, _stream(x)), "pmn_conv2d_mfma")
    return out_a, out_b


F16S_HEAD_SHAPES = {(64, 2), (32, 4), (16, 6)}  # (input channels, dilation) of the reference's stages 3, 2, 1


def offset_heads_f16s(x: torch.Tensor, weights: torch.Tensor, shift: torch.Tensor, cout: int, ca: int, dil: int):
    """pmn_offset_heads_f16s: the offset heads of one stage (propa_conv rows first, then eval_conv; reference
    models/patchmatch.py:288-311) as one dilated 3x3 convolution with bias on the fp16 matrix cores (split operands);
    x [N,H,W,cin] channels-last, weights / shift from params.pack_offset_heads_f16s -> ([N,ca,H,W], [N,cout-ca,H,W] or None) planar."""
    _dev(x, "x")
    _f16_domain_probe(x)
    _dev(shift, "shift")
    N, H, W, cin = x.shape
    coutp = shift.shape[0]
    _dev_as(weights, "offset_heads_f16s: weights", torch.float16)
    if tuple(weights.shape) != (cin // 16, (9 * 2 + 3) // 4, coutp // 16, 2, 64, 8) or not 0 < ca <= cout <= coutp \
            or coutp != (cout + 15) // 16 * 16:
        raise PmnError("offset_heads_f16s: weights are not in pack_offset_heads_f16s layout for this input")
    out_a = torch.empty((N, ca, H, W), dtype=torch.float32, device=x.device)
    out_b = torch.empty((N, cout - ca, H, W), dtype=torch.float32, device=x.device) if ca < cout else None
    _note((x, weights, shift), (out_a, out_b))
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_offset_heads_f16s(x.data_ptr(), weights.data_ptr(), shift.data_ptr(), out_a.data_ptr(), _ptr(out_b), N,
                                               H, W, cin, cout, ca, dil, _stream(x)), "pmn_offset_heads_f16s")
    return out_a, out_b


def fpn_level(x: torch.Tensor, u: Optional[torch.Tensor], w: torch.Tensor, b: torch.Tensor, ca: int):
    """pmn_fpn_level: one level of the folded FPN head, out = bilinear_x2(u) + b + x @ w (reference models/net.py:57-67 with
    the 1x1 convolutions composed, params.fold_fpn).  x [N,H,W,cin], u [N,H/2,W/2,cout] or None, w [cin,cout], b [cout]
    -> (out_a [N,H,W,ca], out_b [N,H,W,cout-ca] or None)."""
    for n_, t_ in (("x", x), ("w", w), ("b", b)):
        _dev(t_, n_)
    N, H, W, cin = x.shape
    cout = w.shape[1]
    if tuple(w.shape) != (cin, cout) or tuple(b.shape) != (cout,) or not 0 < ca <= cout:
        raise PmnError("fpn_level: inconsistent shapes")
    if u is not None:
        _dev(u, "u")
        if tuple(u.shape) != (N, H // 2, W // 2, cout) or H % 2 or W % 2:
            raise PmnError("fpn_level: `u` must be [N,H/2,W/2,cout]")
    out_a = torch.empty((N, H, W, ca), dtype=torch.float32, device=x.device)
    out_b = torch.empty((N, H, W, cout - ca), dtype=torch.float32, device=x.device) if ca < cout else None
    _note((x, u, w, b), (out_a, out_b))
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_fpn_level(x.data_ptr(), _ptr(u), w.data_ptr(), b.data_ptr(), out_a.data_ptr(), _ptr(out_b),
                                       N, H, W, cin, cout, ca, _stream(x)), "pmn_fpn_level")
    return out_a, out_b


def refine_front(img: torch.Tensor, t2: torch.Tensor, w0: torch.Tensor, s0: torch.Tensor, wd: torch.Tensor,
                 sd: torch.Tensor) -> torch.Tensor:
    """pmn_refine_front: cat(relu(bn(deconv(t2))), conv0(img)) of Refinement (reference models/net.py:110-117); img [B,3,H,W],
    t2 [B,H/2,W/2,8] channels-last -> [B,H,W,16]."""
    for n_, t_ in (("img", img), ("t2", t2), ("w0", w0), ("s0", s0), ("wd", wd), ("sd", sd)):
        _dev(t_, n_)
    B, c, H, W = img.shape
    if c != 3 or H % 2 or W % 2 or tuple(t2.shape) != (B, H // 2, W // 2, 8) or tuple(w0.shape) != (3, 3, 3, 8) or \
            tuple(wd.shape) != (3, 3, 8, 8):
        raise PmnError("refine_front: inconsistent shapes")
    out = torch.empty((B, H, W, 16), dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        check(_lib.lib().pmn_refine_front(img.data_ptr(), t2.data_ptr(), w0.data_ptr(), s0.data_ptr(), wd.data_ptr(),
                                          sd.data_ptr(), out.data_ptr(), B, H, W, _stream(img)), "pmn_refine_front")
    return out


def refine_tail(x16: torch.Tensor, w3: torch.Tensor, s3: torch.Tensor, wr: torch.Tensor, dnorm: torch.Tensor,
                depth_min: torch.Tensor, depth_max: torch.Tensor) -> torch.Tensor:
    """pmn_refine_tail: (nearest_x2(dnorm) + res(conv3(x16))) * (depth_max - depth_min) + depth_min (reference
    models/net.py:117-122); x16 [B,H,W,16], dnorm [B,1,H/2,W/2], depth_min / depth_max [B] -> [B,1,H,W]."""
    for n_, t_ in (("x16", x16), ("w3", w3), ("s3", s3), ("wr", wr), ("dnorm", dnorm), ("depth_min", depth_min),
                   ("depth_max", depth_max)):
        _dev(t_, n_)
    B, H, W, c = x16.shape
    if c != 16 or H % 2 or W % 2 or tuple(dnorm.shape) != (B, 1, H // 2, W // 2) or tuple(w3.shape) != (2, 3, 3, 16, 4) or \
            tuple(wr.shape) != (3, 3, 8) or depth_min.numel() != B or depth_max.numel() != B:
        raise PmnError("refine_tail: inconsistent shapes")
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=x16.device)
    with torch.cuda.device(x16.device):
        check(_lib.lib().pmn_refine_tail(x16.data_ptr(), w3.data_ptr(), s3.data_ptr(), wr.data_ptr(), dnorm.data_ptr(),
                                         depth_min.data_ptr(), depth_max.data_ptr(), out.data_ptr(), B, H, W, _stream(x16)),
              "pmn_refine_tail")
    return out


def refine_fused(img: torch.Tensor, t2: torch.Tensor, w0: torch.Tensor, s0: torch.Tensor, wd: torch.Tensor, sd: torch.Tensor,
                 w3a: torch.Tensor, s3: torch.Tensor, wr: torch.Tensor, dnorm: torch.Tensor, depth_min: torch.Tensor,
                 depth_max: torch.Tensor) -> torch.Tensor:
    """pmn_refine_fused: refine_front + refine_tail in one launch, conv3 on the fp16 matrix cores with split operands (reference
    models/net.py:110-122); img [B,3,H,W], t2 [B,H/2,W/2,8], w3a = params.pack_refine_conv3_f16s (float16 [5,2,64,8]), dnorm
    [B,1,H/2,W/2], depth_min / depth_max [B] -> [B,1,H,W]."""
    for n_, t_ in (("img", img), ("t2", t2), ("w0", w0), ("s0", s0), ("wd", wd), ("sd", sd), ("s3", s3), ("wr", wr), ("dnorm", dnorm),
                   ("depth_min", depth_min), ("depth_max", depth_max)):
        _dev(t_, n_)
    if tuple(_dev_as(w3a, "refine_fused: w3a", torch.float16).shape) != (5, 2, 64, 8):
        raise PmnError("refine_fused: w3a must be the float16 [5,2,64,8] tensor of params.pack_refine_conv3_f16s")
    B, c, H, W = img.shape
    if c != 3 or H % 2 or W % 2 or tuple(t2.shape) != (B, H // 2, W // 2, 8) or tuple(dnorm.shape) != (B, 1, H // 2, W // 2) or \
            tuple(w0.shape) != (3, 3, 3, 8) or tuple(wd.shape) != (3, 3, 8, 8) or tuple(wr.shape) != (3, 3, 8) or s3.numel() != 8 or \
            depth_min.numel() != B or depth_max.numel() != B:
        raise PmnError("refine_fused: inconsistent shapes")
    _f16_domain_probe(img, t2)
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        check(_lib.lib().pmn_refine_fused(img.data_ptr(), t2.data_ptr(), w0.data_ptr(), s0.data_ptr(), wd.data_ptr(), sd.data_ptr(),
                                          w3a.data_ptr(), s3.data_ptr(), wr.data_ptr(), dnorm.data_ptr(), depth_min.data_ptr(),
                                          depth_max.data_ptr(), out.data_ptr(), B, H, W, _stream(img)), "pmn_refine_fused")
    return out


def deconv3x3s2(x: torch.Tensor, weights: torch.Tensor, shift: torch.Tensor, relu: bool = True) -> torch.Tensor:
    """pmn_deconv3x3s2: ConvTranspose2d(k3,s2,p1,op1) + folded BN + ReLU; x [N,Hi,Wi,8] -> [N,2Hi,2Wi,8]."""
    _dev(x, "x")
    _dev(weights, "weights")
    _dev(shift, "shift")
    N, Hi, Wi, cin = x.shape
    cout = weights.shape[3]
    out = torch.empty((N, 2 * Hi, 2 * Wi, cout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().pmn_deconv3x3s2(x.data_ptr(), weights.data_ptr(), shift.data_ptr(), out.data_ptr(), N, Hi, Wi, cin,
                                         cout, 1 if relu else 0, _stream(x)), "pmn_deconv3x3s2")
    return out


def stem(img: torch.Tensor, w0: torch.Tensor, s0: torch.Tensor, w1: torch.Tensor, s1: torch.Tensor,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pmn_stem: FeatureNet conv0 + conv1 fused; img [N,3,H,W] -> [N,H,W,8] (optionally into ``out``)."""
    for n_, t_ in (("img", img), ("w0", w0), ("s0", s0), ("w1", w1), ("s1", s1)):
        _dev(t_, n_)
    N, c, H, W = img.shape
    if c != 3 or tuple(w0.shape) != (3, 3, 3, 8) or tuple(w1.shape) != (3, 3, 8, 8):
        raise PmnError("stem: expects a 3-channel image and 3->8->8 weights")
    if out is None:
        out = torch.empty((N, H, W, 8), dtype=torch.float32, device=img.device)
    else:
        _dev(out, "out")
        if tuple(out.shape) != (N, H, W, 8):
            raise PmnError("stem: bad `out` shape")
    with torch.cuda.device(img.device):
        check(_lib.lib().pmn_stem(img.data_ptr(), w0.data_ptr(), s0.data_ptr(), w1.data_ptr(), s1.data_ptr(), out.data_ptr(),
                                  N, H, W, _stream(img)), "pmn_stem")
    return out


def stem_f16s(img: torch.Tensor, w0: torch.Tensor, s0: torch.Tensor, w1a: torch.Tensor, s1: torch.Tensor,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pmn_stem_f16s: FeatureNet conv0 (fp32 VALU) + conv1 (fp16 matrix cores, split operands) fused; img [N,3,H,W] -> [N,H,W,8]
    (optionally into ``out``); w1a = params.pack_stem_conv1_f16s (float16 [3,2,64,8])."""
    for n_, t_ in (("img", img), ("w0", w0), ("s0", s0), ("s1", s1)):
        _dev(t_, n_)
    if tuple(_dev_as(w1a, "stem_f16s: w1a", torch.float16).shape) != (3, 2, 64, 8):
        raise PmnError("stem_f16s: w1a must be the float16 [3,2,64,8] tensor of params.pack_stem_conv1_f16s")
    N, c, H, W = img.shape
    if c != 3 or tuple(w0.shape) != (3, 3, 3, 8):
        raise PmnError("stem_f16s: expects a 3-channel image and 3->8 conv0 weights")
    _f16_domain_probe(img)
    if out is None:
        out = torch.empty((N, H, W, 8), dtype=torch.float32, device=img.device)
    else:
        _dev(out, "out")
        if tuple(out.shape) != (N, H, W, 8):
            raise PmnError("stem_f16s: bad `out` shape")
    with torch.cuda.device(img.device):
        check(_lib.lib().pmn_stem_f16s(img.data_ptr(), w0.data_ptr(), s0.data_ptr(), w1a.data_ptr(), s1.data_ptr(), out.data_ptr(),
                                       N, H, W, _stream(img)), "pmn_stem_f16s")
    return out


def stem_f16s_views(images: "SourceTable", w0: torch.Tensor, s0: torch.Tensor, w1a: torch.Tensor, s1: torch.Tensor) -> torch.Tensor:
    """pmn_stem_f16s_views: the fused stem over ``views`` separately allocated [B,3,H,W] images found through a device table of
    addresses (``images``: a SourceTable with shape (views, B, 3, H, W)) -> [views*B,H,W,8] view-major.  A captured launch reads
    whatever the table holds at replay time (graph.GraphedForward(inputs_in_place=True))."""
    for n_, t_ in (("w0", w0), ("s0", s0), ("s1", s1)):
        _dev(t_, n_)
    if not isinstance(images, SourceTable) or len(images.shape) != 5 or images.shape[2] != 3:
        raise PmnError("stem_f16s_views: a SourceTable of shape (views, B, 3, H, W)")
    if tuple(_dev_as(w1a, "stem_f16s_views: w1a", torch.float16).shape) != (3, 2, 64, 8) or tuple(w0.shape) != (3, 3, 3, 8):
        raise PmnError("stem_f16s_views: 3->8 conv0 weights and the float16 [3,2,64,8] tensor of params.pack_stem_conv1_f16s")
    V, B, _, H, W = images.shape
    out = torch.empty((V * B, H, W, 8), dtype=torch.float32, device=images.device)
    with torch.cuda.device(images.device):
        check(_lib.lib().pmn_stem_f16s_views(images.table.data_ptr(), V, w0.data_ptr(), s0.data_ptr(), w1a.data_ptr(), s1.data_ptr(),
                                             out.data_ptr(), B, H, W, _stream(out)), "pmn_stem_f16s_views")
    return out


def _stem_conv2_packs(what: str, w0: torch.Tensor, s0: torch.Tensor, w1a: torch.Tensor, s1: torch.Tensor, w2b: torch.Tensor,
                      s2: torch.Tensor) -> None:
    for n_, t_ in (("w0", w0), ("s0", s0), ("s1", s1), ("s2", s2)):
        _dev(t_, n_)
    if tuple(_dev_as(w1a, what + ": w1a", torch.float16).shape) != (3, 2, 64, 8) or tuple(w0.shape) != (3, 3, 3, 8):
        raise PmnError(what + ": 3->8 conv0 weights and the float16 [3,2,64,8] tensor of params.pack_stem_conv1_f16s")
    if tuple(_dev_as(w2b, what + ": w2b", torch.float16).shape) != (1, 7, 1, 2, 64, 8) or s2.numel() != 16:
        raise PmnError(what + ": w2b / s2 must be params.pack_conv_f16s of a (5, 2, 8, 16) layer")


def stem_conv2_f16s(img: torch.Tensor, w0: torch.Tensor, s0: torch.Tensor, w1a: torch.Tensor, s1: torch.Tensor, w2b: torch.Tensor,
                    s2: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pmn_stem_conv2_f16s: FeatureNet conv0 + conv1 + conv2 in one launch, conv1's full-resolution map in LDS; img [N,3,H,W] ->
    [N,Ho,Wo,16] channels-last (optionally into ``out``), the bits of ``stem_f16s`` followed by ``conv2d_f16s(.., 5, 2, relu=True)``."""
    _dev(img, "img")
    _stem_conv2_packs("stem_conv2_f16s", w0, s0, w1a, s1, w2b, s2)
    N, c, H, W = img.shape
    if c != 3:
        raise PmnError("stem_conv2_f16s: expects a 3-channel image")
    _f16_domain_probe(img)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, 16), dtype=torch.float32, device=img.device)
    else:
        _dev(out, "out")
        if tuple(out.shape) != (N, Ho, Wo, 16):
            raise PmnError("stem_conv2_f16s: bad `out` shape")
    with torch.cuda.device(img.device):
        check(_lib.lib().pmn_stem_conv2_f16s(img.data_ptr(), w0.data_ptr(), s0.data_ptr(), w1a.data_ptr(), s1.data_ptr(), w2b.data_ptr(),
                                             s2.data_ptr(), out.data_ptr(), N, H, W, _stream(img)), "pmn_stem_conv2_f16s")
    return out


def stem_conv2_f16s_views(images: "SourceTable", w0: torch.Tensor, s0: torch.Tensor, w1a: torch.Tensor, s1: torch.Tensor,
                          w2b: torch.Tensor, s2: torch.Tensor) -> torch.Tensor:
    """pmn_stem_conv2_f16s_views: ``stem_conv2_f16s`` over ``views`` separately allocated [B,3,H,W] images found through a device
    table of addresses (``images``: a SourceTable with shape (views, B, 3, H, W)) -> [views*B,Ho,Wo,16] view-major."""
    if not isinstance(images, SourceTable) or len(images.shape) != 5 or images.shape[2] != 3:
        raise PmnError("stem_conv2_f16s_views: a SourceTable of shape (views, B, 3, H, W)")
    _stem_conv2_packs("stem_conv2_f16s_views", w0, s0, w1a, s1, w2b, s2)
    V, B, _, H, W = images.shape
    out = torch.empty((V * B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 16), dtype=torch.float32, device=images.device)
    with torch.cuda.device(images.device):
        check(_lib.lib().pmn_stem_conv2_f16s_views(images.table.data_ptr(), V, w0.data_ptr(), s0.data_ptr(), w1a.data_ptr(),
                                                   s1.data_ptr(), w2b.data_ptr(), s2.data_ptr(), out.data_ptr(), B, H, W, _stream(out)),
              "pmn_stem_conv2_f16s_views")
    return out


def fuse_view(maps: torch.Tensor, ref_slot: int, src_slots: Sequence[int], mats: torch.Tensor, geo_pixel_thres: float,
              geo_depth_thres: float, geo_mask_thres: int, photo_thres: float, want_depth_avg: bool = False,
              want_geo_sum: bool = False, sizes: Optional[Sequence[Tuple[int, int]]] = None):
    """pmn_fuse_view: consistency filtering + fusion of ONE reference view (reference eval.py:86-190, :207-281).

    maps [V,2,H,W] (depth, confidence of every view of the scan, e.g. the all-gathered buffer), or -- views of different sizes
    -- [V,F] flat slots with ``sizes[v] = (h_v, w_v)``: slot v holds depth [h_v,w_v] then confidence [h_v,w_v] packed at its
    start (F >= 2*h*w of the largest view).  mats = fusion.camera_block(...) (device float32).  Returns (masks [3,H,W] uint8 =
    photo / geo / final, xyz [H,W,3] float32 world points, depth_avg [H,W] float64 or None, geo_sum [H,W] int32 or None), H x W
    = the reference view's size."""
    masks, xyz, davg, gsum, _ = _fuse_view(maps, ref_slot, src_slots, mats, geo_pixel_thres, geo_depth_thres, geo_mask_thres,
                                           photo_thres, want_depth_avg, want_geo_sum, sizes, None)
    return masks, xyz, davg, gsum


def fuse_view_merged(maps: torch.Tensor, ref_slot: int, src_slots: Sequence[int], mats: torch.Tensor, geo_pixel_thres: float,
                     geo_depth_thres: float, geo_mask_thres: int, photo_thres: float, claimed: torch.Tensor,
                     sizes: Optional[Sequence[Tuple[int, int]]] = None):
    """pmn_fuse_view_merged: ``fuse_view`` that writes each surface point once.  ``claimed``: device uint8
    [V,S], contiguous, S >= h*w of the largest view -- slot v = view v's map at its own size, 1 = covered by a point of a view fused
    earlier; zero it before a scan's first view and fuse the scan's views on one stream.  Returns (masks [3,H,W] and xyz [H,W,3]:
    ``fuse_view``'s, bit for bit; emit [H,W] uint8 = final && !claimed[ref_slot]: the pixels whose points belong in the file).
    The launch sets claimed[s] for the source views s that agreed with a final pixel; ``ref_slot`` must not be in ``src_slots``."""
    if not isinstance(claimed, torch.Tensor) or claimed.dtype != torch.uint8 or claimed.dim() != 2 or not claimed.is_contiguous():
        raise PmnError("fuse_view_merged: claimed must be a contiguous uint8 tensor [V,S], one slot per map slot")
    if not isinstance(maps, torch.Tensor) or claimed.device != maps.device:
        raise PmnError("fuse_view_merged: claimed must be on the maps' device (no CPU fallback)")
    if ref_slot in src_slots:
        raise PmnError("fuse_view_merged: the reference slot is in its own source list")
    masks, xyz, _, _, emit = _fuse_view(maps, ref_slot, src_slots, mats, geo_pixel_thres, geo_depth_thres, geo_mask_thres,
                                        photo_thres, False, False, sizes, claimed)
    return masks, xyz, emit


def _fuse_view(maps, ref_slot, src_slots, mats, geo_pixel_thres, geo_depth_thres, geo_mask_thres, photo_thres, want_depth_avg,
               want_geo_sum, sizes, claimed):
    """The checks and the call of ``fuse_view`` (claimed None) and ``fuse_view_merged``."""
    _dev(maps, "maps")
    _dev(mats, "mats")
    if sizes is None:
        if maps.dim() != 4 or maps.shape[1] != 2:
            raise PmnError("fuse_view: maps must be [V,2,H,W] (or [V,F] flat slots with sizes=)")
        V, _, H, W = maps.shape
        stride = 2 * H * W
        sizes = [(H, W)] * V
    else:
        if maps.dim() != 2 or len(sizes) != maps.shape[0]:
            raise PmnError("fuse_view: with sizes= maps must be [V,F] flat slots and sizes must have V entries")
        V, stride = maps.shape
        if any(h < 1 or w < 1 or 2 * h * w > stride for h, w in sizes):
            raise PmnError("fuse_view: a view's maps do not fit its slot")
    n = len(src_slots)
    if n > _lib.MAX_FUSE_SRC:
        raise PmnError(f"fuse_view: at most {_lib.MAX_FUSE_SRC} source views per reference view")
    if not 0 <= ref_slot < V or any(not 0 <= s < V for s in src_slots):
        raise PmnError("fuse_view: slot out of range")
    if mats.numel() != 48 + 64 * n:
        raise PmnError("fuse_view: mats must hold 48 + 64 * n_src floats (fusion.camera_block)")
    if claimed is not None and (claimed.shape[0] != V or any(h * w > claimed.shape[1] for h, w in sizes)):
        raise PmnError("fuse_view_merged: claimed must have one slot per map slot, each with room for the largest view's h*w bytes")
    H, W = sizes[ref_slot]
    slots, slots_p = _host_i32(np.asarray(list(src_slots) if n else [0], np.int32), max(n, 1), "src_slots")
    hw, hw_p = _host_i32(np.asarray([x for s in src_slots for x in sizes[s]] if n else [0, 0], np.int32), max(2 * n, 2), "src_hw")
    masks = torch.empty((3, H, W), dtype=torch.uint8, device=maps.device)
    xyz = torch.empty((H, W, 3), dtype=torch.float32, device=maps.device)
    davg = torch.empty((H, W), dtype=torch.float64, device=maps.device) if want_depth_avg else None
    gsum = torch.empty((H, W), dtype=torch.int32, device=maps.device) if want_geo_sum else None
    emit = None
    with torch.cuda.device(maps.device):
        if claimed is None:
            check(_lib.lib().pmn_fuse_view(maps.data_ptr(), int(stride), int(ref_slot), slots_p, hw_p, n, mats.data_ptr(), H, W,
                                           float(geo_pixel_thres), float(geo_depth_thres), int(geo_mask_thres), float(photo_thres),
                                           masks.data_ptr(), xyz.data_ptr(), _ptr(davg), _ptr(gsum), _stream(maps)),
                  "pmn_fuse_view")
        else:
            emit = torch.empty((H, W), dtype=torch.uint8, device=maps.device)
            check(_lib.lib().pmn_fuse_view_merged(maps.data_ptr(), int(stride), int(ref_slot), slots_p, hw_p, n, mats.data_ptr(), H, W,
                                                  float(geo_pixel_thres), float(geo_depth_thres), int(geo_mask_thres),
                                                  float(photo_thres), masks.data_ptr(), xyz.data_ptr(), _ptr(davg), _ptr(gsum),
                                                  claimed.data_ptr(), int(claimed.shape[1]), emit.data_ptr(), _stream(maps)),
                  "pmn_fuse_view_merged")
    del slots, hw
    return masks, xyz, davg, gsum, emit


def depth_normals(depth: torch.Tensor, intrinsics, radius: int = 2, rel_thres: float = 0.01) -> torch.Tensor:
    """pmn_depth_normals: camera-frame surface normals of depth maps, unit length and facing the camera, zero
    where there is no valid depth or no plane to fit.  depth [H,W] with intrinsics [3,3] -> [3,H,W] (planar: the body of COLMAP's
    normal-map .bin); depth [B,H,W] with intrinsics [B,3,3] -> [B,3,H,W], one launch per map.  ``intrinsics`` (numpy or tensor, at
    the MAP's size) is read on the host; ``radius`` 1..3 is the window radius, ``rel_thres`` the relative depth difference up to which
    a neighbour counts as the same surface (--geo_depth_thres's test)."""
    _dev(depth, "depth")
    if depth.dim() not in (2, 3) or depth.numel() == 0:
        raise PmnError("depth_normals: depth must be [H,W] or [B,H,W], H, W >= 1")
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= 3:
        raise PmnError("depth_normals: radius must be 1, 2 or 3")
    with np.errstate(over="ignore"):
        rel_thres = float(np.float32(rel_thres))  # the kernel's value: 1e-60 is 0 there, 1e60 is inf
    if not (np.isfinite(rel_thres) and rel_thres > 0.0):
        raise PmnError("depth_normals: rel_thres must be a positive finite float32")
    K = np.ascontiguousarray((intrinsics.detach().cpu().numpy() if isinstance(intrinsics, torch.Tensor) else np.asarray(intrinsics)),
                             np.float32)
    batched = depth.dim() == 3
    B = depth.shape[0] if batched else 1
    if tuple(K.shape) != ((B, 3, 3) if batched else (3, 3)):
        raise PmnError("depth_normals: intrinsics must be [3,3] for a [H,W] map, [B,3,3] for [B,H,W] maps")
    if not np.isfinite(K).all():
        raise PmnError("depth_normals: intrinsics must be finite")
    K = K.reshape(B, 9)
    H, W = depth.shape[-2:]
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=depth.device)
    with torch.cuda.device(depth.device):
        for b in range(B):
            k, k_p = _host_f32(K[b], 9, "intrinsics")
            check(_lib.lib().pmn_depth_normals((depth[b] if batched else depth).data_ptr(), H, W, k_p, int(radius), rel_thres,
                                               out[b].data_ptr(), _stream(depth)), "pmn_depth_normals")
            del k
    return out if batched else out[0]



def _colour_planes(tsdf, rgb, cweight, what, layout):
    """rgb and cweight come as a pair, on the device and in the shape of tsdf; ``layout`` words the shape rule for the message."""
    if (rgb is None) != (cweight is None):
        raise PmnError(f"{what}: rgb and cweight come together or not at all")
    if rgb is not None:
        _dev(rgb, "rgb")
        _dev(cweight, "cweight")
        if tuple(rgb.shape) != (3,) + tuple(tsdf.shape) or cweight.shape != tsdf.shape or rgb.device != tsdf.device or \
                cweight.device != tsdf.device:
            raise PmnError(f"{what}: {layout}")


def _volume_planes(tsdf, weight, rgb, cweight, what):
    _dev(tsdf, "tsdf")
    _dev(weight, "weight")
    if tsdf.dim() != 3 or tsdf.numel() == 0 or weight.shape != tsdf.shape or weight.device != tsdf.device:
        raise PmnError(f"{what}: tsdf and weight must be [nz,ny,nx] planes of one volume on one device")
    _colour_planes(tsdf, rgb, cweight, what, "rgb must be [3,nz,ny,nx] and cweight [nz,ny,nx] on the volume's device")
    nz, ny, nx = tsdf.shape
    if nz > 65535 or tsdf.numel() > 2 ** 31 - 1:
        raise PmnError(f"{what}: a volume holds at most 2^31 - 1 samples and 65535 planes")
    return _host_i32(np.asarray([nx, ny, nz]), 3, "dims")


def _positive_f32(v, what):
    with np.errstate(over="ignore"):
        v = float(np.float32(v))
    if not (np.isfinite(v) and v > 0.0):
        raise PmnError(f"{what} must be a positive finite float32")
    return v


def _placement(origin, voxel, trunc, what):
    """-> (origin array, its pointer, voxel, trunc | None) as the library takes them: a finite origin, positive finite float32 sizes."""
    org, org_p = _host_f32(np.asarray(origin, np.float32), 3, "origin")
    if not np.isfinite(org).all():
        raise PmnError(f"{what}: origin must be finite")
    return org, org_p, _positive_f32(voxel, f"{what}: voxel"), None if trunc is None else _positive_f32(trunc, f"{what}: trunc")


def _view_args(maps, slots, sizes, cams, masks, images, dev, what):
    _dev(maps, "maps")
    if maps.dim() < 2 or maps.device != dev:
        raise PmnError(f"{what}: maps must be [S,...] slots on the volume's device")
    S, stride = maps.shape[0], maps[0].numel()
    V = len(slots)
    if not 1 <= V <= _lib.TSDF_MAX_VIEWS:
        raise PmnError(f"{what}: 1 .. {_lib.TSDF_MAX_VIEWS} views per launch, got {V}")
    if len(sizes) != V or any(not 0 <= int(s) < S for s in slots) or any(h < 1 or w < 1 or h * w > stride for h, w in sizes):
        raise PmnError(f"{what}: a slot is out of range or a view's depth map does not fit its slot")
    cam = np.ascontiguousarray(np.asarray(cams, np.float32).reshape(-1))
    if cam.size != 21 * V or not np.isfinite(cam).all():
        raise PmnError(f"{what}: cams must hold 21 finite floats per view (K, then the upper 3x4 of the extrinsic)")

    def table(items, shape_of, name):
        if items is None:
            return None, None
        if len(items) != V:
            raise PmnError(f"{what}: {name} must have one entry (a tensor or None) per view")
        arr = (ctypes.c_void_p * V)()
        for n, t in enumerate(items):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != torch.uint8 or \
                    not t.is_contiguous() or tuple(t.shape) != shape_of(*sizes[n]):
                raise PmnError(f"{what}: {name}[{n}] must be a contiguous uint8 tensor {shape_of(*sizes[n])} on the volume's device "
                               f"(no CPU fallback)")
            arr[n] = t.data_ptr()
        return arr, ctypes.cast(arr, ctypes.c_void_p)

    m_arr, m_p = table(masks, lambda h, w: (h, w), "masks")
    i_arr, i_p = table(images, lambda h, w: (h, w, 3), "images")
    sl, sl_p = _host_i32(np.asarray(list(slots)), V, "slots")
    hw, hw_p = _host_i32(np.asarray([x for s in sizes for x in s]), 2 * V, "sizes")
    return V, int(stride), cam, (m_arr, i_arr, sl, hw), sl_p, hw_p, m_p, i_p


def tsdf_integrate(tsdf: torch.Tensor, weight: torch.Tensor, rgb: Optional[torch.Tensor], cweight: Optional[torch.Tensor], origin,
                   voxel: float, trunc: float, maps: torch.Tensor, slots: Sequence[int], sizes: Sequence[Tuple[int, int]], cams,
                   masks: Optional[Sequence[Optional[torch.Tensor]]] = None,
                   images: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
    """pmn_tsdf_integrate: folds the depth maps of len(slots) views (1 .. _lib.TSDF_MAX_VIEWS) into the volume IN PLACE, one launch
    (DESIGN.md section 15).  tsdf / weight [nz,ny,nx] (initially 1 / 0), rgb [3,nz,ny,nx] + cweight or None + None; ``origin`` 3
    floats and ``voxel`` place sample (i,j,k) at origin + (i,j,k) * voxel.  maps [S,F] float32 slots (or any [S,...] buffer whose slot
    starts with the depth map, e.g. eval.py's [V,2,H,W]); view n is slot ``slots[n]``, ``sizes[n] = (h, w)``, ``cams[n]`` = 21 floats
    (K row-major at map size, then the upper 3x4 of the world-to-camera extrinsic; numpy, read on the host), ``masks[n]`` a uint8
    [h,w] tensor or None, ``images[n]`` a uint8 [h,w,3] tensor or None."""
    dims, dims_p = _volume_planes(tsdf, weight, rgb, cweight, "tsdf_integrate")
    org, org_p, voxel, trunc = _placement(origin, voxel, trunc, "tsdf_integrate")
    V, stride, cam, keep, sl_p, hw_p, m_p, i_p = _view_args(maps, slots, sizes, cams, masks, images, tsdf.device, "tsdf_integrate")
    with torch.cuda.device(tsdf.device):
        check(_lib.lib().pmn_tsdf_integrate(tsdf.data_ptr(), weight.data_ptr(), _ptr(rgb), _ptr(cweight), dims_p, org_p, voxel, trunc,
                                            maps.data_ptr(), stride, sl_p, hw_p, m_p, i_p, cam.ctypes.data_as(ctypes.c_void_p), V,
                                            _stream(tsdf)), "pmn_tsdf_integrate")
    del dims, org, keep


def _popcount_u8(m: torch.Tensor) -> torch.Tensor:
    m = m - ((m >> 1) & 0x55)
    m = (m & 0x33) + ((m >> 2) & 0x33)
    return (m + (m >> 4)) & 0x0F


def _mt_extract(what, tsdf, color, normals, count, emit):
    """The body of mt_extract and mt_extract_blocks over planes shaped like ``tsdf``: count, the scans, the outputs, emit.
    ``count(vmask, ntri)`` and ``emit(vmask, ntri, vscan, tscan, vertices, colors, nrm, faces)`` make the two library calls."""
    dev = tsdf.device
    vmask = torch.empty(tsdf.shape, dtype=torch.uint8, device=dev)
    ntri = torch.empty(tsdf.shape, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        count(vmask, ntri)
        vcount = _popcount_u8(vmask)
        totals = torch.stack((vcount.sum(dtype=torch.int64), ntri.sum(dtype=torch.int64))).tolist()  # the feature's one host read
        nv, nt = int(totals[0]), int(totals[1])
        if nv > 2 ** 31 - 1 or nt > 2 ** 31 - 1:
            raise PmnError(f"{what}: {nv} vertices / {nt} triangles do not fit int32 indices; use a larger voxel")
        vscan = torch.cumsum(vcount.reshape(-1), 0, dtype=torch.int32)
        tscan = torch.cumsum(ntri.reshape(-1), 0, dtype=torch.int32)
        del vcount
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        colors = torch.empty((nv, 3), dtype=torch.uint8, device=dev) if color else None
        nrm = torch.empty((nv, 3), dtype=torch.float32, device=dev) if normals else None
        if nv:
            emit(vmask, ntri, vscan, tscan, vertices, colors, nrm, faces)
    return vertices, faces, colors, nrm


def mt_extract(tsdf: torch.Tensor, weight: torch.Tensor, origin, voxel: float, min_weight: float = 1.0,
               rgb: Optional[torch.Tensor] = None, cweight: Optional[torch.Tensor] = None, normals: bool = True):
    """pmn_mt_count + scan + pmn_mt_emit: the iso-surface tsdf = 0 of a volume by marching tetrahedra.
    Returns (vertices [Nv,3] float32, faces [Nt,3] int32, colors [Nv,3] uint8 or None (with rgb / cweight), normals [Nv,3] float32
    or None), on the volume's device; vertices ordered by owning sample then edge class, faces by cell, tetrahedron, triangle.  The two
    scans are torch.cumsum on the device; ONE host read (the two totals, to size the outputs) is the only synchronisation."""
    dims, dims_p = _volume_planes(tsdf, weight, rgb, cweight, "mt_extract")
    org, org_p, voxel, _ = _placement(origin, voxel, None, "mt_extract")
    min_weight = float(np.float32(min_weight))
    if not np.isfinite(min_weight):
        raise PmnError("mt_extract: min_weight must be finite")
    L, planes, stream = _lib.lib(), (tsdf.data_ptr(), weight.data_ptr()), _stream(tsdf)

    def count(vmask, ntri):
        check(L.pmn_mt_count(*planes, dims_p, min_weight, vmask.data_ptr(), ntri.data_ptr(), stream), "pmn_mt_count")

    def emit(vmask, ntri, vscan, tscan, vertices, colors, nrm, faces):
        check(L.pmn_mt_emit(*planes, _ptr(rgb), _ptr(cweight), dims_p, org_p, voxel, min_weight, vmask.data_ptr(), ntri.data_ptr(),
                            vscan.data_ptr(), tscan.data_ptr(), vertices.data_ptr(), _ptr(colors), _ptr(nrm), faces.data_ptr(), stream),
              "pmn_mt_emit")

    out = _mt_extract("mt_extract", tsdf, rgb is not None, normals, count, emit)
    del dims, org
    return out


# ---- block-sparse volume -----------------------------------------------------------------------------------

SPARSE_BLOCK = 8            # samples per block side
SPARSE_MAX_AXIS = 2 ** 19   # samples per axis of the virtual lattice (exclusive)
SPARSE_MAX_TABLE = 2 ** 28  # blocks of the virtual lattice
SPARSE_MAX_BLOCKS = (2 ** 31 - 1) // SPARSE_BLOCK ** 3  # slots of a pool


def sparse_blocks(dims) -> Tuple[int, int, int]:
    """(nbx, nby, nbz) of a virtual lattice of ``dims`` = (nx, ny, nz) samples; PmnError beyond the limits of include/pmn_hip.h."""
    nx, ny, nz = (int(d) for d in dims)
    nb = tuple(-(-n // SPARSE_BLOCK) for n in (nx, ny, nz))
    if min(nx, ny, nz) < 2 or max(nx, ny, nz) >= SPARSE_MAX_AXIS or nb[0] * nb[1] * nb[2] > SPARSE_MAX_TABLE:
        raise PmnError(f"sparse volume: dims {nx} x {ny} x {nz} must be 2 .. {SPARSE_MAX_AXIS - 1} per axis and at most "
                       f"{SPARSE_MAX_TABLE} blocks of {SPARSE_BLOCK}^3 samples")
    return nb


def _grid_args(dims, origin, voxel, trunc, what):
    nb = sparse_blocks(dims)
    d, d_p = _host_i32(np.asarray([int(x) for x in dims]), 3, "dims")
    org, org_p, voxel, trunc = _placement(origin, voxel, trunc, what)
    return nb, (d, org), d_p, org_p, voxel, trunc


def inverse_cameras(cams) -> np.ndarray:
    """[V,21] float32: K^-1 row-major, then the upper 3x4 of the camera-to-world matrix, of [V,21] cameras (tsdf.camera21), inverted in
    float64; PmnError for a singular or non-finite camera."""
    cams = np.asarray(cams, np.float32).reshape(-1, 21).astype(np.float64)
    out = np.empty((len(cams), 21), np.float32)
    for n, c in enumerate(cams):
        E = np.eye(4)
        E[:3] = c[9:].reshape(3, 4)
        try:
            with np.errstate(all="ignore"):
                out[n, :9] = np.linalg.inv(c[:9].reshape(3, 3)).reshape(9)
                out[n, 9:] = np.linalg.inv(E)[:3].reshape(12)
        except np.linalg.LinAlgError as e:
            raise PmnError(f"tsdf_mark_blocks: camera {n} is singular") from e
    if not np.isfinite(out).all():
        raise PmnError("tsdf_mark_blocks: a camera has no finite float32 inverse")
    return out


def tsdf_mark_blocks(flags: torch.Tensor, overflow: torch.Tensor, dims, origin, voxel: float, trunc: float, maps: torch.Tensor,
                     slots: Sequence[int], sizes: Sequence[Tuple[int, int]], cams,
                     masks: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
    """pmn_tsdf_mark_blocks: sets ``flags`` (uint8 [nbz,nby,nbx], zeroed by the caller; calls accumulate) to 1 for the blocks of the
    virtual lattice ``dims`` = (nx, ny, nz) near the surface of len(slots) views (1 .. _lib.TSDF_MAX_VIEWS), one launch (DESIGN.md
    section 18).  ``overflow`` (int32 [1], zeroed by the caller) counts the pixels whose box was too large to mark: read it with the
    flags.  The view arguments are tsdf_integrate's; the cameras are inverted here, in float64."""
    _dev_as(flags, "flags", torch.uint8)
    _dev_as(overflow, "overflow", torch.int32)
    nb, keep, dims_p, org_p, voxel, trunc = _grid_args(dims, origin, voxel, trunc, "tsdf_mark_blocks")
    if tuple(flags.shape) != nb[::-1]:
        raise PmnError(f"tsdf_mark_blocks: flags must be a contiguous uint8 tensor {nb[::-1]} (nbz, nby, nbx)")
    if overflow.numel() != 1 or overflow.device != flags.device:
        raise PmnError("tsdf_mark_blocks: overflow must be one int32 on the flags' device")
    V, stride, cam, keep2, sl_p, hw_p, m_p, _ = _view_args(maps, slots, sizes, cams, masks, None, flags.device, "tsdf_mark_blocks")
    inv = np.ascontiguousarray(inverse_cameras(cam).reshape(-1))
    with torch.cuda.device(flags.device):
        check(_lib.lib().pmn_tsdf_mark_blocks(flags.data_ptr(), overflow.data_ptr(), dims_p, org_p, voxel, trunc, maps.data_ptr(), stride,
                                              sl_p, hw_p, m_p, inv.ctypes.data_as(ctypes.c_void_p), V, _stream(flags)),
              "pmn_tsdf_mark_blocks")
    del keep, keep2


def _pool_planes(tsdf, weight, rgb, cweight, blocks, what):
    _dev(tsdf, "tsdf")
    _dev(weight, "weight")
    _dev_as(blocks, "blocks", torch.int32)
    B = tsdf.shape[0] if tsdf.dim() == 4 else 0
    shape = (B,) + (SPARSE_BLOCK,) * 3
    if not 1 <= B <= SPARSE_MAX_BLOCKS or tuple(tsdf.shape) != shape or tuple(weight.shape) != shape or weight.device != tsdf.device:
        raise PmnError(f"{what}: tsdf and weight must be [B,8,8,8] pool planes on one device, 1 <= B <= {SPARSE_MAX_BLOCKS}")
    _colour_planes(tsdf, rgb, cweight, what, "rgb must be [3,B,8,8,8] and cweight [B,8,8,8] on the pool's device")
    if tuple(blocks.shape) != (B,) or blocks.device != tsdf.device:
        raise PmnError(f"{what}: blocks must be a contiguous int32 [B] tensor on the pool's device")
    return B


def tsdf_integrate_blocks(tsdf: torch.Tensor, weight: torch.Tensor, rgb: Optional[torch.Tensor], cweight: Optional[torch.Tensor],
                          blocks: torch.Tensor, dims, origin, voxel: float, trunc: float, maps: torch.Tensor, slots: Sequence[int],
                          sizes: Sequence[Tuple[int, int]], cams, masks: Optional[Sequence[Optional[torch.Tensor]]] = None,
                          images: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
    """pmn_tsdf_integrate_blocks: tsdf_integrate on the samples of the blocks ``blocks`` (int32 [B], linear block indices of the virtual
    lattice ``dims``, ascending) of a pool tsdf / weight [B,8,8,8], rgb [3,B,8,8,8] + cweight or None + None, IN PLACE, one launch: a
    pool sample ends with the bits the dense volume holds at its lattice index."""
    B = _pool_planes(tsdf, weight, rgb, cweight, blocks, "tsdf_integrate_blocks")
    nb, keep, dims_p, org_p, voxel, trunc = _grid_args(dims, origin, voxel, trunc, "tsdf_integrate_blocks")
    V, stride, cam, keep2, sl_p, hw_p, m_p, i_p = _view_args(maps, slots, sizes, cams, masks, images, tsdf.device, "tsdf_integrate_blocks")
    with torch.cuda.device(tsdf.device):
        check(_lib.lib().pmn_tsdf_integrate_blocks(tsdf.data_ptr(), weight.data_ptr(), _ptr(rgb), _ptr(cweight), blocks.data_ptr(), B,
                                                   dims_p, org_p, voxel, trunc, maps.data_ptr(), stride, sl_p, hw_p, m_p, i_p,
                                                   cam.ctypes.data_as(ctypes.c_void_p), V, _stream(tsdf)), "pmn_tsdf_integrate_blocks")
    del keep, keep2


def mt_extract_blocks(tsdf: torch.Tensor, weight: torch.Tensor, table: torch.Tensor, blocks: torch.Tensor, dims, origin, voxel: float,
                      min_weight: float = 1.0, rgb: Optional[torch.Tensor] = None, cweight: Optional[torch.Tensor] = None,
                      normals: bool = True):
    """pmn_mt_count_blocks + scan + pmn_mt_emit_blocks: mt_extract over a pool.  ``table`` int32 [nbz,nby,nbx]
    holds every block's slot or -1, ``blocks`` int32 [B] every slot's block.  Returns what mt_extract returns, in pool order (slot,
    sample within the block, class / tetrahedron); as a set of triangles it is the mesh mt_extract gives on the dense planes of the
    same samples.  min_weight must be > 0 (a sample without a slot is unobserved).  The scans are torch.cumsum over B * 512 entries;
    one host read of the totals."""
    B = _pool_planes(tsdf, weight, rgb, cweight, blocks, "mt_extract_blocks")
    nb, keep, dims_p, org_p, voxel, _ = _grid_args(dims, origin, voxel, None, "mt_extract_blocks")
    _dev_as(table, "table", torch.int32)
    if tuple(table.shape) != nb[::-1] or table.device != tsdf.device:
        raise PmnError(f"mt_extract_blocks: table must be a contiguous int32 tensor {nb[::-1]} (nbz, nby, nbx) on the pool's device")
    min_weight = float(np.float32(min_weight))
    if not (np.isfinite(min_weight) and min_weight > 0):
        raise PmnError("mt_extract_blocks: min_weight must be positive and finite")
    L, planes, lists, stream = _lib.lib(), (tsdf.data_ptr(), weight.data_ptr()), (table.data_ptr(), blocks.data_ptr(), B), _stream(tsdf)

    def count(vmask, ntri):
        check(L.pmn_mt_count_blocks(*planes, *lists, dims_p, min_weight, vmask.data_ptr(), ntri.data_ptr(), stream), "pmn_mt_count_blocks")

    def emit(vmask, ntri, vscan, tscan, vertices, colors, nrm, faces):
        check(L.pmn_mt_emit_blocks(*planes, _ptr(rgb), _ptr(cweight), *lists, dims_p, org_p, voxel, min_weight, vmask.data_ptr(),
                                   ntri.data_ptr(), vscan.data_ptr(), tscan.data_ptr(), vertices.data_ptr(), _ptr(colors), _ptr(nrm),
                                   faces.data_ptr(), stream), "pmn_mt_emit_blocks")

    out = _mt_extract("mt_extract_blocks", tsdf, rgb is not None, normals, count, emit)
    del keep
    return out


# ---- rendering ---------------------------------------------------------------------------------------------

def _raster_common(keys: torch.Tensor, counters: torch.Tensor, cam, what: str):
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda:
        raise PmnError(f"{what}: keys must be a tensor on a ROCm GPU (no CPU fallback)")
    if keys.dtype != torch.int64 or keys.dim() != 2 or not keys.is_contiguous() or keys.numel() == 0:
        raise PmnError(f"{what}: keys must be a contiguous [h,w] int64 tensor (the uint64 keys' bits)")
    h, w = keys.shape
    if h > _lib.RASTER_MAX_DIM or w > _lib.RASTER_MAX_DIM:
        raise PmnError(f"{what}: a view is at most {_lib.RASTER_MAX_DIM} pixels per side")
    if not isinstance(counters, torch.Tensor) or counters.device != keys.device or counters.dtype != torch.int32 or \
            counters.numel() != 4 or not counters.is_contiguous():
        raise PmnError(f"{what}: counters must be 4 int32 on the keys' device")
    cam = np.ascontiguousarray(np.asarray(cam, np.float32).reshape(-1))
    if cam.size != 21 or not np.isfinite(cam).all():
        raise PmnError(f"{what}: cam must hold 21 finite floats (K, then the upper 3x4 of the extrinsic)")
    return h, w, cam


def _raster_array(t, dtype, keys, name, what, rows=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != keys.device or t.dtype != dtype or t.dim() != 2 or \
            t.shape[1] != 3 or not t.is_contiguous() or t.shape[0] < 1 or (rows is not None and t.shape[0] != rows):
        raise PmnError(f"{what}: {name} must be a contiguous [{'n' if rows is None else rows},3] {dtype} tensor on the keys' device "
                       f"(no CPU fallback)")
    return t


def raster_triangles(vertices: torch.Tensor, faces: torch.Tensor, cam, keys: torch.Tensor, counters: torch.Tensor,
                     worklist: torch.Tensor, max_box: int = 0) -> None:
    """pmn_raster_triangles: draws the mesh (vertices [Nv,3] float32 world, faces [Nt,3] int32) into ``keys`` ([h,w] int64 holding
    the uint64 z-buffer keys, filled with -1 = all ones by the caller) through the camera ``cam`` (tsdf.camera21 at the view's size).
    ``counters`` int32[4], zeroed by the caller: not drawn because behind the camera / not finite, outside the guard band, zero area;
    [3] = triangles drawn by the wave-per-triangle kernel.  ``worklist`` int32 [>= Nt] scratch.  ``max_box``: bounding-box pixels up
    to which one thread draws a triangle (0 = the library's default).  Two launches, no host read."""
    h, w, cam = _raster_common(keys, counters, cam, "raster_triangles")
    _raster_array(vertices, torch.float32, keys, "vertices", "raster_triangles")
    _raster_array(faces, torch.int32, keys, "faces", "raster_triangles")
    if vertices.shape[0] > 2 ** 31 - 1 or faces.shape[0] > 2 ** 31 - 1:
        raise PmnError("raster_triangles: at most 2^31 - 1 vertices and faces")
    if not isinstance(worklist, torch.Tensor) or worklist.device != keys.device or worklist.dtype != torch.int32 or \
            not worklist.is_contiguous() or worklist.numel() < faces.shape[0]:
        raise PmnError("raster_triangles: worklist must hold one int32 per face on the keys' device")
    if int(max_box) < 0:
        raise PmnError("raster_triangles: max_box must be >= 0")
    with torch.cuda.device(keys.device):
        check(_lib.lib().pmn_raster_triangles(vertices.data_ptr(), vertices.shape[0], faces.data_ptr(), faces.shape[0],
                                              cam.ctypes.data_as(ctypes.c_void_p), h, w, int(max_box), keys.data_ptr(),
                                              counters.data_ptr(), worklist.data_ptr(), _stream(keys)), "pmn_raster_triangles")


def splat_points(points: torch.Tensor, cam, keys: torch.Tensor, counters: torch.Tensor, radius_px: float = 0.0,
                 radius_world: float = 0.0) -> None:
    """pmn_splat_points: draws the cloud (points [N,3] float32 world) into ``keys`` (see raster_triangles).  Footprint: the nearest
    pixel, and with ``radius_px`` (0 .. _lib.SPLAT_MAX_RADIUS) or ``radius_world`` (a disc of radius_world * fx / z pixels, clamped to
    the same maximum) every pixel whose centre lies in the disc.  One launch."""
    h, w, cam = _raster_common(keys, counters, cam, "splat_points")
    _raster_array(points, torch.float32, keys, "points", "splat_points")
    if points.shape[0] > 2 ** 31 - 1:
        raise PmnError("splat_points: at most 2^31 - 1 points (the index plane is int32)")
    with np.errstate(over="ignore"):
        radius_px, radius_world = float(np.float32(radius_px)), float(np.float32(radius_world))
    if not (0.0 <= radius_px <= _lib.SPLAT_MAX_RADIUS) or not (np.isfinite(radius_world) and radius_world >= 0.0) or \
            (radius_px > 0.0 and radius_world > 0.0):
        raise PmnError(f"splat_points: radius_px must be 0 .. {_lib.SPLAT_MAX_RADIUS}, radius_world >= 0 and finite, and only one "
                       f"of them non-zero")
    with torch.cuda.device(keys.device):
        check(_lib.lib().pmn_splat_points(points.data_ptr(), points.shape[0], cam.ctypes.data_as(ctypes.c_void_p), h, w, radius_px,
                                          radius_world, keys.data_ptr(), counters.data_ptr(), _stream(keys)), "pmn_splat_points")


def raster_resolve(keys: torch.Tensor, cam, vertices: torch.Tensor, faces: Optional[torch.Tensor], depth: torch.Tensor,
                   index: torch.Tensor, colors: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None,
                   shade: bool = False, rgb: Optional[torch.Tensor] = None, normal: Optional[torch.Tensor] = None) -> None:
    """pmn_raster_resolve: turns the keys into depth [h,w] float32 (0 = nothing drawn), index [h,w] int32 (-1) and, if given, rgb
    [h,w,3] uint8 and normal [h,w,3] float32 (camera frame, facing the camera).  ``faces`` None: the primitives were points.
    ``colors`` [Nv,3] uint8 / ``normals`` [Nv,3] float32 (world) are per vertex or per point."""
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda or keys.dtype != torch.int64 or keys.dim() != 2 or \
            not keys.is_contiguous() or keys.numel() == 0:
        raise PmnError("raster_resolve: keys must be a contiguous [h,w] int64 tensor on a ROCm GPU (no CPU fallback)")
    h, w = keys.shape
    cam = np.ascontiguousarray(np.asarray(cam, np.float32).reshape(-1))
    if cam.size != 21 or not np.isfinite(cam).all():
        raise PmnError("raster_resolve: cam must hold 21 finite floats (K, then the upper 3x4 of the extrinsic)")
    _raster_array(vertices, torch.float32, keys, "vertices", "raster_resolve")
    nv = vertices.shape[0]
    if faces is not None:
        _raster_array(faces, torch.int32, keys, "faces", "raster_resolve")
    if colors is not None:
        _raster_array(colors, torch.uint8, keys, "colors", "raster_resolve", nv)
    if normals is not None:
        _raster_array(normals, torch.float32, keys, "normals", "raster_resolve", nv)

    def plane(t, dtype, shape, name):
        if not isinstance(t, torch.Tensor) or t.device != keys.device or t.dtype != dtype or tuple(t.shape) != shape or \
                not t.is_contiguous():
            raise PmnError(f"raster_resolve: {name} must be a contiguous {shape} {dtype} tensor on the keys' device")
        return t

    plane(depth, torch.float32, (h, w), "depth")
    plane(index, torch.int32, (h, w), "index")
    if rgb is not None:
        plane(rgb, torch.uint8, (h, w, 3), "rgb")
    if normal is not None:
        plane(normal, torch.float32, (h, w, 3), "normal")
    with torch.cuda.device(keys.device):
        check(_lib.lib().pmn_raster_resolve(keys.data_ptr(), h, w, cam.ctypes.data_as(ctypes.c_void_p), vertices.data_ptr(), nv,
                                            _ptr(faces), 0 if faces is None else faces.shape[0], _ptr(colors), _ptr(normals),
                                            1 if shade else 0, depth.data_ptr(), index.data_ptr(), _ptr(rgb), _ptr(normal),
                                            _stream(keys)), "pmn_raster_resolve")


class PointPacker:
    """pmn_pack_points: the PLY vertex records of a scan's fused reference views, packed on the device view after view into ONE
    record buffer (reference eval.py:270-297).  ``capacity`` = room in points (a view can keep at most H*W).

        packer = PointPacker(capacity, device)
        for every reference view:  packer.append(masks[2], xyz, image_hwc)        # three launches on the current stream
        counts = packer.counts()                                                   # synchronises the current stream
        body = packer.records[:15 * sum(counts)]                                   # device uint8: the PLY body in pair-file order

    ``normals=True`` (pmn_pack_points_normals): 27-byte records x y z nx ny nz red green blue; ``append`` then also takes the view's
    camera-frame normal map [3,H,W] (``depth_normals``) and its camera-to-world rotation, a device float32 [3,3] or the [4,4]
    inverse(E_ref) whose upper-left block it is (a view into pmn_fuse_view's ``mats`` will do: nothing is copied).  Same points in the
    same order; ``record_size`` is the stride of ``records``.
    """

    def __init__(self, capacity: int, device, max_views: int = 1024, normals: bool = False) -> None:
        self.capacity = int(capacity)
        self.normals = bool(normals)
        self.record_size = 27 if self.normals else 15  # x y z [nx ny nz] red green blue: ply.vertex_dtype(True, normals)
        self.records = torch.empty((self.record_size * self.capacity,), dtype=torch.uint8, device=device)
        self.cursor = torch.zeros((1,), dtype=torch.int64, device=device)
        self.view_counts = torch.zeros((max_views,), dtype=torch.int32, device=device)
        self.scratch = None
        self.n = 0

    def reset(self) -> None:
        self.cursor.zero_()
        self.n = 0

    def append(self, final_mask: torch.Tensor, xyz: torch.Tensor, image_hwc: torch.Tensor,
               normals_chw: Optional[torch.Tensor] = None, rotation: Optional[torch.Tensor] = None) -> None:
        _dev(xyz, "xyz")
        if self.normals != (normals_chw is not None) or self.normals != (rotation is not None):
            raise PmnError("pack_points: a packer built with normals=True takes normals_chw and rotation with every view, "
                           "one built without takes neither")
        for t, name in ((final_mask, "final_mask"), (image_hwc, "image_hwc")):
            if not isinstance(t, torch.Tensor) or t.device != self.records.device:
                raise PmnError(f"pack_points: {name} must be a tensor on {self.records.device} (no CPU fallback)")
        H, W = final_mask.shape
        if final_mask.dtype != torch.uint8 or not final_mask.is_contiguous():
            raise PmnError("pack_points: final_mask must be contiguous uint8 [H,W]")
        if tuple(xyz.shape) != (H, W, 3) or xyz.dtype != torch.float32 or not xyz.is_contiguous():
            raise PmnError("pack_points: xyz must be contiguous float32 [H,W,3]")
        if tuple(image_hwc.shape) != (H, W, 3) or image_hwc.dtype not in (torch.uint8, torch.float32) or not image_hwc.is_contiguous():
            raise PmnError("pack_points: image must be contiguous uint8 or float32 [H,W,3]")
        if self.n >= self.view_counts.numel():
            raise PmnError("pack_points: more views than the packer was sized for")
        nb = (H * W + 1023) // 1024
        if self.scratch is None or self.scratch.numel() < nb:
            self.scratch = torch.empty((nb,), dtype=torch.int64, device=self.records.device)
        if self.normals:
            for t, name in ((normals_chw, "normals_chw"), (rotation, "rotation")):
                if not isinstance(t, torch.Tensor) or t.device != self.records.device or t.dtype != torch.float32:
                    raise PmnError(f"pack_points: {name} must be a float32 tensor on {self.records.device} (no CPU fallback)")
            if tuple(normals_chw.shape) != (3, H, W) or not normals_chw.is_contiguous():
                raise PmnError("pack_points: normals_chw must be contiguous float32 [3,H,W]")
            if tuple(rotation.shape) not in ((3, 3), (4, 4)) or rotation.stride(1) != 1 or rotation.stride(0) < 3:
                raise PmnError("pack_points: rotation must be float32 [3,3] or [4,4] with unit column stride")
            with torch.cuda.device(self.records.device):
                check(_lib.lib().pmn_pack_points_normals(final_mask.data_ptr(), xyz.data_ptr(), normals_chw.data_ptr(),
                                                         rotation.data_ptr(), int(rotation.stride(0)), image_hwc.data_ptr(),
                                                         1 if image_hwc.dtype == torch.float32 else 0, H, W, self.records.data_ptr(),
                                                         self.capacity, self.cursor.data_ptr(), self.view_counts[self.n:].data_ptr(),
                                                         self.scratch.data_ptr(), _stream(self.records)), "pmn_pack_points_normals")
            self.n += 1
            return
        with torch.cuda.device(self.records.device):
            check(_lib.lib().pmn_pack_points(final_mask.data_ptr(), xyz.data_ptr(), image_hwc.data_ptr(),
                                             1 if image_hwc.dtype == torch.float32 else 0, H, W, self.records.data_ptr(),
                                             self.capacity, self.cursor.data_ptr(), self.view_counts[self.n:].data_ptr(),
                                             self.scratch.data_ptr(), _stream(self.records)), "pmn_pack_points")
        self.n += 1

    def counts(self):
        """Per-view point counts (host list); raises if a view did not fit."""
        c = self.view_counts[:self.n].cpu().tolist()
        if any(x < 0 for x in c):
            raise PmnError("pack_points: the record buffer is too small for this scan")
        return c


def view_scores(cam_centers: torch.Tensor, xyz: torch.Tensor, obs_ptr: torch.Tensor, obs_pt: torch.Tensor, trk_ptr: torch.Tensor,
                trk_img: torch.Tensor, theta0: float, sigma1: float, sigma2: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pmn_view_scores: the N x N float64 view-selection scores of the COLMAP import (reference colmap_input.py:336-366).

    cam_centers [N,3] float64, xyz [P,3] float64; per image its observations as CSR (obs_ptr [N+1] int64, obs_pt int32 dense point
    indices in the image's order, untriangulated entries dropped, duplicates kept); per point its distinct observing images in
    ascending order as CSR (trk_ptr [P+1] int64, trk_img int32).  patchmatchnet_amd/colmap.py builds them.  Returns score [N,N]
    float64 (or fills ``out``) on the current stream; every entry is written, the diagonal is 0."""
    specs = ((cam_centers, "cam_centers", torch.float64), (xyz, "xyz", torch.float64), (obs_ptr, "obs_ptr", torch.int64),
             (obs_pt, "obs_pt", torch.int32), (trk_ptr, "trk_ptr", torch.int64), (trk_img, "trk_img", torch.int32))
    for t, name, dtype in specs:
        if not isinstance(t, torch.Tensor):
            raise PmnError(f"{name}: expected a torch.Tensor")
        if not t.is_cuda:
            raise PmnError(f"{name}: tensor is on {t.device}; patchmatchnet_amd runs only on a ROCm GPU (no CPU fallback)")
        if t.dtype != dtype:
            raise PmnError(f"{name}: expected {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise PmnError(f"{name}: tensor must be contiguous")
        if t.device != cam_centers.device:
            raise PmnError(f"{name}: every input must be on {cam_centers.device}")
    if cam_centers.dim() != 2 or cam_centers.shape[1] != 3 or cam_centers.shape[0] < 1:
        raise PmnError("view_scores: cam_centers must be [N,3] with N >= 1")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise PmnError("view_scores: xyz must be [P,3]")
    N, P = int(cam_centers.shape[0]), int(xyz.shape[0])
    if obs_ptr.shape != (N + 1,) or trk_ptr.shape != (P + 1,) or obs_pt.dim() != 1 or trk_img.dim() != 1:
        raise PmnError("view_scores: obs_ptr must be [N+1], trk_ptr [P+1], obs_pt and trk_img 1-D")
    if N >= 2 ** 31 or P >= 2 ** 31:
        raise PmnError("view_scores: more than 2^31 - 1 images or points")
    if out is None:
        out = torch.empty((N, N), dtype=torch.float64, device=cam_centers.device)
    elif not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.shape == (N, N)
              and out.device == cam_centers.device):
        raise PmnError("view_scores: out must be a contiguous float64 [N,N] tensor on the inputs' device")
    with torch.cuda.device(cam_centers.device):
        check(_lib.lib().pmn_view_scores(cam_centers.data_ptr(), _ptr(xyz) if P else None, obs_ptr.data_ptr(),
                                         obs_pt.data_ptr() if obs_pt.numel() else None, trk_ptr.data_ptr(),
                                         trk_img.data_ptr() if trk_img.numel() else None, N, P, int(obs_pt.numel()),
                                         int(trk_img.numel()), float(theta0), float(sigma1), float(sigma2), out.data_ptr(),
                                         _stream(cam_centers)),
              "pmn_view_scores")
    return out


def undistort_image(image_u8_hwc: torch.Tensor, camera, dst_camera, want_valid: bool = False, want_coords: bool = False,
                    out: Optional[torch.Tensor] = None):
    """pmn_undistort_image: a distorted picture resampled into an ideal pinhole camera.

    image_u8_hwc: uint8 [H,W,3] or [H,W,1] or [H,W] on the GPU, contiguous, H x W = camera.height x camera.width.  ``camera`` is the
    source colmap.Camera (any model but FOV / THIN_PRISM_FISHEYE), ``dst_camera`` the PINHOLE (or SIMPLE_PINHOLE) camera of the
    output, usually undistort.undistorted_camera(camera).  Returns the uint8 image [H',W',C] (shaped like the input; ``out`` is
    filled and returned when given) on the current stream; with want_valid / want_coords the tuple (image, valid uint8 [H',W'] or
    None, coords float64 [H',W',2] = the sampling position (sx, sy) of every pixel, or None).  Every byte of the outputs is written.
    A pinhole source whose output camera has the same size and intrinsics is copied, not resampled: every pixel is valid and its
    position is itself."""
    from . import undistort as U
    t = image_u8_hwc
    if not isinstance(t, torch.Tensor):
        raise PmnError("undistort_image: expected a torch.Tensor")
    if not t.is_cuda:
        raise PmnError(f"undistort_image: tensor is on {t.device}; patchmatchnet_amd runs only on a ROCm GPU (no CPU fallback)")
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise PmnError("undistort_image: expected a contiguous uint8 tensor")
    if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] not in (1, 3)):
        raise PmnError(f"undistort_image: expected [H,W], [H,W,1] or [H,W,3], got {tuple(t.shape)}")
    C = 1 if t.dim() == 2 else int(t.shape[2])
    Hs, Ws = int(t.shape[0]), int(t.shape[1])
    if (Hs, Ws) != (int(camera.height), int(camera.width)):
        raise PmnError(f"undistort_image: the image is {Ws} x {Hs} but camera {camera.id} is {camera.width} x {camera.height}")
    try:
        U.check_model(camera)
    except U.UndistortError as e:
        raise PmnError(f"undistort_image: {e}") from e
    if dst_camera.model not in U.PINHOLE_MODELS:
        raise PmnError(f"undistort_image: the output camera must be a pinhole, got {dst_camera.model}")
    Hd, Wd = int(dst_camera.height), int(dst_camera.width)
    if Hs < 1 or Ws < 1 or Hd < 1 or Wd < 1 or Hs * Ws * C >= 2 ** 31 or Hd * Wd * C >= 2 ** 31:
        raise PmnError("undistort_image: an image must have at least one pixel and fewer than 2^31 bytes")
    shape = (Hd, Wd) if t.dim() == 2 else (Hd, Wd, C)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=t.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
              and tuple(out.shape) == shape and out.device == t.device):
        raise PmnError(f"undistort_image: out must be a contiguous uint8 {shape} tensor on the image's device")
    elif _ranges_overlap(_range(out), _range(t)):
        raise PmnError("undistort_image: out must not overlap the image")
    valid = torch.empty((Hd, Wd), dtype=torch.uint8, device=t.device) if want_valid else None
    coords = torch.empty((Hd, Wd, 2), dtype=torch.float64, device=t.device) if want_coords else None
    dst = U.focal_and_center(dst_camera)
    if camera.model in U.PINHOLE_MODELS and (Hd, Wd) == (Hs, Ws) and dst == U.focal_and_center(camera):
        out.copy_(t.view(shape))
        if valid is not None:
            valid.fill_(1)
        if coords is not None:
            coords[..., 0] = torch.arange(Wd, dtype=torch.float64, device=t.device)[None, :]
            coords[..., 1] = torch.arange(Hd, dtype=torch.float64, device=t.device)[:, None]
    else:
        params = (ctypes.c_double * len(camera.params))(*[float(v) for v in camera.params])
        pin = (ctypes.c_double * 4)(*dst)
        with torch.cuda.device(t.device):
            check(_lib.lib().pmn_undistort_image(t.data_ptr(), Hs, Ws, C, U.CAMERA_MODEL_IDS[camera.model],
                                                 ctypes.cast(params, ctypes.c_void_p), ctypes.cast(pin, ctypes.c_void_p), Hd, Wd,
                                                 out.data_ptr(), _ptr(valid), _ptr(coords), _stream(t)), "pmn_undistort_image")
    return (out, valid, coords) if (want_valid or want_coords) else out


def depth_metrics(depth_gt: torch.Tensor, depth_min: torch.Tensor, depth_patchmatch, thresholds: Sequence[float] = (1.0, 2.0, 4.0, 8.0),
                  out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pmn_depth_metrics: per sample one row of raw float64 sums and exact counts against the ground truth (train.py --mode test;
    reference train.py:127-181).  Row layout: include/pmn_hip.h (PMN_METRICS_*; _lib.METRICS_*); patchmatchnet_amd/validate.py turns
    rows into the reference's scalars.

    depth_gt [B,H,W] or [B,1,H,W] float32, depth_min [B] float32; depth_patchmatch = the forward's {stage: [maps]} (or a list in stage
    order): stage 0 the refined [B,1,H,W], stage s its iterations at [B,1,H>>s,W>>s].  Returns rows [B, _lib.METRICS_ROW] float64 (or
    fills ``out``) on the current stream, without a synchronisation; ``scratch`` (float64, at least _lib.metrics_scratch(B,H,W)) is
    allocated when not given."""
    _dev(depth_gt, "depth_gt")
    _dev(depth_min, "depth_min")
    if depth_gt.dim() == 4 and depth_gt.shape[1] == 1:
        depth_gt = depth_gt.view(depth_gt.shape[0], depth_gt.shape[2], depth_gt.shape[3])
    if depth_gt.dim() != 3:
        raise PmnError(f"depth_metrics: depth_gt must be [B,H,W] or [B,1,H,W], got {tuple(depth_gt.shape)}")
    B, H, W = (int(x) for x in depth_gt.shape)
    if tuple(depth_min.shape) != (B,):
        raise PmnError(f"depth_metrics: depth_min must be [{B}], got {tuple(depth_min.shape)}")
    stages = [depth_patchmatch[s] for s in sorted(depth_patchmatch)] if isinstance(depth_patchmatch, dict) else list(depth_patchmatch)
    if isinstance(depth_patchmatch, dict) and sorted(depth_patchmatch) != list(range(len(stages))):
        raise PmnError(f"depth_metrics: depth_patchmatch must hold stages 0..n-1, got {sorted(depth_patchmatch)}")
    if not 1 <= len(stages) <= _lib.METRICS_MAX_STAGES:
        raise PmnError(f"depth_metrics: 1 to {_lib.METRICS_MAX_STAGES} stages, got {len(stages)}")
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) > _lib.METRICS_MAX_THRESHOLDS:
        raise PmnError(f"depth_metrics: at most {_lib.METRICS_MAX_THRESHOLDS} thresholds, got {len(thresholds)}")
    maps, iters, hw = [], [], []
    for s, ms in enumerate(stages):
        ms = list(ms)
        if not 1 <= len(ms) <= _lib.METRICS_MAX_ITERS:
            raise PmnError(f"depth_metrics: stage {s} has {len(ms)} maps; 1 to {_lib.METRICS_MAX_ITERS} are supported")
        shape = None
        for k, m in enumerate(ms):
            _dev(m, f"depth_patchmatch[{s}][{k}]")
            if m.device != depth_gt.device:
                raise PmnError(f"depth_patchmatch[{s}][{k}]: on {m.device}, the ground truth on {depth_gt.device}")
            sh = tuple(m.shape)
            if len(sh) == 4 and sh[1] == 1:
                sh = (sh[0], sh[2], sh[3])
            if len(sh) != 3 or sh[0] != B or (shape is not None and sh != shape):
                raise PmnError(f"depth_metrics: depth_patchmatch[{s}][{k}] is {tuple(m.shape)}; expected [{B},1,h,w] like the stage's "
                               "other maps")
            shape = sh
            maps.append(m.data_ptr())
        if shape[1:] != (H >> s, W >> s) or min(shape[1:]) < 1:
            raise PmnError(f"depth_metrics: the stage-{s} maps are {shape[1]}x{shape[2]}, the nearest down-sampling of the {H}x{W} "
                           f"ground truth is {H >> s}x{W >> s} (the model's stage maps match it only when H and W are multiples of "
                           f"{1 << (len(stages) - 1)})")
        iters.append(len(ms))
        hw += [shape[1], shape[2]]
    if out is None:
        out = torch.empty((B, _lib.METRICS_ROW), dtype=torch.float64, device=depth_gt.device)
    elif not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (B, _lib.METRICS_ROW)
              and out.device == depth_gt.device):
        raise PmnError(f"depth_metrics: out must be a contiguous float64 [{B},{_lib.METRICS_ROW}] tensor on the ground truth's device")
    need = _lib.metrics_scratch(B, H, W)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float64, device=depth_gt.device)
    elif not (scratch.is_cuda and scratch.dtype == torch.float64 and scratch.is_contiguous() and scratch.numel() >= need
              and scratch.device == depth_gt.device):
        raise PmnError(f"depth_metrics: scratch must be a contiguous float64 tensor of at least {need} elements on the same device")
    maps_h = (ctypes.c_void_p * len(maps))(*maps)
    iters_h = (ctypes.c_int * len(iters))(*iters)
    hw_h = (ctypes.c_int * len(hw))(*hw)
    thr_h = (ctypes.c_float * max(len(thresholds), 1))(*thresholds)
    with torch.cuda.device(depth_gt.device):
        check(_lib.lib().pmn_depth_metrics(depth_gt.data_ptr(), depth_min.data_ptr(), ctypes.cast(maps_h, ctypes.c_void_p),
                                           ctypes.cast(iters_h, ctypes.c_void_p), ctypes.cast(hw_h, ctypes.c_void_p), len(stages),
                                           ctypes.cast(thr_h, ctypes.c_void_p), len(thresholds), B, H, W, scratch.data_ptr(),
                                           int(scratch.numel()), out.data_ptr(), _stream(depth_gt)),
              "pmn_depth_metrics")
    return out
