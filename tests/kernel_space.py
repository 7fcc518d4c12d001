"""The PatchMatch kernel space: one row per call of the hot-path entry points (pmn_init_hypotheses, pmn_feature_weight,
pmn_warp_correlate / pmn_warp_correlate_views, pmn_aggregate_regress, plus pmn_confidence and pmn_normalize_depth), each naming the
compile-time specialisation its shape selects.  Jointly the rows select every instantiation the C ABI can reach, at the edges where
such kernels go wrong: pixel counts off the tile size, hypothesis / neighbour counts on both sides of every template boundary,
batches whose samples differ, one and many source views, sources smaller than the reference, projections that leave the image,
view weights at reduced resolution and costs large enough to overflow a softmax without max-subtraction.

Plain helper module (no tests here): tests/test_kernel_space.py checks the table against the library on the CPU (launch-plan
recording and the library's own symbol table), tests/test_kernel_space_gpu.py runs every row on the device against the float64
reference tests/ref64.py, tests/test_guard_band_gpu.py runs every row through the raw C ABI between guard bands (buffers(),
arguments(), run_guard() below).
"""
from __future__ import annotations

import ctypes
import struct
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import numpy as np

from guard_band import Buf, recording_addresses

MLP_FLOATS = 340  # PMN_MLP_FLOATS of include/pmn_hip.h

# ---- the rows ---------------------------------------------------------------------------------------------------------------------


@dataclass(frozen=True)
class Row:
    op: str                  # init | feature_weight | warp | aggregate | confidence | normalize
    kernel: str              # the specialisation this row selects (readable form; mangle() gives the symbol)
    B: int = 1
    N: int = 1               # source views (warp)
    C: int = 64
    G: int = 8
    D: int = 8               # hypotheses (init: the resulting D0 + propK; feature_weight: K)
    h: int = 8
    w: int = 8
    hs: int = 0              # source map size (warp; 0 = h, w)
    ws: int = 0
    vw_shift: int = 0        # warp with given view weights: they are [B,N,h>>s,w>>s]
    pixelwise: bool = False  # warp: view weights computed by PixelwiseNet (none given)
    init: str = ""           # init: "noise" (48 random bins) or "depth" (local samples around a previous depth)
    num_sample: int = 0      # init from depth
    depth_shift: int = 0     # init from depth: previous depth at half resolution
    propK: int = 0           # propagated neighbours (init)
    K: int = 9               # evaluation neighbours (aggregate)
    is_inverse: bool = False
    far: bool = False        # warp: projections that send taps / whole hypotheses out of the source image, and points behind it
    big: bool = False        # aggregate: costs of magnitude 105 .. 125
    H: int = 0               # confidence output size
    W: int = 0
    seed: int = 0
    rig: str = ""            # warp: projections and depth samples of this rig of tests/camera_space.py at the row's map size
    device_only: bool = False  # needs > 48 KB of dynamic LDS: recording calls hipFuncSetAttribute, which needs a device

    @property
    def id(self) -> str:
        k = self.kernel.replace(" ", "").replace("true", "T").replace("false", "F")
        return f"{self.op}-{k}-s{self.seed}" + (f"-{self.rig}" if self.rig else "")


def _g(C: int, G: int, mode: int, DT: int, exact: bool) -> str:
    return f"gather_corr_kernel<{C}, {G}, {mode}, {DT}, {'true' if exact else 'false'}>"


def _rows() -> List[Row]:
    R: List[Row] = []
    # -- pmn_init_hypotheses: 64-thread blocks; h*w off 64 and the 2x2 minimum --------------------------------------------------------
    I = "init_hypotheses_kernel"
    F = "init_hypotheses_fixed_kernel"
    R += [
        Row("init", f"{F}<64, 48, 16>", init="noise", propK=16, D=64, B=2, h=9, w=13),
        Row("init", f"{F}<32, 16, 16>", init="depth", num_sample=16, propK=16, D=32, h=10, w=14, depth_shift=1),
        Row("init", f"{F}<16, 8, 8>", init="depth", num_sample=8, propK=8, D=16, B=2, h=7, w=11),
        Row("init", f"{F}<8, 8, 0>", init="depth", num_sample=8, D=8, h=2, w=2),
        Row("init", f"{I}<8>", init="depth", num_sample=1, D=1, h=5, w=13),
        Row("init", f"{I}<8>", init="depth", num_sample=1, propK=4, D=5, B=2, h=6, w=10, depth_shift=1),
        Row("init", f"{I}<8>", init="depth", num_sample=4, propK=4, D=8, h=9, w=9),
        Row("init", f"{I}<16>", init="depth", num_sample=9, D=9, h=3, w=3),
        Row("init", f"{I}<16>", init="depth", num_sample=5, propK=8, D=13, B=2, h=12, w=14, depth_shift=1),
        Row("init", f"{I}<16>", init="depth", num_sample=12, propK=4, D=16, h=8, w=12, depth_shift=1),
        Row("init", f"{I}<32>", init="depth", num_sample=20, propK=4, D=24, h=9, w=7),
        Row("init", f"{I}<32>", init="depth", num_sample=24, propK=8, D=32, B=2, h=11, w=13),
        Row("init", f"{I}<32>", init="depth", num_sample=17, D=17, h=5, w=5),
        Row("init", f"{I}<64>", init="noise", D=48, h=7, w=9),
        Row("init", f"{I}<64>", init="noise", propK=8, D=56, B=2, h=11, w=10),
        Row("init", f"{I}<64>", init="depth", num_sample=48, propK=16, D=64, h=6, w=14, depth_shift=1),
        Row("init", f"{I}<64>", init="depth", num_sample=33, D=33, h=2, w=2),
    ]
    # -- pmn_feature_weight (MODE_NEIGHBOR = 2): DT 16 for K <= 16 (EXACT at the reference's 9), DT 32 for K = 17 (EXACT) ------------
    for C, G, hw, seed in ((64, 8, (5, 7), 0), (32, 8, (9, 7), 1), (16, 4, (13, 11), 2)):
        R += [
            Row("feature_weight", _g(C, G, 2, 16, True), C=C, G=G, D=9, h=hw[0], w=hw[1], seed=seed),
            Row("feature_weight", _g(C, G, 2, 32, True), C=C, G=G, D=17, B=2, h=hw[1], w=hw[0], seed=seed),
            Row("feature_weight", _g(C, G, 2, 16, False), C=C, G=G, D={64: 1, 32: 16, 16: 4}[C], h=2, w=5 + seed, seed=seed),
        ]
    R += [Row("feature_weight", _g(64, 8, 2, 16, False), C=64, G=8, D=16, B=2, h=6, w=9, seed=3)]
    # -- pmn_warp_correlate with given view weights (MODE_VIEWS = 0): DT = next power of two >= D (and >= C/4); EXACT when D == DT.
    #    Tiles: 16 pixels (C 64), 32 (C 32), 64 (C 16).
    V = dict(N=2)
    R += [
        Row("warp", _g(64, 8, 0, 16, False), C=64, G=8, D=1, h=5, w=7, **V),
        Row("warp", _g(64, 8, 0, 16, False), C=64, G=8, D=15, B=2, h=6, w=6, N=4, hs=4, ws=5, vw_shift=1),
        Row("warp", _g(64, 8, 0, 16, True), C=64, G=8, D=16, h=9, w=7, N=1, far=True),
        Row("warp", _g(64, 8, 0, 32, False), C=64, G=8, D=17, h=2, w=2, **V),
        Row("warp", _g(64, 8, 0, 32, True), C=64, G=8, D=32, B=2, h=12, w=12, N=4, vw_shift=2, far=True),
        Row("warp", _g(64, 8, 0, 64, False), C=64, G=8, D=33, h=7, w=5, N=5, hs=5, ws=4),
        Row("warp", _g(64, 8, 0, 64, True), C=64, G=8, D=64, B=2, h=10, w=8, vw_shift=1, **V),
        Row("warp", _g(32, 8, 0, 8, False), C=32, G=8, D=1, h=2, w=2, N=1),
        Row("warp", _g(32, 8, 0, 8, True), C=32, G=8, D=8, B=2, h=7, w=9, N=4, far=True),
        Row("warp", _g(32, 8, 0, 16, False), C=32, G=8, D=9, h=6, w=10, vw_shift=1, hs=4, ws=7, **V),
        Row("warp", _g(32, 8, 0, 16, True), C=32, G=8, D=16, h=11, w=5, **V),
        Row("warp", _g(32, 8, 0, 32, False), C=32, G=8, D=31, B=2, h=8, w=12, N=4, vw_shift=2),
        Row("warp", _g(32, 8, 0, 32, True), C=32, G=8, D=32, h=5, w=13, N=1, far=True),
        Row("warp", _g(32, 8, 0, 64, False), C=32, G=8, D=33, h=5, w=9, **V),
        Row("warp", _g(32, 8, 0, 64, False), C=32, G=8, D=47, B=2, h=6, w=6, vw_shift=1, N=4, device_only=True),
        Row("warp", _g(32, 8, 0, 64, True), C=32, G=8, D=64, h=9, w=7, far=True, device_only=True, **V),
        Row("warp", _g(16, 4, 0, 8, False), C=16, G=4, D=2, h=9, w=7, **V),
        Row("warp", _g(16, 4, 0, 8, True), C=16, G=4, D=8, B=2, h=10, w=14, N=4, vw_shift=1, hs=7, ws=9),
        Row("warp", _g(16, 4, 0, 16, False), C=16, G=4, D=12, h=2, w=2, N=1),
        Row("warp", _g(16, 4, 0, 16, True), C=16, G=4, D=16, h=13, w=11, far=True, **V),
        Row("warp", _g(16, 4, 0, 32, False), C=16, G=4, D=17, B=2, h=8, w=8, vw_shift=2, N=4),
        Row("warp", _g(16, 4, 0, 32, True), C=16, G=4, D=32, h=9, w=11, **V),
        Row("warp", _g(16, 4, 0, 64, False), C=16, G=4, D=33, h=5, w=5, far=True, **V),
        Row("warp", _g(16, 4, 0, 64, True), C=16, G=4, D=64, B=2, h=6, w=12, N=4, hs=5, ws=9, device_only=True),
    ]
    # -- pmn_warp_correlate with PixelwiseNet view weights: C 64 -> pixelwise_wave_kernel<2, D == 64> (8-pixel tiles); C 32 / 16 ->
    #    gather_corr_kernel<C, G, 1, 64, D == 64> --------------------------------------------------------------------------------------
    P = "pixelwise_wave_kernel"
    R += [
        Row("warp", f"{P}<2, false>", pixelwise=True, C=64, G=8, D=1, h=3, w=3, N=1),
        Row("warp", f"{P}<2, false>", pixelwise=True, C=64, G=8, D=48, B=2, h=7, w=9, N=4, far=True),
        Row("warp", f"{P}<2, false>", pixelwise=True, C=64, G=8, D=56, h=5, w=11, N=2, hs=4, ws=8),
        Row("warp", f"{P}<2, true>", pixelwise=True, C=64, G=8, D=64, h=9, w=6, N=2),
        Row("warp", f"{P}<2, true>", pixelwise=True, C=64, G=8, D=64, B=2, h=2, w=2, N=5),
        Row("warp", _g(32, 8, 1, 64, False), pixelwise=True, C=32, G=8, D=24, h=7, w=7, N=2),
        Row("warp", _g(32, 8, 1, 64, False), pixelwise=True, C=32, G=8, D=1, B=2, h=2, w=2, N=1),
        Row("warp", _g(32, 8, 1, 64, True), pixelwise=True, C=32, G=8, D=64, B=2, h=5, w=7, N=4, far=True, device_only=True),
        Row("warp", _g(16, 4, 1, 64, False), pixelwise=True, C=16, G=4, D=8, B=2, h=9, w=11, N=4, hs=6, ws=7),
        Row("warp", _g(16, 4, 1, 64, True), pixelwise=True, C=16, G=4, D=64, h=6, w=11, N=2, device_only=True),
    ]
    # -- pmn_aggregate_regress: K <= 9 -> KMAX 9, else 17.  KMAX 9 with D % 4 == 0: q4 kernel, DQ = D / 4 in {2,4,8,16} or generic 0
    #    (256 / DQ pixels per block); otherwise DL = 16 (D >= 32), 4 (D >= 16), 1 ------------------------------------------------------
    Q = "aggregate_regress_q4_kernel"
    A = "aggregate_regress_kernel"
    R += [
        Row("aggregate", f"{Q}<9, 2>", D=8, K=9, h=13, w=11, is_inverse=True),
        Row("aggregate", f"{Q}<9, 2>", D=8, K=9, B=2, h=16, w=9, big=True),
        Row("aggregate", f"{Q}<9, 4>", D=16, K=9, B=2, h=9, w=8),
        Row("aggregate", f"{Q}<9, 8>", D=32, K=9, h=7, w=5, big=True),
        Row("aggregate", f"{Q}<9, 8>", D=32, K=1, h=2, w=2),
        Row("aggregate", f"{Q}<9, 16>", D=64, K=9, B=2, h=5, w=6, is_inverse=True),
        Row("aggregate", f"{Q}<9, 16>", D=64, K=4, h=4, w=5, big=True),
        Row("aggregate", f"{Q}<9, 0>", D=4, K=9, h=11, w=13),
        Row("aggregate", f"{Q}<9, 0>", D=12, K=9, B=2, h=8, w=7, is_inverse=True),
        Row("aggregate", f"{Q}<9, 0>", D=60, K=9, h=3, w=7, big=True),
        Row("aggregate", f"{A}<9, 16>", D=33, K=9, h=5, w=7),
        Row("aggregate", f"{A}<9, 16>", D=63, K=9, B=2, h=4, w=5, big=True),
        Row("aggregate", f"{A}<9, 4>", D=17, K=9, h=9, w=9),
        Row("aggregate", f"{A}<9, 4>", D=31, K=9, B=2, h=7, w=6, is_inverse=True),
        Row("aggregate", f"{A}<9, 1>", D=1, K=9, h=6, w=7),
        Row("aggregate", f"{A}<9, 1>", D=2, K=9, h=5, w=5, is_inverse=True),
        Row("aggregate", f"{A}<9, 1>", D=15, K=9, B=2, h=2, w=2, big=True),
        Row("aggregate", f"{A}<17, 16>", D=32, K=17, h=6, w=11),
        Row("aggregate", f"{A}<17, 16>", D=64, K=17, B=2, h=5, w=7, is_inverse=True),
        Row("aggregate", f"{A}<17, 16>", D=48, K=17, h=4, w=9, big=True),
        Row("aggregate", f"{A}<17, 4>", D=16, K=17, B=2, h=7, w=7),
        Row("aggregate", f"{A}<17, 4>", D=31, K=10, h=9, w=5, big=True),
        Row("aggregate", f"{A}<17, 1>", D=1, K=17, h=3, w=5),
        Row("aggregate", f"{A}<17, 1>", D=2, K=17, B=2, h=5, w=4, is_inverse=True),
        Row("aggregate", f"{A}<17, 1>", D=15, K=17, h=7, w=9, big=True),
    ]
    # -- pmn_confidence: the 2x kernel at H, W = 2h, 2w, the general kernel elsewhere; pmn_normalize_depth -----------------------------
    C2, CG = "confidence2x_kernel", "confidence_kernel"
    R += [
        Row("confidence", C2, D=1, h=5, w=7, H=10, W=14),
        Row("confidence", C2, D=2, B=2, h=7, w=9, H=14, W=18),
        Row("confidence", C2, D=3, h=9, w=5, H=18, W=10),
        Row("confidence", C2, D=64, B=2, h=11, w=13, H=22, W=26),
        Row("confidence", CG, D=1, h=5, w=7, H=5, W=7),
        Row("confidence", CG, D=2, h=7, w=9, H=13, W=17),
        Row("confidence", CG, D=3, B=2, h=9, w=5, H=20, W=11),
        Row("confidence", CG, D=64, h=11, w=13, H=33, W=27),
        Row("normalize", "normalize_depth_kernel", B=2, h=17, w=19),
        Row("normalize", "normalize_depth_kernel", B=2, h=40, w=33),
    ]
    # -- the production warp on rigs that are not DTU (tests/camera_space.py): projections and depth samples of the rig at the row's
    #    map size.  `far`: their hypotheses leave the source image and fall behind it.  ring rows are 8 x 8 (see _rig_geometry);
    #    mixed rows have a source map smaller than the reference's, with source 0 in front of the reference looking back at it.
    #    (Appended after every other row: a row's seed is its place in the table, and the rows above keep theirs.)
    G = dict(far=True)
    R += [
        Row("warp", _g(64, 8, 0, 16, True), C=64, G=8, D=16, B=2, h=9, w=12, N=2, rig="unit", **G),
        Row("warp", _g(64, 8, 0, 16, False), C=64, G=8, D=12, h=7, w=10, N=2, rig="far_origin", **G),
        Row("warp", _g(64, 8, 0, 16, True), C=64, G=8, D=16, h=8, w=8, N=3, rig="ring", **G),
        Row("warp", _g(64, 8, 0, 16, False), C=64, G=8, D=9, B=2, h=9, w=12, N=1, rig="turned", **G),
        Row("warp", _g(64, 8, 0, 16, True), C=64, G=8, D=16, h=12, w=16, hs=6, ws=8, N=3, rig="mixed", **G),
        Row("warp", _g(64, 8, 0, 16, False), C=64, G=8, D=15, B=2, h=9, w=12, N=4, rig="wide", **G),
        Row("warp", f"{P}<2, true>", pixelwise=True, C=64, G=8, D=64, B=2, h=9, w=12, N=2, rig="unit", **G),
        Row("warp", f"{P}<2, false>", pixelwise=True, C=64, G=8, D=48, h=7, w=10, N=2, rig="far_origin", **G),
        Row("warp", f"{P}<2, true>", pixelwise=True, C=64, G=8, D=64, h=8, w=8, N=3, rig="ring", **G),
        Row("warp", f"{P}<2, false>", pixelwise=True, C=64, G=8, D=20, B=2, h=9, w=12, N=1, rig="turned", **G),
        Row("warp", f"{P}<2, false>", pixelwise=True, C=64, G=8, D=56, h=12, w=16, hs=6, ws=8, N=3, rig="mixed", **G),
        Row("warp", f"{P}<2, true>", pixelwise=True, C=64, G=8, D=64, B=2, h=9, w=12, N=4, rig="wide", **G),
    ]
    for rig, size in (("ring", dict(h=8, w=8)), ("mixed", dict(h=12, w=16, hs=6, ws=8))):
        R += [
            Row("warp", _g(32, 8, 0, 16, True), C=32, G=8, D=16, N=3, rig=rig, **size, **G),
            Row("warp", _g(16, 4, 0, 16, True), C=16, G=4, D=16, N=3, rig=rig, **size, **G),
            Row("warp", _g(32, 8, 1, 64, False), pixelwise=True, C=32, G=8, D=24, N=3, rig=rig, **size, **G),
            Row("warp", _g(16, 4, 1, 64, False), pixelwise=True, C=16, G=4, D=8, N=3, rig=rig, **size, **G),
        ]
    # distinct seeds so that no two rows share inputs
    return [replace(r, seed=100 * i + r.seed) for i, r in enumerate(R)]


ROWS: List[Row] = _rows()

# Compiled but unreachable through the C ABI (kept exact: tests/test_kernel_space.py fails when this list and the library disagree).
DEAD: Dict[str, str] = {
    _g(64, 8, 1, 64, False): "PixelwiseNet launches with C = 64, G = 8 always take pixelwise_wave_kernel (PMN_PW = 2)",
    _g(64, 8, 1, 64, True): "PixelwiseNet launches with C = 64, G = 8 always take pixelwise_wave_kernel (PMN_PW = 2)",
    _g(64, 8, 2, 32, False): "feature weight with DT = 32 means K > 16, and K <= 17 (PMN_MAX_NEIGHBORS) makes K = 17 the EXACT form",
    _g(32, 8, 2, 32, False): "feature weight with DT = 32 means K > 16, and K <= 17 (PMN_MAX_NEIGHBORS) makes K = 17 the EXACT form",
    _g(16, 4, 2, 32, False): "feature weight with DT = 32 means K > 16, and K <= 17 (PMN_MAX_NEIGHBORS) makes K = 17 the EXACT form",
}

# the kernel families behind the four hot-path entry points, with their (Itanium-mangled) parameter type
FAMILIES = {
    "gather_corr_kernel": "10GatherArgs",
    "pixelwise_wave_kernel": "10GatherArgs",
    "init_hypotheses_kernel": "7HypArgs",
    "init_hypotheses_fixed_kernel": "7HypArgs",
    "aggregate_regress_kernel": "7AggArgs",
    "aggregate_regress_q4_kernel": "7AggArgs",
}
OTHER_KERNELS = {  # pmn_confidence / pmn_normalize_depth: plain functions
    "confidence_kernel": "_Z17confidence_kernelPKfiiiiiPfPi",
    "confidence2x_kernel": "_Z19confidence2x_kernelPKfiiiPfPi",
    "normalize_depth_kernel": "_Z22normalize_depth_kernelPKfS0_S0_iPf",
}


def mangle(readable: str, families: Optional[Dict[str, str]] = None, others: Optional[Dict[str, str]] = None) -> str:
    """'gather_corr_kernel<64, 8, 0, 16, true>' -> '_Z18gather_corr_kernelILi64ELi8ELi0ELi16ELb1EEv10GatherArgs'.  ``families`` /
    ``others``: another table's kernel families and plain kernels (tests/conv_space.py); default: this module's."""
    FAMILIES, OTHER_KERNELS = (globals()["FAMILIES"] if families is None else families,
                               globals()["OTHER_KERNELS"] if others is None else others)
    if readable in OTHER_KERNELS:
        return OTHER_KERNELS[readable]
    name, args = readable.split("<", 1)
    targs = ""
    for a in args.rstrip(">").split(","):
        a = a.strip()
        targs += {"true": "Lb1E", "false": "Lb0E"}[a] if a in ("true", "false") else f"Li{int(a)}E"
    return f"_Z{len(name)}{name}I{targs}Ev{FAMILIES[name]}"


# ---- the library's instantiations, from its ELF dynamic symbol table -----------------------------------------------------------------

def dynamic_symbols(path: str) -> List[str]:
    """Names in the .dynsym section of an ELF64 little-endian shared object (stdlib only)."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:
        raise ValueError(f"{path}: not an ELF64 little-endian object")
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = []
    for _name, sh_type, _fl, _addr, off, size, link, _info, _al, entsize in sections:
        if sh_type != 11:  # SHT_DYNSYM
            continue
        stroff = sections[link][4]
        for j in range(size // entsize):
            st_name, = struct.unpack_from("<I", data, off + j * entsize)
            end = data.index(b"\0", stroff + st_name)
            names.append(data[stroff + st_name:end].decode())
    return names


def library_instantiations(path: str, families: Optional[Dict[str, str]] = None) -> Dict[str, str]:
    """{kernel symbol the launch plan records: host stub} for every kernel of ``families`` (default FAMILIES) the library compiles.  A `__global__` f has a
    host stub `_Z<n>__device_stub__f...`; the kernel itself is `_Z<n-15>f...` (the same mangling without the 15-character prefix).
    Raises when the library has no stubs at all (a stripped or foreign build must fail, not pass vacuously)."""
    out = {}
    pre = "__device_stub__"
    for s in dynamic_symbols(path):
        if pre not in s or not s.startswith("_Z"):
            continue
        digits = s[2:s.index(pre)]
        rest = s[s.index(pre) + len(pre):]
        kern = f"_Z{int(digits) - len(pre)}{rest}"
        out[kern] = s
    if not out:
        raise AssertionError(f"{path}: no __device_stub__ symbols in .dynsym")
    fams = FAMILIES if families is None else families
    return {k: v for k, v in out.items() if any(k.startswith(f"_Z{len(f)}{f}I") for f in fams)}


# ---- launch-plan recording (fake device addresses: recording validates arguments and dereferences no device pointer) ---------------

_FAKE = 0x100000


def buffers(row: Row, views: bool = False) -> List[Buf]:
    """The pointer arguments of the row's call: name (include/pmn_hip.h's), role, dtype and element count exactly as the header
    documents it.  ``views`` (warp rows): the call through pmn_warp_correlate_views, one buffer per source view and their table."""
    B, N, C, G, D, h, w = row.B, row.N, row.C, row.G, row.D, row.h, row.w
    F = lambda name, role, count, **kw: Buf(name, role, "float32", count, **kw)  # noqa: E731
    T = lambda name, K: Buf(name, "in", "int32", 2 * K, host=True)  # noqa: E731  host int[2K]: (dy, dx) pairs
    if row.op == "init":
        s = row.depth_shift
        return ([F("noise", "in", B * 48 * h * w)] if row.init == "noise" else [F("depth", "in", B * (h >> s) * (w >> s))]) + \
            [F("depth_min", "in", B), F("depth_max", "in", B)] + \
            ([F("propa_offsets", "in", B * 2 * row.propK * h * w), T("propa_table_host", row.propK)] if row.propK else []) + \
            [F("depth_sample", "out", B * D * h * w), F("xnorm", "out", B * h * w * D)]
    if row.op == "feature_weight":
        return [F("ref_nhwc", "in", B * h * w * C), F("eval_offsets", "in", B * 2 * D * h * w), T("eval_table_host", D),
                F("mlp", "weights", MLP_FLOATS),
                F("out_feature_weight", "out", B * D * h * w)]
    if row.op == "warp":
        hs, ws = row.hs or h, row.ws or w
        if views:
            names = tuple(f"src_view{v}" for v in range(N))
            src = [F(n, "in", B * hs * ws * C) for n in names] + [Buf("src_view_table", "in", "int64", N, table_of=names)]
        else:
            src = [F("src_nhwc", "in", N * B * hs * ws * C)]
        s = row.vw_shift
        return [F("ref_nhwc", "in", B * h * w * C)] + src + [F("rel_proj", "in", B * N * 16), F("depth_sample", "in", B * D * h * w)] + \
            ([] if row.pixelwise else [F("view_weights_in", "in", B * N * (h >> s) * (w >> s))]) + [F("similarity_mlp", "weights", MLP_FLOATS)] + \
            ([F("pixelwise_mlp", "weights", MLP_FLOATS)] if row.pixelwise else []) + [F("cost_out", "out", B * h * w * D)] + \
            ([F("view_weights_out", "out", B * N * h * w), Buf("vw_argmax_out", "out", "int32", B * N * h * w, optional=True)]
             if row.pixelwise else []) + [F("similarity_out", "out", B * G * D * h * w, optional=True)]
    if row.op == "aggregate":
        K = row.K
        return [F("cost", "in", B * h * w * D), F("depth_sample", "in", B * D * h * w), F("xnorm", "in", B * h * w * D),
                F("feature_weight", "in", B * K * h * w), F("eval_offsets", "in", B * 2 * K * h * w), T("eval_table_host", K),
                F("score_out", "out", B * D * h * w), F("depth_out", "out", B * h * w)]
    if row.op == "confidence":
        return [F("score", "in", B * D * h * w), F("confidence_out", "out", B * row.H * row.W),
                Buf("depth_index_out", "out", "int32", B * h * w, optional=True)]
    if row.op == "normalize":
        return [F("depth", "in", B * h * w), F("depth_min", "in", B), F("depth_max", "in", B), F("out", "out", B * h * w)]
    raise ValueError(row.op)


def arguments(row: Row, a: Dict[str, int], views: bool = False, interval_scale: float = 0.01) -> Tuple[str, list]:
    """The row's call through the C ABI with the addresses ``a`` (buffer name -> address; an absent name is NULL) -> (entry point, its
    full argument list).  ``interval_scale``: the one by-value argument that comes from the row's inputs (recording passes 0.01)."""
    g = a.get
    if row.op == "init":
        return "pmn_init_hypotheses", [g("noise"), g("depth"), row.depth_shift, a["depth_min"], a["depth_max"], row.num_sample,
                                       interval_scale, g("propa_offsets"), g("propa_table_host"), row.propK, row.B, row.h, row.w,
                                       a["depth_sample"], a["xnorm"], None]
    if row.op == "feature_weight":
        return "pmn_feature_weight", [a["ref_nhwc"], a["eval_offsets"], a["eval_table_host"], a["mlp"], row.B, row.C, row.G, row.D, row.h,
                                      row.w, a["out_feature_weight"], None]
    if row.op == "warp":
        hs, ws = row.hs or row.h, row.ws or row.w
        return "pmn_warp_correlate_views" if views else "pmn_warp_correlate", [
            a["ref_nhwc"], a["src_view_table" if views else "src_nhwc"], a["rel_proj"], a["depth_sample"], g("view_weights_in"), row.vw_shift,
            a["similarity_mlp"], g("pixelwise_mlp"), row.B, row.N, row.C, row.G, row.D, row.h, row.w, hs, ws, a["cost_out"],
            g("view_weights_out"), g("vw_argmax_out"), g("similarity_out"), None]
    if row.op == "aggregate":
        return "pmn_aggregate_regress", [a["cost"], a["depth_sample"], a["xnorm"], a["feature_weight"], a["eval_offsets"],
                                         a["eval_table_host"], row.K, interval_scale, int(row.is_inverse), row.B, row.D, row.h, row.w,
                                         a["score_out"], a["depth_out"], None]
    if row.op == "confidence":
        return "pmn_confidence", [a["score"], row.B, row.D, row.h, row.w, row.H, row.W, a["confidence_out"], g("depth_index_out"), None]
    if row.op == "normalize":
        return "pmn_normalize_depth", [a["depth"], a["depth_min"], a["depth_max"], row.B, row.h * row.w, a["out"], None]
    raise ValueError(row.op)


def host_tables(row: Row) -> Dict[str, np.ndarray]:
    """The row's host neighbour table under its argument's name: int32 [K,2] = the header's int[2K]."""
    name, K = {"init": ("propa_table_host", row.propK), "feature_weight": ("eval_table_host", row.D),
               "aggregate": ("eval_table_host", row.K)}.get(row.op, ("", 0))
    return {name: np.ascontiguousarray(neighbor_table(row, K), np.int32)} if K else {}


def record_call(L, fn: str, args: list) -> Tuple[int, List[str]]:
    """One entry-point call between pmn_plan_begin and pmn_plan_end -> (return code, recorded kernel names)."""
    p = ctypes.c_void_p()
    assert L.pmn_plan_create(ctypes.byref(p)) == 0
    assert L.pmn_plan_begin(p) == 0
    try:
        rc = getattr(L, fn)(*args)
    finally:
        assert L.pmn_plan_end(p) == 0
    names = [L.pmn_plan_kernel_name(p, i).decode() for i in range(L.pmn_plan_count(p))]
    L.pmn_plan_destroy(p)
    return rc, names


def record(row: Row, L=None) -> Tuple[int, List[str]]:
    """Records the row's call through pmn_plan_begin / pmn_plan_end -> (return code, recorded kernel names)."""
    from patchmatchnet_amd import _lib
    addr, held = recording_addresses(buffers(row), _FAKE, host_tables(row))  # (the neighbour table is read while recording)
    rc, names = record_call(L or _lib.lib(), *arguments(row, addr))
    del held
    return rc, names


# ---- inputs -------------------------------------------------------------------------------------------------------------------------

DEPTH_RANGES = ((425.0, 935.0), (2.0, 9.5))  # per sample: B = 2 rows use both


def depth_range(row: Row):
    lo = np.array([DEPTH_RANGES[b][0] for b in range(row.B)], np.float32)
    hi = np.array([DEPTH_RANGES[b][1] for b in range(row.B)], np.float32)
    return lo, hi


def neighbor_table(row: Row, K: int) -> np.ndarray:
    """[K,2] (dy, dx): the reference's tables for its own counts (propagation 4 / 8 / 16 at dilation 2, evaluation 9 / 17 at
    dilation 2), a seeded table of distinct offsets otherwise."""
    d = 2
    ring = [[-d, -d], [-d, 0], [-d, d], [0, -d], [0, d], [d, -d], [d, 0], [d, d]]
    e = d - 1
    nine = [[-e, -e], [-e, 0], [-e, e], [0, -e], [0, 0], [0, e], [e, -e], [e, 0], [e, e]]
    if row.op == "init" and K in (4, 8, 16):
        t = {4: [[-d, 0], [0, -d], [0, d], [d, 0]], 8: ring, 16: ring + [[2 * a, 2 * b] for a, b in ring]}[K]
    elif row.op != "init" and K == 9:
        t = nine
    elif row.op != "init" and K == 17:
        t = nine + [[2 * a, 2 * b] for a, b in nine if a or b]
    else:
        rng = np.random.default_rng(row.seed + 7)
        cand = [[a, b] for a in range(-3, 4) for b in range(-3, 4)]
        t = [cand[i] for i in rng.permutation(len(cand))[:K]]
    return np.asarray(t, np.int32)


def _smooth(rng, shape) -> np.ndarray:
    """Random feature maps [..., H, W, C] with a 3x3 box blur: texture at the scale of a pixel, but not i.i.d. noise."""
    x = rng.standard_normal(shape)
    H, W = shape[-3], shape[-2]
    p = np.pad(x, [(0, 0)] * (x.ndim - 3) + [(1, 1), (1, 1), (0, 0)], mode="edge")
    y = sum(p[..., i:i + H, j:j + W, :] for i in range(3) for j in range(3)) / 3.0
    return y.astype(np.float32)


def _projection(rng, row: Row, v: int) -> np.ndarray:
    """Relative projection src_proj @ inv(ref_proj) of one view: close to the identity rotation, a translation giving a parallax of
    ~1-4 px over the depth range [2, 8] (less on maps under 8 pixels).  ``far``: 5-20 px (1.5-6 px with a single view), and view 1
    gets a z-translation that puts the nearer hypotheses behind the source camera."""
    P = np.eye(4)
    P[:3, :3] += 0.003 * rng.standard_normal((3, 3))
    P[2, :2] = 1e-3 * rng.standard_normal(2)
    s = (40.0 if row.N > 1 else 12.0) if row.far else 8.0 * min(1.0, min(row.h, row.w) / 8.0)
    P[0, 3], P[1, 3] = rng.uniform(-s, s, 2)
    P[2, 3] = 0.05 * rng.standard_normal()
    if row.far and v == 1:
        P[2, 3] = -4.0  # z = d - 4: hypotheses with d < 4 lie behind the source camera
    return P.astype(np.float32)


RING_T = 4.5                    # depth of the ring rows' camera opposite the reference
RING_PZ = (1, 2, 3)             # planted hypotheses on the axis pixel: pz = k * 2**-12 (2.4e-4 .. 7.3e-4), between 0 and the front test


def _rig_geometry(row: Row):
    """rel_proj [B,N,4,4] and depth samples [B,D,h,w] of the row's rig (tests/camera_space.py): sample b % rig.B, its first N source
    views, intrinsics scaled to the row's h x w the way a stage scale would (rows 0 and 1 by w / W0 and h / H0), the reference's
    float32 sequence for the projections.

    ring rows: source 0 is the camera opposite the reference in its exact form -- on the axis at depth RING_T looking straight
    back, p = (-x d + cx T, (y - 2 cy) d + cy T, T - d) -- and the pixel on the axis (cx, cy) = (w / 2, h / 2) gets hypotheses at
    d = T - k 2**-12 in its first levels.  With cx, cy powers of two every operation of that chain is exact in float32, so these
    hypotheses sit at pz = k 2**-12 for the kernel and for float64 alike: behind the front test, and at the source's principal point
    for a front test at 0."""
    import camera_space as CS
    rig = CS.rigs()[row.rig]
    B, N, D, h, w = row.B, row.N, row.D, row.h, row.w
    assert N <= rig.V - 1
    intr = rig.intrinsics.copy()
    intr[:, :, 0] *= np.float32(w * rig.scale0 / CS.W_MAP)
    intr[:, :, 1] *= np.float32(h * rig.scale0 / CS.H_MAP)
    rel = CS.projections(rig, 1.0, np.float32, intr)
    rel_proj = np.stack([rel[b % rig.B, :N] for b in range(B)]).astype(np.float32)
    depth = np.stack([CS.hypotheses(rig, b % rig.B, D, h, w, seed=row.seed + b) for b in range(B)])
    if row.rig == "ring":
        cx, cy = w // 2, h // 2
        assert cx & (cx - 1) == 0 and cy & (cy - 1) == 0 and D > len(RING_PZ)
        T = RING_T
        rel_proj[:, 0] = np.float32([[-1, 0, 0, cx * T], [0, 1, -2 * cy, cy * T], [0, 0, -1, T], [0, 0, 0, 1]])
        for i, k in enumerate(RING_PZ):
            depth[:, i, cy, cx] = np.float32(T - k * 2.0 ** -12)
    return rel_proj, depth


def inputs(row: Row) -> Dict[str, np.ndarray]:
    """Seeded fp32 inputs of the row's call, in the layouts patchmatchnet_amd.ops takes."""
    rng = np.random.default_rng(row.seed)
    B, h, w = row.B, row.h, row.w
    dmin, dmax = depth_range(row)
    out: Dict[str, np.ndarray] = {"depth_min": dmin, "depth_max": dmax}
    if row.op == "init":
        if row.init == "noise":
            out["noise"] = rng.random((B, 48, h, w), dtype=np.float32)
        else:
            s = row.depth_shift
            u = rng.random((B, 1, h >> s, w >> s))
            out["depth"] = (dmin.reshape(-1, 1, 1, 1) + u * (dmax - dmin).reshape(-1, 1, 1, 1)).astype(np.float32)
        if row.propK:
            out["propa_offsets"] = (1.5 * rng.standard_normal((B, 2 * row.propK, h, w))).astype(np.float32)
            out["propa_table"] = neighbor_table(row, row.propK)
        out["interval_scale"] = np.float32([0.005, 0.0125, 0.025][row.seed % 3])
    elif row.op == "feature_weight":
        out["ref_nhwc"] = _smooth(rng, (B, h, w, row.C))
        out["eval_offsets"] = (1.5 * rng.standard_normal((B, 2 * row.D, h, w))).astype(np.float32)
        out["eval_table"] = neighbor_table(row, row.D)
    elif row.op == "warp":
        hs, ws = row.hs or h, row.ws or w
        out["ref_nhwc"] = _smooth(rng, (B, h, w, row.C))
        out["src_nhwc"] = _smooth(rng, (row.N, B, hs, ws, row.C))
        out["rel_proj"] = np.stack([np.stack([_projection(rng, row, v) for v in range(row.N)]) for _ in range(B)])
        out["depth_sample"] = rng.uniform(2.0, 8.0, (B, row.D, h, w)).astype(np.float32)
        if row.rig:
            out["rel_proj"], out["depth_sample"] = _rig_geometry(row)
        if not row.pixelwise:
            s = row.vw_shift
            out["view_weights"] = rng.uniform(0.05, 1.0, (B, row.N, h >> s, w >> s)).astype(np.float32)
    elif row.op == "aggregate":
        D, K = row.D, row.K
        if row.big:
            # beyond fp32 exp's range (|x| > 88.7 overflows, < -103 flushes to zero): only the max-subtracted softmax survives
            cost = rng.choice([-1.0, 1.0], (B, 1, 1, 1)) * rng.uniform(105.0, 125.0, (B, D, h, w))
        else:
            cost = 3.0 * rng.standard_normal((B, D, h, w))
        out["cost"] = cost.astype(np.float32)
        u = np.sort(rng.random((B, D, h, w)), axis=1)
        ds = (dmin.reshape(-1, 1, 1, 1) + u * (dmax - dmin).reshape(-1, 1, 1, 1)).astype(np.float32)
        out["depth_sample"] = ds
        one = np.float32(1.0)
        inv_min, inv_max = (one / dmin).reshape(-1, 1, 1, 1), (one / dmax).reshape(-1, 1, 1, 1)
        out["xnorm"] = ((one / ds - inv_max) / (inv_min - inv_max)).astype(np.float32)
        out["feature_weight"] = rng.uniform(0.05, 1.0, (B, K, h, w)).astype(np.float32)
        out["eval_offsets"] = (1.5 * rng.standard_normal((B, 2 * K, h, w))).astype(np.float32)
        out["eval_table"] = neighbor_table(row, K)
        out["interval_scale"] = np.float32([0.005, 0.0125, 0.025][row.seed % 3])
    elif row.op == "confidence":
        z = 2.0 * rng.standard_normal((B, row.D, h, w))
        e = np.exp(z - z.max(axis=1, keepdims=True))
        out["score"] = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    elif row.op == "normalize":
        u = rng.uniform(-0.1, 1.1, (B, 1, h, w))
        out["depth"] = (dmin.reshape(-1, 1, 1, 1) + u * (dmax - dmin).reshape(-1, 1, 1, 1)).astype(np.float32)
    return out


def nets(row: Row):
    """Seeded random (similarity, pixelwise, feature-weight) MLP modules for the row's group count, in eval mode: weights,
    BatchNorm affine parameters and running statistics all drawn (running_var > 0)."""
    import torch

    from patchmatchnet_amd.patchmatch import FeatureWeightNet, PixelwiseNet, SimilarityNet
    gen = torch.Generator().manual_seed(row.seed + 11)
    mods = (SimilarityNet(row.G), PixelwiseNet(row.G), FeatureWeightNet(max(row.D, 1), row.G))
    with torch.no_grad():
        for m in mods:
            for name, t in list(m.named_parameters()) + list(m.named_buffers()):
                if t.dtype != torch.float32:
                    continue
                if name.endswith("running_var"):
                    t.copy_(0.5 + torch.rand(t.shape, generator=gen))
                elif name.endswith("bn.weight"):
                    t.copy_(0.5 + torch.rand(t.shape, generator=gen))
                else:
                    t.copy_(0.5 * torch.randn(t.shape, generator=gen))
    return tuple(m.eval() for m in mods)


# ---- float64 expectations, tolerances and the errors of plausible kernel mistakes ---------------------------------------------------

# Output -> (tolerance, metric).  The kernel-level thresholds tests/test_hip_parity.py::test_kernels_against_golden holds
# (hypotheses 2e-6 relative, similarity 3e-5, view weights 1e-5, feature weight 2e-5, score 2e-4, depth 2e-5 relative); xnorm in
# [0, 1] absolute; cost (the SimilarityNet output, tens of units) relative to max(|ref|, 1), at 5e-4: fp32 evaluation of the MLP with
# the released weights is 2.1e-4 from float64 on the golden similarity (tests/test_kernel_space.py).
TOL = {
    "depth_sample": (2e-6, "rel"),
    "xnorm": (2e-6, "abs"),
    "similarity": (3e-5, "abs"),
    "view_weights": (1e-5, "abs"),
    "cost": (5e-4, "scaled"),
    "feature_weight": (2e-5, "abs"),
    "score": (2e-4, "abs"),
    "depth": (2e-5, "rel"),
    "confidence": (1e-6, "abs"),
    "normalized": (1e-6, "scaled"),
}


def error(key: str, got, ref) -> float:
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return float("inf")
    d = np.abs(got - ref)
    metric = TOL[key][1]
    if metric == "rel":
        d = d / np.abs(ref)
    elif metric == "scaled":
        d = d / np.maximum(np.abs(ref), 1.0)
    d = np.where(np.isnan(d), np.inf, d)
    return float(d.max()) if d.size else 0.0


def _planar_src(x) -> List[np.ndarray]:
    return [s.transpose(0, 3, 1, 2) for s in x["src_nhwc"]]


def reference(row: Row, x: Dict[str, np.ndarray], mlps=None) -> Dict[str, np.ndarray]:
    """ref64's outputs for the row's call (the keys of TOL the call produces; warp also returns 'responses' [B,N,D,h,w])."""
    import ref64 as R
    if row.op == "init":
        ds, xn = R.init_hypotheses(x.get("noise"), x.get("depth"), row.depth_shift, x["depth_min"], x["depth_max"], row.num_sample,
                                   float(x["interval_scale"]), x.get("propa_offsets"), x.get("propa_table"), row.h, row.w)
        return {"depth_sample": ds, "xnorm": xn}
    if row.op == "feature_weight":
        return {"feature_weight": R.feature_weight(x["ref_nhwc"].transpose(0, 3, 1, 2), x["eval_offsets"], x["eval_table"], mlps[2],
                                                   row.G)}
    if row.op == "warp":
        r = R.warp_correlate(x["ref_nhwc"].transpose(0, 3, 1, 2), _planar_src(x), x["rel_proj"], x["depth_sample"],
                             x.get("view_weights"), row.vw_shift, mlps[0], mlps[1], row.G)
        return r
    if row.op == "aggregate":
        score, depth, _ = R.aggregate_regress(x["cost"], x["depth_sample"], x["xnorm"], x["feature_weight"], x["eval_offsets"],
                                              x["eval_table"], float(x["interval_scale"]), row.is_inverse)
        return {"score": score, "depth": depth}
    if row.op == "confidence":
        conf, idx, idxf = R.confidence(x["score"], row.H, row.W)
        return {"confidence": conf, "depth_index": idx, "index_float": idxf}
    if row.op == "normalize":
        return {"normalized": R.normalize_depth(x["depth"], x["depth_min"], x["depth_max"])}
    raise ValueError(row.op)


def _tail(a: np.ndarray) -> np.ndarray:
    """The output with its last pixel never written (zero): what a wrong tail guard / tile count leaves."""
    a = np.array(a, np.float64, copy=True)
    a[..., -1, -1] = 0.0
    return a


def mistakes(row: Row, x: Dict[str, np.ndarray], ref: Dict[str, np.ndarray], mlps=None) -> Dict[str, Tuple[str, np.ndarray]]:
    """name -> (output key, what ref64 gives for that output when the computation makes one plausible kernel mistake)."""
    import ref64 as R
    out: Dict[str, Tuple[str, np.ndarray]] = {}
    B = row.B
    roll = lambda a: np.roll(a, 1, axis=0)  # noqa: E731  sample b reads sample b-1's data (a batch stride / index mistake)
    if row.op == "init":
        out["tail pixel unwritten"] = ("depth_sample", _tail(ref["depth_sample"]))
        if B > 1:
            y = dict(x, depth_min=roll(x["depth_min"]), depth_max=roll(x["depth_max"]))
            if row.init == "noise" or row.num_sample > 1:  # (one sample around a previous depth does not read the range)
                out["depth range of the other sample"] = ("depth_sample", reference(row, y)["depth_sample"])
            out["xnorm with the other sample's range"] = ("xnorm", R.xnorm_of(ref["depth_sample"], y["depth_min"], y["depth_max"]))
        if row.propK:
            y = dict(x, propa_offsets=x["propa_offsets"].reshape(B, -1, 2, row.h, row.w)[:, :, ::-1].reshape(x["propa_offsets"].shape))
            out["x / y offsets swapped"] = ("depth_sample", reference(row, y)["depth_sample"])
        if row.init == "noise":
            y = dict(x, noise=np.roll(x["noise"], 1, axis=1))
            out["noise plane of the neighbouring bin"] = ("depth_sample", reference(row, y)["depth_sample"])
        elif row.num_sample > 1:
            y = dict(x, interval_scale=np.float32(x["interval_scale"] * 0.5))
            out["half the sampling interval"] = ("depth_sample", reference(row, y)["depth_sample"])
    elif row.op == "feature_weight":
        fw = ref["feature_weight"]
        out["tail pixel unwritten"] = ("feature_weight", _tail(fw))
        y = dict(x, eval_offsets=x["eval_offsets"].reshape(B, -1, 2, row.h, row.w)[:, :, ::-1].reshape(x["eval_offsets"].shape))
        out["x / y offsets swapped"] = ("feature_weight", reference(row, y, mlps)["feature_weight"])
        y = dict(x, eval_table=np.zeros_like(x["eval_table"]))
        out["fixed neighbour table ignored"] = ("feature_weight", reference(row, y, mlps)["feature_weight"])
        if row.D == 17:
            t = x["eval_table"].copy()
            t[9:] = t[np.r_[0:4, 5:9]]
            out["9-neighbour table where 17 was asked"] = ("feature_weight", reference(row, dict(x, eval_table=t), mlps)["feature_weight"])
    elif row.op == "warp":
        sim = ref["similarity"]
        out["tail pixel unwritten"] = ("cost", _tail(ref["cost"]))
        if row.D > 1:
            s = sim.copy()
            s[:, :, -1] = 0.0
            out["last hypothesis dropped"] = ("similarity", s)
        if row.N > 1:
            y = dict(x, src_nhwc=x["src_nhwc"][:-1], rel_proj=x["rel_proj"][:, :-1])
            if "view_weights" in x:
                y["view_weights"] = x["view_weights"][:, :-1]
            out["last view dropped"] = ("similarity", reference(replace(row, N=row.N - 1), y, mlps)["similarity"])
        if B > 1:
            out["projection of the other sample"] = ("similarity", reference(row, dict(x, rel_proj=roll(x["rel_proj"])), mlps)["similarity"])
        if row.vw_shift:
            s = row.vw_shift
            vw = x["view_weights"]
            ys = np.minimum(np.arange(row.h) >> (s - 1), vw.shape[2] - 1)
            xs = np.minimum(np.arange(row.w) >> (s - 1), vw.shape[3] - 1)
            full = np.ascontiguousarray(vw[:, :, ys][:, :, :, xs])  # index (y >> (s-1), x >> (s-1)): one shift too few
            r = reference(replace(row, vw_shift=0), dict(x, view_weights=full), mlps)
            out["view weights read one level too fine"] = ("similarity", r["similarity"])
        if (row.hs or row.h) != row.h or (row.ws or row.w) != row.w:
            r = R.warp_correlate(x["ref_nhwc"].transpose(0, 3, 1, 2), [np.pad(s, ((0, 0), (0, 0), (0, row.h - s.shape[2]),
                                                                                  (0, row.w - s.shape[3]))) for s in _planar_src(x)],
                                 x["rel_proj"], x["depth_sample"], x.get("view_weights"), row.vw_shift, mlps[0], mlps[1], row.G)
            out["reference size used for the source map"] = ("similarity", r["similarity"])
        if row.rig and (row.hs or row.h) < row.h:
            kw = {"sentinel": (min(row.w, row.ws or row.w) - 1, min(row.h, row.hs or row.h) - 1)}
            r = R.warp_correlate(x["ref_nhwc"].transpose(0, 3, 1, 2), _planar_src(x), x["rel_proj"], x["depth_sample"],
                                 x.get("view_weights"), row.vw_shift, mlps[0], mlps[1], row.G, warp_kw=kw)
            out["sentinel of a behind-camera hypothesis lands inside a smaller source map"] = ("similarity", r["similarity"])
        if row.rig == "ring":
            r = R.warp_correlate(x["ref_nhwc"].transpose(0, 3, 1, 2), _planar_src(x), x["rel_proj"], x["depth_sample"],
                                 x.get("view_weights"), row.vw_shift, mlps[0], mlps[1], row.G, warp_kw={"front_eps": 0.0})
            out["front test at 0 instead of 1e-3"] = ("similarity", r["similarity"])
        if row.pixelwise and row.D > 1:
            out["view weight of the first hypothesis, not the max"] = ("view_weights", ref["responses"][:, :, 0])
    elif row.op == "aggregate":
        out["tail pixel unwritten"] = ("depth", _tail(ref["depth"]))
        if row.D > 1:
            sc, dp, pre = R.aggregate_regress(x["cost"], x["depth_sample"], x["xnorm"], x["feature_weight"], x["eval_offsets"],
                                              x["eval_table"], float(x["interval_scale"]), row.is_inverse)
            p = R.softmax(pre[:, :-1])
            out["last hypothesis dropped"] = ("depth", R.regress(x["depth_sample"][:, :-1], p, row.is_inverse) if row.D > 2 else
                                              np.asarray(x["depth_sample"][:, 0], np.float64))
        if row.K == 17 and row.D > 1:  # (one hypothesis: the score is 1 whatever the neighbours)
            y = dict(x, eval_table=x["eval_table"][:9], eval_offsets=x["eval_offsets"][:, :18], feature_weight=x["feature_weight"][:, :9])
            r = reference(replace(row, K=9), y)
            out["9-neighbour table where 17 was asked"] = ("score", r["score"])
        if B > 1:
            r = reference(row, dict(x, feature_weight=roll(x["feature_weight"])))
            out["feature weight of the other sample"] = ("score", r["score"])
        if row.is_inverse:
            out["linear instead of inverse-depth regression"] = ("depth", reference(replace(row, is_inverse=False), x)["depth"])
        if row.big:
            _, _, pre = R.aggregate_regress(x["cost"], x["depth_sample"], x["xnorm"], x["feature_weight"], x["eval_offsets"],
                                            x["eval_table"], float(x["interval_scale"]), row.is_inverse)
            with np.errstate(over="ignore", invalid="ignore"):
                e = np.exp(pre.astype(np.float32))
                out["softmax without max-subtraction (fp32)"] = ("score", (e / e.sum(axis=1, keepdims=True)).astype(np.float64))
    elif row.op == "confidence":
        out["tail pixel unwritten"] = ("confidence", _tail(ref["confidence"]))
        if row.D > 4:  # (up to 4 hypotheses the window always holds all of them)
            sc = np.concatenate([x["score"][:, 1:], np.zeros_like(x["score"][:, :1])], axis=1)  # window idx .. idx+3
            c = R.confidence(x["score"], row.H, row.W)
            s = np.asarray(x["score"], np.float64)
            pad = np.concatenate([s, np.zeros((B, 4) + s.shape[2:])], axis=1)
            win = sum(np.take_along_axis(pad, (c[1] + j)[:, None], axis=1)[:, 0] for j in range(4))
            ys = np.minimum(np.floor(np.arange(row.H) * (row.h / row.H)).astype(np.int64), row.h - 1)
            xs = np.minimum(np.floor(np.arange(row.W) * (row.w / row.W)).astype(np.int64), row.w - 1)
            del sc
            out["window shifted by one"] = ("confidence", win[:, ys][:, :, xs])
    elif row.op == "normalize":
        out["tail pixel unwritten"] = ("normalized", _tail(ref["normalized"]))
        out["depth range of the other sample"] = ("normalized", R.normalize_depth(x["depth"], roll(x["depth_min"]), roll(x["depth_max"])))
    return out


# ---- the row through the raw C ABI between guard bands (tests/guard_band.py) ------------------------------------------------------------

# output buffer -> the key of reference() that holds the same elements
REF_KEY = {"depth_sample": "depth_sample", "xnorm": "xnorm", "out_feature_weight": "feature_weight", "cost_out": "cost",
           "view_weights_out": "view_weights", "vw_argmax_out": "view_weights", "similarity_out": "similarity", "score_out": "score",
           "depth_out": "depth", "confidence_out": "confidence", "depth_index_out": "depth_index", "out": "normalized"}


def payloads(row: Row, x: Dict[str, np.ndarray], mlps, views: bool = False) -> Dict[str, np.ndarray]:
    """The host array behind every input and weight buffer of buffers(row, views), in the layout the C ABI reads: inputs(row)'s
    arrays, cost and xnorm hypothesis-last, the packed MLP blocks, the host neighbour table, the source views one by one for the
    table entry."""
    last = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))  # noqa: E731
    p = dict(x, **host_tables(row))
    if row.op == "feature_weight":
        p["mlp"] = mlps[2].packed()
    elif row.op == "warp":
        p.update({f"src_view{v}": s for v, s in enumerate(x["src_nhwc"])}, similarity_mlp=mlps[0].packed(), pixelwise_mlp=mlps[1].packed(),
                 view_weights_in=x.get("view_weights"))
    elif row.op == "aggregate":
        p.update(cost=last(x["cost"]), xnorm=last(x["xnorm"]))
    return {b.name: p[b.name] for b in buffers(row, views) if b.role != "out" and not b.table_of}


def ops_outputs(row: Row, x: Dict[str, np.ndarray], mlps, views: bool = False, dev: str = "cuda:0") -> Dict[str, np.ndarray]:
    """The row through patchmatchnet_amd.ops on ordinary tensors -> every output buffer of buffers(row) as the array its storage holds."""
    import torch

    import patchmatchnet_amd as P
    ops = P.ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    n = lambda v: v.contiguous().cpu().numpy()  # noqa: E731
    last = lambda v: n(v.permute(0, 2, 3, 1))  # noqa: E731  hypothesis-last storage behind a [B,D,h,w] view
    with torch.no_grad():
        if row.op == "init":
            ds, xn = ops.init_hypotheses(t(x["noise"]) if "noise" in x else None, t(x["depth"]) if "depth" in x else None, row.depth_shift,
                                         t(x["depth_min"]), t(x["depth_max"]), row.num_sample, float(x["interval_scale"]),
                                         t(x["propa_offsets"]) if row.propK else None, x.get("propa_table"), row.h, row.w)
            out = {"depth_sample": n(ds), "xnorm": last(xn)}
        elif row.op == "feature_weight":
            out = {"out_feature_weight": n(ops.feature_weight(t(x["ref_nhwc"]), t(x["eval_offsets"]), x["eval_table"], t(mlps[2].packed()),
                                                              row.G))}
        elif row.op == "warp":
            src = t(x["src_nhwc"])
            held = [src[v].clone() for v in range(row.N)] if views else None
            if views:
                src = ops.SourceTable(torch.tensor([m.data_ptr() for m in held], dtype=torch.int64, device=dev), src.shape)
            cost, vw, am, sim = ops.warp_correlate(t(x["ref_nhwc"]), src, t(x["rel_proj"]), t(x["depth_sample"]),
                                                   t(x["view_weights"]) if "view_weights" in x else None, row.vw_shift, t(mlps[0].packed()),
                                                   t(mlps[1].packed()) if row.pixelwise else None, row.G, want_similarity=True,
                                                   want_argmax=row.pixelwise)
            out = {"cost_out": last(cost), "similarity_out": n(sim)}
            if row.pixelwise:
                out.update(view_weights_out=n(vw), vw_argmax_out=n(am))
        elif row.op == "aggregate":
            score, dep = ops.aggregate_regress(t(x["cost"]), t(x["depth_sample"]), t(x["xnorm"]), t(x["feature_weight"]), t(x["eval_offsets"]),
                                               x["eval_table"], float(x["interval_scale"]), row.is_inverse)
            out = {"score_out": n(score), "depth_out": n(dep)}
        elif row.op == "confidence":
            conf, idx = ops.confidence(t(x["score"]), row.H, row.W, want_index=True)
            out = {"confidence_out": n(conf), "depth_index_out": n(idx)}
        elif row.op == "normalize":
            out = {"out": n(ops.normalize_depth(t(x["depth"]), t(x["depth_min"]), t(x["depth_max"])))}
        else:
            raise ValueError(row.op)
        torch.cuda.synchronize()
    return out


def run_guard(row: Row, views: bool = False, dev: str = "cuda:0") -> None:
    """The row through the raw C ABI on ``dev`` with every buffer between guard bands, then guard_band.check: no band touched, no
    input changed, every output the bytes of the ops wrapper's."""
    import torch

    import guard_band as GB
    from patchmatchnet_amd import _lib
    x, mlps = inputs(row), nets(row)
    want = ops_outputs(row, x, mlps, views, dev)
    arenas = GB.build(buffers(row, views), payloads(row, x, mlps, views), dev)
    fn, args = arguments(row, {k: a.ptr for k, a in arenas.items()}, views, float(x.get("interval_scale", 0.01)))
    with torch.cuda.device(dev):
        rc = getattr(_lib.lib(), fn)(*args)
        torch.cuda.synchronize()
    assert rc == 0, (fn, rc)
    GB.check(arenas, want)
