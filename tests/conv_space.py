"""The convolution kernel space: one row per call of the convolution-side entry points (pmn_conv2d, pmn_conv2d_mfma, pmn_conv2d_f16s,
pmn_conv2d_f16s_pair, pmn_offset_heads_f16s, pmn_fpn_level, pmn_fpn_tail, pmn_deconv3x3s2, pmn_stem, pmn_stem_f16s,
pmn_stem_f16s_views, pmn_stem_conv2_f16s, pmn_stem_conv2_f16s_views, pmn_refine_front, pmn_refine_tail, pmn_refine_fused), each naming
the kernel instantiation its shape selects.
Rows use the smallest shapes at which these kernels can go wrong: 1x1 (2x2 where the ABI wants even sizes) and 3x5 images, exactly
one tile / one pixel short / one past (16x16; 16x32 for the f16s stem; 14x14 for the pair kernel; 16x16 half-resolution outputs =
32x32 input pixels for the fused conv0 + conv1 + conv2 kernel), odd and even sizes under stride 2,
tile counts below, at and past the 8-way pmn_xcd_tile remap with N = 1, 2, 3, offset heads on images smaller than their dilation,
relu 0 and 1, BatchNorm-folded and bias-only weights, image bases off by one float, two depth ranges.  Every row fits in 64x64
pixels; the two conv_kernel<..., TP = 4, ...> rows need N*Ho*Wo >= 1,500,000 (launch_conv in csrc/conv.hip: `pix >= 1500000L`): the
cin = 1 row is THE large row (1 x 1200 x 1250 = exactly the threshold, Wo % 4 == 2); the cin = 3 instantiation can be reached by no
smaller workload either, so it gets a second row of that size, 379 images of 64x62 (1,503,872 pixels).

Plain helper module (no tests here): tests/test_conv_space.py checks the table on the CPU, tests/test_conv_space_gpu.py runs every
row on the device against tests/conv_ref64.py, tests/test_guard_band_gpu.py runs every row through the raw C ABI between guard
bands (buffers(), arguments(), run_guard() below)."""
from __future__ import annotations

import functools
import json
import os
import subprocess
import sys
import zlib
from dataclasses import dataclass, replace
from typing import Dict, List, Tuple

import numpy as np

import conv_ref64 as R
import kernel_space as KS
from guard_band import Buf, recording_addresses

Env = Tuple[Tuple[str, str], ...]
E_S0C8: Env = (("PMN_CONV_CC5", "8"), ("PMN_CONV_SPLIT", "0"))
E_C8: Env = (("PMN_CONV_CC5", "8"),)
# conv_tiled_kernel<32, 4, 64, 64, 5, 2, false, false> needs PMN_CONV_SPLIT=0 with PMN_CONV_CC5 unset (pmn_conv2d: `cc5 == 4 && K == 5`
# after the split64 == 32 block is skipped): a third environment, so the device test starts three child processes, not two.
E_S0: Env = (("PMN_CONV_SPLIT", "0"),)
ENVS = (E_S0C8, E_C8, E_S0)


@dataclass(frozen=True)
class Row:
    op: str                  # conv2d | mfma1x1 | f16s | pair | heads | fpn_level | fpn_tail | deconv | stem | stem_f16s | stem_views |
    #                          stem_conv2 | stem_conv2_views | refine_front | refine_tail | refine_fused
    kernel: str              # the instantiation this row selects (readable form; mangle() gives the symbol)
    N: int = 1
    H: int = 16              # input size (deconv: the half-resolution input; refine: the full-resolution output)
    W: int = 16
    cin: int = 0
    cout: int = 0
    K: int = 3
    S: int = 1
    pad: int = 1
    dil: int = 1
    relu: int = 1
    bn: bool = True          # BatchNorm-folded weights (False: bias only)
    ca: int = 0              # split outputs: channels of the first
    up: bool = False         # an x2 bilinearly up-sampled map is added
    nchw_in: bool = False
    planar: bool = False     # planar [N,C,H,W] output
    misalign: bool = False   # image base off by one float: the scalar-staging kernel, same bits as the aligned call
    views: int = 0           # stem_views, stem_conv2_views: N = views * B
    env: Env = ()            # PMN_CONV_SPLIT / PMN_CONV_CC5 of the process that runs the row (read once per process)
    large: bool = False      # the one large row
    res_max: float = 0.0     # refine_tail / refine_fused: conv3 and res weights are scaled so that max |res| is this, in normalised depth
    device_only: bool = False  # > 48 KB of dynamic LDS: recording needs a device
    seed: int = 0

    @property
    def id(self) -> str:
        k = self.kernel.replace(" ", "").replace("true", "T").replace("false", "F")
        e = "".join(f"-{a[4:]}{b}" for a, b in self.env)
        return f"{self.op}-{k}-{self.N}x{self.H}x{self.W}{'-mis' if self.misalign else ''}{e}-s{self.seed}"


def _b(v: bool) -> str:
    return "true" if v else "false"


def _t(cin, cc, co, cop, k, s, planar=False, up=False) -> str:
    return f"conv_tiled_kernel<{cin}, {cc}, {co}, {cop}, {k}, {s}, {_b(planar)}, {_b(up)}>"


# (H, W, N).  First half: 1x1, 3x5, one tile, one short, a strip.  Second half: one past (4 tiles x 2 = 8), 18 = 8 * 2 + 2 tiles,
# 12 tiles, 8 tiles, tall (8 tiles).  A kernel's rows alternate between the halves (add() below).
SZ = [(1, 1, 1), (3, 5, 2), (16, 16, 1), (15, 15, 3), (7, 40, 1), (17, 17, 2), (17, 33, 3), (33, 49, 1), (32, 64, 1), (64, 9, 2)]
SZ_EVEN = [(2, 2, 1), (16, 16, 1), (14, 14, 3), (6, 40, 2), (18, 18, 2), (18, 34, 3), (34, 50, 1), (32, 64, 1)]


def _key(op, kernel, env=(), misalign=False) -> str:
    return f"{op}|{kernel}|{env}|{int(misalign)}"


def _rows() -> List[Row]:
    rows: List[Row] = []
    count: Dict[str, int] = {}

    def add(op, kernel, sizes=SZ, n=1, **kw):
        """n rows of one kernel.  Sizes, relu and BatchNorm / bias come from a hash of the kernel and the row's index j among that
        kernel's rows, never from its place in the table, so an edit elsewhere leaves them alone: sizes alternate between the two
        halves of ``sizes`` (an image of at most a tile, then one of several tiles), relu alternates with j, bn with j // 2."""
        key = _key(op, kernel, kw.get("env", ()))
        h = zlib.crc32(key.encode())
        half = len(sizes) // 2
        for _ in range(n):
            j = count.get(key, 0)
            count[key] = j + 1
            H, W, N = sizes[(h + half * (j % 2) + j // 2) % len(sizes)]
            d = dict(H=H, W=W, N=N, relu=((h >> 8) + j) % 2, bn=((h >> 9) + j // 2) % 2 == 0)
            d.update(kw)
            rows.append(Row(op, kernel, **d))

    # ---- pmn_conv2d: conv_kernel (planar image in, 8 channels out); TP = 4 from N*Ho*Wo >= 1,500,000 (launch_conv) -------------------
    add("conv2d", "conv_kernel<3, 8, 3, 1, 2, true, false>", n=3, cin=3, cout=8, nchw_in=True)
    add("conv2d", "conv_kernel<1, 8, 3, 1, 2, true, false>", n=3, cin=1, cout=8, nchw_in=True)
    rows.append(Row("conv2d", "conv_kernel<1, 8, 3, 1, 4, true, false>", N=1, H=1200, W=1250, cin=1, cout=8, nchw_in=True, large=True))
    rows.append(Row("conv2d", "conv_kernel<3, 8, 3, 1, 4, true, false>", N=379, H=64, W=62, cin=3, cout=8, nchw_in=True, relu=0, bn=False))
    # ---- pmn_conv2d: conv_tiled_kernel, the 3x3 / 5x5 stride 2 / 1x1 layers ----------------------------------------------------------
    for cin, cout, cc in ((8, 8, 8), (16, 8, 16), (16, 16, 16), (32, 32, 16)):
        add("conv2d", _t(cin, cc, cout, cout, 3, 1), n=2, cin=cin, cout=cout)
    add("conv2d", _t(64, 16, 32, 64, 3, 1), n=2, cin=64, cout=64)
    add("conv2d", _t(64, 16, 64, 64, 3, 1), n=2, cin=64, cout=64, env=E_S0C8)
    L5 = dict(K=5, S=2, pad=2)
    add("conv2d", _t(8, 4, 16, 16, 5, 2), n=2, cin=8, cout=16, **L5)
    add("conv2d", _t(16, 4, 32, 32, 5, 2), n=2, cin=16, cout=32, **L5)
    add("conv2d", _t(32, 4, 32, 64, 5, 2), n=2, cin=32, cout=64, **L5)
    add("conv2d", _t(8, 8, 16, 16, 5, 2), n=2, cin=8, cout=16, env=E_C8, device_only=True, **L5)
    add("conv2d", _t(16, 8, 32, 32, 5, 2), n=2, cin=16, cout=32, env=E_C8, device_only=True, **L5)
    add("conv2d", _t(32, 8, 32, 64, 5, 2), n=2, cin=32, cout=64, env=E_C8, device_only=True, **L5)
    add("conv2d", _t(32, 8, 64, 64, 5, 2), n=2, cin=32, cout=64, env=E_S0C8, device_only=True, **L5)
    add("conv2d", _t(32, 4, 64, 64, 5, 2), n=1, cin=32, cout=64, env=E_S0, **L5)
    P1 = dict(K=1, pad=0)
    for cin, cout in ((16, 64), (32, 64), (64, 32), (64, 16)):
        add("conv2d", _t(cin, 16, cout, cout, 1, 1), n=2, cin=cin, cout=cout, **P1)
    add("conv2d", _t(64, 16, 32, 64, 1, 1), n=2, cin=64, cout=64, **P1)
    add("conv2d", _t(64, 16, 64, 64, 1, 1), n=2, cin=64, cout=64, env=E_S0C8, **P1)
    for cin in (16, 32, 64):  # the FPN lateral form: two blocks of 32 channels, bilinear x2 of `up` seeds the accumulators
        add("conv2d", _t(cin, 16, 32, 64, 1, 1, up=True), sizes=SZ_EVEN, n=2, cin=cin, cout=64, up=True, bn=False, **P1)
    # ---- pmn_conv2d: the planar offset-head forms, every (cin, COUTP) of the dispatch; dilation as the cascade uses it -----------------
    for cin, dil in ((64, 2), (32, 4), (16, 6)):
        for cp, cout in ((8, 2), (16, 10), (32, 18), (48, 34)):
            add("conv2d", _t(cin, 8, min(cp, 16), cp, 3, 1, planar=True), n=2 if cp == 32 else 1, cin=cin, cout=cout, pad=dil, dil=dil,
                planar=True, relu=0, bn=False)
    add("conv2d", _t(8, 8, 8, 8, 3, 1, planar=True), n=2, cin=8, cout=1, planar=True, relu=0, bn=False)
    # ---- pmn_conv2d_mfma: the product library carries the split 1x1 form alone (conv_mfma.hip, #ifndef PMN_EXPERIMENTAL) --------------
    add("mfma1x1", "conv_mfma_kernel<64, 32, 128, 1, 1, 1, 4, 1, 4, false>", n=3, cin=64, cout=112, ca=64, K=1, pad=0, relu=0, bn=False)
    add("mfma1x1", "conv_mfma_kernel<64, 32, 128, 1, 1, 1, 4, 1, 4, false>", n=2, cin=64, cout=128, ca=16, K=1, pad=0, relu=0, bn=False)
    # ---- pmn_conv2d_f16s: all six layers (tiles 16 wide x 16 or 8 rows) ---------------------------------------------------------------
    F = "conv_f16s_kernel"
    add("f16s", f"{F}<16, 16, 3, 1, 16, 16, 4, 4, 1, 0, true>", n=3, cin=16, cout=16)
    add("f16s", f"{F}<32, 32, 3, 1, 16, 16, 2, 4, 1, 0, false>", n=3, cin=32, cout=32)
    add("f16s", f"{F}<64, 64, 3, 1, 16, 16, 2, 3, 1, 0, true>", n=3, cin=64, cout=64)
    add("f16s", f"{F}<8, 16, 5, 2, 8, 8, 2, 4, 1, 0, true>", n=3, cin=8, cout=16, **L5)
    add("f16s", f"{F}<16, 32, 5, 2, 8, 8, 2, 4, 1, 0, false>", n=3, cin=16, cout=32, **L5)
    add("f16s", f"{F}<32, 64, 5, 2, 16, 24, 2, 2, 1, 0, true>", n=3, cin=32, cout=64, device_only=True, **L5)
    # ---- pmn_conv2d_f16s_pair: 14x14 tiles --------------------------------------------------------------------------------------------
    for H, W, N in ((1, 1, 1), (3, 5, 2), (14, 14, 1), (13, 13, 3), (15, 15, 2), (15, 29, 3), (29, 43, 1)):
        rows.append(Row("pair", "conv_f16s_pair16_kernel<4>", N=N, H=H, W=W, cin=16, cout=16, relu=1 if (H + N) % 2 else 0))
    # ---- pmn_offset_heads_f16s: (cin, dil) x coutp 32 / 48 / 64, ca == cout and ca < cout; images smaller than the dilation -----------
    for cin, dil, wps in ((64, 2, 3), (32, 4, 4), (16, 6, 4)):
        for cp, cout, ca in ((32, 18, 18), (32, 32, 16), (48, 34, 16), (48, 48, 48), (64, 50, 32), (64, 64, 64)):
            add("heads", f"{F}<{cin}, {cp}, 3, 1, 16, 16, 2, {min(wps, 3) if cp == 64 else wps}, {dil}, 1, false>", cin=cin, cout=cout,
                ca=ca, pad=dil, dil=dil, relu=0, bn=False)
    # ---- pmn_fpn_level / pmn_fpn_tail / pmn_deconv3x3s2 / pmn_stem ----------------------------------------------------------------------
    add("fpn_level", "fpn_level_kernel<64, 112, 64, false>", n=4, cin=64, cout=112, ca=64, device_only=True)
    add("fpn_level", "fpn_level_kernel<32, 48, 32, true>", sizes=SZ_EVEN, n=4, cin=32, cout=48, ca=32, up=True, device_only=True)
    add("fpn_level", "fpn_level_kernel<16, 16, 16, true>", sizes=SZ_EVEN, n=4, cin=16, cout=16, ca=16, up=True)
    add("fpn_tail", "fpn_tail_kernel<16, 64, 16>", sizes=SZ_EVEN, n=5, cin=16, cout=16, up=True)
    add("deconv", "deconv3x3s2_kernel<8, 8>", n=6, cin=8, cout=8)
    add("stem", "stem_kernel", n=7, cin=3, cout=8, relu=1, bn=True)
    # ---- pmn_stem_f16s (tiles 16 wide x 32 rows): VEC4 staging with W % 4 == 0 and an aligned base, scalar otherwise ----------------
    SV, SS = "stem_f16s_kernel<true, 32>", "stem_f16s_kernel<false, 32>"
    for H, W, N in ((1, 4, 1), (32, 16, 1), (33, 20, 2), (31, 12, 3), (40, 32, 1)):
        rows.append(Row("stem_f16s", SV, N=N, H=H, W=W, cin=3, cout=8))
    for H, W, N in ((1, 1, 1), (3, 5, 2), (31, 15, 3), (33, 17, 2), (64, 9, 1)):
        rows.append(Row("stem_f16s", SS, N=N, H=H, W=W, cin=3, cout=8))
    for H, W, N in ((32, 16, 1), (33, 20, 2)):
        rows.append(Row("stem_f16s", SS, N=N, H=H, W=W, cin=3, cout=8, misalign=True))
    rows.append(Row("stem_views", SV, N=6, views=3, H=33, W=20, cin=3, cout=8))
    rows.append(Row("stem_views", SS, N=2, views=2, H=17, W=15, cin=3, cout=8))
    # ---- pmn_stem_conv2_f16s[_views]: conv0 + conv1 + conv2 in one launch.  A workgroup is 16 x 16 half-resolution outputs = 32 x 32
    #      input pixels; 81 KB of dynamic LDS, so the rows are device_only.  Sizes are the full-resolution input.  <true>: 1x4 the
    #      smallest; 32x32 exactly one tile; 30x32 one output row short of it; 34x36 x 2 one past it both ways = 2 * 2 * 2 = 8 workgroups,
    #      the pmn_xcd_tile boundary; 64x64 = 4, below it; 64x40 x 3 = 12, past it and no multiple of 8.  <false>: 1x1; 3x5 x 2; 31x31 =
    #      16 x 16 outputs whose last stride-2 taps fall off the image; 33x33 x 2 = 8 workgroups; 63x9 a tall strip; 34x35 x 3 = 12.
    #      BatchNorm-folded and bias-only weights (all three layers) alternate with the row's index among its kernel's rows, from
    #      the hash add() uses ---------------------------------------------------------------------------------------------------------
    C2V, C2S = "stem_f16s_kernel_conv2<true>", "stem_f16s_kernel_conv2<false>"
    nth2: Dict[str, int] = {}

    def conv2_row(op, kernel, H, W, N, **kw):
        key = _key(op, kernel, (), kw.get("misalign", False))
        j = nth2[key] = nth2.get(key, -1) + 1
        rows.append(Row(op, kernel, N=N, H=H, W=W, cin=3, cout=16, K=5, S=2, pad=2, device_only=True,
                        bn=((zlib.crc32(key.encode()) >> 9) + j) % 2 == 0, **kw))

    for H, W, N in ((1, 4, 1), (32, 32, 1), (30, 32, 1), (34, 36, 2), (64, 64, 1), (64, 40, 3)):
        conv2_row("stem_conv2", C2V, H, W, N)
    for H, W, N in ((1, 1, 1), (3, 5, 2), (31, 31, 1), (33, 33, 2), (63, 9, 1), (34, 35, 3)):
        conv2_row("stem_conv2", C2S, H, W, N)
    for H, W, N in ((32, 32, 1), (34, 36, 2)):
        conv2_row("stem_conv2", C2S, H, W, N, misalign=True)
    # (views, B): 3 x 2 with the images allocated apart and in an order unrelated to the view index (run_device); 2 x 1 through the
    # scalar staging; 2 x 2 at 3x4, where every pixel is a border pixel of all three layers
    conv2_row("stem_conv2_views", C2V, 33, 20, 6, views=3)
    conv2_row("stem_conv2_views", C2S, 17, 15, 2, views=2)
    conv2_row("stem_conv2_views", C2V, 3, 4, 4, views=2)
    # ---- Refinement: B = 2 rows use both depth ranges (kernel_space.DEPTH_RANGES); every refine_tail / refine_fused row carries
    #      res_max = 0.25 (set below): case() scales the res weights so that max |res| is 0.25 in normalised depth units, inside
    #      [0.05, 0.5], so the residual is NOT small against dnorm in [0, 1] ----------------------------------------------------------
    RS = ((2, 2, 1), (16, 16, 2), (14, 14, 2), (18, 18, 1), (18, 34, 2), (34, 50, 1), (32, 64, 2), (6, 40, 2))
    for H, W, N in RS:
        rows.append(Row("refine_front", "refine_front_kernel", N=N, H=H, W=W, cin=3, cout=16))
    for H, W, N in RS:
        rows.append(Row("refine_tail", "refine_tail_kernel", N=N, H=H, W=W, cin=16, cout=1, device_only=True))
    for H, W, N in RS:
        rows.append(Row("refine_fused", f"refine_fused_kernel<{_b(W % 4 == 0)}>", N=N, H=H, W=W, cin=3, cout=1, device_only=True))
    for H, W, N in ((16, 16, 2), (32, 64, 2), (6, 40, 1)):
        rows.append(Row("refine_fused", "refine_fused_kernel<false>", N=N, H=H, W=W, cin=3, cout=1, device_only=True, misalign=True))
    rows.append(Row("fpn_tail", "fpn_tail_kernel<16, 64, 16>", N=1, H=2, W=2, cin=16, cout=16, up=True))
    rows.append(Row("stem", "stem_kernel", N=1, H=1, W=1, cin=3, cout=8))
    rows.append(Row("stem", "stem_kernel", N=2, H=3, W=5, cin=3, cout=8))
    out, nth = [], {}
    for r in rows:  # the seed too: a hash of the kernel and the row's index among that kernel's rows
        key = _key(r.op, r.kernel, r.env, r.misalign)
        j = nth[key] = nth.get(key, -1) + 1
        out.append(replace(r, seed=zlib.crc32(f"{key}|{j}".encode()) % 100000,
                           res_max=0.25 if r.op in ("refine_tail", "refine_fused") else 0.0))
    assert len({r.id for r in out}) == len(out)
    return out


ROWS: List[Row] = _rows()

# Compiled but unreachable through the C ABI (exact: tests/test_conv_space.py fails when this list and the library disagree).  Empty:
# every instantiation of the families below that libpmn_hip.so compiles is selected by some row.  (pmn_conv2d_mfma's layer forms and
# its planar dilated form are compiled into the research build only -- conv_mfma.hip, #ifndef PMN_EXPERIMENTAL -- so the product
# library has nothing of them to reach.)
DEAD: Dict[str, str] = {}

FAMILIES = {
    "conv_kernel": "PKfS1_S1_S1_Pf8ConvArgs",
    "conv_tiled_kernel": "PKfS1_S1_S1_Pf8ConvArgs",
    "conv_mfma_kernel": "PKfPK15HIP_vector_typeIfLj4EES1_PfS6_12MfmaConvArgs",
    "conv_f16s_kernel": "PKfPKDv8_DF16_S1_Pf8F16sArgs",
    "conv_f16s_pair16_kernel": "PKfPKDv8_DF16_S1_S4_S1_Pf8F16sArgs",
    "fpn_level_kernel": "PKfS1_S1_S1_PfS2_iii",
    "fpn_tail_kernel": "PKfS1_S1_S1_S1_Pfiii",
    "deconv3x3s2_kernel": "PKfS1_S1_Pfiiii",
    "stem_f16s_kernel": "PKfS1_S1_PKDv8_DF16_S1_PfiiiPKS1_i",
    "stem_f16s_kernel_conv2": "PKfS1_S1_PKDv8_DF16_S1_S4_S1_PfiiiiiPKS1_i",
    "refine_fused_kernel": "PKfS1_S1_S1_S1_S1_PKDv8_DF16_S1_S1_S1_S1_S1_Pfiii",
}
OTHER_KERNELS = {
    "stem_kernel": "_Z11stem_kernelPKfS0_S0_S0_S0_Pfiii",
    "refine_front_kernel": "_Z19refine_front_kernelPKfS0_S0_S0_S0_S0_Pfiii",
    "refine_tail_kernel": "_Z18refine_tail_kernelPKfS0_S0_S0_S0_S0_S0_Pfiii",
}


def mangle(readable: str) -> str:
    return KS.mangle(readable, FAMILIES, OTHER_KERNELS)


STEM_CONV2 = ("stem_conv2", "stem_conv2_views")  # input H x W -> output (H - 1) // 2 + 1 x (W - 1) // 2 + 1 x 16 (K = 5, S = 2, pad = 2)


def out_hw(row: Row) -> Tuple[int, int]:
    if row.op == "deconv":
        return 2 * row.H, 2 * row.W
    f = lambda n: (n + 2 * row.pad - row.dil * (row.K - 1) - 1) // row.S + 1  # noqa: E731
    return (f(row.H), f(row.W)) if row.op in ("conv2d", "mfma1x1", "f16s", "heads") + STEM_CONV2 else (row.H, row.W)


# ---- launch-plan recording ---------------------------------------------------------------------------------------------------------

# op -> (entry point, its pointer arguments in the header's order and by the header's names).  The table entries take `views` after
# the table; the images a table points to are buffers of the call (img0, img1, ...) but no arguments of it.
_STEM = ("w0", "s0", "w1a", "s1")
_FRONT = ("t2", "w0", "s0", "wd", "sd")
_TAIL = ("wr", "dnorm", "depth_min", "depth_max", "out")
ABI = {
    "conv2d": ("pmn_conv2d", ("in", "weights", "shift", "up", "out")),
    "mfma1x1": ("pmn_conv2d_mfma", ("in", "weights", "shift", "out", "out_b")),
    "f16s": ("pmn_conv2d_f16s", ("in", "weights", "shift", "out")),
    "pair": ("pmn_conv2d_f16s_pair", ("in", "weights_a", "shift_a", "weights_b", "shift_b", "out")),
    "heads": ("pmn_offset_heads_f16s", ("in", "weights", "shift", "out_a", "out_b")),
    "fpn_level": ("pmn_fpn_level", ("x", "u", "w", "b", "out_a", "out_b")),
    "fpn_tail": ("pmn_fpn_tail", ("x", "up", "w_in", "b_in", "w_out", "out")),
    "deconv": ("pmn_deconv3x3s2", ("in", "weights", "shift", "out")),
    "stem": ("pmn_stem", ("img", "w0", "s0", "w1", "s1", "out")),
    "stem_f16s": ("pmn_stem_f16s", ("img",) + _STEM + ("out",)),
    "stem_views": ("pmn_stem_f16s_views", ("img_table",) + _STEM + ("out",)),
    "stem_conv2": ("pmn_stem_conv2_f16s", ("img",) + _STEM + ("w2b", "s2", "out")),
    "stem_conv2_views": ("pmn_stem_conv2_f16s_views", ("img_table",) + _STEM + ("w2b", "s2", "out")),
    "refine_front": ("pmn_refine_front", ("img",) + _FRONT + ("x16",)),
    "refine_tail": ("pmn_refine_tail", ("x16", "w3", "s3") + _TAIL),
    "refine_fused": ("pmn_refine_fused", ("img",) + _FRONT + ("w3a", "s3") + _TAIL),
}


def buffers(row: Row) -> List[Buf]:
    """The buffers of the row's call: name (include/pmn_hip.h's), role, dtype and element count exactly as the header documents it,
    padded pack layouts included and nothing more."""
    from patchmatchnet_amd import params
    N, H, W, cin, cout, ca, K = row.N, row.H, row.W, row.cin, row.cout, row.ca, row.K
    Ho, Wo = out_hw(row)
    up = lambda c, m: -(-c // m) * m  # noqa: E731
    I = lambda name, count, **kw: Buf(name, "in", "float32", count, **kw)  # noqa: E731,E741
    P = lambda name, count, dtype="float32": Buf(name, "weights", dtype, count)  # noqa: E731
    O = lambda name, count: Buf(name, "out", "float32", count)  # noqa: E731,E741
    op = row.op
    img = I("img", N * 3 * H * W, misalign=row.misalign)
    stem = [P("w0", 3 * 3 * 3 * 8), P("s0", 8), P("w1a", 3 * 2 * 64 * 8, "float16"), P("s1", 8)]
    conv2 = [P("w2b", 1 * 7 * 1 * 2 * 64 * 8, "float16"), P("s2", 16)]
    front = [I("t2", N * (H // 2) * (W // 2) * 8), P("w0", 3 * 3 * 3 * 8), P("s0", 8), P("wd", 3 * 3 * 8 * 8), P("sd", 8)]
    tail = [P("wr", 3 * 3 * 8), I("dnorm", N * (H // 2) * (W // 2)), I("depth_min", N), I("depth_max", N), O("out", N * H * W)]
    if op == "conv2d":  # weights [K][K][cin][coutp], coutp = cout rounded up to 8 (cout <= 8) or to a multiple of 16
        cp = 8 if cout <= 8 else up(cout, 16)
        return [I("in", N * cin * H * W), P("weights", K * K * cin * cp), P("shift", cp)] + \
            ([I("up", N * (Ho // 2) * (Wo // 2) * cout)] if row.up else []) + [O("out", N * Ho * Wo * cout)]
    if op == "mfma1x1":  # weights [K*K][cin/8][coutp/32][64][4], coutp = cout rounded up to 32
        cp = up(cout, 32)
        return [I("in", N * H * W * 64), P("weights", (64 // 8) * (cp // 32) * 64 * 4), P("shift", cp), O("out", N * H * W * ca),
                O("out_b", N * H * W * (cout - ca))]
    if op == "f16s":  # weights float16 [cin/CC][k-steps][cout/16][2][64][8], k-steps = K*K*(CC/8) blocks of 8 channels, four per step
        CC = params.f16s_chunk(cin, K)
        return [I("in", N * H * W * cin), P("weights", (cin // CC) * up(K * K * (CC // 8), 4) // 4 * (cout // 16) * 2 * 64 * 8, "float16"),
                P("shift", cout), O("out", N * Ho * Wo * cout)]
    if op == "pair":  # two (k 3, stride 1, 16 -> 16) layers as pmn_conv2d_f16s takes them: [1][5][1][2][64][8]
        return [I("in", N * H * W * 16), P("weights_a", 5 * 2 * 64 * 8, "float16"), P("shift_a", 16), P("weights_b", 5 * 2 * 64 * 8, "float16"),
                P("shift_b", 16), O("out", N * H * W * 16)]
    if op == "heads":  # weights float16 [cin/16][k-steps][coutp/16][2][64][8], coutp = cout rounded up to 16; 9 taps x 2 blocks = 5 steps
        cp = up(cout, 16)
        return [I("in", N * H * W * cin), P("weights", (cin // 16) * 5 * (cp // 16) * 2 * 64 * 8, "float16"), P("shift", cp),
                O("out_a", N * ca * H * W)] + ([O("out_b", N * (cout - ca) * H * W)] if ca < cout else [])
    if op == "fpn_level":
        return [I("x", N * H * W * cin)] + ([I("u", N * (H // 2) * (W // 2) * cout)] if row.up else []) + \
            [P("w", cin * cout), P("b", cout), O("out_a", N * H * W * ca)] + ([O("out_b", N * H * W * (cout - ca))] if ca < cout else [])
    if op == "fpn_tail":
        return [I("x", N * H * W * 16), I("up", N * (H // 2) * (W // 2) * 64), P("w_in", 16 * 64), P("b_in", 64), P("w_out", 64 * 16),
                O("out", N * H * W * 16)]
    if op == "deconv":
        return [I("in", N * H * W * 8), P("weights", 3 * 3 * 8 * 8), P("shift", 8), O("out", N * 2 * H * 2 * W * 8)]
    if op == "stem":
        return [img, P("w0", 3 * 3 * 3 * 8), P("s0", 8), P("w1", 3 * 3 * 8 * 8), P("s1", 8), O("out", N * H * W * 8)]
    if op == "stem_f16s":
        return [img] + stem + [O("out", N * H * W * 8)]
    if op == "stem_conv2":
        return [img] + stem + conv2 + [O("out", N * Ho * Wo * 16)]
    if op in ("stem_views", "stem_conv2_views"):  # a device table of `views` addresses, entry v = a dense [B,3,H,W] image of its own
        names = tuple(f"img{v}" for v in range(row.views))
        return [Buf("img_table", "in", "int64", row.views, table_of=names)] + [I(n, (N // row.views) * 3 * H * W) for n in names] + stem + \
            (conv2 + [O("out", N * Ho * Wo * 16)] if op == "stem_conv2_views" else [O("out", N * H * W * 8)])
    if op == "refine_front":
        return [img] + front + [O("x16", N * H * W * 16)]
    if op == "refine_tail":  # w3 [2][3][3][16][4]
        return [I("x16", N * H * W * 16), P("w3", 2 * 3 * 3 * 16 * 4), P("s3", 8)] + tail
    if op == "refine_fused":  # w3a float16 [5][2][64][8]
        return [img] + front + [P("w3a", 5 * 2 * 64 * 8, "float16"), P("s3", 8)] + tail
    raise ValueError(op)


def arguments(row: Row, a: Dict[str, int]) -> Tuple[str, list]:
    """The row's call through the C ABI with the addresses ``a`` (buffer name -> address; an absent name is NULL) -> (entry point, its
    full argument list)."""
    N, H, W = row.N, row.H, row.W
    fn, names = ABI[row.op]
    ptrs = [a.get(n) for n in names]
    if row.op == "conv2d":
        Ho, Wo = out_hw(row)
        tail = [N, H, W, row.cin, row.cout, row.K, row.S, row.pad, row.dil, row.relu, int(row.nchw_in), int(row.planar),
                Ho // 2 if row.up else 0, Wo // 2 if row.up else 0]
    elif row.op == "mfma1x1":
        tail = [N, H, W, 64, row.cout, row.ca, 1, 1, 0, 1, row.relu, 0]
    elif row.op == "f16s":
        tail = [N, H, W, row.cin, row.cout, row.K, row.S, row.relu]
    elif row.op == "pair":
        tail = [N, H, W, 16, row.relu]
    elif row.op == "heads":
        tail = [N, H, W, row.cin, row.cout, row.ca, row.dil]
    elif row.op == "fpn_level":
        tail = [N, H, W, row.cin, row.cout, row.ca]
    elif row.op == "fpn_tail":
        tail = [N, H, W, 16, 64, 16]
    elif row.op == "deconv":
        tail = [N, H, W, 8, 8, row.relu]
    elif row.op in ("stem_views", "stem_conv2_views"):
        ptrs.insert(1, row.views)
        tail = [N // row.views, H, W]
    else:
        tail = [N, H, W]
    return fn, ptrs + tail + [None]


def record(row: Row, L=None) -> Tuple[int, List[str]]:
    """Records the row's call in THIS process (whatever its environment) -> (return code, recorded kernel names)."""
    from patchmatchnet_amd import _lib
    addr, _ = recording_addresses(buffers(row), 0x100000, {})  # (no host buffers on this side)
    return KS.record_call(L or _lib.lib(), *arguments(row, addr))


def child(env: Env, what: str, timeout: float) -> subprocess.CompletedProcess:
    """A fresh interpreter with ``env`` set that runs conv_space.child_main(what) (the variables are read once per process)."""
    here = os.path.dirname(os.path.abspath(__file__))
    e = {k: v for k, v in os.environ.items() if k not in ("PMN_CONV_SPLIT", "PMN_CONV_CC5")}
    e.update(dict(env))
    e["PYTHONPATH"] = os.pathsep.join([here, os.path.dirname(here)] + ([e["PYTHONPATH"]] if e.get("PYTHONPATH") else []))
    code = f"import conv_space as C; C.child_main({what!r}, {tuple(env)!r})"
    return subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=timeout)


def child_main(what: str, env: Env) -> None:
    out = {}
    for row in ROWS:
        if row.env != tuple(env):
            continue
        if what == "record":
            out[row.id] = record(row)
        elif what == "guard":  # (an AssertionError of guard_band.check ends the child with its message and a non-zero code)
            run_guard(row)
            out[row.id] = "ok"
        else:
            rc, names = record(row)
            got, errs = run_device(row), {}
            ref = reference(row)
            errs = {"rc": rc, "names": names, "err": error(row, got, ref)}
            out[row.id] = errs
    print("CONV_SPACE_JSON " + json.dumps(out))


@functools.lru_cache(maxsize=None)
def record_env(env: Env) -> Dict[str, Tuple[int, List[str]]]:
    r = child(env, "record", 300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CONV_SPACE_JSON ")][-1]
    return {k: (v[0], v[1]) for k, v in json.loads(line[len("CONV_SPACE_JSON "):]).items()}


# ---- weights and inputs (seeded; float32 as the kernels get them) ------------------------------------------------------------------

def _layer(rng, cout, cin, K, bn, transposed=False):
    shape = (cin, cout, K, K) if transposed else (cout, cin, K, K)
    d = {"w": (rng.standard_normal(shape) * (1.5 / np.sqrt(cin * K * K))).astype(np.float32)}
    if bn:
        d["bn"] = tuple(a.astype(np.float32) for a in (0.5 + rng.random(cout), 0.3 * rng.standard_normal(cout), 0.3 * rng.standard_normal(cout),
                                                       0.5 + rng.random(cout)))
    else:
        d["bias"] = (0.3 * rng.standard_normal(cout)).astype(np.float32)
    return d


@functools.lru_cache(maxsize=8)
def case(row: Row) -> Dict:
    """The row's unpacked weights and inputs: planar float32 arrays (x [N,C,H,W]); dicts w / bn / bias per layer."""
    rng = np.random.default_rng(1000 + row.seed)
    N, H, W = row.N, row.H, row.W
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    c: Dict = {}
    if row.op in ("conv2d", "mfma1x1", "f16s", "heads"):
        c["x"] = f(N, row.cin, H, W)
        c["l"] = _layer(rng, row.cout, row.cin, row.K, row.bn)
        if not row.relu:  # relu = 0 must show: a tiny image whose outputs are all positive gets the layer negated
            l = c["l"]
            if R.conv_bn(c["x"], l["w"], l.get("bn"), l.get("bias"), **_conv_kw(row))[0].min() > -0.1:
                if "bn" in l:
                    l["bn"] = (-l["bn"][0], -l["bn"][1]) + l["bn"][2:]
                else:
                    l["w"], l["bias"] = -l["w"], -l["bias"]
        if row.up:
            Ho, Wo = out_hw(row)
            c["u"] = f(N, row.cout, Ho // 2, Wo // 2)
    elif row.op == "pair":
        c["x"] = f(N, 16, H, W)
        c["la"], c["lb"] = _layer(rng, 16, 16, 3, True), _layer(rng, 16, 16, 3, True)
    elif row.op == "fpn_level":
        c["x"] = f(N, row.cin, H, W)
        c["w"] = (rng.standard_normal((row.cin, row.cout)) / np.sqrt(row.cin)).astype(np.float32)
        c["b"] = (0.3 * rng.standard_normal(row.cout)).astype(np.float32)
        if row.up:
            c["u"] = f(N, row.cout, H // 2, W // 2)
    elif row.op == "fpn_tail":
        c["x"], c["u"] = f(N, 16, H, W), f(N, 64, H // 2, W // 2)
        c["inner"], c["outer"] = _layer(rng, 64, 16, 1, False), {"w": (rng.standard_normal((16, 64, 1, 1)) / 8.0).astype(np.float32)}
    elif row.op == "deconv":
        c["x"] = f(N, 8, H, W)
        c["l"] = _layer(rng, 8, 8, 3, row.bn, transposed=True)
    elif row.op in ("stem", "stem_f16s", "stem_views"):
        c["x"] = rng.random((N, 3, H, W)).astype(np.float32) * 2 - 1
        c["la"], c["lb"] = _layer(rng, 8, 3, 3, True), _layer(rng, 8, 8, 3, True)
    elif row.op in STEM_CONV2:  # BatchNorm or bias on all three layers: a nonzero shift each, so ReLU(shift) != 0 outside the image
        c["x"] = rng.random((N, 3, H, W)).astype(np.float32) * 2 - 1
        c["la"], c["lb"], c["lc"] = _layer(rng, 8, 3, 3, row.bn), _layer(rng, 8, 8, 3, row.bn), _layer(rng, 16, 8, 5, row.bn)
    elif row.op.startswith("refine"):
        lo = np.array([KS.DEPTH_RANGES[b % 2][0] for b in range(N)], np.float32)
        hi = np.array([KS.DEPTH_RANGES[b % 2][1] for b in range(N)], np.float32)
        c.update(dmin=lo, dmax=hi, img=rng.random((N, 3, H, W)).astype(np.float32) * 2 - 1, t2=np.maximum(f(N, 8, H // 2, W // 2), 0),
                 dnorm=rng.random((N, 1, H // 2, W // 2)).astype(np.float32), c0=_layer(rng, 8, 3, 3, True),
                 dc=_layer(rng, 8, 8, 3, True, transposed=True), c3=_layer(rng, 8, 16, 3, True))
        c["x16"] = np.maximum(f(N, 16, H, W), 0)
        wr = rng.standard_normal((1, 8, 3, 3))
        x16 = c["x16"] if row.op == "refine_tail" else R.refine_front(c["img"], c["t2"], c["c0"], c["dc"])[0]
        m, _ = R.conv_bn(x16, c["c3"]["w"], c["c3"]["bn"], relu=True, pad=1)
        res, _ = R.conv2d(m, wr, pad=1)
        c["wr"] = (wr * ((row.res_max or 0.25) / np.abs(res).max())).astype(np.float32)  # max |res| = row.res_max (refine_front: unused)
    return c


def _conv_kw(row: Row) -> Dict:
    return dict(stride=row.S, pad=row.pad, dil=row.dil)


def reference(row: Row, **mk) -> Dict[str, np.ndarray]:
    """conv_ref64's outputs of the row: y (planar float64) and A, its magnitude bound; refine rows: depth, norm, res.  Keyword
    arguments select one kernel mistake (conv_ref64's)."""
    c = case(row)
    relu = bool(row.relu)
    if row.op in ("conv2d", "mfma1x1", "f16s", "heads"):
        ac = mk.pop("align_corners", False)
        force_relu = mk.pop("force_relu", False)
        y, A = R.conv_bn(c["x"], c["l"]["w"], c["l"].get("bn"), c["l"].get("bias"), relu=False, **_conv_kw(row), **mk)
        if row.up:
            u = R.bilinear2(c["u"], ac)
            y, A = y + u, A + np.abs(u)
        return {"y": np.maximum(y, 0) if relu or force_relu else y, "A": A}
    if row.op == "pair":
        y, A = R.chain2(c["x"], c["la"], c["lb"], relu=relu or mk.pop("force_relu", False), **mk)
    elif row.op in ("stem", "stem_f16s", "stem_views"):
        y, A = R.chain2(c["x"], c["la"], c["lb"], relu=True, **mk)
    elif row.op in STEM_CONV2:
        x = c["x"]
        if mk.pop("swap_view_batch", False):  # image n read at table entry n % views, sample n // views (n = view * B + sample is right)
            V, B = row.views, row.N // row.views
            x = x[[(n % V) * B + n // V for n in range(row.N)]]
        y, A = R.chain3(x, c["la"], c["lb"], c["lc"], **mk)
    elif row.op == "fpn_level":
        y, A = R.fpn_level(c["x"], c.get("u"), c["w"], c["b"], **mk)
    elif row.op == "fpn_tail":
        y, A = R.fpn_tail(c["x"], c["u"], c["inner"]["w"], c["inner"]["bias"], c["outer"]["w"], **mk)
    elif row.op == "deconv":
        force_relu = mk.pop("force_relu", False)
        y, A = R.deconv_bn(c["x"], c["l"]["w"], c["l"].get("bn"), relu=relu or force_relu, **mk)
    elif row.op == "refine_front":
        y, A = R.refine_front(c["img"], c["t2"], c["c0"], c["dc"], **mk)
    elif row.op == "refine_tail":
        return R.refine_tail(c["x16"], c["c3"], c["wr"], c["dnorm"], c["dmin"], c["dmax"], **mk)
    elif row.op == "refine_fused":
        return R.refine_fused(c["img"], c["t2"], c["c0"], c["dc"], c["c3"], c["wr"], c["dnorm"], c["dmin"], c["dmax"], **mk)
    else:
        raise ValueError(row.op)
    return {"y": y, "A": A}


# ---- error metrics, families and tolerances --------------------------------------------------------------------------------------------

METRIC = {"conv2d": "single", "mfma1x1": "single", "f16s": "single", "heads": "single", "fpn_level": "single", "deconv": "single",
          "refine_front": "single", "pair": "fused", "stem": "fused", "stem_f16s": "fused", "stem_views": "fused", "fpn_tail": "fused",
          "stem_conv2": "fused", "stem_conv2_views": "fused",
          "refine_tail": "refine", "refine_fused": "refine"}
F16S_OPS = ("f16s", "pair", "heads", "stem_f16s", "stem_views", "stem_conv2", "stem_conv2_views", "refine_fused")


def family(row: Row) -> str:
    if row.op == "conv2d":
        return row.kernel.split("<")[0]
    return "stem_f16s" if row.op == "stem_views" else "stem_conv2" if row.op == "stem_conv2_views" else row.op


def error(row: Row, got, ref: Dict[str, np.ndarray]) -> float:
    """single-layer rows: max |got - ref| / A element-wise; fused rows: per output channel, max error over the channel's max magnitude;
    refine rows: normalised depth (out - min) / span, error over the row's max |res|."""
    got = np.asarray(got, np.float64)
    m = METRIC[row.op]
    if m == "refine":
        c = case(row)
        lo, hi = R.f64(c["dmin"]).reshape(-1, 1, 1, 1), R.f64(c["dmax"]).reshape(-1, 1, 1, 1)
        if got.shape != ref["depth"].shape:
            return float("inf")
        d = np.abs((got - lo) / (hi - lo) - ref["norm"]) / np.abs(ref["res"]).max()
    else:
        y = ref["y"]
        if got.shape != y.shape:
            return float("inf")
        d = np.abs(got - y)
        if m == "single":
            d = d / np.maximum(ref["A"], 1e-30)
        else:
            d = d.max(axis=(0, 2, 3)) / np.maximum(np.abs(y).max(axis=(0, 2, 3)), 1e-30)
    d = np.where(np.isnan(d), np.inf, d)
    return float(d.max())


# family -> tolerance.  fp32 kernels: 8 x the largest error, over the family's rows, of a torch CPU float32 evaluation of the row layer by
# layer against conv_ref64 in the row's metric (the margin covers another accumulation order and FMA contraction).  Split-fp16 kernels: 4 x
# the largest error of the emulation of their arithmetic (conv_ref64.f16s_conv; fp32 stages in torch float32), which leaves accumulation
# order alone.  tests/test_conv_space.py re-measures and asserts margin x measured <= TOL.  MEASURED holds the values these came from.
MARGIN = {False: 8.0, True: 4.0}
MEASURED: Dict[str, float] = {  # largest error over the family's rows (torch 2.x CPU float32 / the emulation), in the family's metric
    "conv_kernel": 3.245e-07, "conv_tiled_kernel": 2.669e-07, "mfma1x1": 3.627e-07, "deconv": 2.063e-07, "fpn_level": 2.952e-07,
    "fpn_tail": 7.888e-07, "stem": 4.658e-07, "refine_front": 1.950e-07, "refine_tail": 6.594e-07,                # float32, x 8
    "f16s": 7.952e-08, "heads": 1.085e-07, "pair": 9.739e-07, "stem_f16s": 6.627e-07, "refine_fused": 5.815e-07,  # emulation, x 4
    "stem_conv2": 1.035e-06,                                                                                      # emulation, x 4
}
TOL: Dict[str, float] = {
    "conv_kernel": 2.6e-6, "conv_tiled_kernel": 2.2e-6, "mfma1x1": 3.0e-6, "deconv": 1.7e-6, "fpn_level": 2.4e-6, "fpn_tail": 6.4e-6,
    "stem": 3.8e-6, "refine_front": 1.6e-6, "refine_tail": 5.3e-6,
    "f16s": 3.2e-7, "heads": 4.4e-7, "pair": 3.9e-6, "stem_f16s": 2.7e-6, "refine_fused": 2.4e-6, "stem_conv2": 4.2e-6,
}


def is_f16s(row: Row) -> bool:
    return row.op in F16S_OPS


# ---- the float32 evaluation (torch CPU, layer by layer) and the split-fp16 emulation ---------------------------------------------------

def _tconv(x, l, relu, stride=1, pad=0, dil=1):
    import torch
    import torch.nn.functional as Fn
    y = Fn.conv2d(x, torch.from_numpy(l["w"]), torch.from_numpy(l["bias"]) if "bias" in l else None, stride, pad, dil)
    if "bn" in l:
        g, b, m, v = (torch.from_numpy(a) for a in l["bn"])
        y = Fn.batch_norm(y, m, v, g, b, False, 0.0, R.BN_EPS)
    return torch.relu(y) if relu else y


def _tdeconv(x, l, relu):
    import torch
    import torch.nn.functional as Fn
    y = Fn.conv_transpose2d(x, torch.from_numpy(l["w"]), None, 2, 1, 1)
    if "bn" in l:
        g, b, m, v = (torch.from_numpy(a) for a in l["bn"])
        y = Fn.batch_norm(y, m, v, g, b, False, 0.0, R.BN_EPS)
    return torch.relu(y) if relu else y


def _emu(x32, l, K, S, dil, CC, relu, **kw):
    w, sh = R.fold(l["w"], l.get("bn"), l.get("bias"))
    return R.f16s_conv(np.asarray(x32, np.float32), w.astype(np.float32).astype(np.float64), sh.astype(np.float32), K, S, dil, CC, relu, **kw)


def evaluate(row: Row, dtype="float32", drop_lo=False) -> np.ndarray:
    """The row in torch on the CPU, layer by layer with torch.nn.functional (conv2d, conv_transpose2d, interpolate, batch_norm), in
    ``dtype``.  float64: the check that conv_ref64 itself is right.  float32: what fp32 arithmetic costs; the split-fp16 layers of
    the f16s ops then go through the emulation conv_ref64.f16s_conv."""
    import torch
    import torch.nn.functional as Fn
    from patchmatchnet_amd import params
    c = case(row)
    dt = getattr(torch, dtype)
    emu = dtype == "float32" and is_f16s(row)

    def T(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dt)

    def L(l):
        return {k: (tuple(a.astype(dtype) for a in v) if k == "bn" else v.astype(dtype)) for k, v in l.items()}

    up2 = lambda u: Fn.interpolate(T(u), scale_factor=2, mode="bilinear", align_corners=False)  # noqa: E731
    relu = bool(row.relu)
    if row.op in ("conv2d", "mfma1x1", "f16s", "heads"):
        if emu:
            return _emu(c["x"], c["l"], row.K, row.S, row.dil, 16 if row.op == "heads" else params.f16s_chunk(row.cin, row.K), relu,
                        drop_lo=drop_lo)
        y = _tconv(T(c["x"]), L(c["l"]), False, row.S, row.pad, row.dil)
        if row.up:
            y = up2(c["u"]) + y
        return (torch.relu(y) if relu else y).numpy()
    if row.op in ("pair", "stem", "stem_f16s", "stem_views"):
        r = relu or row.op != "pair"
        if emu and row.op == "pair":
            return _emu(_emu(c["x"], c["la"], 3, 1, 1, 16, r, drop_lo=drop_lo), c["lb"], 3, 1, 1, 16, r, drop_lo=drop_lo)
        m = _tconv(T(c["x"]), L(c["la"]), r, 1, 1)
        if emu:
            return _emu(m.numpy(), c["lb"], 3, 1, 1, 8, True, drop_lo=drop_lo)
        return _tconv(m, L(c["lb"]), r, 1, 1).numpy()
    if row.op in STEM_CONV2:  # the stem_f16s chain followed by the 8 -> 16, 5x5, stride 2 f16s layer; drop_lo: True, "conv1" or "conv2"
        m = _tconv(T(c["x"]), L(c["la"]), True, 1, 1)
        if emu:
            m = _emu(m.numpy(), c["lb"], 3, 1, 1, 8, True, drop_lo=drop_lo in (True, "conv1"))
            return _emu(m, c["lc"], 5, 2, 1, params.f16s_chunk(8, 5), True, drop_lo=drop_lo in (True, "conv2"))
        return _tconv(_tconv(m, L(c["lb"]), True, 1, 1), L(c["lc"]), True, 2, 2).numpy()
    if row.op == "fpn_level":
        y = Fn.conv2d(T(c["x"]), T(c["w"].T[:, :, None, None]), T(c["b"]))
        return (up2(c["u"]) + y if row.up else y).numpy()
    if row.op == "fpn_tail":
        return _tconv(up2(c["u"]) + _tconv(T(c["x"]), L(c["inner"]), False), L(c["outer"]), False).numpy()
    if row.op == "deconv":
        return _tdeconv(T(c["x"]), L(c["l"]), relu).numpy()
    front = lambda: torch.cat([_tdeconv(T(c["t2"]), L(c["dc"]), True), _tconv(T(c["img"]), L(c["c0"]), True, 1, 1)], 1)  # noqa: E731
    if row.op == "refine_front":
        return front().numpy()
    x16 = T(c["x16"]) if row.op == "refine_tail" else front()
    m = T(_emu(x16.numpy(), c["c3"], 3, 1, 1, 16, True, drop_lo=drop_lo)) if emu else _tconv(x16, L(c["c3"]), True, 1, 1)
    res = Fn.conv2d(m, T(c["wr"]), None, 1, 1)
    lo, hi = T(c["dmin"]).view(-1, 1, 1, 1), T(c["dmax"]).view(-1, 1, 1, 1)
    return ((Fn.interpolate(T(c["dnorm"]), scale_factor=2, mode="nearest") + res) * (hi - lo) + lo).numpy()


# ---- plausible kernel mistakes -----------------------------------------------------------------------------------------------------------

def _out(ref):
    return ref["depth"] if "depth" in ref else ref["y"]


def mistakes(row: Row, ref: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """name -> the row's output when the computation makes one plausible kernel mistake (from conv_ref64; 'lo terms dropped' from the
    emulation)."""
    out: Dict[str, np.ndarray] = {}
    t = np.array(_out(ref), copy=True)
    t[..., -1, -1] = 0.0 if "y" in ref else case(row)["dmin"].astype(np.float64).reshape(-1, 1)
    out["tail pixel unwritten"] = t
    Ho, Wo = out_hw(row)
    if row.op in ("conv2d", "f16s", "heads") and row.K > 1:
        out["clamp instead of zero padding"] = reference(row, border="clamp")["y"]
        if Wo > 16:
            out["tap column dropped at a tile seam"] = reference(row, drop=(0, 16))["y"]
    if row.op in ("conv2d", "mfma1x1", "f16s", "heads", "pair", "deconv") and not row.relu:
        out["relu applied when 0 was asked"] = reference(row, force_relu=True)["y"]
    if row.up and row.op in ("conv2d", "fpn_level", "fpn_tail") and max(Ho, Wo) > 2:
        out["bilinear up-sampling with aligned corners"] = reference(row, align_corners=True)["y"]
    if row.op in ("pair", "stem", "stem_f16s", "stem_views"):
        out["input padded instead of the intermediate map"] = reference(row, pad_input=True)["y"]
    if row.op in STEM_CONV2:
        # Exempt: nothing from M1, M2, M3, M5, M6 -- they differ on every row, the 1x1 image included (its one output has no interior
        # taps, only rim ones).  M4 needs an output with o % 16 == 15 (Ho or Wo >= 16) along an axis that is not exactly the
        # 32-pixel tile pitch long (rolling 32 pixels by 32 moves nothing), which leaves out the small rows, the 32x32 rows, and
        # 30x32, whose 15 output rows have no such output and whose 32 columns roll onto themselves.  M7 is for the table entry and needs
        # B > 1: with one sample per view n % views = n // B and the swapped lookup is the right one.
        out["M1: conv1's map not zeroed outside the image"] = reference(row, conv1_off_image=True)["y"]
        out["M2: conv0's map not zeroed outside the image"] = reference(row, conv0_off_image=True)["y"]
        out["M3: conv2 samples conv1 at 2 o - 1"] = reference(row, origin=-1)["y"]
        out["M3: conv2 samples conv1 at 2 o + 1"] = reference(row, origin=1)["y"]
        if (Ho >= 16 and row.H != 32) or (Wo >= 16 and row.W != 32):
            out["M4: a tile's last row / column from the neighbouring tile's patch"] = reference(row, tile_roll=32)["y"]
        out["M5: lo terms dropped in conv1"] = evaluate(row, "float32", drop_lo="conv1").astype(np.float64)
        out["M5: lo terms dropped in conv2"] = evaluate(row, "float32", drop_lo="conv2").astype(np.float64)
        out["M6: no ReLU after conv1"] = reference(row, relu1=False)["y"]
        if row.op == "stem_conv2_views" and row.N > row.views:
            out["M7: view and sample index swapped in the table lookup"] = reference(row, swap_view_batch=True)["y"]
    if row.op == "deconv":
        out["last row and column missing"] = reference(row, short=True)["y"]
        out["parity classes swapped"] = reference(row, swap=True)["y"]
    if row.op == "refine_front":
        out["last row and column of the transposed convolution missing"] = reference(row, short=True)["y"]
        out["parity classes swapped"] = reference(row, swap=True)["y"]
    if row.op == "refine_fused":
        out["last row and column of the transposed convolution missing"] = reference(row, front_kw=dict(short=True))["depth"]
        out["parity classes swapped"] = reference(row, front_kw=dict(swap=True))["depth"]
    if row.op in ("refine_tail", "refine_fused"):
        if max(row.H, row.W) > 2:  # (a 1x1 dnorm has one value whatever the index)
            out["nearest x2 indexed one pixel off"] = reference(row, near_shift=1)["depth"]
        out["conv3 channel halves swapped"] = reference(row, swap_halves=True)["depth"]
        out["x16 padded instead of the conv3 map"] = reference(row, pad_input=True)["depth"]
        if row.N > 1:
            out["depth range of sample 0 used for sample 1"] = reference(row, roll_range=True)["depth"]
    if is_f16s(row):
        out["lo terms dropped"] = evaluate(row, "float32", drop_lo=True).astype(np.float64)
    return out


# ---- the row's buffers on the host, the row on the device --------------------------------------------------------------------------------

def payloads(row: Row) -> Dict[str, np.ndarray]:
    """The host array behind every input and weight buffer of buffers(row), in the layout the C ABI reads: case(row)'s planar maps
    channels-last where the entry point wants them, the weights through their packers in patchmatchnet_amd.params."""
    import torch

    from patchmatchnet_amd import params
    c = case(row)
    cl = lambda a: np.asarray(a).transpose(0, 2, 3, 1)  # noqa: E731  planar -> channels-last

    def TW(l):
        return {k: (tuple(torch.from_numpy(a) for a in v) if k == "bn" else torch.from_numpy(v)) for k, v in l.items()}

    def pk(fn, l, **kw):
        L = TW(l)
        return fn(L["w"], **({"bn": L["bn"]} if "bn" in L else {"bias": L["bias"]} if "bias" in L else {}), **kw)

    p: Dict = {}
    if row.op == "conv2d":
        p["in"] = c["x"] if row.nchw_in else cl(c["x"])
        p["weights"], p["shift"] = pk(params.pack_conv, c["l"])
        if row.up:
            p["up"] = cl(c["u"])
    elif row.op in ("mfma1x1", "f16s"):
        p["in"] = cl(c["x"])
        p["weights"], p["shift"] = pk(params.pack_conv_mfma if row.op == "mfma1x1" else params.pack_conv_f16s, c["l"])
    elif row.op == "pair":
        p["in"] = cl(c["x"])
        (p["weights_a"], p["shift_a"]), (p["weights_b"], p["shift_b"]) = pk(params.pack_conv_f16s, c["la"]), pk(params.pack_conv_f16s, c["lb"])
    elif row.op == "heads":
        L = TW(c["l"])
        p["in"] = cl(c["x"])
        p["weights"], p["shift"] = params.pack_offset_heads_f16s(L["w"], L["bias"])
    elif row.op == "fpn_level":
        p.update(x=cl(c["x"]), w=c["w"], b=c["b"])
        if row.up:
            p["u"] = cl(c["u"])
    elif row.op == "fpn_tail":
        p.update(x=cl(c["x"]), up=cl(c["u"]))
        (p["w_in"], p["b_in"]), (p["w_out"], _) = pk(params.pack_conv, c["inner"]), pk(params.pack_conv, c["outer"])
    elif row.op == "deconv":
        L = TW(c["l"])
        p["in"] = cl(c["x"])
        p["weights"], p["shift"] = params.pack_deconv(L["w"], L.get("bn"))
    elif row.op in ("stem", "stem_f16s", "stem_views") + STEM_CONV2:
        if row.views:
            B = row.N // row.views
            p.update({f"img{v}": c["x"][v * B:(v + 1) * B] for v in range(row.views)})
        else:
            p["img"] = c["x"]
        p["w0"], p["s0"] = pk(params.pack_conv, c["la"])
        Lb = TW(c["lb"])
        if row.op == "stem":
            p["w1"], p["s1"] = pk(params.pack_conv, c["lb"])
        elif row.op in STEM_CONV2:  # (pack_stem_conv1_f16s takes BatchNorm tensors: a bias alone is scale 1, mean 0, variance 1 at eps 0)
            bn1, eps = (Lb["bn"], R.BN_EPS) if "bn" in Lb else ((torch.ones(8), Lb["bias"], torch.zeros(8), torch.ones(8)), 0.0)
            p["w1a"], p["s1"] = params.pack_stem_conv1_f16s(Lb["w"], bn1, eps)
            p["w2b"], p["s2"] = pk(params.pack_conv_f16s, c["lc"])
        else:
            p["w1a"], p["s1"] = params.pack_stem_conv1_f16s(Lb["w"], Lb["bn"])
    else:
        T0, Td, T3 = TW(c["c0"]), TW(c["dc"]), TW(c["c3"])
        w3, s3, wr = params.pack_refine_tail(T3["w"], T3["bn"], torch.from_numpy(c["wr"]))
        p.update(wr=wr, dnorm=c["dnorm"], depth_min=c["dmin"], depth_max=c["dmax"])
        if row.op != "refine_tail":
            p.update(img=c["img"], t2=cl(c["t2"]))
            p["w0"], p["s0"] = params.pack_conv(T0["w"], bn=T0["bn"])
            p["wd"], p["sd"] = params.pack_deconv(Td["w"], Td["bn"])
        if row.op == "refine_tail":
            p.update(x16=cl(c["x16"]), w3=w3, s3=s3)
        elif row.op == "refine_fused":
            p["w3a"], p["s3"] = params.pack_refine_conv3_f16s(T3["w"], T3["bn"])
    return {b.name: np.ascontiguousarray(p[b.name]) for b in buffers(row) if b.role != "out" and not b.table_of}


def abi_outputs(row: Row, y: np.ndarray) -> Dict[str, np.ndarray]:
    """The planar output of the row (run_device's, or the reference's) as the arrays the call's output buffers hold."""
    cl = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))  # noqa: E731
    ca = row.ca
    if row.op in ("mfma1x1", "fpn_level"):
        return dict({"out" if row.op == "mfma1x1" else "out_a": cl(y[:, :ca])}, **({"out_b": cl(y[:, ca:])} if ca < row.cout else {}))
    if row.op == "heads":
        return dict(out_a=np.ascontiguousarray(y[:, :ca]), **({"out_b": np.ascontiguousarray(y[:, ca:])} if ca < row.cout else {}))
    if row.op == "refine_front":
        return {"x16": cl(y)}
    return {"out": y if row.planar or row.op in ("refine_tail", "refine_fused") else cl(y)}


# ---- the row on the device -----------------------------------------------------------------------------------------------------------------

def run_device(row: Row, want_aligned: bool = False):
    """The row through patchmatchnet_amd.ops on cuda:0 -> planar float32 numpy output (with ``want_aligned``: (output, the output of
    the same call on an aligned base / through pmn_stem_f16s per view), for the same-bits checks; the stem_conv2 ops give a LIST of
    outputs that must hold the same bits: pmn_stem_f16s + pmn_conv2d_f16s on the aligned image, per view for the table entry, and
    for a base off by one float the aligned pmn_stem_conv2_f16s call too)."""
    import torch

    import patchmatchnet_amd as P
    ops = P.ops
    dev = "cuda:0"
    host = payloads(row)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def pl(x):  # channels-last device tensor -> planar numpy
        return x.permute(0, 3, 1, 2).contiguous().cpu().numpy()

    def mis(a):  # the same values at a base one float past a 16-byte boundary
        buf = torch.empty(a.size + 4, dtype=torch.float32, device=dev)
        v = buf[1:1 + a.size].view(a.shape)
        v.copy_(t(a))
        assert v.data_ptr() % 16 == 4
        return v

    d = {k: t(v) for k, v in host.items() if not (row.op == "stem_conv2_views" and k.startswith("img"))}  # (those: allocated apart below)
    g = lambda *names: tuple(d[n] for n in names)  # noqa: E731
    relu = bool(row.relu)
    other = None
    with torch.no_grad():
        if row.op == "conv2d":
            y = ops.conv2d(*g("in", "weights", "shift"), row.cout, row.K, row.S, row.pad, row.dil, relu, d.get("up"), row.nchw_in, row.planar)
            out = y.cpu().numpy() if row.planar else pl(y)
        elif row.op == "mfma1x1":
            a, b = ops.pointwise_split_mfma(*g("in", "weights", "shift"), row.cout, row.ca)
            out = np.concatenate([pl(a), pl(b)], 1)
        elif row.op == "f16s":
            out = pl(ops.conv2d_f16s(*g("in", "weights", "shift"), row.K, row.S, relu))
        elif row.op == "pair":
            out = pl(ops.conv2d_f16s_pair(*g("in", "weights_a", "shift_a", "weights_b", "shift_b"), relu))
        elif row.op == "heads":
            a, b = ops.offset_heads_f16s(*g("in", "weights", "shift"), row.cout, row.ca, row.dil)
            out = np.concatenate([a.cpu().numpy()] + ([b.cpu().numpy()] if b is not None else []), 1)
        elif row.op == "fpn_level":
            a, b = ops.fpn_level(d["x"], d.get("u"), d["w"], d["b"], row.ca)
            out = np.concatenate([pl(a)] + ([pl(b)] if b is not None else []), 1)
        elif row.op == "fpn_tail":
            out = pl(ops.fpn_tail(*g("x", "up", "w_in", "b_in", "w_out")))
        elif row.op == "deconv":
            out = pl(ops.deconv3x3s2(*g("in", "weights", "shift"), relu))
        elif row.op == "stem":
            out = pl(ops.stem(*g("img", "w0", "s0", "w1", "s1")))
        elif row.op == "stem_f16s":
            w = g("w0", "s0", "w1a", "s1")
            out = pl(ops.stem_f16s(mis(host["img"]) if row.misalign else d["img"], *w))
            if want_aligned:
                other = pl(ops.stem_f16s(d["img"], *w))
        elif row.op == "stem_views":
            w = g("w0", "s0", "w1a", "s1")
            V, B = row.views, row.N // row.views
            imgs = [d[f"img{v}"] for v in range(V)]
            tab = ops.SourceTable(torch.tensor([i.data_ptr() for i in imgs], dtype=torch.int64, device=dev), (V, B, 3, row.H, row.W))
            out = pl(ops.stem_f16s_views(tab, *w))
            if want_aligned:
                other = np.concatenate([pl(ops.stem_f16s(i, *w)) for i in imgs], 0)
        elif row.op in STEM_CONV2:
            w = g("w0", "s0", "w1a", "s1", "w2b", "s2")
            two = lambda im: ops.conv2d_f16s(ops.stem_f16s(im, *w[:4]), *w[4:], 5, 2, relu=True)  # noqa: E731
            if row.op == "stem_conv2":
                out = pl(ops.stem_conv2_f16s(mis(host["img"]) if row.misalign else d["img"], *w))
                if want_aligned:  # the two launches on the aligned image, and for a base off by one float the aligned call itself
                    other = [pl(two(d["img"]))] + ([pl(ops.stem_conv2_f16s(d["img"], *w))] if row.misalign else [])
            else:
                V, B = row.views, row.N // row.views
                imgs, spacers = {}, []
                for v in reversed(range(V)):  # allocated apart and backwards: the table's order is unrelated to the addresses'
                    spacers.append(torch.empty(1000 * (v + 1) + 4, device=dev))
                    imgs[v] = t(host[f"img{v}"])
                imgs = [imgs[v] for v in range(V)]
                assert all(ops.SourceTable.image_in_place(i) for i in imgs)
                tab = ops.SourceTable(torch.tensor([i.data_ptr() for i in imgs], dtype=torch.int64, device=dev), (V, B, 3, row.H, row.W))
                out = pl(ops.stem_conv2_f16s_views(tab, *w))
                if want_aligned:
                    other = [np.concatenate([pl(two(i)) for i in imgs], 0)]
        elif row.op == "refine_front":
            out = pl(ops.refine_front(*g("img", "t2", "w0", "s0", "wd", "sd")))
        elif row.op == "refine_tail":
            out = ops.refine_tail(*g("x16", "w3", "s3", "wr", "dnorm", "depth_min", "depth_max")).cpu().numpy()
        else:
            args = g("t2", "w0", "s0", "wd", "sd", "w3a", "s3", "wr", "dnorm", "depth_min", "depth_max")
            out = ops.refine_fused(mis(host["img"]) if row.misalign else d["img"], *args).cpu().numpy()
            if want_aligned:
                other = ops.refine_fused(d["img"], *args).cpu().numpy()
        torch.cuda.synchronize()
    return (out, other) if want_aligned else out


def run_guard(row: Row, dev: str = "cuda:0") -> None:
    """The row through the raw C ABI on ``dev`` with every buffer between guard bands (tests/guard_band.py), then guard_band.check:
    no band touched, no input changed, every output the bytes of run_device's, the ops wrapper on ordinary tensors."""
    import torch

    import guard_band as GB
    from patchmatchnet_amd import _lib
    want = abi_outputs(row, run_device(row))
    arenas = GB.build(buffers(row), payloads(row), dev)
    fn, args = arguments(row, {k: a.ptr for k, a in arenas.items()})
    with torch.cuda.device(dev):
        rc = getattr(_lib.lib(), fn)(*args)
        torch.cuda.synchronize()
    assert rc == 0, (fn, rc)
    GB.check(arenas, want)
