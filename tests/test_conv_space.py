"""CPU checks of the convolution kernel space (tests/conv_space.py): every row selects the instantiation it declares (launch-plan
recording, no device; rows that carry an environment record in a fresh child process with it), the rows jointly reach every
instantiation of the convolution kernel families in the library's symbol table, the float64 reference (tests/conv_ref64.py) agrees with
torch.nn.functional in float64 on every row, the tolerances are what float32 arithmetic (or the split-fp16 emulation) needs times a
fixed margin, and each is far below the error of a plausible kernel mistake.  The rows of pmn_stem_conv2_f16s and
pmn_stem_conv2_f16s_views (stem_f16s_kernel_conv2: 16 x 16 half-resolution outputs = 32 x 32 input pixels per workgroup, 81 KB of LDS)
record on a device only, like every form above 48 KB; their table, reference, emulation and mistakes (a fused intermediate map that
is not zero outside the image among them) are checked here.  The device side is tests/test_conv_space_gpu.py."""
import numpy as np
import pytest
import torch

import conv_ref64 as R
import conv_space as CS
import kernel_space as KS

IDS = [r.id for r in CS.ROWS]


def _lib():
    from patchmatchnet_amd import _lib
    return _lib


def _record(row):
    return CS.record_env(row.env)[row.id] if row.env else CS.record(row)


@pytest.mark.parametrize("row", CS.ROWS, ids=IDS)
def test_row_records_its_kernel(row):
    rc, names = _record(row)
    if row.device_only and rc == -3:
        # > 48 KB of dynamic LDS: hipFuncSetAttribute needs a device, so without one nothing is recorded (the GPU test records it)
        assert names == [] and not torch.cuda.is_available()
        return
    assert rc == 0, rc
    assert names == [CS.mangle(row.kernel)], (row.kernel, names)


def test_rows_cover_every_reachable_instantiation():
    lib = _lib()
    inst = KS.library_instantiations(lib.LIB_PATH, CS.FAMILIES)  # raises when the library has no stubs
    stubs = {s for s in KS.dynamic_symbols(lib.LIB_PATH) if "__device_stub__" in s}
    for name, sym in CS.OTHER_KERNELS.items():  # the plain (non-template) kernels are in the library too
        assert f"_Z{len(name) + 15}__device_stub__{name}{sym[len(f'_Z{len(name)}{name}'):]}" in stubs, name
    dead = {CS.mangle(k) for k in CS.DEAD}
    assert dead <= set(inst), sorted(dead - set(inst))
    declared = {CS.mangle(r.kernel) for r in CS.ROWS}
    recorded = set()
    for r in CS.ROWS:
        rc, names = _record(r)
        recorded.update(names)
        if rc == -3 and r.device_only:
            recorded.add(CS.mangle(r.kernel))  # declared, checked by test_row_records_its_kernel and on the device
    others = {CS.mangle(k) for k in CS.OTHER_KERNELS}
    assert recorded == declared
    assert not dead & recorded, sorted(dead & recorded)
    missing = set(inst) - dead - recorded
    assert not missing, f"instantiations no row reaches: {sorted(missing)}"
    assert recorded - others == set(inst) - dead
    print(f"\nconvolution kernel space: {len(recorded - others)} reachable instantiations covered (+ {len(others)} plain kernels), "
          f"{len(dead)} listed as dead, of the library's {len(inst)}")


def test_table_holds_the_shapes_it_promises():
    rows = CS.ROWS
    big = [r for r in rows if max(r.H, r.W) > 64]
    assert [r.kernel for r in big] == ["conv_kernel<1, 8, 3, 1, 4, true, false>"] and big[0].large
    r = big[0]
    assert r.N * r.H * r.W == 1500000 and r.W % 4 == 2  # launch_conv: pix >= 1500000L
    for fam in {CS.family(r) for r in rows}:
        fr = [r for r in rows if CS.family(r) == fam and not r.large]
        assert min(max(r.H, r.W) for r in fr) <= 5, fam
    tiles = {r.N * -(-CS.out_hw(r)[0] // 16) * -(-CS.out_hw(r)[1] // 16) for r in rows if r.kernel.startswith("conv_tiled")}
    assert any(t < 8 for t in tiles) and 8 in tiles and any(t > 8 and t % 8 for t in tiles)
    assert {r.N for r in rows} >= {1, 2, 3}
    assert any(r.op == "heads" and max(r.H, r.W) < r.dil for r in rows) and any(r.planar and max(r.H, r.W) < r.dil for r in rows)
    for op in ("conv2d", "f16s", "pair", "deconv"):
        assert {r.relu for r in rows if r.op == op} == {0, 1}, op
    assert {r.bn for r in rows if r.op == "f16s"} == {True, False}
    assert {r.op for r in rows if r.misalign} == {"stem_f16s", "stem_conv2", "refine_fused"} and all(r.W % 4 == 0 for r in rows if r.misalign)
    # the fused conv0 + conv1 + conv2 kernel: a workgroup is 16 x 16 half-resolution outputs; the family's own tile counts and weights
    fc = [r for r in rows if CS.family(r) == "stem_conv2"]
    assert {r.op for r in fc} == {"stem_conv2", "stem_conv2_views"} and all(r.device_only and max(r.H, r.W) <= 64 for r in fc)
    assert {r.kernel for r in fc} == {"stem_f16s_kernel_conv2<true>", "stem_f16s_kernel_conv2<false>"}
    assert all((r.kernel.endswith("<true>")) == (r.W % 4 == 0 and not r.misalign) for r in fc)
    assert any(max(r.H, r.W) <= 5 for r in fc)
    groups = {r.N * -(-CS.out_hw(r)[0] // 16) * -(-CS.out_hw(r)[1] // 16) for r in fc}
    assert 8 in groups and any(g < 8 for g in groups) and any(g > 8 and g % 8 for g in groups)
    assert {r.N for r in fc} >= {1, 2, 3} and {r.bn for r in fc} == {True, False}
    assert any(CS.out_hw(r) == (16, 16) and (r.H, r.W) == (32, 32) for r in fc)  # exactly one tile
    assert {(r.views, r.N // r.views) for r in fc if r.views} == {(3, 2), (2, 1), (2, 2)}
    for r in fc:  # a nonzero shift on every layer, a positive one among them: ReLU(shift) != 0 where a layer's map must be ZERO
        c = CS.case(r)
        for l in (c["la"], c["lb"], c["lc"]):
            sh = R.fold(l["w"], l.get("bn"), l.get("bias"))[1]
            assert (sh != 0).all() and (sh > 0).any(), r.id
    for r in rows:
        if r.op.startswith("refine") and r.op != "refine_front":
            m = np.abs(CS.reference(r)["res"]).max()
            assert 0.05 <= m <= 0.5, (r.id, m)
    assert any(r.op == "refine_fused" and r.N == 2 for r in rows)


def test_image_in_place_keeps_unaligned_images_out_of_the_table():
    """pmn_stem_conv2_f16s_views (like pmn_stem_f16s_views) picks the float4 staging from W % 4 == 0 alone: it cannot see the
    addresses in the table.  ops.SourceTable.image_in_place is what refuses an image whose base is not 16-byte aligned.  No device
    here, so a real tensor's answers are passed on with is_cuda forced."""
    from patchmatchnet_amd import ops

    class OnDevice:
        is_cuda = True

        def __init__(self, t):
            self.t, self.dtype = t, t.dtype

        def is_contiguous(self):
            return self.t.is_contiguous()

        def data_ptr(self):
            return self.t.data_ptr()

    buf = torch.zeros(3 * 4 * 4 + 8)
    first = (-buf.data_ptr() // 4) % 4  # the first float of buf on a 16-byte boundary
    aligned, off_by_one = (buf[first + d:first + d + 48].view(1, 3, 4, 4) for d in (0, 1))
    assert aligned.data_ptr() % 16 == 0 and off_by_one.data_ptr() % 16 == 4 and off_by_one.is_contiguous()
    assert ops.SourceTable.image_in_place(OnDevice(aligned))
    assert not ops.SourceTable.image_in_place(OnDevice(off_by_one))
    assert not ops.SourceTable.image_in_place(OnDevice(aligned.double())) and not ops.SourceTable.image_in_place(OnDevice(aligned[:, :, ::2]))
    assert not ops.SourceTable.image_in_place(aligned)  # (a host tensor is never read in place)


def test_f16s_emulation_agrees_with_the_lane_level_one():
    """conv_ref64.f16s_conv (vectorised) against tests/test_f16s_emulation.py::emulate (lane by lane).  emulate accumulates in float64
    and rounds once, to its float32 output; f16s_conv(acc64=True) does the same sums in float64 and returns them unrounded.  The two
    then hold the same split products in the same k order, so they differ by emulate's one output rounding, at most 2^-24 |y|, plus
    float64 noise.  The fp32 accumulators that the tolerances are measured with are this same code with the accumulators cast to
    float32 after every MFMA, nothing else."""
    from patchmatchnet_amd import params
    from test_f16s_emulation import emulate
    rng = np.random.default_rng(5)
    for K, S, cin, cout, dil in ((3, 1, 16, 16, 1), (5, 2, 8, 16, 1), (3, 1, 32, 32, 4)):
        x = rng.standard_normal((1, cin, 9, 19)).astype(np.float32)
        w = torch.from_numpy((rng.standard_normal((cout, cin, K, K)) * 0.2).astype(np.float32))
        b = torch.from_numpy(rng.standard_normal(cout).astype(np.float32))
        if dil == 1:
            wpk, sh = params.pack_conv_f16s(w, bias=b)
            CC = params.f16s_chunk(cin, K)
        else:
            wpk, sh = params.pack_offset_heads_f16s(w, b)
            CC = 16
        a = emulate(np.ascontiguousarray(x.transpose(0, 2, 3, 1)), wpk, sh, K, S, cin, cout, relu=False, dil=dil, CC=CC).transpose(0, 3, 1, 2)
        v = R.f16s_conv(x, w.double().numpy(), sh, K, S, dil, CC, False, acc64=True)
        _, A = R.conv2d(x, w.numpy(), b.numpy(), stride=S, pad=dil * (K // 2), dil=dil)
        assert a.shape == v.shape and v.dtype == np.float64
        assert (np.abs(a.astype(np.float64) - v) <= 2.0 ** -24 * np.abs(v) + 1e-13 * A).all()


@pytest.mark.parametrize("row", CS.ROWS, ids=IDS)
def test_ref64_agrees_with_torch_float64(row):
    ref = CS.reference(row)
    want = CS.evaluate(row, "float64")
    got = ref["depth"] if "depth" in ref else ref["y"]
    assert got.shape == want.shape
    scale = np.abs(want).max() if "depth" in ref else np.maximum(ref["A"], 1e-30)
    assert (np.abs(got - want) / scale).max() < 1e-12


def _measure():
    worst = {}
    for row in CS.ROWS:
        e = CS.error(row, CS.evaluate(row, "float32"), CS.reference(row))
        f = CS.family(row)
        worst[f] = max(worst.get(f, 0.0), e)
    return worst


def test_tolerances_are_the_measured_float32_error_times_the_margin():
    worst = _measure()
    fams = {CS.family(r): CS.is_f16s(r) for r in CS.ROWS}
    assert set(CS.TOL) == set(fams)
    for f, e in sorted(worst.items()):
        m = CS.MARGIN[fams[f]]
        print(f"MEASURED {f}: {'emulation' if fams[f] else 'float32'} {e:.3e} x {m:g} = {m * e:.3e} (TOL {CS.TOL[f]:.2e})")
        assert m * e <= CS.TOL[f], (f, e, CS.TOL[f])
        assert CS.TOL[f] <= 1.25 * m * CS.MEASURED[f], f  # and the table is not looser than its own measurement says


@pytest.mark.parametrize("row", CS.ROWS, ids=IDS)
def test_tolerances_discriminate(row):
    """Every plausible mistake conv_ref64 can express for the row exceeds the row's tolerance by at least 10x."""
    ref = CS.reference(row)
    ms = CS.mistakes(row, ref)
    assert ms, row
    tol = CS.TOL[CS.family(row)]
    for name, wrong in ms.items():
        err = CS.error(row, wrong, ref)
        assert err > 10 * tol, f"{name}: error {err:.3e} is within 10x the tolerance {tol:.1e}"
