"""CPU checks of the guard-band helper (tests/guard_band.py) and of the bookkeeping behind tests/test_guard_band_gpu.py: the band
rule and the fills; the checker passes a call that writes its outputs and nothing else and fails on one byte before a payload, one
byte after it, one byte written into an input and one output byte left at its poison; and, for every row of tests/kernel_space.py and
tests/conv_space.py, the element count each buffer declares is the size of the array the row's inputs, packers and reference give,
and the argument list carries every buffer's address exactly once -- a mistake in the test's own sizes is caught here, before a raw
pointer reaches a device."""
import numpy as np
import pytest
import torch

import conv_space as CS
import guard_band as GB
import kernel_space as KS

F32_NAN = np.array([np.nan], np.float32).view(np.uint8)


def test_band_rule():
    assert GB.band_bytes(0) == GB.band_bytes(4) == GB.band_bytes(4096) == 4096
    assert GB.band_bytes(4097) == 4352 and GB.band_bytes(5000) == 5120  # as long as the payload, rounded up to 256
    assert GB.band_bytes((1 << 20) - 1) == GB.band_bytes(1 << 20) == GB.band_bytes(48 << 20) == 1 << 20
    assert all(GB.band_bytes(n) % 256 == 0 and GB.band_bytes(n) >= min(n, 1 << 20) for n in range(0, 3 << 20, 4093))


def test_fills():
    data = np.arange(1500, dtype=np.float32)
    a = GB.Arena(GB.Buf("x", "in", "float32", 1500), data)
    assert (a.lo, a.hi, a.filled.size) == (6144, 6144 + 6000, 6144 + 6000 + 6144) and a.ptr % 16 == 0
    assert np.array_equal(a.filled[a.lo:a.hi].view(np.float32), data)
    for band in (a.filled[:a.lo], a.filled[a.hi:]):
        assert np.array_equal(band.reshape(-1, 4), np.broadcast_to(F32_NAN, (band.size // 4, 4)))
    assert np.array_equal(a.t.numpy(), a.filled) and a.t.numpy() is not a.filled
    m = GB.Arena(GB.Buf("img", "in", "float32", 1500, misalign=True), data)  # one float further in, the gap filled like the band
    assert m.lo == 6148 and m.ptr % 16 == 4 and np.isnan(m.filled[:m.lo].view(np.float32)).all()
    assert np.isnan(m.filled[m.hi:].view(np.float32)).all() and m.filled.size - m.hi == 6144
    h = GB.Arena(GB.Buf("w", "weights", "float16", 64), np.ones(64, np.float16))
    assert np.isnan(h.filled[:h.lo].view(np.float16)).all() and np.isnan(h.filled[h.hi:].view(np.float16)).all()
    assert (h.filled[:2] == [0x00, 0x7E]).all()  # quiet: the top mantissa bit is set
    assert (a.filled[:4] == [0x00, 0x00, 0xC0, 0x7F]).all()
    i = GB.Arena(GB.Buf("t", "in", "int64", 3), np.array([1, 2, 3], np.int64))
    assert (i.filled[:i.lo] == 0xFF).all() and (i.filled[i.hi:] == 0xFF).all() and i.hi - i.lo == 24
    o = GB.Arena(GB.Buf("out", "out", "float32", 10))
    assert (o.filled == 0xFF).all() and o.filled.size == 4096 + 40 + 4096
    t = GB.Arena(GB.Buf("tab_host", "in", "int32", 4, host=True), np.arange(4, dtype=np.int32), device="meta")  # stays in host memory
    assert t.t.device.type == "cpu" and (t.filled[:t.lo] == 0xFF).all() and (t.filled[t.hi:] == 0xFF).all() and t.hi - t.lo == 16
    with pytest.raises(AssertionError):
        GB.Arena(GB.Buf("x", "in", "float32", 1499), data)  # the declared count is not the array's size
    with pytest.raises(AssertionError):
        GB.Arena(GB.Buf("x", "in", "float32", 1500), data.astype(np.float64))


BUFS = [GB.Buf("x", "in", "float32", 300), GB.Buf("w", "weights", "float16", 128), GB.Buf("tab", "in", "int64", 2, table_of=("x", "w")),
        GB.Buf("nbr_host", "in", "int32", 18, host=True), GB.Buf("y", "out", "float32", 77), GB.Buf("idx", "out", "int32", 5)]


def _call():
    """Arenas on the CPU after a 'call' that wrote its two outputs and nothing else; the outputs hold NaN payloads and 0xFF bytes."""
    rng = np.random.default_rng(0)
    data = {"x": rng.standard_normal(300).astype(np.float32), "w": rng.standard_normal(128).astype(np.float16)}
    data["x"][7] = np.nan
    data["nbr_host"] = rng.integers(-3, 4, 18).astype(np.int32)
    arenas = GB.build(BUFS, data)
    want = {"y": rng.standard_normal(77).astype(np.float32), "idx": np.array([0, -1, 5, 7, 3], np.int32)}
    want["y"][3] = np.nan
    for k, v in want.items():
        a = arenas[k]
        a.t[a.lo:a.hi] = torch.from_numpy(v.view(np.uint8))
    return arenas, want


def test_checker_passes_a_call_that_writes_its_outputs_only():
    arenas, want = _call()
    assert list(arenas) == [b.name for b in BUFS]
    assert arenas["tab"].filled[arenas["tab"].lo:arenas["tab"].hi].view(np.int64).tolist() == [arenas["x"].ptr, arenas["w"].ptr]
    GB.check(arenas, want)  # NaN payloads in an input and in an output compare equal: raw bytes


@pytest.mark.parametrize("name", [b.name for b in BUFS])
@pytest.mark.parametrize("where", ["before", "after"])
def test_checker_fails_on_one_byte_outside_a_payload(name, where):
    arenas, want = _call()
    a = arenas[name]
    for at in ((a.lo - 1, 0) if where == "before" else (a.hi, a.t.numel() - 1)):  # next to the payload, and at the arena's far end
        arenas, want = _call()
        arenas[name].t[at] ^= 1
        with pytest.raises(AssertionError, match=f"{name}: band {where} the payload: 1 of"):
            GB.check(arenas, want)


@pytest.mark.parametrize("name", ["x", "w", "tab", "nbr_host"])
def test_checker_fails_on_one_byte_written_into_an_input(name):
    for at in (0, -1):
        arenas, want = _call()
        a = arenas[name]
        a.t[a.lo if at == 0 else a.hi - 1] ^= 0x80
        with pytest.raises(AssertionError, match=f"{name}: (in|weights) payload against what was uploaded: 1 of"):
            GB.check(arenas, want)


@pytest.mark.parametrize("name", ["y", "idx"])
def test_checker_fails_on_one_output_byte_left_at_its_poison(name):
    for at in (0, -1):
        arenas, want = _call()
        a = arenas[name]
        i = a.lo if at == 0 else a.hi - 1
        assert int(a.filled[i]) == 0xFF and int(a.t[i]) != 0xFF  # (the expected byte there is not the poison's)
        a.t[i] = 0xFF
        with pytest.raises(AssertionError, match=f"{name}: output payload against the ops wrapper's: 1 of"):
            GB.check(arenas, want)
    arenas, want = _call()  # an output that is short of the declared count is no match either
    with pytest.raises(AssertionError, match="bytes, expected"):
        GB.check(arenas, dict(want, **{name: want[name][:-1]}))


def _addresses_once(bufs, fn_args, row_id):
    """With a distinct address per buffer the argument list holds every buffer's address once -- through its table for a table's
    members -- and no other address."""
    addr = {b.name: 0x10000000 + 0x1000 * i for i, b in enumerate(bufs)}
    args = fn_args(addr)
    inside = {n for b in bufs for n in b.table_of}
    got = sorted(v for v in args if isinstance(v, int) and not isinstance(v, bool) and v >= 0x10000000)
    assert got == sorted(addr[b.name] for b in bufs if b.name not in inside), row_id
    assert inside <= set(addr) and len({b.name for b in bufs}) == len(bufs), row_id


def test_kernel_space_declares_the_sizes_its_inputs_and_reference_have():
    for row in KS.ROWS:
        x, mlps = KS.inputs(row), KS.nets(row)
        ref = KS.reference(row, x, mlps)
        for views in (False, True) if row.op == "warp" else (False,):
            bufs = KS.buffers(row, views)
            p = KS.payloads(row, x, mlps, views)
            assert set(p) == {b.name for b in bufs if b.role != "out" and not b.table_of}, row.id
            for b in bufs:
                if b.role == "out":
                    assert ref[KS.REF_KEY[b.name]].size == b.count, (row.id, b.name)
                elif b.table_of:
                    assert b.count == len(b.table_of) == row.N and b.dtype == "int64", row.id
                else:
                    assert p[b.name].size == b.count and p[b.name].dtype == np.dtype(b.dtype), (row.id, b.name)
            # the host neighbour table, int[2K] of (dy, dx) pairs, is a buffer of every call that takes one
            K = {"init": row.propK, "feature_weight": row.D, "aggregate": row.K}.get(row.op, 0)
            tabs = [b for b in bufs if b.host]
            assert [(b.name, b.role, b.dtype, b.count) for b in tabs] == \
                ([("propa_table_host" if row.op == "init" else "eval_table_host", "in", "int32", 2 * K)] if K else []), row.id
            assert all(np.array_equal(p[b.name], KS.neighbor_table(row, K)) for b in tabs)
            _addresses_once(bufs, lambda a: KS.arguments(row, a, views)[1], row.id)
            addr, held = GB.recording_addresses(bufs, 0x100000, KS.host_tables(row))  # recording: real host arenas, fake device addresses
            assert set(held) == {b.name for b in tabs} and all(addr[b.name] == held[b.name].ptr for b in tabs)
            assert all(addr[b.name] == 0x100000 for b in bufs if not b.host and not b.optional) and not any(b.name in addr for b in bufs if b.optional)
    assert any(b.name == "src_view_table" for r in KS.ROWS if r.op == "warp" for b in KS.buffers(r, True))
    assert {b.name for r in KS.ROWS for b in KS.buffers(r) if b.host} == {"propa_table_host", "eval_table_host"}


def test_conv_space_declares_the_sizes_its_packers_and_reference_have():
    for row in CS.ROWS:
        bufs = CS.buffers(row)
        p = CS.payloads(row)
        out = CS.abi_outputs(row, CS._out(CS.reference(row)))
        assert set(out) == {b.name for b in bufs if b.role == "out"}, row.id
        for b in bufs:
            if b.role == "out":
                assert out[b.name].size == b.count, (row.id, b.name)
            elif b.table_of:
                assert b.count == len(b.table_of) == row.views and b.dtype == "int64", row.id
            else:
                assert p[b.name].size == b.count and p[b.name].dtype == np.dtype(b.dtype), (row.id, b.name)
            assert b.misalign == (row.misalign and b.name == "img"), (row.id, b.name)
        assert {b.name for b in bufs} - {n for b in bufs for n in b.table_of} <= set(CS.ABI[row.op][1]), row.id
        _addresses_once(bufs, lambda a: CS.arguments(row, a)[1], row.id)
    assert sum(r.misalign for r in CS.ROWS) >= 3 and sum(bool(r.views) for r in CS.ROWS) >= 5
