"""Guard bands for calls through the raw C ABI: every buffer of a call is carved out of a larger uint8 allocation

    [ band | payload | band ]

so that a load or store one image, row, tile or channel group off its buffer lands in memory the test owns, and is seen.  A band is
min(max(payload bytes, 4 KiB), 1 MiB) rounded up to 256 bytes (the payload keeps its alignment).  Input and weight arenas hold the
row's data between bands of quiet NaN (0xFF bytes for integer buffers): a value read from a band poisons the output.  The host
neighbour tables (*_host arguments, copied into the kernel-argument segment) get the same arena in host memory.  Output arenas
hold 0xFF everywhere, payload included: an element that is never written stays poison.  After the call check() compares raw bytes
(uint8 views, so NaN compares equal to itself): (a) every band holds its fill, (b) every input and weight payload holds what was
uploaded, (c) every output payload holds the bytes the same call gives through patchmatchnet_amd.ops on ordinary tensors.

Plain helper module (no tests here): tests/test_guard_band.py checks the checker on the CPU, tests/test_guard_band_gpu.py runs every
row of tests/kernel_space.py and tests/conv_space.py through it on the device."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, Mapping, Tuple

import numpy as np

BAND_MIN, BAND_MAX, BAND_ALIGN = 4096, 1 << 20, 256


@dataclass(frozen=True)
class Buf:
    """One pointer argument of a row's call, as include/pmn_hip.h documents it."""
    name: str
    role: str                        # in | out | weights
    dtype: str                       # numpy dtype name
    count: int                       # elements, padded pack layouts included and nothing more
    optional: bool = False           # an output the entry point takes or leaves: record() passes NULL, the device test a real buffer
    host: bool = False               # a *_host argument: the arena stays in host memory whatever the device, record() passes it too
    misalign: bool = False           # payload one float past a 16-byte boundary
    table_of: Tuple[str, ...] = ()   # a device table of addresses: the buffers whose addresses it holds, in order

    @property
    def nbytes(self) -> int:
        return self.count * np.dtype(self.dtype).itemsize


def band_bytes(payload_bytes: int) -> int:
    b = min(max(payload_bytes, BAND_MIN), BAND_MAX)
    return -(-b // BAND_ALIGN) * BAND_ALIGN


def band_fill(dtype: str) -> np.ndarray:
    """The bytes a band of an input or weight arena repeats: a quiet NaN of the buffer's type, 0xFF for integers."""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return np.array([np.nan], dt).view(np.uint8)
    return np.full(dt.itemsize, 0xFF, np.uint8)


class Arena:
    """A buffer between two bands.  ``data``: the payload of an input or weight buffer (``buf.count`` elements); outputs take none.
    ``device``: where the arena lives ("cpu" works: the checker is tested without a device); a host buffer's stays on the CPU."""

    def __init__(self, buf: Buf, data=None, device="cpu") -> None:
        import torch  # (here, not at the top: the table modules import this one, and only an arena needs torch)
        self.buf = buf
        band = band_bytes(buf.nbytes)
        self.lo = band + (4 if buf.misalign else 0)
        self.hi = self.lo + buf.nbytes
        total = self.hi + band
        if buf.role == "out":
            assert data is None, buf.name
            host = np.full(total, 0xFF, np.uint8)
        else:
            pat = band_fill(buf.dtype)  # (lo and the payload are multiples of the pattern's length: both bands stay in phase)
            host = np.resize(pat, total)
            d = np.ascontiguousarray(data)
            assert d.dtype == np.dtype(buf.dtype) and d.size == buf.count, (buf.name, d.dtype, d.size, buf.count)
            host[self.lo:self.hi] = d.reshape(-1).view(np.uint8)
        self.filled = host  # what the arena holds before the call
        self.t = torch.from_numpy(host.copy()).to("cpu" if buf.host else device)
        assert self.ptr % 16 == (4 if buf.misalign else 0), (buf.name, self.ptr)

    @property
    def ptr(self) -> int:
        """Address of the payload."""
        return self.t.data_ptr() + self.lo


def build(bufs: Iterable[Buf], data: Mapping[str, np.ndarray], device="cpu") -> Dict[str, Arena]:
    """One arena per buffer; an address table is built last, from the arenas it points to."""
    bufs = list(bufs)
    out: Dict[str, Arena] = {}
    for b in bufs:
        if not b.table_of:
            out[b.name] = Arena(b, None if b.role == "out" else data[b.name], device)
    for b in bufs:
        if b.table_of:
            out[b.name] = Arena(b, np.array([out[n].ptr for n in b.table_of], b.dtype), device)
    return {b.name: out[b.name] for b in bufs}


def _same(now: np.ndarray, want: np.ndarray, what: str) -> None:
    assert now.size == want.size, f"{what}: {now.size} bytes, expected {want.size}"
    bad = np.flatnonzero(now != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {now.size} bytes differ, the first at byte {int(bad[0])} "
                           f"(holds 0x{int(now[bad[0]]):02x}, expected 0x{int(want[bad[0]]):02x}), the last at byte {int(bad[-1])}")


def check(arenas: Mapping[str, Arena], expected: Mapping[str, np.ndarray]) -> None:
    """The three assertions, on raw bytes.  ``expected``: output name -> the array the payload must hold, in the ABI's layout."""
    for name, a in arenas.items():
        now = a.t.cpu().numpy()
        _same(now[:a.lo], a.filled[:a.lo], f"{name}: band before the payload")
        _same(now[a.hi:], a.filled[a.hi:], f"{name}: band after the payload")
        if a.buf.role == "out":
            want = np.ascontiguousarray(expected[name]).reshape(-1).view(np.uint8)
            _same(now[a.lo:a.hi], want, f"{name}: output payload against the ops wrapper's")
        else:
            _same(now[a.lo:a.hi], a.filled[a.lo:a.hi], f"{name}: {a.buf.role} payload against what was uploaded")


def recording_addresses(bufs: Iterable[Buf], base: int, data: Mapping[str, np.ndarray]):
    """What launch-plan recording passes -> (name -> address, the host arenas behind it: keep them alive over the call): ``base`` for
    every device pointer it gives (+ 4 for a misaligned one), nothing for optional ones, and a real host arena holding ``data[name]``
    for every host buffer, which the entry point reads while it records."""
    bufs = list(bufs)
    held = build([b for b in bufs if b.host], data)
    addr = {b.name: base + (4 if b.misalign else 0) for b in bufs if not b.optional and not b.host}
    addr.update({k: a.ptr for k, a in held.items()})
    return addr, held
