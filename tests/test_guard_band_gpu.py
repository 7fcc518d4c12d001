"""Every row of the PatchMatch kernel space (tests/kernel_space.py) and of the convolution kernel space (tests/conv_space.py) through
the raw C ABI on the device with every buffer of the call between guard bands (tests/guard_band.py): after the call (a) every band
holds its fill -- nothing was stored past, or before, a buffer; (b) every input and weight payload holds what was uploaded; (c)
every output payload holds the bytes the same row gives through patchmatchnet_amd.ops on ordinary tensors -- with quiet NaN on
every side of every input, and every output element written over its 0xFF poison.  The float64 comparisons of that wrapper output
are tests/test_kernel_space_gpu.py and tests/test_conv_space_gpu.py.  warp rows run twice, through pmn_warp_correlate and through
pmn_warp_correlate_views with one banded arena per source view; the table entries of the stem likewise have one arena per image.
Rows that carry an environment run in one fresh child process per environment (conv_space.child, mode "guard"), one after the
other, each under its own time limit; the first that does not return 0 ends the test.  No row is skipped or exempted.  The file's
wall time is printed when the module finishes (`-s`) and recorded in DESIGN.md."""
import json
import time

import pytest
import torch

import conv_space as CS
import kernel_space as KS

pytestmark = pytest.mark.gpu

HERE = [r for r in CS.ROWS if not r.env]


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\nGUARD BANDS: {len(KS.ROWS)} + {len(CS.ROWS)} rows in {time.perf_counter() - t0:.1f} s")


def _gpu():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    import patchmatchnet_amd as P
    P.lib()


@pytest.mark.parametrize("row", KS.ROWS, ids=[r.id for r in KS.ROWS])
def test_patchmatch_row_touches_only_its_buffers(row):
    _gpu()
    KS.run_guard(row)
    if row.op == "warp":
        KS.run_guard(row, views=True)


@pytest.mark.parametrize("row", HERE, ids=[r.id for r in HERE])
def test_conv_row_touches_only_its_buffers(row):
    _gpu()
    CS.run_guard(row)


def test_conv_rows_that_carry_an_environment_touch_only_their_buffers():
    _gpu()
    assert {row.env for row in CS.ROWS if row.env} == set(CS.ENVS)
    for env in CS.ENVS:  # three children, one after the other; the first that does not return 0 ends the test
        r = CS.child(env, "guard", 120)
        assert r.returncode == 0, f"{dict(env)}: child returned {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("CONV_SPACE_JSON ")][-1]
        res = json.loads(line[len("CONV_SPACE_JSON "):])
        rows = [row for row in CS.ROWS if row.env == env]
        assert rows and res == {row.id: "ok" for row in rows}
