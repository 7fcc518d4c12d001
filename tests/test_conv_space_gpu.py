"""Every row of the convolution kernel space (tests/conv_space.py) on the device: the op through patchmatchnet_amd.ops, the plan the
device records for it (it selects the declared instantiation, the > 48 KB LDS forms included) and the output against the float64
reference tests/conv_ref64.py in the row's metric at the family's tolerance (conv_space.TOL).  pmn_stem_f16s_views equals
pmn_stem_f16s per view and a call on a base off by one float equals the aligned call, bit for bit; pmn_stem_conv2_f16s[_views]
(conv0 + conv1 + conv2 in one launch) equals pmn_stem_f16s followed by pmn_conv2d_f16s, per view for the table entry, bit for bit,
besides meeting the float64 reference of the three layers, whose maps are zero outside the image.  Rows that carry an environment
(PMN_CONV_SPLIT / PMN_CONV_CC5 are read once per process) run in one fresh child process per environment, three in all (see
conv_space.E_S0), one after the other, each under its own time limit; the first that does not return 0 ends the test.  The measured
maxima per family are printed when the module finishes (`-s`) and recorded in DESIGN.md."""
import json

import numpy as np
import pytest
import torch

import conv_space as CS

pytestmark = pytest.mark.gpu

HERE = [r for r in CS.ROWS if not r.env]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _family_maxima():
    yield
    for f, e in sorted(WORST.items()):  # of the rows that ran (all of them unless tests were deselected)
        print(f"\nFAMILY {f}: maximum error {e:.3e}, tolerance {CS.TOL[f]:.1e}", end="")
    print()


def _gpu():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    import patchmatchnet_amd as P
    P.lib()
    return P


def _check(row, err):
    f = CS.family(row)
    WORST[f] = max(WORST.get(f, 0.0), err)
    print(f"MEASURED {row.id} {err:.3e} (tolerance {CS.TOL[f]:.1e}; family maximum so far {WORST[f]:.3e})")
    assert err < CS.TOL[f], f"{row.id}: error {err:.3e} >= {CS.TOL[f]:.1e}"


@pytest.mark.parametrize("row", HERE, ids=[r.id for r in HERE])
def test_row_against_float64_reference(row):
    _gpu()
    rc, names = CS.record(row)  # with a device every row records
    assert rc == 0 and names == [CS.mangle(row.kernel)], (rc, names, row.kernel)
    same = row.misalign or row.op == "stem_views" or row.op in CS.STEM_CONV2
    got = CS.run_device(row, want_aligned=same)
    if same:
        got, other = got
        if row.op in CS.STEM_CONV2:  # [pmn_stem_f16s + pmn_conv2d_f16s (per view), and off an aligned base the aligned call]
            assert len(other) == 1 + row.misalign
            for i, o in enumerate(other):
                assert np.array_equal(got, o), "not the bits of " + ("the aligned call" if i else "pmn_stem_f16s + pmn_conv2d_f16s")
        else:
            assert np.array_equal(got, other), "not the bits of the aligned call" if row.misalign else "not the bits of pmn_stem_f16s per view"
    _check(row, CS.error(row, got, CS.reference(row)))


def test_feature_net_gives_the_same_bits_for_a_view_off_by_one_float():
    """FeatureNet.forward_hip on a list of views (W % 4 == 0), one of them at a base one float past a 16-byte boundary: that view
    goes through stem_f16s_kernel_conv2<false>, its aligned copy through <true>, and all three levels hold the same bits.
    (ops.SourceTable.image_in_place keeps such a view out of the table entry, which cannot see addresses.)"""
    P = _gpu()
    import goldenutil as GU
    _, params, kw = GU.load_case("default")
    model = P.PatchmatchNet(**kw)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    feat = model.cuda().eval().feature
    assert feat.fuse_stem_conv2 and feat.f16_split
    g = torch.Generator().manual_seed(5)
    a, b = (torch.rand(1, 3, 40, 48, generator=g).cuda() for _ in range(2))
    buf = torch.empty(b.numel() + 4, device="cuda")
    shifted = buf[1:1 + b.numel()].view_as(b).copy_(b)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    assert P.ops.SourceTable.image_in_place(b) and not P.ops.SourceTable.image_in_place(shifted)
    with torch.no_grad():
        want, got = feat.forward_hip([a, b]), feat.forward_hip([a, shifted])
    torch.cuda.synchronize()
    assert "conv2_f16s" in feat._packed() and feat.f16_domain_error is None  # the fused kernel is what ran
    assert all(torch.equal(got[k], want[k]) for k in (1, 2, 3))


def test_rows_that_carry_an_environment():
    _gpu()
    assert {row.env for row in CS.ROWS if row.env} == set(CS.ENVS)
    for env in CS.ENVS:  # three children, one after the other; the first that does not return 0 ends the test
        r = CS.child(env, "run", 120)
        assert r.returncode == 0, f"{dict(env)}: child returned {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("CONV_SPACE_JSON ")][-1]
        res = json.loads(line[len("CONV_SPACE_JSON "):])
        rows = [row for row in CS.ROWS if row.env == env]
        assert rows and set(res) == {row.id for row in rows}
        for row in rows:
            v = res[row.id]
            assert v["rc"] == 0 and v["names"] == [CS.mangle(row.kernel)], (row.id, v)
            _check(row, v["err"])
