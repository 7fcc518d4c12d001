"""Merged fusion on the CPU: the numpy restatement of the rule (tests/fusion_merge_ref.py on top of
oracle/fusion_oracle.py) shrinks the cloud to about 1 / (views that see a point) and leaves nothing further than a pixel footprint
from a kept point; claims do not cascade; eval.py knows the flag.  tests/test_fusion_merge_gpu.py holds pmn_fuse_view_merged to the
same restatement."""
import os
import sys

import numpy as np
import pytest

import fusion_merge_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"5 views 120x160": (5, 120, 160, 3), "4 views 60x80": (4, 60, 80, 2)}  # V, H, W, --geo_mask_thres
_CACHE = {}


def _case(name):
    """(views, pairs, thresholds, merge_scan result), computed once per case and left unchanged."""
    if name not in _CACHE:
        V, H, W, n = CASES[name]
        views = MR.consistent_scene(V, H, W)
        ids = sorted(views)
        pairs = [(r, [s for s in ids if s != r]) for r in ids]
        thr = (1.0, 0.01, n, 0.5)
        _CACHE[name] = (views, pairs, thr, MR.merge_scan(views, pairs, *thr))
    return _CACHE[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_merged_cloud_is_smaller_and_leaves_no_gap(name):
    """merged / full <= 0.5 and the largest gap <= 2 x the median spacing (measured: 0.257 and 0.321; 1.04 in both cases -- the
    bounds leave room for another seed, not for a broken rule)."""
    _, _, _, r = _case(name)
    n_full, n_merged = len(r["full_vertices"]), len(r["vertices"])
    gap, spacing = MR.gap_over_spacing(r["full_vertices"], r["vertices"], r["first_view_vertices"])
    print("%s: %d points now, %d merged, ratio %.3f; largest gap %.3f / median spacing %.3f = %.2f; %d of %d claims within %g of a "
          "rounding tie" % (name, n_full, n_merged, n_merged / n_full, gap, spacing, gap / spacing, r["ties"], r["claims"], MR.TIE_WINDOW))
    assert n_full > 10000 and n_merged > 0
    assert n_merged <= 0.5 * n_full
    assert gap <= 2.0 * spacing
    assert len(r["colors"]) == n_merged and r["colors"].dtype == np.uint8 and r["vertices"].dtype == np.float32


@pytest.mark.parametrize("name", sorted(CASES))
def test_first_view_emits_its_final_mask_and_emit_is_a_subset(name):
    _, pairs, _, r = _case(name)
    first = pairs[0][0]
    np.testing.assert_array_equal(r["emit"][first], r["final"][first])
    assert r["final"][first].sum() > 1000
    for ref, _ in pairs:
        assert not (r["emit"][ref] & ~r["final"][ref]).any(), ref
    assert any((r["final"][ref] & ~r["emit"][ref]).any() for ref, _ in pairs[1:])  # ... and later views do skip pixels


def test_claims_do_not_cascade():
    """A view's skipped pixels depend on WHICH views were fused before it, not on their order: every final pixel lays its claims
    whether or not it was itself claimed, so reversing the earlier views changes no flag of the last one."""
    views, pairs, thr, r = _case("4 views 60x80")
    last = pairs[-1][0]
    again = MR.merge_scan(views, pairs[:-1][::-1] + pairs[-1:], *thr)
    np.testing.assert_array_equal(again["emit"][last], r["emit"][last])
    assert (r["final"][last] & ~r["emit"][last]).sum() > 1000  # the comparison is about a view that really skips pixels
    # the views in between DO change with the order (the first one emits everything): the test above is not vacuous
    assert not np.array_equal(again["emit"][pairs[0][0]], r["emit"][pairs[0][0]])


def test_eval_parser_knows_the_flag():
    sys.path.insert(0, ROOT)
    import eval as pm_eval
    p = pm_eval.build_parser()
    assert p.parse_args([]).fuse_merge == 0
    assert p.parse_args(["--fuse_merge", "1"]).fuse_merge == 1
    with pytest.raises(SystemExit):
        p.parse_args(["--fuse_merge", "2"])
    assert "world size" in p.format_help() or "number of ranks" in p.format_help()
