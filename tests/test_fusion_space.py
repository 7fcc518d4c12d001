"""CPU checks of the fusion kernel space (tests/fusion_space.py): the row ids are unique, every edge the table is there for is hit by
at least one row, the extended-precision reference (tests/fusion_ref64.py) agrees with oracle/fusion_oracle.py on the decided pixels
of the friendly rows, and the share of fragile (pixel, source) entries stays under its cap -- a condition on the table, computed from
the reference alone.  The device side is tests/test_fusion_space_gpu.py."""
import numpy as np
import pytest

import fusion_ref64 as R64
import fusion_space as FS
from oracle import fusion_oracle as FO

FRAGILE_CAP = 1e-3


def _row(name):
    return next(r for r in FS.FUSE_ROWS if r.name == name)


def test_row_ids_are_unique():
    for rows in (FS.FUSE_ROWS, FS.PACK_ROWS):
        ids = [r.id for r in rows]
        assert len(set(ids)) == len(ids)
    assert all(r.H * r.W <= 40 * 72 and all(h * w <= 40 * 72 for h, w in r.src_sizes) for r in FS.FUSE_ROWS)


def test_fuse_rows_cover_the_shapes_counts_and_thresholds():
    rows = FS.FUSE_ROWS
    assert {(1, 1), (2, 3), (8, 32), (9, 33), (7, 31), (40, 72)} <= {(r.H, r.W) for r in rows}
    assert any(any(h * w < r.H * r.W for h, w in r.src_sizes) and any(h * w > r.H * r.W for h, w in r.src_sizes) for r in rows)
    assert any(r.slot_pad > 0 and r.claim_pad > 0 for r in rows)
    for r in rows:
        sc = FS.scene(r)
        need = max(2 * h * w for h, w in sc["sizes"])
        assert sc["maps"].shape[1] == need + r.slot_pad and sc["claim_room"] == need // 2 + r.claim_pad
        if r.reorder:
            assert sc["ref_slot"] != 0 and list(sc["src_slots"]) == sorted(sc["src_slots"], reverse=True) and r.n_src > 1
    assert any(r.reorder and r.src_sizes for r in rows)
    assert {0, 1, 5, 32} <= {r.n_src for r in rows}
    assert any(r.mask_thres == 0 and r.n_src > 0 for r in rows) and any(r.mask_thres == 1 for r in rows)
    assert any(r.mask_thres == r.n_src > 1 for r in rows) and any(r.mask_thres == r.n_src + 1 for r in rows)
    assert any(r.n_src == 32 and r.prefill for r in rows)  # bit 31 of the merged kernel's ``agreed`` mask lays claims
    v = FS.reference(_row("nsrc32"))["view"]
    assert (v["verdict"][31] & v["final"] & v["decided"]).any()
    # a threshold of n_src is met somewhere and n_src + 1 nowhere
    assert FS.reference(_row("thres-nsrc"))["view"]["geo"].any() and not FS.reference(_row("thres-nsrc-plus-1"))["view"]["geo"].any()
    assert FS.reference(_row("nsrc0-thres0"))["view"]["geo"].all() and not FS.reference(_row("nsrc0-thres1"))["view"]["geo"].any()


def test_fuse_rows_cover_the_source_camera_edges():
    v = FS.reference(_row("camera-away"))["view"]
    h, w = FS.scene(_row("camera-away"))["sizes"][1]
    assert ((v["xs"][0] <= -1) | (v["xs"][0] >= w) | (v["ys"][0] <= -1) | (v["ys"][0] >= h)).all() and not v["kz_negative"][0].any()
    assert not v["verdict"][0].any() and v["verdict"][1:].any()
    v = FS.reference(_row("camera-behind"))["view"]
    assert v["kz_negative"][0].all()  # the whole surface behind source 0, projected into its image
    assert ((v["xs"][0] > 0) & (v["xs"][0] < w - 1) & (v["ys"][0] > 0) & (v["ys"][0] < h - 1)).mean() > 0.5
    assert v["kz_negative"][1].any() and not v["kz_negative"][1].all()  # part of it behind source 1
    for name in ("camera-bands", "camera-bands-9x33"):
        v = FS.reference(_row(name))["view"]
        h, w = FS.scene(_row(name))["sizes"][1]
        xs, ys = v["xs"][0], v["ys"][0]
        in_x, in_y = (xs > -1) & (xs < w), (ys > -1) & (ys < h)
        bands = {"left": (xs > -1) & (xs < 0) & in_y, "right": (xs >= w - 1) & (xs < w) & in_y,
                 "top": (ys > -1) & (ys < 0) & in_x, "bottom": (ys >= h - 1) & (ys < h) & in_x}
        for side, hit in bands.items():
            assert hit.any(), (name, side)
        assert name != "camera-bands" or ((xs <= -1).any() and (xs >= w).any())  # ... and beyond them
    v = FS.reference(_row("camera-huge-focal"))["view"]
    over = np.abs(v["xs"][0]) * 32 >= 2.0 ** 30  # most coordinates overflow the remap's fixed point, the middle columns do not
    assert over.mean() > 0.5 and not over.all()


def test_fuse_rows_cover_the_depth_and_confidence_values():
    for name, which in (("bad-ref", [0]), ("bad-src", [1, 2, 3, 4, 5]), ("bad-both-mixed", [0, 1, 2, 3, 4])):
        views = FS.scene(_row(name))["views"]
        for i in which:
            d = views[i]["depth"]
            assert (d == 0).any() and (d < 0).any() and np.isnan(d).any() and np.isposinf(d).any(), (name, i)
    v = FS.reference(_row("rel-tie"))["view"]  # rel exactly on geo_depth_thres fails (the comparison is strict), one ulp below passes
    thr = np.float32(FS.THRESHOLDS[1])
    on, below = v["rel"][0] == thr, v["rel"][0] == np.nextafter(thr, np.float32(0.0))
    print("rel-tie: %d pixels on the threshold, %d one ulp below" % (on.sum(), below.sum()))
    assert on.sum() >= 5 and below.sum() >= 5 and not v["verdict"][0][on].any() and v["verdict"][0][below].all()
    assert not v["fragile"][0][on | below].any()
    sc = FS.scene(_row("conf-tie"))
    tie = sc["views"][0]["confidence"] == np.float32(FS.THRESHOLDS[2])
    assert tie.sum() > 100 and not FS.reference(_row("conf-tie"))["view"]["photo"][tie].any()  # the comparison is strict


def test_fuse_rows_cover_every_mask_value_and_the_claims():
    seen = {k: set() for k in ("photo", "geo", "final", "emit")}
    most_on = 0.0
    for r in FS.FUSE_ROWS:
        ref = FS.reference(r)
        for k in ("photo", "geo", "final"):
            seen[k] |= set(np.unique(ref["view"][k]).tolist())
        seen["emit"] |= set(np.unique(ref["merged"]["emit"]).tolist())
        most_on = max(most_on, float(ref["view"]["geo"].mean()))
        if r.prefill:
            pre = ref["merged_prefilled"]
            assert (ref["view"]["final"] & ~pre["emit"]).any() and pre["emit"].any(), r.id  # earlier claims do skip pixels
            assert (pre["claimed_after"] != FS.scene(r)["prefilled"]).any(), r.id            # ... and new ones are laid
    assert all(s == {False, True} for s in seen.values()), seen
    assert most_on > 0.5
    assert FS.reference(_row("40x72"))["view"]["geo"].mean() > 0.5
    for name in ("spikes", "spikes-mixed"):
        assert FS.reference(_row(name))["merged"]["rejected"] > 0, name  # the claim's own depth test turns a certain claim down
    assert sum(FS.reference(r)["merged"]["claimed_after"].sum() > 0 for r in FS.FUSE_ROWS) > len(FS.FUSE_ROWS) // 2


@pytest.mark.parametrize("row", [r for r in FS.FUSE_ROWS if r.friendly and r.n_src > 0], ids=lambda r: r.id)
def test_reference_agrees_with_the_fusion_oracle_on_decided_pixels(row):
    """Pins tests/fusion_ref64.py to oracle/fusion_oracle.py (itself pinned against the reference project): on decided pixels the
    float64 numpy evaluation has to give the same counts, masks and -- bit for bit -- averaged depth; its world points lie within one
    float32 ulp (plus the magnitude window) of the reference's."""
    sc, ref = FS.scene(row), FS.reference(row)["view"]
    thr = sc["thresholds"]
    want = FO.fuse_view(sc["views"][0], sc["views"][1:], *thr)
    ok = ref["decided"]
    np.testing.assert_array_equal(ref["photo"], want["photo"])
    for k in ("geo_sum", "geo", "final"):
        np.testing.assert_array_equal(ref[k][ok], want[k][ok], err_msg=k)
    assert ref["depth_avg"][ok].tobytes() == want["depth_avg"][ok].tobytes()
    assert int(np.abs(ref["geo_sum"] - want["geo_sum"])[~ok].max(initial=0)) <= int(ref["n_fragile"].max(initial=0))
    both = ok & ref["final"] & want["final"]
    idx = np.cumsum(want["final"].reshape(-1)) - 1
    got, exp = want["vertices"][idx[both.reshape(-1)]].astype(np.float64), ref["xyz"][both].astype(np.float64)
    assert (np.abs(got - exp) <= R64.ulp32(ref["xyz"][both]) + ref["xyz_slack"][both]).all()


def test_fragile_share_is_under_its_cap():
    total = [0, 0]
    for r in FS.FUSE_ROWS:
        a, b = FS.fragile_share(r)
        print("FRAGILE %-32s %6d of %8d  %.2e" % (r.id, a, b, a / max(b, 1)))
        assert a <= FRAGILE_CAP * b, (r.id, a, b)
        total[0] += a
        total[1] += b
    print("FRAGILE %-32s %6d of %8d  %.2e" % ("table", total[0], total[1], total[0] / total[1]))
    assert total[0] <= FRAGILE_CAP * total[1]
    assert R64.W_REL == 2.0 ** -40 and R64.W_MAG == 2.0 ** -45


def test_fragile_rule_on_hand_made_values():
    L = np.longdouble
    one = L(1)
    mid = one + L(2.0 ** -24)  # the midpoint between 1 and the next float32
    v = np.array([mid, mid * (1 + L(2.0 ** -41)), mid * (1 + L(2.0 ** -39)), one, L(np.inf), L(np.nan)], L)
    assert R64._near_f32_boundary(v, R64.W_REL * np.abs(v)).tolist() == [True, True, False, False, False, False]
    # a coordinate whose float32 cast may fall either way matters only where cvRound(32 f) or rintf(f) changes
    b = np.float32(17.5 / 32)  # cvRound(32 b) = 18, of the float32 below it 17: the midpoint between the two is unstable
    tie = (L(b) + L(np.nextafter(b, np.float32(0)))) / 2
    v = np.array([tie, L(b), mid, L(3e9) + L(128)], L)  # (3e9 + 128: a float32 midpoint far beyond |32 f| < 2^30)
    assert R64._coordinate_unstable(v, np.array([L(2.0 ** -45)] * 4, L)).tolist() == [True, False, False, False]


def test_pack_rows_cover_the_counts_masks_and_forms():
    rows = FS.PACK_ROWS
    assert {1, 3, 4, 5, 1023, 1024, 1025, 2 ** 20, 2 ** 20 + 1} <= {r.H * r.W for r in rows}
    assert {"zeros", "ones", "p01", "p5", "last"} <= {r.mask for r in rows}
    for n in (1, 3, 4, 5, 1023, 1024, 1025):
        forms = {(r.float_image, r.normals) for r in rows if r.H * r.W == n}
        assert len(forms) >= 2 and {r.rot_stride for r in rows if r.H * r.W == n and r.normals} <= {3, 4}
    assert {3, 4} <= {r.rot_stride for r in rows if r.normals}
    assert {"exact", "short", "roomy"} <= {r.capacity for r in rows}
    assert any(r.cursor0 > 0 and r.capacity == "short" for r in rows) and any(r.second for r in rows)
    assert any(r.H * r.W > 2 ** 20 and r.mask == "p5" for r in rows)  # the scan's carry between 1024-block chunks, with points behind it
    pool = FS.colour_pool()
    assert 0.0 in pool and 1.0 in pool and pool.min() >= 0 and pool.max() <= 1
    k = (pool * 255).astype(np.uint8)
    below = np.nextafter(np.float32(128.0) / np.float32(255.0), np.float32(0.0))
    assert below in pool and int((np.array([below]) * 255).astype(np.uint8)[0]) == 127 and {0, 127, 128, 254, 255} <= set(k.tolist())


def test_pack_reference_on_a_hand_made_view():
    xyz = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    view = dict(mask=np.array([[0, 7, 0], [1, 0, 255]], np.uint8), xyz=xyz,
                image=np.array([[[0, 0, 0], [1.0, 0.5, 0.0], [0, 0, 0]], [[0.999, 0.2, 1.0], [0, 0, 0], [0.25, 0.75, 0.1]]], np.float32),
                normals=np.stack([np.full((2, 3), 1.0), np.zeros((2, 3)), np.full((2, 3), -2.0)]).astype(np.float32))
    view["normals"][:, 1, 0] = 0
    rot = np.array([[0, 1, 0, 9], [0, 0, 1, 9], [1, 0, 0, 9], [9, 9, 9, 9]], np.float32)
    rec = FS.pack_reference(view, rot)
    assert rec.shape == (3, 27) and rec.dtype == np.uint8
    assert rec[:, :12].copy().view(np.float32).tolist() == [[3, 4, 5], [9, 10, 11], [15, 16, 17]]
    assert rec[:, 12:24].copy().view(np.float32).tolist() == [[0, -2, 1], [0, 0, 0], [0, -2, 1]]
    assert rec[:, 24:].tolist() == [[255, 127, 0], [254, 51, 255], [63, 191, 25]]
    assert FS.pack_reference({k: v for k, v in view.items() if k != "normals"}, None).shape == (3, 15)
