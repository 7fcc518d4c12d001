"""Every row of the fusion kernel space (tests/fusion_space.py) on the device.

pmn_fuse_view and pmn_fuse_view_merged against the extended-precision reference tests/fusion_ref64.py, per pixel: the photometric
mask everywhere; on DECIDED pixels (no source within the rounding window of a float32 cast or of geo_pixel_thres) geo_sum, the
geometric and final masks, the float64 averaged depth and the emit flag bit for bit, and the world point of a final pixel within one
float32 ulp (plus the magnitude window, fusion_ref64's docstring); on the other pixels geo_sum within the number of fragile sources;
the claim bytes equal to the reference's except those only uncertain pixels could set, the bytes no view owns untouched; the merged
entry point's masks and points equal to the plain one's bit for bit.  No share-of-pixels tolerance anywhere.

pmn_pack_points and pmn_pack_points_normals against numpy byte for byte: the whole record buffer including the bytes before the
starting cursor and behind the capacity, the per-view counts and the cursor."""
import ctypes

import numpy as np
import pytest
import torch

import fusion_ref64 as R64
import fusion_space as FS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ops():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import ops
    return ops


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_kind(got, want):
    """Non-finite components match in kind: NaN with NaN, an infinity with the infinity of the same sign."""
    return (np.isnan(got) == np.isnan(want)).all() and (np.isinf(got) == np.isinf(want)).all() \
        and (np.sign(got[np.isinf(got)]) == np.sign(want[np.isinf(got)])).all()


@pytest.mark.parametrize("row", FS.FUSE_ROWS, ids=[r.id for r in FS.FUSE_ROWS])
def test_fuse_row_against_the_reference(row):
    ops = _ops()
    sc, ref = FS.scene(row), FS.reference(row)
    view = ref["view"]
    args = (t(sc["maps"]), sc["ref_slot"], list(sc["src_slots"]), t(sc["mats"])) + tuple(sc["thresholds"])
    masks_d, xyz_d, davg, gsum = ops.fuse_view(*args, want_depth_avg=True, want_geo_sum=True, sizes=sc["sizes"])
    torch.cuda.synchronize()
    masks, xyz, davg, gsum = masks_d.cpu().numpy().astype(bool), xyz_d.cpu().numpy(), davg.cpu().numpy(), gsum.cpu().numpy()
    assert set(np.unique(masks_d.cpu().numpy()).tolist()) <= {0, 1}
    ok = view["decided"]
    print("ROW %s: %d pixels, %d undecided, %d fragile entries; geo on %.2f, final on %.2f"
          % (row.id, ok.size, int((~ok).sum()), int(view["fragile"].sum()), view["geo"].mean(), view["final"].mean()))
    np.testing.assert_array_equal(masks[0], view["photo"])
    np.testing.assert_array_equal(gsum[ok], view["geo_sum"][ok])
    np.testing.assert_array_equal(masks[1][ok], view["geo"][ok])
    np.testing.assert_array_equal(masks[2][ok], view["final"][ok])
    assert davg[ok].tobytes() == view["depth_avg"][ok].tobytes()
    assert (np.abs(gsum - view["geo_sum"])[~ok] <= view["n_fragile"][~ok]).all()
    keep = ok & view["final"]
    got, want = xyz[keep], view["xyz"][keep]
    assert _same_kind(got, want)
    fin = np.isfinite(want)
    err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    bound = R64.ulp32(want[fin]) + view["xyz_slack"][keep][fin]
    print("ROW %s: world points: %d components, %d differ, largest error / bound %.3f"
          % (row.id, err.size, int((err > 0).sum()), float((err / bound).max(initial=0.0))))
    assert (err <= bound).all()
    # the merged entry point: on empty claims, and on claims an earlier part of the scan has left
    passes = [("merged", FS.empty_claims(row))] + ([("merged_prefilled", sc["prefilled"])] if row.prefill else [])
    for key, before in passes:
        claimed = t(before)
        m2, xyz2, emit = ops.fuse_view_merged(*args, claimed, sizes=sc["sizes"])
        torch.cuda.synchronize()
        assert torch.equal(m2, masks_d)
        assert xyz2.cpu().numpy().tobytes() == xyz.tobytes()  # (bytes: the NaN points of invalid pixels compare too)
        want = ref[key]
        emit = emit.cpu().numpy()
        assert set(np.unique(emit).tolist()) <= {0, 1}
        np.testing.assert_array_equal(emit.astype(bool)[ok], want["emit"][ok])
        np.testing.assert_array_equal(emit.astype(bool), masks[2] & (before[sc["ref_slot"]][:ok.size].reshape(ok.shape) == 0))
        after, maybe = claimed.cpu().numpy(), want["maybe"]
        np.testing.assert_array_equal(after[~maybe], want["claimed_after"][~maybe])
        assert ((after[maybe] == before[maybe]) | (after[maybe] == 1)).all()
        assert after[sc["ref_slot"]].tobytes() == before[sc["ref_slot"]].tobytes()
        for s, (h, w) in enumerate(sc["sizes"]):
            assert (after[s, h * w:] == FS.CLAIM_SENTINEL).all()
        print("ROW %s %s: %d claim bytes set, %d uncertain, %d certain claims rejected by the depth test"
              % (row.id, key, int((after != before).sum()), int(maybe.sum()), want["rejected"]))


def test_more_than_max_sources_is_a_shape_error():
    """n_src = PMN_MAX_FUSE_SRC + 1 through the C ABI: PMN_ERR_SHAPE (-2) from both entry points, nothing launched."""
    _ops()
    from patchmatchnet_amd import _lib
    L = _lib.lib()
    n = _lib.MAX_FUSE_SRC + 1
    H, W = 9, 33
    maps = torch.ones((n + 1, 2 * H * W), device=DEV)
    mats = torch.zeros((48 + 64 * n,), device=DEV)
    masks = torch.full((3, H, W), 0x55, dtype=torch.uint8, device=DEV)
    emit = torch.full((H, W), 0x55, dtype=torch.uint8, device=DEV)
    xyz = torch.zeros((H, W, 3), device=DEV)
    claimed = torch.zeros((n + 1, H * W), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(k, merged):
        slots = (ctypes.c_int * k)(*range(1, k + 1))
        sizes = (ctypes.c_int * (2 * k))(*([H, W] * k))
        head = (maps.data_ptr(), maps.shape[1], 0, ctypes.addressof(slots), ctypes.addressof(sizes), k, mats.data_ptr(), H, W, 1.0, 0.01,
                1, 0.5, masks.data_ptr(), xyz.data_ptr(), None, None)
        if merged:
            return L.pmn_fuse_view_merged(*head, claimed.data_ptr(), H * W, emit.data_ptr(), stream)
        return L.pmn_fuse_view(*head, stream)

    assert call(n, False) == -2 and call(n, True) == -2
    torch.cuda.synchronize()
    assert bool((masks == 0x55).all()) and bool((emit == 0x55).all()) and not bool(claimed.any())
    assert call(n - 1, False) == 0 and call(n - 1, True) == 0  # PMN_MAX_FUSE_SRC itself launches
    torch.cuda.synchronize()
    assert not bool((masks == 0x55).any()) and not bool((emit == 0x55).any())


@pytest.mark.parametrize("row", FS.PACK_ROWS, ids=[r.id for r in FS.PACK_ROWS])
def test_pack_row_byte_for_byte(row):
    ops = _ops()
    from patchmatchnet_amd._lib import PmnError
    x = FS.pack_inputs(row)
    rec, guard, fill = (27 if row.normals else 15), 64, 0xAA
    packer = ops.PointPacker(x["capacity"] + guard, torch.device(DEV), max_views=4, normals=row.normals)
    packer.capacity = x["capacity"]  # what the kernels are told; the ``guard`` records behind it have to stay as they are
    packer.records.fill_(fill)
    packer.cursor.fill_(row.cursor0)
    packer.view_counts.fill_(-7)
    rot = t(x["rotation"]) if row.normals else None
    assert rot is None or rot.stride(0) == row.rot_stride
    for v in x["views"]:
        packer.append(t(v["mask"]), t(v["xyz"]), t(v["image"]), t(v["normals"]) if row.normals else None, rot)
    torch.cuda.synchronize()
    want = np.full(rec * (x["capacity"] + guard), fill, np.uint8)
    at, counts = row.cursor0, []
    for records in x["want"]:
        if at + len(records) > x["capacity"]:
            counts.append(-1)  # refused: nothing written, the cursor stays
            continue
        want[rec * at:rec * (at + len(records))] = records.reshape(-1)
        at += len(records)
        counts.append(len(records))
    got_counts = packer.view_counts.cpu().tolist()
    print("PACK %s: %s points of %s pixels, counts %s, cursor %d -> %d"
          % (row.id, x["totals"], [v["mask"].size for v in x["views"]], got_counts[:len(counts)], row.cursor0, int(packer.cursor)))
    assert got_counts == counts + [-7] * (4 - len(counts))
    assert int(packer.cursor) == at
    assert (row.capacity == "short") == (-1 in counts)
    assert packer.records.cpu().numpy().tobytes() == want.tobytes()
    if -1 in counts:
        with pytest.raises(PmnError, match="too small"):
            packer.counts()
    else:
        assert packer.counts() == counts
