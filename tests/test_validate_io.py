"""CPU tests of validation against ground-truth depth (train.py --mode test): the dataset's ground-truth path, the host aggregation of
pmn_depth_metrics rows into the reference's scalars, the row layout shared by header and binding, and the command line."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _train_cli():
    """This repository's train.py, loaded by path (a bare ``import train`` can find another checkout's file first on sys.path)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pmn_train_cli", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_scan(root, scan="scan1", n_views=3, H=24, W=32, depth_min="425.0"):
    from PIL import Image
    d = os.path.join(root, scan)
    for sub in ("images", "cams", "depth_gt"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    rng = np.random.default_rng(0)
    for v in range(n_views):
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(os.path.join(d, "images", "{:0>8}.jpg".format(v)))
        with open(os.path.join(d, "cams", "{:0>8}_cam.txt".format(v)), "w") as f:
            f.write("extrinsic\n1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n\nintrinsic\n%f 0 %f\n0 %f %f\n0 0 1\n\n%s 935.0\n"
                    % (W, W / 2, W, H / 2, depth_min))
    with open(os.path.join(d, "pair.txt"), "w") as f:
        f.write("%d\n" % n_views)
        for v in range(n_views):
            others = [u for u in range(n_views) if u != v]
            f.write("%d\n%d " % (v, len(others)) + " ".join("%d 1.0" % u for u in others) + "\n")
    with open(os.path.join(root, "list.txt"), "w") as f:
        f.write(scan + "\n")
    return d


def _dataset(root, **kw):
    from patchmatchnet_amd.mvs import MVSDataset
    return MVSDataset(root, scan_list=os.path.join(root, "list.txt"), **kw)


def _write_gt(root, scan, v, gt):
    from patchmatchnet_amd import data_io
    data_io.save_pfm(os.path.join(root, scan, "depth_gt", "{:0>8}.pfm".format(v)), np.asarray(gt, np.float32))


# ---- the dataset's ground truth --------------------------------------------------------------------------------------------------

def test_ground_truth_values_mask_and_missing_file(tmp_path):
    root = str(tmp_path)
    _write_scan(root, depth_min="425.1")  # 425.1 is not a float32: the mask compares with the float32 the camera file parses to
    dmin = np.float32(425.1)
    gt = np.linspace(400.0, 900.0, 24 * 32, dtype=np.float32).reshape(24, 32)
    gt[3, 4] = dmin                               # exactly depth_min: valid
    gt[3, 5] = np.nextafter(dmin, np.float32(0))  # one ulp below: not valid
    gt[3, 6] = np.nan
    _write_gt(root, "scan1", 0, gt)
    _write_gt(root, "scan1", 1, gt[::-1].copy())
    ds = _dataset(root, num_views=2, load_depth_gt=True)
    s = ds[0]
    assert s["depth_gt"].shape == (1, 24, 32) and s["depth_gt"].dtype == np.float32
    np.testing.assert_array_equal(s["depth_gt"][0], gt)
    assert s["mask"].dtype == bool and s["mask"].shape == (1, 24, 32)
    np.testing.assert_array_equal(s["mask"][0], gt >= dmin)
    assert s["mask"][0, 3, 4] and not s["mask"][0, 3, 5] and not s["mask"][0, 3, 6]
    assert type(s["depth_min"]) is np.float32 and s["depth_min"] == dmin
    np.testing.assert_array_equal(ds[1]["depth_gt"][0], gt[::-1])
    # the view without a file: the reference's empty arrays, and the dataset names it
    s2 = ds[2]
    assert s2["depth_gt"].shape == (0,) and s2["mask"].shape == (0,)
    assert ds.missing_depth_gt() == [("scan1", 2)]


def test_ground_truth_is_resized_like_the_images(tmp_path):
    from patchmatchnet_amd import data_io
    root = str(tmp_path)
    _write_scan(root, H=48, W=64)
    rng = np.random.default_rng(1)
    gt = (500.0 + 100.0 * rng.random((48, 64))).astype(np.float32)
    _write_gt(root, "scan1", 0, gt)
    s = _dataset(root, num_views=2, max_dim=40, load_depth_gt=True)[0]
    assert s["images"][0].shape == (3, 30, 40)
    assert s["depth_gt"].shape == (1, 30, 40)
    want = data_io.resize_bilinear(gt[..., None], 30, 40)[..., 0]
    np.testing.assert_array_equal(s["depth_gt"][0], want)
    np.testing.assert_array_equal(s["mask"][0], want >= np.float32(425.0))


def test_samples_without_the_flag_are_unchanged(tmp_path):
    root = str(tmp_path)
    _write_scan(root)
    _write_gt(root, "scan1", 0, np.full((24, 32), 600.0, np.float32))
    plain, with_gt = _dataset(root, num_views=2)[0], _dataset(root, num_views=2, load_depth_gt=True)[0]
    assert set(plain) == {"images", "intrinsics", "extrinsics", "depth_min", "depth_max", "ref_view", "view_ids", "scan", "light",
                          "filename"}
    assert set(with_gt) == set(plain) | {"depth_gt", "mask"}
    for k, v in plain.items():
        w = with_gt[k]
        if k == "images":
            for a, b in zip(v, w):
                np.testing.assert_array_equal(a, b)
        elif isinstance(v, np.ndarray):
            np.testing.assert_array_equal(v, w)
        else:
            assert v == w and type(v) is type(w), k


# ---- the row layout and the host aggregation -------------------------------------------------------------------------------------

def test_row_layout_matches_the_header():
    from patchmatchnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pmn_hip.h")).read()
    for name, value in (("MAX_STAGES", _lib.METRICS_MAX_STAGES), ("MAX_ITERS", _lib.METRICS_MAX_ITERS),
                        ("MAX_THRESHOLDS", _lib.METRICS_MAX_THRESHOLDS), ("COUNT", _lib.METRICS_COUNT), ("ABS", _lib.METRICS_ABS),
                        ("THR", _lib.METRICS_THR), ("SL1", _lib.METRICS_SL1), ("ROW", _lib.METRICS_ROW),
                        ("PIXELS_PER_BLOCK", _lib.METRICS_PIXELS_PER_BLOCK), ("MAX_BLOCKS", _lib.METRICS_MAX_BLOCKS)):
        assert re.search(r"#define PMN_METRICS_%s %d\b" % (name, value), hdr), name
    assert (MR.ROW, MR.COUNT, MR.ABS, MR.THR, MR.SL1, MR.MAX_ITERS) == (
        _lib.METRICS_ROW, _lib.METRICS_COUNT, _lib.METRICS_ABS, _lib.METRICS_THR, _lib.METRICS_SL1, _lib.METRICS_MAX_ITERS)
    # the layout fits: counts, sums and thresholds do not overlap
    assert _lib.METRICS_ABS >= _lib.METRICS_MAX_STAGES and _lib.METRICS_THR >= _lib.METRICS_ABS + _lib.METRICS_MAX_STAGES
    assert _lib.METRICS_SL1 >= _lib.METRICS_THR + _lib.METRICS_MAX_THRESHOLDS
    assert _lib.METRICS_ROW == _lib.METRICS_SL1 + _lib.METRICS_MAX_STAGES * _lib.METRICS_MAX_ITERS
    assert _lib.metrics_scratch(3, 512, 640) == 3 * 80 * 36 and _lib.metrics_scratch(1, 1200, 1600) == 128 * 36
    assert _lib.metrics_scratch(2, 1, 1) == 2 * 36


def _batch(rng, B, H, W, iters, empty=()):
    gt = (500.0 + 60.0 * rng.random((B, H, W))).astype(np.float32)
    dmin = np.full(B, 505.0, np.float32)
    for b in empty:
        gt[b] = 400.0
    maps = [[(gt[:, ::1 << s, ::1 << s][:, :H >> s, :W >> s] + rng.normal(0, 1.0 + 2 * s, (B, H >> s, W >> s))).astype(np.float32)
             for _ in range(n)] for s, n in enumerate(iters)]
    gt[:, 0, :8] = np.where(gt[:, 0, :8] >= dmin[:, None], np.float32(520.0), gt[:, 0, :8])
    maps[0][-1][:, 0, :8] = gt[:, 0, :8] + np.asarray([-8, 8, 4, -4, 2, -2, 1, -1], np.float32)  # |d - gt| exactly at the thresholds
    return gt, dmin, maps


@pytest.mark.parametrize("iters", [(1, 1, 2, 2), (1, 2, 2, 2)])
def test_batch_scalars_are_the_reference_formulas(iters):
    """rows (stated in numpy) -> batch_scalars == the reference's torch formulas; the last batch is partial (equal weight per
    batch, DictAverageMeter) and one of its images has an empty mask (NaN, as torch's mean of an empty tensor)."""
    from patchmatchnet_amd import validate as V
    rng = np.random.default_rng(7)
    avg, want_avg = V.DictAverage(), {}
    batches = [(3, ()), (3, (1,)), (1, ())]
    for bi, (B, empty) in enumerate(batches):
        gt, dmin, maps = _batch(rng, B, 32, 40, iters, empty)
        rows = MR.rows_numpy(gt, dmin, maps, V.THRESHOLDS)
        got = V.batch_scalars(rows, list(iters))
        gt_t = torch.from_numpy(gt)[:, None]
        mask_t = gt_t >= torch.from_numpy(dmin)[:, None, None, None]
        want = MR.reference_scalars({s: [torch.from_numpy(m)[:, None] for m in ms] for s, ms in enumerate(maps)}, gt_t, mask_t)
        MR.assert_close_dict(got, want, 1e-5)
        if empty:
            assert math.isnan(got["depth-error-stage-0"]) and math.isnan(got["threshold-1mm-error"])
            assert not math.isnan(got["loss"])  # the loss pools the batch's pixels
        avg.update(got)
        for k, v in want.items():
            want_avg[k] = want_avg.get(k, 0.0) + v
    mean = avg.mean()
    for k, v in want_avg.items():
        w = v / len(batches)
        assert (math.isnan(w) and math.isnan(mean[k])) or abs(mean[k] - w) <= 1e-5 * abs(w) + 1e-12, k


def test_aggregation_by_hand():
    """Two images, hand-made rows: per-image means, the batch mean, and the pooled loss."""
    from patchmatchnet_amd import _lib
    from patchmatchnet_amd import validate as V
    rows = np.zeros((2, _lib.METRICS_ROW))
    rows[:, 0:4] = [[10, 4, 1, 1], [30, 6, 2, 0]]            # valid pixels per stage (image 1: stage 3 empty)
    rows[:, 4:8] = [[5, 2, 1, 3], [60, 3, 4, 0]]             # sum |d - gt| of each stage's last map
    rows[:, 8:12] = [[2, 1, 0, 0], [15, 3, 3, 0]]            # above 1, 2, 4, 8 at stage 0
    rows[:, 16] = [1, 3]                                     # stage 0
    rows[:, 21:23] = [[2, 4], [2, 6]]                        # stage 1, two iterations
    rows[:, 26] = [1, 1]                                     # stage 2
    rows[:, 31] = [9, 0]                                     # stage 3
    got = V.batch_scalars(rows, [1, 2, 1, 1])
    assert got["loss"] == pytest.approx(4 / 40 + 4 / 10 + 10 / 10 + 2 / 3 + 9 / 1)
    assert got["depth-error-stage-0"] == pytest.approx((5 / 10 + 60 / 30) / 2)
    assert got["depth-error-stage-1"] == pytest.approx((2 / 4 + 3 / 6) / 2)
    assert math.isnan(got["depth-error-stage-3"])
    assert got["threshold-1mm-error"] == pytest.approx((2 / 10 + 15 / 30) / 2)
    assert got["threshold-8mm-error"] == 0.0
    assert list(got) == ["loss"] + [f"depth-error-stage-{i}" for i in range(4)] + [f"threshold-{t}mm-error" for t in (1, 2, 4, 8)]
    per = V.image_metrics(rows[1], [1, 2, 1, 1])
    assert per["depth-error-stage-0"] == 2.0 and per["smooth-l1-stage-1-iter-1"] == 1.0 and math.isnan(per["depth-error-stage-3"])


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_cli_parses_the_reference_flags():
    train = _train_cli()
    a = train.build_parser().parse_args(["--mode", "test", "--input_folder", "d", "--test_list", "t.txt", "--train_list", "x.txt",
                                         "--epochs", "3", "--resume", "--lr_epochs", "1,2:2", "--patchmatch_iteration", "2", "2", "2"])
    assert a.mode == "test" and a.image_max_dim == 640 and a.batch_size == 12 and a.rand_seed == 1 and a.num_views == 5
    assert a.patchmatch_iteration == [2, 2, 2] and a.propagation_range == [6, 4, 2] and a.evaluate_neighbors == [9, 9, 9]
    assert a.hip_graph == 1 and a.metrics_json == ""
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--hip_graph", "2"])
    assert "torchrun" in train.build_parser().format_help()


def test_train_mode_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--mode", "train", "--input_folder", ROOT],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and "not supported" in lines[0], r.stderr


def test_latest_checkpoint(tmp_path):
    train = _train_cli()
    assert train.find_latest_checkpoint(str(tmp_path)) == ""
    for n in ("params_000002.ckpt", "params_000010.ckpt", "params_000009.ckpt", "module_000011.pt", "notes.txt"):
        (tmp_path / n).write_bytes(b"")
    assert train.find_latest_checkpoint(str(tmp_path)) == str(tmp_path / "params_000010.ckpt")


def test_missing_ground_truth_is_refused_by_name(tmp_path):
    train = _train_cli()
    root = str(tmp_path)
    _write_scan(root)
    _write_gt(root, "scan1", 0, np.full((24, 32), 600.0, np.float32))
    ckpt = os.path.join(ROOT, "tests", "golden", "params_000007.npz")
    with pytest.raises(Exception, match=r"2 of 3 samples have no ground-truth depth map \(scan1/depth_gt/00000001.pfm"):
        train.main(["--mode", "test", "--input_folder", root, "--test_list", os.path.join(root, "list.txt"), "--checkpoint_path", ckpt])
