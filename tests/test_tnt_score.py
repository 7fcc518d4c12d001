"""CPU checks of the Tanks and Temples score's host side (patchmatchnet_amd/registration.py, eval_tnt.py): the file readers, the
closed-form alignments, the command line and the ABI table.  Nothing here needs a GPU."""
import json
import os
import re
import sys

import numpy as np
import pytest

import tnt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def scene():
    return R.synthetic_scene(0)


def _write_log(path, mats):
    with open(path, "w") as f:
        for i, T in enumerate(mats):
            f.write(f"{i} {i} 0\n")
            for row in T:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")


def test_readers_round_trip(tmp_path, scene):
    from patchmatchnet_amd import registration as RG
    _write_log(tmp_path / "a.log", scene["traj_est"])
    got = RG.read_trajectory_log(str(tmp_path / "a.log"))
    assert got.shape == (12, 4, 4) and np.array_equal(got, scene["traj_est"])
    poly, axis, lo, hi = scene["volume"]
    with open(tmp_path / "crop.json", "w") as f:
        json.dump({"class_name": "SelectionPolygonVolume", "bounding_polygon": poly.tolist(), "orthogonal_axis": "Z", "axis_min": lo,
                   "axis_max": hi, "version_major": 1, "version_minor": 0}, f)
    vol = RG.read_crop_json(str(tmp_path / "crop.json"))
    assert np.array_equal(vol.polygon, poly) and vol.axis == 2 and vol.axis_min == lo and vol.axis_max == hi
    np.savetxt(tmp_path / "trans.txt", scene["gt_trans"], fmt="%.17g")
    assert np.array_equal(RG.read_transform(str(tmp_path / "trans.txt")), scene["gt_trans"])
    # malformed files are named
    with open(tmp_path / "bad.log", "w") as f:
        f.write("0 0 0\n1 0 0 0\n0 1 0 0\n")
    with pytest.raises(ValueError, match="bad.log"):
        RG.read_trajectory_log(str(tmp_path / "bad.log"))
    with open(tmp_path / "bad.json", "w") as f:
        json.dump({"bounding_polygon": poly.tolist(), "orthogonal_axis": "Z", "axis_min": lo}, f)
    with pytest.raises(ValueError, match="axis_max"):
        RG.read_crop_json(str(tmp_path / "bad.json"))
    np.savetxt(tmp_path / "bad.txt", np.eye(3))
    with pytest.raises(ValueError, match="4 x 4"):
        RG.read_transform(str(tmp_path / "bad.txt"))


def test_umeyama_recovers_the_similarity_of_the_trajectories(scene):
    from patchmatchnet_amd import registration as RG
    a, b = scene["traj_est"][:, :3, 3], scene["traj_gt"][:, :3, 3]
    T = RG.umeyama(a, b, with_scale=True)
    S = scene["similarity"]
    assert np.abs(T - S).max() <= 1e-12 * np.abs(S).max()
    assert np.array_equal(T[3], [0, 0, 0, 1])
    # rigid: the rotation part is orthonormal even though the clouds differ in scale
    Rg = RG.umeyama(a, b, with_scale=False)[:3, :3]
    assert np.abs(Rg @ Rg.T - np.eye(3)).max() < 1e-14 and np.linalg.det(Rg) > 0
    # a mirrored target still gives a proper rotation (the reflection fix)
    Rm = RG.umeyama(a, b * np.array([1.0, 1.0, -1.0]), with_scale=False)[:3, :3]
    assert abs(np.linalg.det(Rm) - 1.0) < 1e-12
    with pytest.raises(RG.PmnError):
        RG.umeyama(a[:2], b[:2])


def test_kabsch_step_from_the_seventeen_sums(scene):
    from patchmatchnet_amd import registration as RG
    rng = np.random.default_rng(3)
    p = rng.standard_normal((200, 3))
    q = R.apply_pose(scene["motion"], p) + 1e-3 * rng.standard_normal((200, 3))
    centre = np.array([0.3, -0.2, 0.7])
    a, b = p - centre, q - centre
    sums = np.concatenate([[200.0], a.sum(0), b.sum(0), (a[:, :, None] * b[:, None, :]).sum(0).reshape(-1), [((p - q) ** 2).sum()]])
    got = RG.kabsch_from_sums(sums, centre)
    want = R.kabsch(p, q)
    assert np.abs(got - want).max() < 1e-12
    assert np.abs(got - scene["motion"]).max() < 1e-3
    with pytest.raises(RG.PmnError, match="3"):
        RG.kabsch_from_sums(np.r_[2.0, np.zeros(16)], centre)


def test_cli_parser():
    import eval_tnt
    base = ["--dataset_dir", "/data/Barn", "--ply_path", "fused.ply", "--results_path", "out"]
    a = eval_tnt.parse_args(base + ["--mvs_folder", "mvs"])
    assert a.scene == "Barn" and a.tau == 0.01 and a.max_points == 4_000_000 and a.hist_max is None and not a.no_registration
    assert a.round_a == [1.0, 80.0] and a.round_b == [0.5, 20.0] and a.round_c_dist == 2.0 and a.icp_iterations == 20
    a = eval_tnt.parse_args(["--dataset_dir", "/data/x", "--ply_path", "p", "--results_path", "o", "--tau", "0.5", "--no_registration"])
    assert a.scene == "x" and a.tau == 0.5
    assert eval_tnt.parse_args(base + ["--scene", "Truck", "--no_registration"]).tau == 0.005
    for bad in (["--dataset_dir", "/data/unknown", "--ply_path", "p", "--results_path", "o", "--no_registration"],  # no tau for the scene
                base,                                                                                               # no cameras
                base[2:] + ["--no_registration"]):                                                                  # no dataset_dir
        with pytest.raises(SystemExit):
            eval_tnt.parse_args(bad)


def test_signature_table_and_header():
    from patchmatchnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pmn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("pmn_icp_accumulate", "pmn_voxel_mean", "pmn_crop_prism"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    for macro, value in (("PMN_ICP_SUMS", _lib.ICP_SUMS), ("PMN_ICP_LIMBS", _lib.ICP_LIMBS), ("PMN_ICP_BLOCK_POINTS", _lib.ICP_BLOCK_POINTS),
                         ("PMN_VOXEL_LONG_RUN", _lib.VOXEL_LONG_RUN), ("PMN_VOXEL_MAX_CHANNELS", _lib.VOXEL_MAX_CHANNELS),
                         ("PMN_CROP_MAX_VERTICES", _lib.CROP_MAX_VERTICES)):
        assert f"#define {macro} {value}\n" in hdr
    assert _lib.ICP_SUMS == 17 and R.LONG_RUN == _lib.VOXEL_LONG_RUN
    assert _lib.icp_scratch(1) == 85 and _lib.icp_scratch(256) == 85 and _lib.icp_scratch(257) == 170
    assert "Added under ABI 25" in hdr[hdr.index("pmn_raster_resolve("):] and _lib.ABI_VERSION == 25


def test_bad_arguments_are_refused_before_any_launch():
    """The entry points check their arguments on the host (no GPU needed to see the error code); the module has no CPU path."""
    import torch

    from patchmatchnet_amd import _lib, registration as RG
    L = _lib.lib()
    assert L.pmn_icp_accumulate(None, None, 1, None, 1.0, None, None, None, 1, None, None, 1.0, None, 0, None, None) == -1
    assert L.pmn_voxel_mean(None, None, 0, 1, None, 1, None, None, None) == -1
    assert L.pmn_crop_prism(None, 1, None, 3, 0, 0.0, 1.0, None, None, None) == -1
    pts = torch.zeros(4, 3)
    vol = RG.CropVolume(R.POLYGON, 2, 0.0, 1.0)
    with pytest.raises(RG.PmnError, match="no CPU fallback"):
        RG.crop(pts, vol)
    with pytest.raises(RG.PmnError, match="no CPU fallback"):
        RG.voxel_downsample(pts, 0.1)
    with pytest.raises(RG.PmnError, match="no CPU fallback"):
        RG.tnt_score(pts, pts, vol, 0.01)


def test_reference_scene_has_no_ties_at_tau(scene):
    """The seed of the GPU test of tnt_score: the reference's initial transform is the known motion."""
    init = scene["gt_trans"] @ R.kabsch(scene["traj_est"][:, :3, 3], scene["traj_gt"][:, :3, 3], True)
    assert np.abs(init - scene["motion"]).max() < 1e-12
    poly, axis, lo, hi = scene["volume"]
    m = R.crop_mask(scene["gt"], poly, axis, lo, hi)
    assert 0.3 * len(m) < m.sum() < 0.95 * len(m)
