"""CPU-side checks of the DTU score: the PLY / mask readers, the numpy reference (tests/dtu_ref.py) on hand-computable cases, the
command line's file discovery with the scoring stubbed, and the argument checks of the ABI-25 entry points (nothing launches)."""
import ctypes
import json
import os

import numpy as np
import pytest

import dtu_ref as R


# ---- PLY reader -----------------------------------------------------------------------------------------------------------------

def _cloud(n=37, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * 50).astype(np.float32), rng.integers(0, 256, (n, 3)).astype(np.uint8)


def test_reads_what_write_ply_writes(tmp_path):
    from patchmatchnet_amd import fusion, pointcloud as PC
    v, c = _cloud()
    path = str(tmp_path / "fused.ply")
    fusion.write_ply(path, v, c)
    got = PC.read_ply_vertices(path)
    assert got.dtype == np.float32 and got.shape == (37, 3) and got.flags["C_CONTIGUOUS"]
    assert (got == v).all()


def test_reads_ascii_big_endian_and_extra_properties(tmp_path):
    from patchmatchnet_amd import pointcloud as PC
    v, _ = _cloud(11, 1)
    asc = tmp_path / "a.ply"
    asc.write_text("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 11\nproperty float x\nproperty float y\nproperty float z\n"
                   "end_header\n" + "".join("%r %r %r\n" % tuple(float(t) for t in row) for row in v))
    assert (PC.read_ply_vertices(str(asc)) == v).all()
    # big-endian, normals between and after the coordinates, z before y, double x, faces after the vertices
    rec = np.zeros(11, np.dtype([("x", ">f8"), ("nx", ">f4"), ("z", ">f4"), ("y", ">f4"), ("red", "u1"), ("ny", ">f4")]))
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    rec["nx"], rec["ny"], rec["red"] = 7.0, -3.0, 200
    big = tmp_path / "b.ply"
    with open(big, "wb") as f:
        f.write(b"ply\nformat binary_big_endian 1.0\nelement vertex 11\nproperty double x\nproperty float nx\nproperty float z\n"
                b"property float y\nproperty uchar red\nproperty float ny\nelement face 2\nproperty list uchar int vertex_indices\n"
                b"end_header\n")
        rec.tofile(f)
        f.write(np.array([3, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 2], np.uint8).tobytes() * 2)
    assert (PC.read_ply_vertices(str(big)) == v).all()
    # ascii with colours and faces
    asc2 = tmp_path / "c.ply"
    asc2.write_text("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
                    "element face 1\nproperty list uchar int vertex_indices\nend_header\n1 2 3 255\n4 5.5 6 0\n3 0 1 0\n")
    assert PC.read_ply_vertices(str(asc2)).tolist() == [[1.0, 2.0, 3.0], [4.0, 5.5, 6.0]]


def test_ply_errors_name_the_file(tmp_path):
    from patchmatchnet_amd import pointcloud as PC
    bad = tmp_path / "list.ply"
    bad.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                    b"property list uchar int seen_by\nend_header\n")
    with pytest.raises(ValueError, match="list.ply"):
        PC.read_ply_vertices(str(bad))
    bad = tmp_path / "noz.ply"
    bad.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n" + b"\0" * 8)
    with pytest.raises(ValueError, match="noz.ply.*'z'"):
        PC.read_ply_vertices(str(bad))


# ---- mask loaders -----------------------------------------------------------------------------------------------------------------

def test_mat_and_npz_loaders_agree(tmp_path):
    sio = pytest.importorskip("scipy.io")
    from patchmatchnet_amd import pointcloud as PC
    s = R.synthetic_scan(3, n_stl=10, n_data=60)
    sio.savemat(str(tmp_path / "ObsMask1_10.mat"), {"ObsMask": s["ObsMask"], "BB": s["BB"], "Res": s["Res"]})
    sio.savemat(str(tmp_path / "Plane1.mat"), {"P": s["P"]})
    np.savez(str(tmp_path / "ObsMask1_10.npz"), ObsMask=s["ObsMask"], BB=s["BB"], Res=s["Res"])
    np.savez(str(tmp_path / "Plane1.npz"), P=s["P"])
    a = PC.load_obs_mask(str(tmp_path / "ObsMask1_10.mat"))
    b = PC.load_obs_mask(str(tmp_path / "ObsMask1_10.npz"))
    assert a[0].dtype == bool and (a[0] == b[0]).all() and (a[0] == s["ObsMask"]).all()
    assert (a[1] == b[1]).all() and (a[1] == s["BB"]).all() and a[2] == b[2] == s["Res"]
    pa, pb = PC.load_plane(str(tmp_path / "Plane1.mat")), PC.load_plane(str(tmp_path / "Plane1.npz"))
    assert pa.shape == (4,) and (pa == pb).all() and (pa == s["P"].reshape(4)).all()


def test_npz_loader_without_scipy_and_missing_field(tmp_path):
    from patchmatchnet_amd import pointcloud as PC
    np.savez(str(tmp_path / "m.npz"), ObsMask=np.ones((2, 3, 4), np.uint8), BB=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="Res"):
        PC.load_obs_mask(str(tmp_path / "m.npz"))
    with pytest.raises(FileNotFoundError):
        PC.load_plane(str(tmp_path / "absent.npz"))


# ---- the reference on hand-computable cases -----------------------------------------------------------------------------------------

def test_reduce_is_inclusive_at_dst():
    # 0.25 and 0.5 are exact in float32, so the pair is EXACTLY dst apart: rangesearch's <= removes the second point
    pts = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.75, 0.0, 0.0]], np.float32)
    assert R.reduce_points(pts, 0.25, [0, 1, 2]).tolist() == [True, False, True]
    assert R.reduce_points(pts, 0.25, [1, 0, 2]).tolist() == [False, True, True]
    assert R.reduce_points(pts, np.nextafter(0.25, 0), [0, 1, 2]).tolist() == [True, True, True]
    # the order decides: the middle point first removes both ends at dst = 0.5
    assert R.reduce_points(pts, 0.5, [1, 0, 2]).tolist() == [False, True, False]
    assert R.reduce_points(pts, 0.5, [0, 1, 2]).tolist() == [True, False, True]
    # duplicates are neighbours at distance 0
    assert R.reduce_points(np.zeros((3, 3), np.float32), 0.0, [2, 0, 1]).tolist() == [False, False, True]


def test_matlab_round_and_mask_indexing():
    assert R.matlab_round([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999999999999994, 2.4]).tolist() == [1, 2, 3, -1, -2, 0, 2]
    obs = np.zeros((3, 4, 5), bool)
    obs[0, 0, 0] = obs[2, 3, 4] = obs[1, 0, 0] = True
    bb = np.array([[10.0, 20.0, 30.0], [99.0, 99.0, 99.0]])
    q = np.array([[10.0, 20.0, 30.0],      # Qv = (1,1,1)
                  [9.5, 20.0, 30.0],       # (10 - 9.5) / 1 -> Qv.x = round(0.5) = 1: half a voxel below BB(1,:) is still voxel 1
                  [9.25, 20.0, 30.0],      # round(0.25) = 0: outside
                  [10.5, 20.0, 30.0],      # round(1.5) = 2
                  [12.0, 23.0, 34.0],      # (3,4,5): the last voxel
                  [12.5, 23.0, 34.0],      # round(3.5) = 4 > size
                  [11.0, 21.0, 30.0]], np.float32)  # (2,2,1): not set
    assert R.data_in_mask(q, obs, bb, 1.0).tolist() == [True, True, False, True, True, False, False]


def test_blocks_are_half_open_and_unblocked_points_keep_max_dist():
    bb = np.array([[0.0, 0.0, 0.0], [70.0, 50.0, 50.0]])  # Range = (1, 0, 0): blocks [0,60) and [60,120) in x, [0,60) in y and z
    to = np.array([[59.0, 1.0, 1.0]], np.float32)
    frm = np.array([[58.0, 1.0, 1.0],     # in block 0
                    [60.0, 1.0, 1.0],     # exactly on block 0's upper face: belongs to block 1, whose grown box still holds `to`
                    [119.5, 1.0, 1.0],    # block 1, distance 60.5: the MATLAB does not clamp
                    [120.0, 1.0, 1.0],    # on the last block's upper face: in no block
                    [58.0, 60.0, 1.0],    # y on the upper face of the only y block: in no block
                    [-0.5, 1.0, 1.0]], np.float32)
    assert R.max_dist_cp(to, frm, bb).tolist() == [1.0, 1.0, 60.5, 60.0, 60.0, 60.0]
    # a block whose grown box holds no to-point
    assert R.max_dist_cp(np.array([[-100.0, 0, 0]], np.float32), frm[:1], bb).tolist() == [60.0]


def test_median_and_variance():
    s = R.stats([4.0, 1.0, 3.0, 2.0])
    assert s == {"n": 4, "mean": 2.5, "median": 2.5, "var": 5.0 / 3.0}
    assert R.stats([5.0, 1.0, 3.0])["median"] == 3.0
    assert R.totals([{"acc_mean": 1.0, "comp_mean": 2.0}, {"acc_mean": 3.0, "comp_mean": 5.0}]) == {"acc": 2.0, "comp": 3.5, "overall": 2.75}


def test_device_side_helpers_match_the_reference_on_cpu_tensors():
    """The masks and statistics are plain torch: they can be compared without a GPU."""
    import torch
    from patchmatchnet_amd import pointcloud as PC
    s = R.synthetic_scan(1, n_stl=500, n_data=900)
    x = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999999999999994, 2.4, -2.6], dtype=torch.float64)
    assert PC.matlab_round(x).tolist() == R.matlab_round(x.numpy()).tolist()
    d = torch.from_numpy(s["data"])
    obs = torch.from_numpy(s["ObsMask"].astype(np.uint8))
    got = PC.data_in_mask(d, obs, s["BB"], s["Res"]).numpy()
    assert (got == R.data_in_mask(s["data"], s["ObsMask"], s["BB"], s["Res"])).all() and 0 < got.sum() < len(got)
    got = PC.above_plane(torch.from_numpy(s["stl"]), s["P"]).numpy()
    assert (got == R.stl_above_plane(s["stl"], s["P"])).all() and 0 < got.sum() < len(got)
    f = s["data"].astype(np.float64)
    want = np.ones(len(f), bool)
    for a, bounds in enumerate(R.block_bounds(s["BB"])):
        want &= np.any([(f[:, a] >= lo) & (f[:, a] < hi) for lo, hi in bounds], 0)
    got = PC.in_blocks(d, s["BB"], 60.0).numpy()
    assert (got == want).all() and 0 < got.sum() < len(got)
    for n in (1, 2, 7, 8):
        v = np.random.default_rng(n).random(n)
        st = PC._stats(torch.from_numpy(v), "acc")
        ref = R.stats(v)
        for k in ("n", "mean", "median", "var"):
            assert st[f"acc_{k}"] == pytest.approx(ref[k], rel=1e-14, nan_ok=True)


def test_synthetic_scan_has_every_kind_of_point():
    s = R.synthetic_scan(0)
    d, bb = s["data"].astype(np.float64), s["BB"]
    nd, _ = R.nearest_distance(s["data"][:2000], s["stl"])
    assert (nd > 20).any() and (nd > 60).any() and (nd < 1).any()
    assert (d < bb[0]).any() and (d > bb[1]).any()
    assert ((d[:, 0] < bb[0, 0]) & (d[:, 0] >= bb[0, 0] - s["Res"] / 2)).any()
    assert len(np.unique(s["data"], axis=0)) < len(s["data"])  # exact duplicates
    hole = (s["stl"][:, 0] > 62) & (s["stl"][:, 0] < 78) & (s["stl"][:, 1] > 22) & (s["stl"][:, 1] < 43)
    assert R.nearest_distance(s["stl"][hole][:50], s["data"])[0].min() > 1.0  # the missed patch


# ---- command line -------------------------------------------------------------------------------------------------------------------

def _layout(root, scans, naming):
    data, ply = root / "data", root / "ply"
    (data / "Points" / "stl").mkdir(parents=True)
    (data / "ObsMask").mkdir()
    for n in scans:
        (data / "Points" / "stl" / f"stl{n:03d}_total.ply").write_bytes(b"ply\n")
        (data / "ObsMask" / f"ObsMask{n}_10.npz").write_bytes(b"")
        (data / "ObsMask" / f"Plane{n}.npz").write_bytes(b"")
        p = ply / (f"patchmatchnet{n:03d}_l3.ply" if naming == "reference" else f"scan{n}/fused.ply")
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"ply\n")
    return ["--data_path", str(data), "--ply_path", str(ply), "--results_path", str(root / "out")]


@pytest.mark.parametrize("naming", ["reference", "eval"])
def test_cli_discovery_force_and_missing_files(tmp_path, monkeypatch, capsys, naming):
    import eval_dtu
    assert eval_dtu.USED_SETS == [1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118]
    calls = []

    def stub(args, scan, files):
        calls.append((scan, files["ply"]))
        return {"acc_mean": float(scan), "acc_median": 0.5, "comp_mean": 2.0 * scan, "comp_median": 0.25, "seconds": {}}

    monkeypatch.setattr(eval_dtu, "score_scan", stub)
    argv = _layout(tmp_path, [1, 4], naming) + ["--scans", "1", "4", "9"]
    assert eval_dtu.main(argv) == 1  # scan 9 has no files: named, skipped, non-zero exit
    out = capsys.readouterr()
    assert "scan 9" in out.err and "patchmatchnet009_l3.ply" in out.err and os.path.join("scan9", "fused.ply") in out.err
    assert [c[0] for c in calls] == [1, 4]
    assert calls[0][1].endswith("patchmatchnet001_l3.ply" if naming == "reference" else os.path.join("scan1", "fused.ply"))
    assert "mean/median Data (acc.) 1.000000/0.500000" in out.out and "mean/median Stl (comp.) 8.000000/0.250000" in out.out
    assert "final evaluation result on all scans: acc.: 2.500000, comp.: 5.000000, overall: 3.750000" in out.out
    js = json.load(open(tmp_path / "out" / "dtu_scores.json"))
    from patchmatchnet_amd import _lib
    assert js["abi"] == _lib.ABI_VERSION == 25 and js["seed"] == 0 and js["dst"] == 0.2 and set(js["scans"]) == {"1", "4"}
    assert js["total"] == {"acc": 2.5, "comp": 5.0, "overall": 3.75}
    # a second run recomputes nothing; --force recomputes; other settings invalidate the stored scores
    assert eval_dtu.main(argv[:-1]) == 0 and len(calls) == 2
    assert eval_dtu.main(argv[:-1] + ["--force"]) == 0 and len(calls) == 4
    assert eval_dtu.main(argv[:-1] + ["--seed", "3"]) == 0 and len(calls) == 6
    # the reference's name wins where both exist
    if naming == "eval":
        (tmp_path / "ply" / "patchmatchnet001_l3.ply").write_bytes(b"ply\n")
        assert eval_dtu.main(argv[:-3] + ["1", "--force"]) == 0 and calls[-1][1].endswith("patchmatchnet001_l3.ply")


# ---- ABI 25 argument checks ---------------------------------------------------------------------------------------------------------

def test_new_entry_points_reject_bad_arguments_without_launching():
    from patchmatchnet_amd import _lib
    L = _lib.lib()
    o, d = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_int * 3)(4, 4, 4)
    p = 4096  # any non-null address: a failed check returns before anything reads it
    assert L.pmn_nn_distance(None, None, 8, o, 1.0, d, None, None, 8, 60.0, None, None, None) == -1
    assert L.pmn_nn_distance(p, p, 0, o, 1.0, d, p, None, 8, 60.0, p, None, None) == -1        # n_to = 0
    assert L.pmn_nn_distance(p, p, 8, o, 1.0, d, p, None, 0, 60.0, p, None, None) == -1        # n_from = 0
    assert L.pmn_nn_distance(p, p, 8, o, -1.0, d, p, None, 8, 60.0, p, None, None) == -1       # negative cell
    assert L.pmn_nn_distance(p, p, 8, o, float("nan"), d, p, None, 8, 60.0, p, None, None) == -1
    assert L.pmn_nn_distance(p, p, 8, o, 1.0, d, p, None, 8, 0.0, p, None, None) == -1         # max_dist = 0
    assert L.pmn_nn_distance(p, p, 2 ** 31, o, 1.0, d, p, None, 8, 60.0, p, None, None) == -1  # n_to >= 2^31
    assert L.pmn_nn_distance(p, p, 8, o, 1.0, (ctypes.c_int * 3)(4, 0, 4), p, None, 8, 60.0, p, None, None) == -1
    big = (ctypes.c_int * 3)(2 ** 30, 2 ** 30, 2 ** 30)
    assert L.pmn_nn_distance(p, p, 8, o, 1.0, big, p, None, 8, 60.0, p, None, None) == -2      # key beyond 63 bits
    assert L.pmn_reduce_round(None, None, 8, o, 1.0, d, 0.2, None, None, None, None) == -1
    assert L.pmn_reduce_round(p, p, 0, o, 1.0, d, 0.2, p, p, p, None) == -1
    assert L.pmn_reduce_round(p, p, 8, o, -2.0, d, 0.2, p, p, p, None) == -1
    assert L.pmn_reduce_round(p, p, 8, o, 1.0, d, -0.2, p, p, p, None) == -1
    assert L.pmn_reduce_round(p, p, 8, o, 1.0, d, 0.2, p, p, None, None) == -1
    assert L.pmn_reduce_round(p, p, 8, o, 1.0, big, 0.2, p, p, p, None) == -2
    assert L.pmn_reduce_round(p, p, 8, o, 1e-4, d, 0.2, p, p, p, None) == -2                   # dst / cell > 1024


def test_wrappers_refuse_cpu_tensors():
    import torch
    from patchmatchnet_amd import PmnError, pointcloud as PC
    pts = torch.zeros(4, 3)
    with pytest.raises(PmnError, match="ROCm GPU"):
        PC.build_grid(pts, 1.0)
    with pytest.raises(PmnError, match="ROCm GPU"):
        PC.reduce_points(pts, 0.2)
    with pytest.raises(PmnError, match="ROCm GPU"):
        PC.dtu_score_scan(pts, pts, np.ones((2, 2, 2), bool), np.zeros((2, 3)), 1.0, np.ones(4))
