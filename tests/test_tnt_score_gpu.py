"""GPU checks of the Tanks and Temples score (pmn_icp_accumulate, pmn_voxel_mean, pmn_crop_prism, patchmatchnet_amd/registration.py,
eval_tnt.py) against the numpy float64 statement tests/tnt_ref.py.

Bounds.  pmn_icp_accumulate: the count is exact and every sum lies within (n + 2) * 2^-53 * sum |term| of the exactly rounded sum
(math.fsum): the worst case of ANY order of n float64 additions plus one rounding per product -- derived, not tuned.  Voxel means and
crop masks follow bit-level definitions and are compared for equality.  icp() on the noise-free scene: the recovered pose maps the
points onto their originals with RMS <= 2 sqrt(3) M 2^-24 (two float32 roundings per coordinate, M the largest |coordinate|).
tnt_score on the noisy scene: see test_tnt_score_matches_the_reference."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tnt_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TAU = R.TAU
POSE = R.rigid(R.rotation((2.0, -1.0, 0.5), 1.5), (0.004, -0.003, 0.002))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


@pytest.fixture(scope="module")
def scene():
    return R.synthetic_scene(0)


@pytest.fixture(scope="module")
def target(scene):
    return np.ascontiguousarray(scene["gt"][::3])  # 3000 points


def _source(target, n, seed=1):
    """n points near the target's surface: target points (with repetition) plus tau-sized noise."""
    rng = np.random.default_rng(seed)
    return (target[rng.integers(0, len(target), n)].astype(np.float64) + TAU * rng.standard_normal((n, 3))).astype(np.float32)


def _volume(scene):
    from patchmatchnet_amd import registration as RG
    poly, axis, lo, hi = scene["volume"]
    return RG.CropVolume(poly, axis, lo, hi)


@pytest.mark.parametrize("n_src", [1, 63, 64, 65, 5001, 20001])
def test_icp_accumulate_matches_the_reference(target, n_src):
    from patchmatchnet_amd import pointcloud as PC, registration as RG
    src = _source(target, n_src)
    centre = R.bbox_centre(target)
    p = R.apply_pose(POSE, src)
    d2, _, second = R.nearest(p, target, second=True)
    assert (d2 != second).all()  # no ties: the matched set is unique
    src_d, tgt_d = _dev(src), _dev(target)
    seen = []
    for max_dist in (80 * TAU, 2 * TAU):
        want, mag = R.icp_sums(src, target, POSE, centre, max_dist)
        n = int(want[0])
        bound = (n + 2) * 2.0 ** -53 * mag
        for cell in (0.02, 0.3, 50.0):
            grid = PC.build_grid(tgt_d, cell)
            assert np.array_equal(RG.grid_centre(grid), centre)
            for order in (None, RG.query_order(src_d, grid, POSE)):
                got = RG.icp_accumulate(src_d, grid, POSE, centre, max_dist, order).cpu().numpy()
                err = np.abs(got - want)
                print(f"n {n_src} max_dist {max_dist} cell {cell} order {order is not None}: matched {int(got[0])}, "
                      f"max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
                assert got[0] == n
                assert (err <= bound).all(), (got, want, bound)
                seen.append((max_dist, got))
    for max_dist, got in seen:  # neither the cell nor the order changes a bit
        first = next(g for m, g in seen if m == max_dist)
        assert np.array_equal(got, first)
    if n_src >= 63:
        assert 0 < R.icp_sums(src, target, POSE, centre, 2 * TAU)[0][0] < n_src  # the tight distance drops some pairs


def test_icp_accumulate_edge_cases(target):
    from patchmatchnet_amd import PmnError, pointcloud as PC, registration as RG
    centre = R.bbox_centre(target)
    tgt_d = _dev(target)
    grid = PC.build_grid(tgt_d, 0.3)
    # far outside the grid, just outside it, inside it
    lo, hi = target.min(0), target.max(0)
    src = np.array([[50, 50, 50], [-1e4, 0, 0], [0, 0, 1e6], hi + np.float32(0.05), lo - np.float32(0.05), target[7], target[100] + np.float32(1e-3)],
                   np.float32)
    for max_dist in (0.8, 0.02, 1e7):
        want, mag = R.icp_sums(src, target, np.eye(4), centre, max_dist)
        got = RG.icp_accumulate(_dev(src), grid, np.eye(4), centre, max_dist).cpu().numpy()
        print(f"edge max_dist {max_dist}: matched {int(got[0])} of {len(src)}")
        assert got[0] == want[0] and (np.abs(got - want) <= (want[0] + 2) * 2.0 ** -53 * mag).all()
    # no match at all: zeros, and icp() refuses
    far = _dev(src[:3])
    got = RG.icp_accumulate(far, grid, np.eye(4), centre, 0.5).cpu().numpy()
    assert np.array_equal(got, np.zeros(17))
    with pytest.raises(PmnError, match="3 pairs"):
        RG.icp(far, grid, np.eye(4), 0.5)
    # two runs, and any order: the same bits
    s = _dev(_source(target, 5001, seed=2))
    a = RG.icp_accumulate(s, grid, POSE, centre, 0.2)
    b = RG.icp_accumulate(s, grid, POSE, centre, 0.2)
    perm = torch.randperm(5001, generator=torch.Generator().manual_seed(3)).int().to(DEV)
    c = RG.icp_accumulate(s, grid, POSE, centre, 0.2, perm)
    d = RG.icp_accumulate(s, grid, POSE, centre, 0.2, RG.query_order(s, grid, POSE))
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d) and a[0] > 0
    with pytest.raises(PmnError, match="with_scale"):
        RG.icp(s, grid, np.eye(4), 0.2, with_scale=True)
    with pytest.raises(PmnError, match="scratch"):
        RG.icp_accumulate(s, grid, POSE, centre, 0.2, scratch=torch.empty(10, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("voxel", [TAU / 2, TAU, 0.5, 100.0])
def test_voxel_downsample_is_bit_equal(scene, voxel):
    from patchmatchnet_amd import registration as RG
    pts = scene["gt"]
    attr = np.random.default_rng(5).random((len(pts), 3)).astype(np.float32)
    want, want_attr = R.voxel_downsample(pts, voxel, attr)
    got, got_attr = RG.voxel_downsample(_dev(pts), voxel, _dev(attr))
    got, got_attr = got.cpu().numpy(), got_attr.cpu().numpy()
    origin = pts.min(0).astype(np.float64) - voxel / 2
    n_voxels = len(np.unique(np.floor((pts.astype(np.float64) - origin) / voxel), axis=0))
    print(f"voxel {voxel}: {len(pts)} points -> {len(got)} voxels")
    assert got.shape == want.shape == (n_voxels, 3) and got.dtype == np.float32
    assert np.array_equal(got, want) and np.array_equal(got_attr, want_attr)
    assert np.array_equal(RG.voxel_downsample(_dev(pts), voxel).cpu().numpy(), want)
    if voxel == 100.0:
        assert n_voxels == 1 and len(pts) > R.LONG_RUN  # the long-run path
    if voxel == 0.5:  # both paths in one launch
        _, counts = np.unique(np.floor((pts.astype(np.float64) - origin) / voxel), axis=0, return_counts=True)
        assert (counts > R.LONG_RUN).any() and (counts <= R.LONG_RUN).any()


def test_voxel_downsample_of_one_point():
    from patchmatchnet_amd import registration as RG
    p = np.array([[0.25, -3.0, 7.5]], np.float32)
    got = RG.voxel_downsample(_dev(p), 0.01)
    assert np.array_equal(got.cpu().numpy(), p)


@pytest.mark.parametrize("with_pose", [False, True])
def test_crop_matches_the_reference(scene, with_pose):
    from patchmatchnet_amd import registration as RG
    poly, axis, lo, hi = scene["volume"]
    rng = np.random.default_rng(9)
    f = np.float32
    special = [[0.0, 0.0, lo], [0.0, 0.0, hi], [0.1, 0.1, np.nextafter(f(lo), f(-9))], [0.1, 0.1, np.nextafter(f(hi), f(9))]]
    special += [[x, v[1], 0.0] for v in poly for x in (-2.0, v[0] - 0.05, v[0], v[0] + 0.05, 2.0)]  # on a vertex's y
    special += [[1e6, 0, 0], [0, -1e6, 0], [0, 0, 1e6], [-3e4, 2e4, 0.1]]
    pts = np.concatenate([scene["gt"], np.asarray(special, np.float32), rng.uniform(-1.5, 1.5, (3000, 3)).astype(np.float32)])
    pose = POSE if with_pose else None
    want = R.crop_mask(pts, poly, axis, lo, hi, pose)
    got = RG.crop(_dev(pts), _volume(scene), pose).cpu().numpy()
    print(f"crop pose {with_pose}: {got.sum()} of {len(pts)} inside")
    assert got.dtype == bool and 0 < want.sum() < len(pts)
    assert np.array_equal(got, want)
    if not with_pose:
        assert want[len(scene["gt"])] and want[len(scene["gt"]) + 1] and not want[len(scene["gt"]) + 2] and not want[len(scene["gt"]) + 3]
        # the other two axes: the same polygon read in (y, z) and in (x, z)
        for ax, cols in ((0, (2, 0, 1)), (1, (0, 2, 1))):
            p2, poly2 = np.ascontiguousarray(pts[:, cols]), poly[:, cols]
            assert np.array_equal(RG.crop(_dev(p2), RG.CropVolume(poly2, ax, lo, hi)).cpu().numpy(), R.crop_mask(p2, poly2, ax, lo, hi))


def test_icp_recovers_the_known_motion(scene):
    from patchmatchnet_amd import pointcloud as PC, registration as RG
    est, gt = _dev(scene["est"]), _dev(scene["gt"])
    pose = np.eye(4)
    for dist, cell in ((80 * TAU, 2 * TAU), (20 * TAU, 2 * TAU), (2 * TAU, 2 * TAU)):
        r = RG.icp(est, PC.build_grid(gt, cell), pose, dist)
        pose = r["pose"]
        print(f"icp max_dist {dist}: {r['iterations']} iterations, fitness {r['fitness']}, rmse {r['rmse']:.3e}")
        assert len(r["history"]) == r["iterations"] + 1 <= 21
    moved = R.apply_pose(pose, scene["est"])
    orig = scene["gt"][scene["pick"]].astype(np.float64)
    rms = float(np.sqrt(((moved - orig) ** 2).sum(1).mean()))
    bound = 2 * np.sqrt(3) * float(np.abs(scene["gt"]).max()) * 2.0 ** -24
    rot = float(np.linalg.norm(pose[:3, :3] @ scene["motion"][:3, :3].T - np.eye(3)))
    print(f"rms {rms:.3e} (bound {bound:.3e}), rotation error {rot:.3e}, translation error {np.abs(pose[:3, 3] - scene['motion'][:3, 3]).max():.3e}")
    assert r["fitness"] == 1.0
    assert rms <= bound
    assert rot <= bound  # |R R_g^T - I|_F moves a point at radius M by at most that times M; M is about 1


@pytest.fixture(scope="module")
def noisy_reference(scene):
    init = scene["gt_trans"] @ R.kabsch(scene["traj_est"][:, :3, 3], scene["traj_gt"][:, :3, 3], True)
    return init, R.tnt_score(scene["est_noisy"], scene["gt"], scene["volume"], TAU, init)


def test_tnt_score_matches_the_reference(scene, noisy_reference):
    """A free-running ICP can amplify a 1e-13 difference in the sums, so the full loop has no derived bound.  If the two final poses
    agree to 1e-9 in every entry the three counts behind P and R must equal the reference's exactly (no reference distance lies within
    1e-9 of tau: asserted); otherwise |dF| <= (1 + #points whose reference distance is within 1e-6 of tau) * 100 / min(#est, #gt).
    Measured on an MI355X: DESIGN.md 17."""
    from patchmatchnet_amd import registration as RG
    init, (ref, d_est, d_gt) = noisy_reference
    near = lambda eps: int((np.abs(d_est - TAU) < eps).sum() + (np.abs(d_gt - TAU) < eps).sum())
    assert near(1e-9) == 0
    got, g_est, g_gt = RG.tnt_score(_dev(scene["est_noisy"]), _dev(scene["gt"]), _volume(scene), TAU, init=init, return_distances=True)
    dpose = float(np.abs(np.asarray(got["pose"]) - ref["pose"]).max())
    dF = abs(got["fscore"] - ref["fscore"])
    print(f"tnt_score: P {got['precision']:.4f} R {got['recall']:.4f} F {got['fscore']:.4f}; reference F {ref['fscore']:.4f}; |dF| {dF:.3e}; "
          f"max pose difference {dpose:.3e}; reference distances within 1e-9 / 1e-6 of tau: {near(1e-9)} / {near(1e-6)}; rounds {got['rounds']}")
    assert len(got["rounds"]) == 3 and len(got["precision_curve"]) == len(got["recall_curve"]) == len(got["hist_edges"]) == 100
    assert got["precision_curve"][-1] <= 100.0 and got["recall_curve"][19] == pytest.approx(got["recall"], abs=1.0)
    if dpose <= 1e-9:
        for k in ("n_est", "n_gt", "n_est_within_tau", "n_gt_within_tau"):
            assert got[k] == ref[k], (k, got[k], ref[k])
        assert got["precision"] == ref["precision"] and got["recall"] == ref["recall"] and got["fscore"] == ref["fscore"]
    else:
        assert dF <= (1 + near(1e-6)) * 100.0 / min(ref["n_est"], ref["n_gt"])
    assert g_est.dtype == torch.float64 and g_est.numel() == got["n_est"] and g_gt.numel() == got["n_gt"]


def _write_log(path, mats):
    with open(path, "w") as f:
        for i, T in enumerate(mats):
            f.write(f"{i} {i} 0\n")
            for row in T:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")


def _run_cli(argv, timeout=300):
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, os.path.join(ROOT, "eval_tnt.py")] + argv,
                          capture_output=True, text=True, cwd=ROOT)


def test_eval_tnt_end_to_end(tmp_path, scene, noisy_reference):
    from patchmatchnet_amd import fusion, registration as RG
    init, _ = noisy_reference
    data, mvs, out = tmp_path / "Synth", tmp_path / "mvs", tmp_path / "out"
    os.makedirs(data)
    os.makedirs(mvs / "cams")
    grey = lambda p: np.full((len(p), 3), 128, np.uint8)
    fusion.write_ply(str(data / "Synth.ply"), scene["gt"], grey(scene["gt"]))
    fusion.write_ply(str(tmp_path / "fused.ply"), scene["est_noisy"], grey(scene["est_noisy"]))
    poly, axis, lo, hi = scene["volume"]
    with open(data / "Synth.json", "w") as f:
        json.dump({"bounding_polygon": poly.tolist(), "orthogonal_axis": "Z", "axis_min": lo, "axis_max": hi}, f)
    _write_log(data / "Synth_COLMAP_SfM.log", scene["traj_gt"])
    _write_log(tmp_path / "own.log", scene["traj_est"])
    np.savetxt(data / "Synth_trans.txt", scene["gt_trans"], fmt="%.17g")
    for i, T in enumerate(scene["traj_est"]):  # MVSNet camera files hold world-to-camera matrices in text
        with open(mvs / "cams" / f"{i:08d}_cam.txt", "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join("%.9g" % v for v in row) for row in np.linalg.inv(T)) + "\n\nintrinsic\n"
                    "500 0 320\n0 500 240\n0 0 1\n\n0.5 5.0\n")
    base = ["--dataset_dir", str(data), "--ply_path", str(tmp_path / "fused.ply"), "--tau", str(TAU)]
    r = _run_cli(base + ["--results_path", str(out), "--trajectory", str(tmp_path / "own.log")])
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.load(open(out / "tnt_scores.json"))
    for key in ("precision", "recall", "fscore", "pose", "rounds", "hist_edges", "precision_curve", "recall_curve", "tau", "abi"):
        assert key in js, key
    assert len(js["rounds"]) == 3 and all({"fitness", "rmse"} <= set(x) for x in js["rounds"]) and np.asarray(js["pose"]).shape == (4, 4)
    direct = RG.tnt_score(_dev(scene["est_noisy"]), _dev(scene["gt"]), _volume(scene), TAU, init=np.asarray(js["init_transform"]))
    assert js["fscore"] == direct["fscore"] and js["precision"] == direct["precision"] and js["recall"] == direct["recall"]
    assert np.abs(np.asarray(js["init_transform"]) - init).max() < 1e-9
    assert "f-score : %.4f" % direct["fscore"] in r.stdout
    # cameras from the MVS folder (float32 text): the same alignment to the files' precision
    r = _run_cli(base + ["--results_path", str(tmp_path / "out_mvs"), "--mvs_folder", str(mvs)])
    assert r.returncode == 0, r.stdout + r.stderr
    js_mvs = json.load(open(tmp_path / "out_mvs" / "tnt_scores.json"))
    assert np.abs(np.asarray(js_mvs["init_transform"]) - init).max() < 1e-5 and abs(js_mvs["fscore"] - js["fscore"]) < 1.0
    # a cloud already in the ground truth's frame
    fusion.write_ply(str(tmp_path / "aligned.ply"), R.transform(scene["motion"], scene["est_noisy"]), grey(scene["est_noisy"]))
    r = _run_cli(["--dataset_dir", str(data), "--ply_path", str(tmp_path / "aligned.ply"), "--tau", str(TAU), "--no_registration",
                  "--results_path", str(tmp_path / "out_fixed")])
    assert r.returncode == 0, r.stdout + r.stderr
    js_fixed = json.load(open(tmp_path / "out_fixed" / "tnt_scores.json"))
    fixed = RG.tnt_score(_dev(R.transform(scene["motion"], scene["est_noisy"])), _dev(scene["gt"]), _volume(scene), TAU, register=False)
    assert js_fixed["rounds"] == [] and js_fixed["fscore"] == fixed["fscore"] and js_fixed["pose"] == np.eye(4).tolist()
    assert abs(js_fixed["fscore"] - js["fscore"]) < 1.0
