"""GPU tests of the COLMAP import: pmn_view_scores against the numpy restatement (colmap_synth.oracle_scores), its determinism, the
colmap_input.py CLI against the reference's recorded files (tests/golden/colmap_reference.npz), and the round trip
colmap_input.py -> eval.py -> colmap_output.py on the photo-consistent synthetic scene."""
import os

import numpy as np
import pytest
import torch

import colmap_synth as CS
import goldenutil as GU
import synth
from patchmatchnet_amd import colmap as C
from patchmatchnet_amd import ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _device_scores(m, theta0, sigma1, sigma2):
    extr = [C.extrinsic_matrix(im) for im in m.images]
    centers = np.stack([C.camera_center(e) for e in extr])
    up = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (centers, m.xyz) + C.view_selection_inputs(m)]
    out = ops.view_scores(*up, theta0, sigma1, sigma2)
    return out.cpu().numpy(), up


def _model(tmp_path, kw):
    d = str(tmp_path / "sparse")
    CS.write_model(d, *CS.make_model(**kw))
    return C.read_model(d)


def _check_close(got, want):
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    g, w = got[~nan], want[~nan]
    rel = np.abs(g - w) / np.maximum(np.abs(w), 1e-300)
    assert ((g == w) | (rel <= 1e-12)).all(), float(rel[g != w].max())
    assert (np.diag(got) == 0).all()
    np.testing.assert_array_equal(got, got.T)


@pytest.mark.parametrize("name", ["A", "B", "large"])
def test_view_scores_match_the_numpy_oracle(tmp_path, name):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    kw = CS.large_case() if name == "large" else CS.CASES[name]["model"]
    a = CS.CASES.get(name, CS.CASES["A"])["args"]
    m = _model(tmp_path, kw)
    got, up = _device_scores(m, a["theta0"], a["sigma1"], a["sigma2"])
    want = CS.oracle_scores(m, a["theta0"], a["sigma1"], a["sigma2"])
    _check_close(got, want)
    if name == "B":
        assert np.isnan(got).any() and got[1, 6] == 0.0
    # two calls (the second into a buffer full of garbage: every entry is written) give the same bits
    out = torch.full_like(torch.from_numpy(got).to(DEV), float("inf"))
    again = ops.view_scores(*up, a["theta0"], a["sigma1"], a["sigma2"], out=out).cpu().numpy()
    assert again.tobytes() == got.tobytes()


def test_view_scores_refuses_bad_arguments():
    z64 = torch.zeros((2, 3), dtype=torch.float64, device=DEV)
    ptr = torch.zeros(3, dtype=torch.int64, device=DEV)
    with pytest.raises(ops.PmnError):
        ops.view_scores(z64.float(), z64, ptr, torch.zeros(0, dtype=torch.int32, device=DEV), ptr[:3], torch.zeros(0, dtype=torch.int32, device=DEV), 5, 1, 10)
    with pytest.raises(ops.PmnError):  # trk_ptr must be [P+1]
        ops.view_scores(z64, z64, ptr, torch.zeros(0, dtype=torch.int32, device=DEV), ptr[:2], torch.zeros(0, dtype=torch.int32, device=DEV), 5, 1, 10)


def _cam_lines(data: bytes):
    lines = data.decode().split("\n")
    return lines[:-2], [float(v) for v in lines[-2].split()]


@pytest.mark.parametrize("name", ["A", "B"])
def test_colmap_input_cli_matches_the_reference_files(tmp_path, name):
    import colmap_input
    g = np.load(os.path.join(GU.GOLDEN_DIR, "colmap_reference.npz"))
    src, out = str(tmp_path / "colmap"), str(tmp_path / "mvs")
    os.makedirs(out)
    assert CS.write_case(src, CS.CASES[name]["model"]) == str(g[f"{name}__model_sha256"])
    a = CS.CASES[name]["args"]
    colmap_input.main(["--input_folder", src, "--output_folder", out, "--num_src_images", str(a["num_src_images"]), "--theta0",
                       str(a["theta0"]), "--sigma1", str(a["sigma1"]), "--sigma2", str(a["sigma2"])])
    n = CS.CASES[name]["model"]["n_images"]
    for v in range(n):
        got, want = _cam_lines(open(os.path.join(out, "cams", "%08d_cam.txt" % v), "rb").read()), _cam_lines(
            g[f"{name}__cams__{v:08d}"].tobytes())
        assert got[0] == want[0], v
        np.testing.assert_allclose(got[1], want[1], rtol=0, atol=1e-6)
    gl = open(os.path.join(out, "pair.txt")).read().split("\n")
    wl = g[f"{name}__pair"].tobytes().decode().split("\n")
    assert gl[:1] == wl[:1] and len(gl) == len(wl)
    for k in range(n):
        assert gl[1 + 2 * k] == wl[1 + 2 * k]
        x, y = gl[2 + 2 * k].split(), wl[2 + 2 * k].split()
        assert x[0] == y[0]
        gi, gs = [int(v) for v in x[1::2]], np.array([float(v) for v in x[2::2]])
        wi, ws = [int(v) for v in y[1::2]], np.array([float(v) for v in y[2::2]])
        np.testing.assert_allclose(gs, ws, rtol=0, atol=1e-6, equal_nan=True)
        for r in range(len(wi)):  # the same id wherever the scores around the position are distinct by more than 1e-9 relative
            near = [ws[q] for q in (r - 1, r + 1) if 0 <= q < len(ws)]
            if all(np.isnan(ws[r]) != np.isnan(s) or abs(ws[r] - s) > 1e-9 * max(abs(ws[r]), 1e-300) for s in near):
                assert gi[r] == wi[r], (k, r)
    assert sorted(os.listdir(os.path.join(out, "images"))) == ["%08d.jpg" % v for v in range(n)]


def _scene_model(root, n_views, H, W, step_px=6):
    """The photo-consistent scene of tests/synth.py as a COLMAP model: the surface points seen by view 0 on a pixel grid, observed by
    every view they project into, PINHOLE cameras with the scene's intrinsics and poses.  Returns the rendered depth maps."""
    from PIL import Image as PilImage
    cams = synth.arc_cameras(n_views, H, W)
    imgs, intr, extr, depths = synth.render_scene(n_views, H, W, seed=0, cameras=cams, all_depths=True)
    K = intr[0].astype(np.float64)
    E = extr[0].astype(np.float64)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    v, u = np.mgrid[step_px // 2:H:step_px, step_px // 2:W:step_px]
    d0 = depths[0].cpu().numpy().astype(np.float64)[v, u]
    ray = np.linalg.inv(K[0]) @ np.stack([u.ravel(), v.ravel(), np.ones(u.size)])
    Xc = ray * d0.ravel()
    R0, t0 = E[0, :3, :3], E[0, :3, 3]
    X = (R0.T @ (Xc - t0[:, None])).T  # world points
    pids = {}
    images, cameras = [], []
    for i in range(n_views):
        arr = (imgs[i][0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        PilImage.fromarray(arr).save(os.path.join(root, "images", "view_%02d.jpg" % i), quality=95)
        x = K[i] @ (E[i, :3, :3] @ X.T + E[i, :3, 3:4])
        px, py = x[0] / x[2], x[1] / x[2]
        inside = (x[2] > 0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
        ids = np.where(inside, np.arange(len(X)) + 1, -1)
        for k in np.flatnonzero(inside):
            pids.setdefault(k + 1, []).append((i + 1, int(k)))
        cameras.append((i + 1, "PINHOLE", W, H, [K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2]]))
        images.append((i + 1, list(CS.rot_to_quat(E[i, :3, :3])), list(E[i, :3, 3]), i + 1, "view_%02d.jpg" % i, ids))
    points = [(k, list(X[k - 1]), [128, 128, 128], 0.5, tr) for k, tr in sorted(pids.items())]
    CS.write_model(os.path.join(root, "sparse"), cameras, images, points)
    return [d.cpu().numpy() for d in depths]


def test_round_trip_on_the_synthetic_scene(tmp_path):
    import colmap_input
    import colmap_output
    import eval as pm_eval
    from patchmatchnet_amd import data_io
    n, H, W = 5, 128, 160
    src, mvs, res, ws = (str(tmp_path / d) for d in ("colmap", "mvs", "results", "ws"))
    for d in (mvs, res, ws):
        os.makedirs(d)
    gt = _scene_model(src, n, H, W)
    colmap_input.main(["--input_folder", src, "--output_folder", mvs, "--num_src_images", "4"])
    pm_eval.main(["--input_folder", mvs, "--output_folder", res, "--checkpoint_path", os.path.join(GU.GOLDEN_DIR, "params_000007.npz"),
                  "--num_views", "4", "--output_type", "depth", "--num_workers", "0", "--file_format", ".pfm"])
    colmap_output.main(["--input_folder", mvs, "--results_folder", res, "--output_folder", ws])
    errs = []
    for v in range(n):
        d = data_io.read_map(os.path.join(res, "depth_est", "%08d.pfm" % v))[..., 0]
        assert d.shape == (H, W) and np.isfinite(d).all()
        rel = np.abs(d - gt[v]) / gt[v]
        errs.append(float(np.median(rel)))
        for kind in ("depth_maps", "confidence_maps"):
            p = os.path.join(ws, "stereo", kind, "%08d.jpg.geometric.bin" % v)
            assert data_io.read_map(p).shape == (H, W, 1)
    print("median relative depth error per view:", ["%.2e" % e for e in errs])
    # gate: median relative error 3 % per view (first measured run: 1.6 - 1.9 %, 128 x 160 views)
    assert max(errs) < 0.03, errs
    for rel in ("sparse/cameras.txt", "sparse/images.txt", "sparse/points3D.txt", "stereo/patch-match.cfg", "stereo/fusion.cfg"):
        assert os.path.isfile(os.path.join(ws, rel)), rel
    assert sorted(os.listdir(os.path.join(ws, "images"))) == ["%08d.jpg" % v for v in range(n)]
