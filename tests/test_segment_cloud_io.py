"""segment_cloud.py: its argument errors, which must not need a GPU (exit code 2, one line), the camera-side rule, and -- marked gpu --
one scan end to end on the planted scene of tests/plane_ref.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import plane_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None, gpu=False):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    if not gpu:
        e["HIP_VISIBLE_DEVICES"] = ""  # no device may be needed to refuse
    return subprocess.run([sys.executable, os.path.join(ROOT, "segment_cloud.py")] + args, capture_output=True, text=True, timeout=600,
                          cwd=ROOT, env=e)


def _refused(r, word):
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout)
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("segment_cloud.py: ") and word in lines[0], r.stderr


def _write_cams(folder, centres):
    os.makedirs(os.path.join(folder, "cams"), exist_ok=True)
    for i, C in enumerate(centres):
        E = np.eye(4)
        E[:3, 3] = -np.asarray(C, np.float64)
        with open(os.path.join(folder, "cams", f"{i:08d}_cam.txt"), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(repr(float(v)) for v in row) for row in E) + "\n\nintrinsic\n"
                    "100 0 50\n0 100 40\n0 0 1\n\n1.0 2.0\n")


def test_segment_cloud_argument_errors(tmp_path):
    from patchmatchnet_amd import ply
    cloud, mesh, out = str(tmp_path / "fused.ply"), str(tmp_path / "mesh.ply"), str(tmp_path / "noplane.ply")
    ply.write_ply(cloud, np.eye(5, 3, dtype=np.float32), np.zeros((5, 3), np.uint8))  # no normals
    ply.write_ply_mesh(mesh, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    base = ["--input", cloud, "--output", out]
    _refused(_run(["--input", cloud]), "--output")
    _refused(_run(base + ["--threshold", "0.1", "--threshold_spacings", "2"]), "exclude each other")
    _refused(_run(base + ["--threshold", "-0.5"]), "--threshold")
    _refused(_run(base + ["--threshold", "nan"]), "--threshold")
    _refused(_run(base + ["--threshold_spacings", "inf"]), "--threshold_spacings")
    _refused(_run(base + ["--hypotheses", "0"]), "--hypotheses")
    _refused(_run(base + ["--max_planes", "0"]), "--max_planes")
    _refused(_run(base + ["--seed", "-1"]), "--seed")
    _refused(_run(base + ["--min_inliers", "5", "--min_inlier_share", "0.1"]), "exclude each other")
    _refused(_run(base + ["--min_inlier_share", "1.5"]), "--min_inlier_share")
    _refused(_run(base + ["--normal_angle", "120"]), "--normal_angle")
    _refused(_run(base + ["--threshold", "0.1", "--normal_angle", "20"]), "needs normals in the file")
    _refused(_run(base + ["--drop_beyond"]), "--mvs_folder")
    _refused(_run(base + ["--threshold", "0.1", "--drop_beyond", "--mvs_folder", str(tmp_path / "nowhere")]), "no cameras")
    _refused(_run(base + ["--mvs_folder", str(tmp_path)]), "--drop_beyond")
    _refused(_run(["--input", mesh, "--output", out]), "a mesh")
    _refused(_run(base, env={"WORLD_SIZE": "2"}), "torchrun")
    _refused(_run(["--input", str(tmp_path / "missing.ply"), "--output", out]), "no such file")
    _refused(_run(["--input", str(tmp_path), "--scan_list", str(tmp_path / "none.txt")]), "scan list")
    lst = tmp_path / "list.txt"
    lst.write_text("scan1\n")
    _refused(_run(["--input", str(tmp_path), "--scan_list", str(lst), "--planes", str(tmp_path / "p.npz")]), "--scan_list")
    assert not os.path.exists(out)


def test_flags_parse_and_the_camera_side_rule(tmp_path):
    import segment_cloud as S
    a = S.build_parser().parse_args(["--input", "x.ply"])
    assert (a.threshold, a.threshold_spacings, a.hypotheses, a.seed, a.refine, a.max_planes) == (None, None, 1024, 0, 3, 1)
    assert (a.min_inliers, a.min_inlier_share, a.normal_angle, a.keep, a.drop_beyond) == (None, None, None, "rest", False)
    a = S.build_parser().parse_args(["--input", "x", "--keep", "planes", "--max_planes", "3", "--min_inlier_share", "0.05",
                                     "--normal_angle", "15", "--color_by_plane", "--labels", "l.npy", "--planes", "p.npz"])
    assert (a.keep, a.max_planes, a.min_inlier_share, a.normal_angle, a.color_by_plane) == ("planes", 3, 0.05, 15.0, True)
    plane = np.array([0.0, 0.0, 1.0, -1.0])
    above, below, inside = [0, 0, 3.0], [5, 5, -2.0], [1, 1, 1.05]
    assert S.camera_side(plane, 0.1, [above, above, below]) == 1 and S.camera_side(plane, 0.1, [below, inside]) == -1
    with pytest.raises(ValueError, match="split evenly"):
        S.camera_side(plane, 0.1, [above, below, inside])  # a centre inside the band counts for neither side
    _write_cams(str(tmp_path), R.planted_cameras())
    from cloud_normals import camera_centres
    assert np.abs(camera_centres(str(tmp_path)) - R.planted_cameras()).max() < 1e-5


@pytest.mark.gpu
def test_segment_cloud_end_to_end(tmp_path):
    import torch
    from patchmatchnet_amd import ply, pointcloud as PC
    import cluster_cloud
    pts, planted, plane, normals = R.planted_scene(0)
    n, thr = len(pts), 2.0 * R.PLANTED_S
    colors = np.random.default_rng(4).integers(0, 256, (n, 3)).astype(np.uint8)
    src, dst, lab, npz, rep = (str(tmp_path / f) for f in ("scan/fused.ply", "out/noplane.ply", "out/labels.npy", "out/plane.npz",
                                                           "out/report.json"))
    os.makedirs(tmp_path / "scan")
    ply.write_ply(src, pts, colors, normals)
    _write_cams(str(tmp_path / "scan"), R.planted_cameras())
    want = R.segment_plane(pts, thr, seed=3)
    r = _run(["--input", src, "--output", dst, "--threshold", repr(thr), "--seed", "3", "--labels", lab, "--planes", npz, "--report", rep,
              "--drop_beyond", "--mvs_folder", str(tmp_path / "scan")], gpu=True)
    assert r.returncode == 0, r.stderr
    (a, b, c, d), p = (float(v) for v in want["plane"]), pts.astype(np.float64)
    res = a * p[:, 0] + b * p[:, 1] + c * p[:, 2] + d  # the cameras of the scene all stand on the positive side of the planted normal
    assert ((R.planted_cameras() @ want["plane"][:3] + d) > thr).all()
    under = res < -thr
    assert under.sum() > 100 and not (under & planted).any()  # the clutter placed under the table
    keep = ~want["inliers"] & ~under
    m = ply.read_ply_model(dst)  # the records of the kept points, unchanged and in order
    assert m["faces"] is None and np.array_equal(m["vertices"], pts[keep]) and np.array_equal(m["colors"], colors[keep])
    assert np.array_equal(m["normals"], normals[keep])
    got = np.load(lab)
    assert got.dtype == np.int32 and np.array_equal(got == 0, want["inliers"]) and np.array_equal(got == -1, ~want["inliers"])
    lib = PC.segment_planes(torch.from_numpy(pts).to("cuda:0"), thr, max_planes=1, seed=3)
    assert np.array_equal(got, lib["labels"].cpu().numpy())
    P = PC.load_plane(npz)  # what eval_dtu.py reads
    assert P.shape == (4,) and np.array_equal(P, want["plane"])
    one = json.load(open(rep))["files"][0]
    assert one["points"] == n and one["kept"] == int(keep.sum()) and one["dropped_beyond"] == int(under.sum())
    assert one["planes"][0]["plane"] == want["plane"].tolist() and one["planes"][0]["inliers"] == want["count"]
    assert one["planes"][0]["hypothesis"] == want["hypothesis"] and one["planes"][0]["refits"] == want["refits"]
    for word in (f"{n} points read", f"{want['count']} inliers", f"hypothesis {want['hypothesis']}", f"{want['refits']} refits",
                 f"{int(under.sum())} points dropped", f"{int(keep.sum())} points written"):
        assert word in r.stdout, (word, r.stdout)
    # the planes alone, coloured; the normal test; the default threshold
    dst2 = str(tmp_path / "out/planes.ply")
    r = _run(["--input", src, "--output", dst2, "--seed", "3", "--keep", "planes", "--color_by_plane", "--normal_angle", "20",
              "--report", rep], gpu=True)
    assert r.returncode == 0, r.stderr
    one = json.load(open(rep))["files"][0]
    d = torch.from_numpy(pts).to("cuda:0")
    assert one["spacing"] == PC.cloud_spacing(d) and one["threshold"] == 2.0 * one["spacing"]
    lib = PC.segment_planes(d, one["threshold"], max_planes=1, seed=3, normals=torch.from_numpy(normals).to("cuda:0"), normal_angle=20.0)
    on = lib["labels"].cpu().numpy() == 0
    m = ply.read_ply_model(dst2)
    assert np.array_equal(m["vertices"], pts[on]) and on[planted].mean() >= 0.5
    assert np.array_equal(m["colors"], cluster_cloud.cluster_colors(np.zeros(int(on.sum()), np.int64)))
