"""smooth_cloud.py, the command-line tool over pointcloud.smooth_mls: its refusals and cloud_tool.write_kept(vertices=...) on the CPU,
one round trip on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cloud_normals_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIANGLE = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))


def test_every_refusal_comes_before_a_device(tmp_path, monkeypatch, capsys):
    """Exit code 2, nothing on stdout, one line on stderr that starts with the tool's name, no output file, and no device visible."""
    import smooth_cloud
    from patchmatchnet_amd import ply
    cloud, mesh, out = str(tmp_path / "fused.ply"), str(tmp_path / "mesh.ply"), str(tmp_path / "out.ply")
    ply.write_ply(cloud, np.eye(5, 3, dtype=np.float32), np.zeros((5, 3), np.uint8))   # no normals
    ply.write_ply_mesh(mesh, *TRIANGLE)
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    io = ["--input", cloud, "--output", out]
    cases = [(io, {"WORLD_SIZE": "2"}, "torchrun (WORLD_SIZE > 1) is not supported"),
             (["--input", mesh, "--output", out], {}, "a mesh (1 faces), not a cloud; mesh.py --smooth"),
             (io + ["--iterations", "0"], {}, "--iterations must be at least 1, got 0"),
             (io + ["--iterations", "-2"], {}, "--iterations must be at least 1"),
             (io + ["--k", "0"], {}, "--k must be in 1..32, got 0"),
             (io + ["--k", "33"], {}, "--k must be in 1..32, got 33"),
             (io + ["--degree", "0"], {}, "--degree must be 1 or 2, got 0"),
             (io + ["--degree", "3"], {}, "--degree must be 1 or 2, got 3"),
             (io + ["--radius", "0"], {}, "--radius must be positive and finite"),
             (io + ["--radius", "inf"], {}, "--radius must be positive and finite"),
             (io + ["--radius_spacings", "nan"], {}, "--radius_spacings must be positive and finite"),
             (io + ["--radius_spacings", "-3"], {}, "--radius_spacings must be positive and finite"),
             (io + ["--radius", "1", "--radius_spacings", "3"], {}, "--radius or --radius_spacings, not both"),
             (io + ["--cell", "0"], {}, "--cell must be positive and finite"),
             (io + ["--normals", "refit"], {}, "--normals refit needs normals (nx ny nz) in the input file to decide the side; cloud_normals.py"),
             (["--input", cloud], {}, "--output is required for a single file"),
             (["--input", str(tmp_path / "missing.ply"), "--output", out], {}, "no such file: ")]
    for argv, env, word in cases:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            assert smooth_cloud.main(argv) == 2, argv
        got = capsys.readouterr()
        lines = got.err.splitlines()
        assert got.out == "" and len(lines) == 1 and lines[0].startswith("smooth_cloud.py: ") and word in lines[0], (argv, got.err)
        assert not os.path.exists(out), argv


def test_refusal_as_a_process(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HIP_VISIBLE_DEVICES"] = ""
    out = str(tmp_path / "out.ply")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "smooth_cloud.py"), "--input", str(tmp_path / "fused.ply"), "--output", out,
                        "--iterations", "0"], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 2 and r.stdout == "" and r.stderr == "smooth_cloud.py: --iterations must be at least 1, got 0\n"
    assert not os.path.exists(out)


def test_the_tool_is_a_cloud_tool():
    """Importing it imports no GPU code, and the default it restates is the library's."""
    code = "import sys, smooth_cloud; sys.exit(any(m == 'torch' or m.startswith('patchmatchnet_amd') for m in sys.modules))"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT, timeout=120).returncode == 0
    import smooth_cloud
    from patchmatchnet_amd import pointcloud as PC
    assert smooth_cloud.RADIUS_SPACINGS == PC.MLS_RADIUS_SPACINGS


def test_write_kept_writes_the_given_vertices(tmp_path):
    import cloud_tool
    from patchmatchnet_amd import ply
    rng = np.random.default_rng(1)
    v, moved = rng.standard_normal((6, 3)).astype(np.float32), rng.standard_normal((6, 3)).astype(np.float32)
    c = rng.integers(0, 255, (6, 3)).astype(np.uint8)
    n = rng.standard_normal((6, 3)).astype(np.float32)
    dst = str(tmp_path / "out.ply")
    everything, some = np.ones(6, bool), np.array([True, False, True, True, False, False])
    for keep in (everything, some):
        cloud_tool.write_kept(dst, {"vertices": v, "colors": c, "normals": n}, keep, vertices=moved)
        m = ply.read_ply_model(dst)
        assert np.array_equal(m["vertices"], moved[keep]) and np.array_equal(m["colors"], c[keep]) and np.array_equal(m["normals"], n[keep])
    cloud_tool.write_kept(dst, {"vertices": v, "colors": None, "normals": None}, some, vertices=moved, normals=-n)
    m = ply.read_ply_model(dst)
    assert np.array_equal(m["vertices"], moved[some]) and np.array_equal(m["normals"], -n[some]) and (m["colors"] == 255).all()
    cloud_tool.write_kept(dst, {"vertices": v, "colors": c, "normals": n}, some)   # without it: the file's own, as before
    assert np.array_equal(ply.read_ply_model(dst)["vertices"], v[some])


def _cli(args, timeout=120):
    return subprocess.run([sys.executable, os.path.join(ROOT, "smooth_cloud.py")] + args, capture_output=True, text=True, timeout=timeout,
                          cwd=ROOT, env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})


def _body(path, n_bytes):
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    assert len(body) % n_bytes == 0
    return head.decode(), np.frombuffer(body, np.uint8).reshape(-1, n_bytes)


def _sheet(n, seed):
    """A noisy sheet without outliers, colours, and unit normals that point up or down at random."""
    rng = np.random.default_rng(seed)
    pts = R.sheet_cloud(n, planted=0, seed=seed)
    colors = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    normals = (np.array([[0.0, 0.0, 1.0]]) * np.where(rng.random(n) < 0.4, -1.0, 1.0)[:, None]).astype(np.float32)
    return pts, colors, normals


@pytest.mark.gpu
def test_smooth_cloud_round_trip(tmp_path):
    import torch
    from patchmatchnet_amd import _lib, ply, pointcloud as PC
    pts, colors, normals = _sheet(1000, 3)
    src, dst, rep = str(tmp_path / "fused.ply"), str(tmp_path / "out" / "fused_smooth.ply"), str(tmp_path / "r" / "report.json")
    ply.write_ply(src, pts, colors, normals)
    dev_pts = torch.from_numpy(pts).to("cuda:0")
    # --normals keep, the default: positions are smooth_mls', everything else is the file's, byte for byte
    r = _cli(["--input", src, "--output", dst, "--k", "16", "--iterations", "2", "--report", rep])
    assert r.returncode == 0, r.stderr
    want, want_n, info = PC.smooth_mls(dev_pts, k=16, iterations=2, return_normals=True)
    want, want_n = want.cpu().numpy(), want_n.cpu().numpy()
    head_in, rec_in = _body(src, 27)
    head_out, rec_out = _body(dst, 27)
    assert head_out == head_in and len(rec_out) == len(pts)
    assert np.array_equal(rec_out[:, :12], want.view(np.uint8).reshape(-1, 12)) and not np.array_equal(rec_out[:, :12], rec_in[:, :12])
    assert np.array_equal(rec_out[:, 12:], rec_in[:, 12:])   # normals and colours
    assert info["status"][2] > 900 and sum(info["status"]) == len(pts) and 0.0 < info["mean_displacement_spacings"] < 1.0
    js = json.load(open(rep))
    assert list(js) == ["abi", "radius", "radius_spacings", "k", "degree", "iterations", "normals", "cell", "files"]
    assert js["abi"] == _lib.ABI_VERSION and (js["radius"], js["radius_spacings"], js["k"], js["degree"], js["iterations"], js["normals"],
                                              js["cell"]) == (None, None, 16, 2, 2, "keep", None)
    f = js["files"][0]
    assert (f["input"], f["output"], f["points"], f["normals"]) == (src, dst, len(pts), "keep")
    for key, value in info.items():
        assert f[key] == value, key
    line = [ln for ln in r.stdout.splitlines() if "points read" in ln]
    s0, s1, s2 = info["status"]
    assert len(line) == 1 and f"{len(pts)} points read, {s0} not fitted, {s1} on a plane, {s2} on a quadric" in line[0]
    assert f"moved {info['mean_displacement_spacings']:.4g} spacings on average, {info['max_displacement_spacings']:.4g} at most" in line[0]
    # --normals refit: unit normals of the fitted surfaces on the side of the file's
    dst2 = str(tmp_path / "refit.ply")
    r = _cli(["--input", src, "--output", dst2, "--k", "16", "--iterations", "2", "--normals", "refit"])
    assert r.returncode == 0, r.stderr
    m = ply.read_ply_model(dst2)
    assert np.array_equal(m["vertices"], want) and np.array_equal(m["colors"], colors)
    side = (want_n.astype(np.float64) * normals.astype(np.float64)).sum(1) < 0
    assert 0 < side.sum() < len(pts) and np.array_equal(m["normals"], np.where(side[:, None], -want_n, want_n))
    assert np.abs(np.linalg.norm(m["normals"].astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -22
    assert ((m["normals"].astype(np.float64) * normals.astype(np.float64)).sum(1) > 0).all()
    # --normals drop, --degree 1 and a radius in scene units
    dst3 = str(tmp_path / "drop.ply")
    r = _cli(["--input", src, "--output", dst3, "--degree", "1", "--radius", "4.5", "--normals", "drop"])
    assert r.returncode == 0, r.stderr
    m = ply.read_ply_model(dst3)
    plane, info1 = PC.smooth_mls(dev_pts, radius=4.5, degree=1)
    assert m["normals"] is None and np.array_equal(m["vertices"], plane.cpu().numpy()) and np.array_equal(m["colors"], colors)
    assert info1["status"][2] == 0 and info1["status"][1] > 900


@pytest.mark.gpu
def test_smooth_cloud_scan_list(tmp_path):
    import torch
    from patchmatchnet_amd import ply, pointcloud as PC
    (tmp_path / "list.txt").write_text("scan1\nscan9\n")
    want = {}
    for scan, seed in (("scan1", 5), ("scan9", 6)):
        pts, colors, _ = _sheet(600, seed)
        ply.write_ply(str(tmp_path / "out" / scan / "fused.ply"), pts, colors)
        want[scan] = (PC.smooth_mls(torch.from_numpy(pts).to("cuda:0"))[0].cpu().numpy(), colors)
    r = _cli(["--input", str(tmp_path / "out"), "--scan_list", str(tmp_path / "list.txt")])
    assert r.returncode == 0, r.stderr
    for scan, (moved, colors) in want.items():
        m = ply.read_ply_model(str(tmp_path / "out" / scan / "fused_smooth.ply"))
        assert np.array_equal(m["vertices"], moved) and np.array_equal(m["colors"], colors) and m["normals"] is None
