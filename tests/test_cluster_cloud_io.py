"""CPU checks of cluster_cloud.py: its argument errors, which must not need a GPU (exit code 2, one line), and its palette."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    e["HIP_VISIBLE_DEVICES"] = ""  # no device may be needed to refuse
    return subprocess.run([sys.executable, os.path.join(ROOT, "cluster_cloud.py")] + args, capture_output=True, text=True, timeout=300,
                          cwd=ROOT, env=e)


def _refused(r, word):
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout)
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("cluster_cloud.py: ") and word in lines[0], r.stderr


def test_cluster_cloud_argument_errors(tmp_path):
    from patchmatchnet_amd import ply
    cloud, mesh, out = str(tmp_path / "fused.ply"), str(tmp_path / "mesh.ply"), str(tmp_path / "clusters.ply")
    ply.write_ply(cloud, np.zeros((5, 3), np.float32), np.zeros((5, 3), np.uint8))
    ply.write_ply_mesh(mesh, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    _refused(_run(["--input", cloud]), "--output")
    _refused(_run(["--input", cloud, "--output", out, "--eps", "-0.5"]), "--eps")
    _refused(_run(["--input", cloud, "--output", out, "--eps", "nan"]), "--eps")
    _refused(_run(["--input", cloud, "--output", out, "--eps_spacings", "inf"]), "--eps_spacings")
    _refused(_run(["--input", cloud, "--output", out, "--min_points", "0"]), "--min_points")
    _refused(_run(["--input", cloud, "--output", out, "--keep_clusters", "-1"]), "--keep_clusters")
    _refused(_run(["--input", cloud, "--output", out, "--cell", "0"]), "--cell")
    _refused(_run(["--input", mesh, "--output", out]), "mesh.py --keep_components")
    _refused(_run(["--input", cloud, "--output", out], env={"WORLD_SIZE": "2"}), "torchrun")
    _refused(_run(["--input", str(tmp_path / "missing.ply"), "--output", out]), "no such file")
    _refused(_run(["--input", str(tmp_path), "--scan_list", str(tmp_path / "none.txt")]), "scan list")
    assert not os.path.exists(out)


def test_palette_is_a_fixed_hash_of_the_label():
    import cluster_cloud
    from meshops_ref import mix64
    labels = np.array([-1, 0, 1, 2, 1, 0, 4000, -1], np.int64)
    rgb = cluster_cloud.cluster_colors(labels)
    assert rgb.dtype == np.uint8 and rgb.shape == (8, 3)
    h = mix64((labels + 1).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    want = np.stack([64 + ((h >> np.uint64(s)) & np.uint64(255)) * 3 // 4 for s in (0, 8, 16)], 1).astype(np.uint8)
    want[labels < 0] = 128
    assert np.array_equal(rgb, want)
    assert np.array_equal(rgb[1], rgb[5]) and np.array_equal(rgb[2], rgb[4]) and (rgb[[0, 7]] == 128).all()
    many = cluster_cloud.cluster_colors(np.arange(64))
    assert len({tuple(c) for c in many.tolist()}) == 64 and many.min() >= 64  # one colour per label, none dark
