"""CPU checks around cloud cleaning: the brute-force yardstick tests/knn_ref.py against a pure-Python loop, the inputs of the GPU
filter tests (no mean near the threshold), and clean_cloud.py's argument errors, which must not need a GPU."""
import math
import os
import subprocess
import sys

import numpy as np

import knn_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knn_ref_against_a_pure_python_loop():
    pts = np.random.default_rng(0).integers(-1, 2, (12, 3)).astype(np.float32) * np.float32(0.37)
    pts[5] = pts[2]  # a duplicate
    k, max_dist, radius = 4, 1.1, float(np.float32(0.37))
    p = [[float(v) for v in row] for row in pts]
    for same in (True, False):
        qs = p if same else np.array([[0.1, -0.2, 0.3], [50.0, 0.0, 0.0]], np.float32).tolist() + p[:3]
        rows, counts = [], []
        for i, q in enumerate(qs):
            d2 = sorted((q[0] - c[0]) * (q[0] - c[0]) + (q[1] - c[1]) * (q[1] - c[1]) + (q[2] - c[2]) * (q[2] - c[2])
                        for j, c in enumerate(p) if not (same and j == i))
            rows.append([v if v < max_dist * max_dist else max_dist * max_dist for v in d2[:k]])
            counts.append(sum(math.sqrt(v) <= radius for v in d2))
        query = np.asarray(qs, np.float32)
        got = K.knn_d2(query, pts, k, max_dist, same)
        assert got.tolist() == rows
        means = []
        for r in rows:
            s = 0.0
            for v in r:
                s += max_dist if v == max_dist * max_dist else math.sqrt(v)
            means.append(s / k)
        assert K.knn_mean(got, max_dist).tolist() == means
        assert K.radius_count(query, pts, radius, same).tolist() == counts
        assert max(counts) >= 2 and (same or any(max_dist * max_dist in r for r in rows))
    assert K.knn_d2(None, pts[:3], 4, max_dist, True)[:, 2:].tolist() == [[max_dist * max_dist] * 2] * 3  # fewer points than k


def test_filter_inputs_have_no_mean_near_the_threshold():
    """The keep masks of tests/test_knn_gpu.py are compared exactly; that is fair only where the reference alone shows no mean within
    a relative 1e-9 of the threshold.  The same inputs, checked here without a GPU."""
    cases = [(K.surface_cloud()[0], 20, 2.0, 5.0), (K.surface_cloud()[0], 8, 1.0, 3.0), (K.lattice_cloud(), 8, 1.0, 2.0),
             (K.duplicate_cloud(), 8, 1.0, 2.0), (K.surface_cloud(3000, seed=2)[0], 20, 2.0, 5.0)]
    for pts, k, ratio, max_dist in cases:
        keep, mean, threshold = K.statistical_outliers(pts, k, ratio, max_dist)
        assert (np.abs(mean - threshold) > 1e-9 * threshold).all()
        assert keep.any() and not keep.all()
    pts, planted, offset = K.surface_cloud()
    keep = K.statistical_outliers(pts, 20, 2.0, 5.0)[0]
    assert not keep[planted & (offset > 2.0)].any() and (~keep[~planted]).mean() <= 0.01
    keep = K.radius_outliers(pts, 2.0, 4)[0]
    assert not keep[planted & (offset > 2.0)].any() and (~keep[~planted]).mean() <= 0.03


def _run(args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    e["HIP_VISIBLE_DEVICES"] = ""  # no device may be needed to refuse
    return subprocess.run([sys.executable, os.path.join(ROOT, "clean_cloud.py")] + args, capture_output=True, text=True, timeout=300,
                          cwd=ROOT, env=e)


def _refused(r, word):
    assert r.returncode != 0 and r.stdout == ""
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("clean_cloud.py: ") and word in lines[0], r.stderr


def test_clean_cloud_argument_errors(tmp_path):
    from patchmatchnet_amd import fusion
    cloud, mesh, out = str(tmp_path / "fused.ply"), str(tmp_path / "mesh.ply"), str(tmp_path / "clean.ply")
    fusion.write_ply(cloud, np.zeros((5, 3), np.float32), np.zeros((5, 3), np.uint8))
    with open(mesh, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                b"element face 1\nproperty list uchar int vertex_indices\nend_header\n")
        np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], "<f4").tofile(f)
        f.write(b"\x03" + np.array([0, 1, 2], "<i4").tobytes())
    _refused(_run(["--input", str(tmp_path / "missing.ply"), "--output", out]), "no such file")
    _refused(_run(["--input", mesh, "--output", out]), "mesh.py --keep_components")
    _refused(_run(["--input", cloud, "--output", out, "--method", "radius", "--min_neighbors", "2"]), "--radius")
    _refused(_run(["--input", cloud, "--output", out], env={"WORLD_SIZE": "2"}), "torchrun")
    _refused(_run(["--input", cloud, "--output", out, "--k", "33"]), "--k")
    _refused(_run(["--input", str(tmp_path), "--scan_list", str(tmp_path / "none.txt")]), "scan list")
    assert not os.path.exists(out)
