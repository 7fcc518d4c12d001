"""pmn_mesh_distance on the device against the numpy brute force tests/mesh_distance_ref.py.

Tolerance: nothing is fixed here.  Every case measures the yardstick's own float64-versus-longdouble disagreement on its inputs
(mesh_distance_ref.gate), prints it, and gates at 4 x that figure.  `face` is accepted when the yardstick's distance to the returned
face is within the gate of the yardstick's minimum (ties on shared edges and vertices are the common case); the lower-index rule is
tested only where the squares are bit-equal, on a face listed twice."""
import numpy as np
import pytest
import torch

import mesh_distance_ref as R
from test_mesh_distance_ref import TRI_F, TRI_V, seven_regions

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _search(v, f, q, max_dist, cell=None, cover=None):
    from patchmatchnet_amd import meshops
    fg = meshops.build_face_grid(_up(v), _up(f), cell=cell, cover=cover)
    d, face, closest = meshops.point_mesh_distance(_up(q), fg, max_dist, return_face=True, return_closest=True)
    return fg, d.cpu().numpy(), face.cpu().numpy(), closest.cpu().numpy()


def _compare(name, v, f, q, got, wide=None):
    """The outputs of a search whose cap no query reaches, against the brute force."""
    d, face, closest = got
    wide = wide if wide is not None else R.brute_force(v, f, q)
    allowed, allowed_c, figures = R.gate(v, f, q, wide)
    dw = np.sqrt(wide[0])
    err = np.abs(d.astype(np.longdouble) - dw)
    print(f"{name}: {len(q)} queries, {len(f)} faces; float64 against longdouble {figures}; kernel against longdouble: worst "
          f"|d - d_ref| / allowed {float((err / allowed).max()):.3f}, faces other than the yardstick's arg-min "
          f"{int((face != wide[1]).sum())}")
    assert (face >= 0).all() and (face < len(f)).all()
    assert (err <= allowed).all()
    at_face = wide[3][np.arange(len(q)), face]
    assert (at_face - dw <= allowed).all()                         # the returned face attains the minimum within the gate
    same = face == wide[1]
    assert same.any()
    assert (np.abs(closest.astype(np.longdouble) - wide[2])[same] <= allowed_c).all()
    # whatever the face: the point is on it, and at the distance
    on = R.face_distance(v, f, closest, face)
    away = np.sqrt(((q.astype(np.longdouble) - closest.astype(np.longdouble)) ** 2).sum(1))
    assert (on <= 2 * allowed_c).all() and (np.abs(away - dw) <= allowed + 2 * allowed_c).all()
    return wide


@pytest.mark.parametrize("n", [1, 63, 65, 5003])
def test_one_triangle_seven_regions(n):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    q7, d7, c7 = seven_regions()
    rng = np.random.default_rng(n)
    q = np.concatenate([q7, rng.uniform(-6, 9, (max(n - len(q7), 0), 3)).astype(np.float32)])[:n]
    _, d, face, closest = _search(TRI_V, TRI_F, q, 100.0)
    m = min(n, len(q7))
    # the hand-derived values: sqrt of a sum that is exact in float64, so the kernel's correctly rounded sqrt must give these very
    # bits, and the nearest points are exact (small dyadic coordinates) -- no tolerance
    assert np.array_equal(d[:m], d7[:m]) and np.array_equal(closest[:m], c7[:m])
    _compare(f"one triangle, n = {n}", TRI_V, TRI_F, q, (d, face, closest))


def test_icosphere_inside_outside_and_on_the_surface():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    v, f = R.icosphere(3)
    rng = np.random.default_rng(7)
    u = rng.normal(size=(5000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    radius = np.concatenate([rng.uniform(0.0, 0.99, 1700), rng.uniform(1.01, 6.0, 1700), np.ones(1600)])
    q = (u * radius[:, None]).astype(np.float32)
    b = rng.dirichlet((1, 1, 1), 1500)
    fi = rng.integers(0, len(f), 1500)
    q[3400:4900] = np.einsum("nk,nkc->nc", b, v.astype(np.float64)[f[fi]]).astype(np.float32)  # on the faces, to float32 rounding
    q[4900:] = v[rng.integers(0, len(v), 100)]                                                  # on the vertices, exactly
    fg, d, face, closest = _search(v, f, q, 50.0)
    assert int(fg.levels.max()) == 0
    _compare("icosphere", v, f, q, (d, face, closest))
    assert d[3400:].max() < 1e-6 and d[4900:].max() == 0.0


def _strips():
    """Two strips of 2 x 1250 squares that share the edge y = 0, the second folded up by 60 degrees: 5 000 faces."""
    v1, f1 = R.plane_grid(1250, 1, step=0.5, origin=(0.0, -0.5))
    v2, f2 = R.plane_grid(1250, 1, step=0.5, origin=(0.0, 0.0))
    v2 = np.stack([v2[:, 0], v2[:, 1] * 0.5, v2[:, 1] * np.float32(np.sqrt(0.75))], 1).astype(np.float32)
    return np.concatenate([v1, v2]), np.concatenate([f1, f2 + len(v1)]).astype(np.int32)


def test_strips_any_face_order_same_bits():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    v, f = _strips()
    assert len(f) == 5000
    rng = np.random.default_rng(8)
    q = np.stack([rng.uniform(-2, 627, 700), rng.uniform(-1.5, 1.5, 700), rng.uniform(-1, 1.5, 700)], 1).astype(np.float32)
    q[:100, 1:] = 0.0  # on the shared edge: four or six faces tie
    orders = {"natural": np.arange(len(f)), "reversed": np.arange(len(f))[::-1].copy(), "permuted": rng.permutation(len(f))}
    out, wide = {}, None
    for name, order in orders.items():
        _, d, face, closest = _search(v, f[order], q, 1000.0)
        out[name] = (d, order[face], closest)
        if wide is None:
            wide = _compare("two strips", v, f, q, out[name])
    allowed, allowed_c, _ = R.gate(v, f, q, wide)
    for name in ("reversed", "permuted"):
        assert out[name][0].tobytes() == out["natural"][0].tobytes(), name       # dist: bit-equal under any order of the faces
        assert (np.abs(out[name][2] - out["natural"][2]) <= 2 * allowed_c).all(), name
        assert (wide[3][np.arange(len(q)), out[name][1]] - np.sqrt(wide[0]) <= allowed).all(), name


def test_giant_face_among_small_ones():
    """2 000 faces of edge about 1 and one of edge 5 000, the cell left at its default (a small multiple of the small faces' edge): the nearest surface of the first
    queries is the interior of the giant face, thousands of cells from its centroid -- what a one-entry-per-face grid cannot find."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    v, f = R.plane_grid(40, 25, step=1.0, origin=(100.0, 100.0), z=3.0)
    assert len(f) == 2000
    giant = np.array([[0, 0, 0], [5000, 0, 0], [0, 5000, 0]], np.float32)
    v, f = np.concatenate([v, giant]), np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)
    rng = np.random.default_rng(9)
    far = np.stack([rng.uniform(0, 4600, 300), rng.uniform(0, 350, 300), rng.uniform(-9, 9, 300)], 1)        # over the giant face
    far = far[(far[:, 0] < 90) | (far[:, 0] > 150) | (far[:, 1] < 90) | (far[:, 1] > 135)]
    small = np.stack([rng.uniform(100, 140, 300), rng.uniform(100, 125, 300), rng.uniform(1.6, 8, 300)], 1)    # nearer to the small ones
    q = np.concatenate([far, small, [[3000.0, 3000.0, 0.0], [-50.0, 2500.0, 1.0]]]).astype(np.float32)
    fg, d, face, closest = _search(v, f, q, 1.0e4)
    from patchmatchnet_amd import meshops
    assert abs(fg.grid.cell - meshops.FACE_CELL_EDGES * np.sqrt(2.0)) < 1e-5  # the default: from the median longest edge, sqrt(2)
    assert int(fg.levels[2000]) >= 9 and fg.radius < 4 * fg.grid.cell
    wide = _compare("giant face", v, f, q, (d, face, closest))
    assert (wide[1][:len(far)] == 2000).all() and (face[:len(far)] == 2000).all()
    assert (wide[1][len(far):len(far) + 300] < 2000).sum() > 200
    centroid = giant.mean(0)
    assert np.linalg.norm(closest[:len(far)] - centroid, axis=1).max() > 1000 * fg.grid.cell


def test_degenerate_duplicate_and_invalid_faces():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import PmnError, meshops
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0], [10, 0, 0], [14, 0, 0], [12, 0, 0], [20, 5, 5]], np.float32)
    f = np.array([[0, 1, 2], [3, 3, 4], [6, 6, 6], [3, 5, 4], [0, 1, 2], [3, 4, 4]], np.int32)
    q = np.array([[1, 1, 2], [12, 3, 0], [16, 0, 0], [20, 5, 7], [11, 0, 1], [2, -2, 0]], np.float32)
    want = np.array([2.0, 3.0, 2.0, 2.0, 1.0, 2.0])
    _, d, face, closest = _search(v, f, q, 100.0)
    assert np.array_equal(d, want)
    assert face[0] == 0 and face[5] == 0          # the face listed twice: the lower index
    assert face[3] == 2 and np.array_equal(closest[3], [20, 5, 5])
    assert face[1] == 1 and face[2] == 1 and face[4] == 1  # (a, a, b), collinear and (a, b, b) give bit-equal squares: the lowest
    assert np.array_equal(closest[[1, 2, 4]], [[12, 0, 0], [14, 0, 0], [11, 0, 0]])
    _compare("degenerate faces", v, f, q, (d, face, closest))
    only = np.array([[3, 5, 4]], np.int32)        # a collinear face alone is its longest segment
    assert np.array_equal(_search(v, only, q, 100.0)[1], R.face_distance(v, only, q, np.zeros(6, int), np.float64))  # the same operations
    for bad in (7, 2 ** 31 - 1, -1, -2 ** 31):
        g = f.copy()
        g[2, 1] = bad
        fg = meshops.build_face_grid(_up(v), _up(g))
        with pytest.raises(PmnError, match="1 faces have a vertex index outside"):
            meshops.point_mesh_distance(_up(q), fg, 100.0)


def test_far_queries_and_the_cap():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import meshops
    v, f = R.plane_grid(6, 6)
    q = np.array([[3, 3, 3],                       # exactly at max_dist = 3: the cap
                  [3, 3, np.nextafter(np.float32(3), np.float32(0))],  # just inside
                  [3, 3, -2.5], [-4, 3, 0], [1.0e6, -2.0e6, 3.0e6], [3, 3, 1.0e4], [2, 2, 0]], np.float32)
    fg = meshops.build_face_grid(_up(v), _up(f))
    d, face, closest = (t.cpu().numpy() for t in meshops.point_mesh_distance(_up(q), fg, 3.0, True, True))
    assert np.array_equal(d, [3.0, float(q[1, 2]), 2.5, 3.0, 3.0, 3.0, 0.0])
    capped = np.array([True, False, False, True, True, True, False])
    assert np.array_equal(face < 0, capped) and (face[capped] == -1).all()
    assert np.isnan(closest[capped]).all() and np.array_equal(closest[~capped], [[3, 3, 0], [3, 3, 0], [2, 2, 0]])
    # a cap nobody reaches: the far queries against the brute force
    d2, face2, closest2 = (t.cpu().numpy() for t in meshops.point_mesh_distance(_up(q), fg, 1.0e7, True, True))
    _compare("far queries", v, f, q, (d2, face2, closest2))
    # any subset of the optional outputs: the same dist bits
    for rf, rc in ((False, False), (True, False), (False, True)):
        out = meshops.point_mesh_distance(_up(q), fg, 3.0, return_face=rf, return_closest=rc)
        first = out if not (rf or rc) else out[0]
        assert first.cpu().numpy().tobytes() == d.tobytes()
        if rf:
            assert np.array_equal(out[1].cpu().numpy(), face)
        if rc:
            assert out[1].cpu().numpy().tobytes() == closest.tobytes()


def test_argument_checks():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import PmnError, meshops
    v, f = _up(TRI_V), _up(TRI_F)
    fg = meshops.build_face_grid(v, f)
    q = _up(np.zeros((4, 3), np.float32))
    for bad in (q.cpu(), q.double(), q[:, :2], q.reshape(-1), q[:0]):
        with pytest.raises(PmnError):
            meshops.point_mesh_distance(bad, fg, 1.0)
    nan = q.clone()
    nan[1, 1] = float("nan")
    with pytest.raises(PmnError, match="non-finite"):
        meshops.point_mesh_distance(nan, fg, 1.0)
    for md in (0.0, -1.0, float("inf"), float("nan"), 1.0e200):
        with pytest.raises(PmnError, match="max_dist"):
            meshops.point_mesh_distance(q, fg, md)
    with pytest.raises(PmnError, match="on cpu"):  # device mismatch: a face grid built from host tensors
        meshops.point_mesh_distance(q, meshops.build_face_grid(v.cpu(), f.cpu()), 1.0)
    with pytest.raises(PmnError):
        meshops.point_mesh_distance(q, fg.grid, 1.0)
    with pytest.raises(PmnError):
        meshops.build_face_grid(v, f.cpu())


# ---- the command lines ------------------------------------------------------------------------------------------------------------------

def _run(script, args, env_extra=None):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, script)] + args, cwd=root, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)  # a fresh process


def _rounding(*arrays):
    """What 'on the surface' means for points blended from a face's vertices in float32 (meshops_ref.sample_ref): three weights that
    sum to 1 within 3 units of 2^-24 and five rounded operations per coordinate leave a point within 8 * 2^-24 * max |coordinate| of
    the face per coordinate, sqrt(3) times that in all: below 16 * 2^-24 * max |coordinate|."""
    return 16.0 * 2.0 ** -24 * max(float(np.abs(a).max()) for a in arrays)


def test_eval_tnt_recall_against_the_surface(tmp_path):
    """A coarse sphere mesh (320 faces) as the reconstruction, and 20 000 points drawn ON that mesh as the ground truth.  Against the
    triangles every ground-truth distance is float32 rounding; against the vertices or samples it is of the order of their spacing."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    import json
    import os
    import meshops_ref as M
    from patchmatchnet_amd import fusion, registration as RG, tsdf
    v, f = R.icosphere(2)
    gt = M.sample_ref(v, f, 20000 / (4 * np.pi), seed=3)[0]
    tau, spacing = 0.002, 0.05
    data = tmp_path / "Ball"
    os.makedirs(data)
    fusion.write_ply(str(data / "Ball.ply"), gt, np.full((len(gt), 3), 128, np.uint8))
    tsdf.write_ply_mesh(str(tmp_path / "mesh.ply"), v, f)
    fusion.write_ply(str(tmp_path / "cloud.ply"), v, np.full((len(v), 3), 128, np.uint8))
    # the distances themselves, in process
    _, _, d_plain = RG.tnt_score(_up(v), _up(gt), None, tau, register=False, return_distances=True, hist_max=10.0)
    _, _, d_mesh = RG.tnt_score(_up(v), _up(gt), None, tau, register=False, return_distances=True, hist_max=10.0, mesh=(_up(v), _up(f)))
    bound = _rounding(v, gt)
    print(f"ground truth on the surface: distance to the triangles max {float(d_mesh.max()):.3e} (float32 rounding bound {bound:.3e}), "
          f"to the vertices median {float(d_plain.median()):.3e}, vertex spacing about 0.3")
    assert float(d_mesh.max()) <= bound and float(d_plain.median()) > 1.0e3 * bound and d_mesh.shape == d_plain.shape
    base = ["--dataset_dir", str(data), "--tau", str(tau), "--no_registration", "--no_crop", "--ply_path", str(tmp_path / "mesh.ply"),
            "--sample_spacing", str(spacing)]
    runs = {}
    for name, extra in (("plain", []), ("mesh", ["--mesh_distance", "1"])):
        p = _run("eval_tnt.py", base + ["--results_path", str(tmp_path / name)] + extra)
        assert p.returncode == 0, p.stdout
        runs[name] = json.load(open(tmp_path / name / "tnt_scores.json"))
    a, b = runs["plain"], runs["mesh"]
    print(f"tau {tau}: recall by samples at spacing {spacing} {a['recall']:.4f}, by the surface {b['recall']:.4f}")
    assert b["recall"] == 100.0 and a["recall"] < 10.0               # per cent
    assert b["precision"] == a["precision"]                      # the other leg is unchanged
    assert set(b) - set(a) == {"mesh_distance"} and not set(a) - set(b) and b["mesh_distance"] is True
    cloud = _run("eval_tnt.py", base[:-4] + ["--ply_path", str(tmp_path / "cloud.ply"), "--results_path", str(tmp_path / "cloud"),
                                             "--mesh_distance", "1"])
    assert cloud.returncode != 0 and "Traceback" not in cloud.stdout
    assert "cloud.ply: --mesh_distance needs a mesh" in cloud.stdout


def test_eval_dtu_completeness_against_the_surface(tmp_path):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    import json
    import os
    import dtu_ref
    import meshops_ref as M
    from patchmatchnet_amd import fusion, tsdf
    s = dtu_ref.synthetic_scan(11, n_stl=3000, n_data=5000)
    gx, gy = np.meshgrid(np.arange(0.0, 100.1, 5.0), np.arange(0.0, 100.1, 5.0), indexing="ij")
    mv = np.stack([gx.ravel(), gy.ravel(), dtu_ref.height(gx.ravel(), gy.ravel())], 1).astype(np.float32)
    idx = np.arange(21 * 21).reshape(21, 21)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    mf = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)
    stl = M.sample_ref(mv, mf, 0.5, seed=2)[0]                   # the ground truth: points ON the mesh
    data, ply = tmp_path / "data", tmp_path / "ply"
    os.makedirs(data / "ObsMask")
    tsdf.write_ply_mesh(str(ply / "scan1" / "mesh.ply"), mv, mf)
    fusion.write_ply(str(ply / "scan1" / "fused.ply"), s["data"], np.full((len(s["data"]), 3), 128, np.uint8))
    fusion.write_ply(str(data / "Points" / "stl" / "stl001_total.ply"), stl, np.zeros((len(stl), 3), np.uint8))
    np.savez(str(data / "ObsMask" / "ObsMask1_10.npz"), ObsMask=s["ObsMask"], BB=s["BB"], Res=s["Res"])
    np.savez(str(data / "ObsMask" / "Plane1.npz"), P=s["P"])
    argv = ["--data_path", str(data), "--ply_path", str(ply), "--results_path", str(tmp_path / "out"), "--scans", "1", "--ply_name",
            "mesh.ply"]
    r = _run("eval_dtu.py", argv)
    assert r.returncode == 0, r.stdout
    js = json.load(open(tmp_path / "out" / "dtu_scores.json"))
    assert set(js) == {"dst", "max_dist", "seed", "abi", "method", "light", "scans", "scans_scored", "total"}  # a plain run: its keys
    r2 = _run("eval_dtu.py", argv + ["--mesh_distance", "1"])   # into the SAME results folder: the plain scores are not taken for it
    assert r2.returncode == 0 and "already in" not in r2.stdout, r2.stdout
    js2 = json.load(open(tmp_path / "out" / "dtu_scores.json"))
    p, m = js["scans"]["1"], js2["scans"]["1"]
    bound = _rounding(mv, stl)
    print(f"stl on the mesh: completeness against the triangles mean {m['comp_mean']:.3e} (float32 rounding bound {bound:.3e}), against "
          f"the vertices {p['comp_mean']:.3e} (vertex spacing 5); {m['comp_n']} points")
    assert set(js2) - set(js) == {"mesh_distance"} and js2["mesh_distance"] is True and set(m) == set(p)
    assert m["comp_n"] == p["comp_n"] > 1000 and m["comp_mean"] <= bound and p["comp_mean"] > 100.0 * bound
    for k in ("acc_n", "acc_mean", "acc_median", "acc_var", "n_data_in", "n_data_reduced"):  # the other leg is unchanged
        assert m[k] == p[k] or (m[k] != m[k] and p[k] != p[k]), k
    r3 = _run("eval_dtu.py", argv)                               # and back: a plain run does not take the surface scores for its own
    assert r3.returncode == 0 and "already in" not in r3.stdout, r3.stdout
    assert set(json.load(open(tmp_path / "out" / "dtu_scores.json"))) == set(js)
    fused = _run("eval_dtu.py", argv[:-2] + ["--mesh_distance", "1", "--force"])
    assert fused.returncode != 0 and "Traceback" not in fused.stdout and "fused.ply: --mesh_distance needs a mesh" in fused.stdout


def test_compare_mesh_in_a_child_process(tmp_path):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    import json
    from patchmatchnet_amd import tsdf
    pv, pf = R.plane_grid(12, 9, step=0.5)
    sv, sf = R.icosphere(1)
    v, f = np.concatenate([pv, sv + np.float32([3, 2, 5])]).astype(np.float32), np.concatenate([pf, sf + len(pv)]).astype(np.int32)
    t = 0.25
    tsdf.write_ply_mesh(str(tmp_path / "a.ply"), v, f)
    tsdf.write_ply_mesh(str(tmp_path / "flat.ply"), pv, pf)
    tsdf.write_ply_mesh(str(tmp_path / "shifted.ply"), pv + np.float32([0, 0, t]), pf)
    p = _run("compare_mesh.py", ["--a", str(tmp_path / "a.ply"), "--b", str(tmp_path / "a.ply"), "--spacing", "0.2", "--seed", "5",
                                 "--report", str(tmp_path / "self.json")])
    assert p.returncode == 0, p.stdout
    js = json.load(open(tmp_path / "self.json"))
    bound = _rounding(v)
    print(p.stdout)
    assert js["a_to_b"] == js["b_to_a"] and js["a_to_b"]["count"] > 500 and js["a_to_b"]["queries"] == "samples"
    assert 0.0 <= js["hausdorff"] <= bound and js["a_to_b"]["max"] == js["hausdorff"]   # a mesh against itself: 0 within rounding
    assert "hausdorff:" in p.stdout and "a -> b" in p.stdout and "b -> a" in p.stdout
    p = _run("compare_mesh.py", ["--a", str(tmp_path / "flat.ply"), "--b", str(tmp_path / "shifted.ply"), "--report", str(tmp_path / "shift.json")])
    assert p.returncode == 0, p.stdout
    js = json.load(open(tmp_path / "shift.json"))
    print(p.stdout)
    for leg in ("a_to_b", "b_to_a"):   # a flat region moved by t along its normal: every vertex is at t (0.25 and 0: exact in float64)
        assert all(js[leg][k] == t for k in ("mean", "rms", "median", "p95", "max")), js[leg]
        assert js[leg]["target"] == "triangles"
    assert js["hausdorff"] == t
    p = _run("compare_mesh.py", ["--a", str(tmp_path / "a.ply"), "--b", str(tmp_path / "a.ply")], {"WORLD_SIZE": "2"})
    assert p.returncode == 2 and "torchrun" in p.stdout
