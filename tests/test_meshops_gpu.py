"""GPU checks of the mesh operations: pmn_mesh_components, meshops.remove_components and pmn_mesh_face_samples /
pmn_mesh_sample against the numpy yardstick tests/meshops_ref.py, then through ops.mt_extract, mesh.py, eval_tnt.py and eval_dtu.py.

Gates.  Labels, kept faces and vertices, sample positions, face indices and colour bytes follow bit-level definitions: every comparison
is array_equal, no allowance.  The one bound (the sampled sphere) is derived in its test."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dtu_ref
import meshops_ref as M
import synth
import tsdf_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEV = "cuda:0"


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _labels(faces, nv):
    from patchmatchnet_amd import meshops
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    label, roots, count = meshops.components(_up(np.asarray(faces, np.int32).reshape(-1, 3)), nv)
    assert label.dtype == torch.int32 and roots.dtype == torch.int32 and count.dtype == torch.int64
    return label.cpu().numpy(), roots.cpu().numpy(), count.cpu().numpy()


def _check_components(name, faces, nv):
    want, wroots, wcount = M.component_sizes_ref(faces, nv)
    got, roots, count = _labels(faces, nv)
    print(f"{name}: {nv} vertices, {len(faces)} faces, {len(wroots)} components; labels equal {np.array_equal(got, want)}")
    assert np.array_equal(got, want), name
    assert np.array_equal(roots, wroots) and np.array_equal(count, wcount), name
    return got


@pytest.fixture(scope="module")
def icosphere():
    return M.icosphere(3)  # 642 vertices, 1280 faces


@pytest.fixture(scope="module")
def mix(icosphere):
    """300 tetrahedra, an icosphere of 1280 faces, 37 unreferenced vertices, a second icosphere of the SAME size (the tie) and a strip."""
    far = (icosphere[0] + np.float32([0, 50, 0]), icosphere[1])
    return M.join(M.tetrahedra(300), icosphere, (np.zeros((37, 3), np.float32), np.zeros((0, 3), np.int32)), far, M.strip(9))


def test_components_of_a_strip():
    v, f = M.strip(5003)  # the deep chain: every face hooks onto the one before it
    nv = len(v)
    assert _check_components("strip, natural order", f, nv).max() == 0
    _check_components("strip, reversed", np.ascontiguousarray(f[::-1]), nv)
    _check_components("strip, permuted", M.permute_faces(f, 1), nv)
    # two strips and a relabelling: the partition maps through it, every label is the new minimum
    v2, f2 = M.join((v, f), M.strip(700))
    before = _check_components("two strips", f2, len(v2))
    _, f3, new = M.relabel_vertices(v2, f2, seed=2)
    after = _check_components("two strips, relabelled", f3, len(v2))
    assert np.array_equal(before == 0, after[new] == after[new[0]])
    for lab in np.unique(after):
        assert lab == np.nonzero(after == lab)[0].min()


def test_components_of_disjoint_and_degenerate_meshes(icosphere):
    v, f = M.tetrahedra(300)
    nv = len(v) + 37
    assert nv % 64 != 0
    got = _check_components("300 tetrahedra + 37 unreferenced vertices", f, nv)
    assert np.array_equal(got[len(v):], np.arange(len(v), nv)) and len(np.unique(got)) == 337
    # two icospheres joined only by the LAST face of the array
    v2, f2 = M.join(icosphere, icosphere)
    assert len(np.unique(_check_components("two icospheres", f2, len(v2)))) == 2
    f3 = np.concatenate([f2, [[5, 642 + 7, 642 + 7]]]).astype(np.int32)
    assert _check_components("two icospheres joined by the last face", f3, len(v2)).max() == 0
    # duplicate faces, (a, a, b) and (a, a, a)
    f4 = np.concatenate([f, f[:100], f[::-1][:50], [[1203, 1203, 1236], [1204, 1204, 1204], [1205, 3, 3]]]).astype(np.int32)
    got = _check_components("duplicates and degenerate faces", f4, nv)
    assert got[1236] == 1203 and got[1203] == 1203 and got[1204] == 1204 and got[1205] == 0
    # no face; one vertex
    assert np.array_equal(_check_components("no face", np.zeros((0, 3), np.int32), 100), np.arange(100))
    assert _check_components("one vertex", np.zeros((0, 3), np.int32), 1).tolist() == [0]
    assert _check_components("one vertex, one face", np.zeros((1, 3), np.int32), 1).tolist() == [0]


def test_components_are_reproducible_and_refuse_bad_indices(icosphere):
    from patchmatchnet_amd import PmnError, meshops
    v, f = M.join(icosphere, M.strip(3000), M.tetrahedra(50))
    f = M.permute_faces(f, 4)
    fd = _up(f)
    a, b = meshops.components(fd, len(v)), meshops.components(fd, len(v))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    nv = len(v)
    bad = f.copy()
    bad[10, 1], bad[2000, 0], bad[-1, 2] = -1, nv, 2 ** 31 - 1  # three faces, one bad index each: skipped, never dereferenced
    with pytest.raises(PmnError, match=r"\b3 faces"):
        meshops.components(_up(bad), nv)
    with pytest.raises(PmnError, match=r"\b3 faces"):
        meshops.sample_surface(_up(v), _up(bad), density=1.0)
    with pytest.raises(PmnError, match=r"\b3 faces"):
        meshops.remove_components(_up(v), _up(bad), min_faces=1)
    good = np.delete(bad, [10, 2000, len(bad) - 1], axis=0)
    _check_components("the valid faces afterwards", good, nv)


@pytest.mark.parametrize("min_faces,keep_largest", [(5, 0), (0, 1), (5, 2), (1281, 0), (0, 400)])
def test_remove_components_matches_the_reference(mix, min_faces, keep_largest):
    from patchmatchnet_amd import meshops
    v, f = mix
    f = M.permute_faces(f, 7)
    rng = np.random.default_rng(8)
    col = rng.integers(0, 256, (len(v), 3), dtype=np.uint8)
    nrm = rng.standard_normal((len(v), 3)).astype(np.float32)
    wv, wf, wc, wn, found, kept = M.remove_components_ref(v, f, col, nrm, min_faces, keep_largest)
    gv, gf, gc, gn, counts = meshops.remove_components(_up(v), _up(f), _up(col), _up(nrm), min_faces=min_faces,
                                                       keep_largest=keep_largest, return_counts=True)
    print(f"min_faces {min_faces} keep_largest {keep_largest}: {found} components, {kept} kept, {len(wv)} of {len(v)} vertices, "
          f"{len(wf)} of {len(f)} faces")
    assert counts == (found, kept) and found == 300 + 2 + 37 + 1
    assert gf.dtype == torch.int32 and gv.dtype == torch.float32 and gc.dtype == torch.uint8
    assert np.array_equal(gf.cpu().numpy(), wf) and np.array_equal(gv.cpu().numpy(), wv)
    assert np.array_equal(gc.cpu().numpy(), wc) and np.array_equal(gn.cpu().numpy(), wn)  # attributes follow their vertices
    if len(wf):
        assert 0 <= int(gf.min()) and int(gf.max()) == len(wv) - 1 and len(np.unique(gf.cpu().numpy())) == len(wv)
    if (min_faces, keep_largest) == (0, 1):  # the tie between the two icospheres goes to the smaller root: the first one
        assert np.array_equal(gv.cpu().numpy(), M.icosphere(3)[0])
        t = R.topology(gv.cpu().numpy(), gf.cpu().numpy())
        assert t["closed"] and t["euler"] == 2
    if (min_faces, keep_largest) == (5, 2):
        assert kept == 2 and len(wf) == 2560
    if min_faces == 1281:
        assert gv.shape == (0, 3) and gf.shape == (0, 3) and gc.shape == (0, 3)
    # without colours and normals: None stays None
    out = meshops.remove_components(_up(v), _up(f), min_faces=min_faces, keep_largest=keep_largest)
    assert len(out) == 4 and out[2] is None and out[3] is None and torch.equal(out[1], gf)
    dv, df = _up(v), _up(f)
    same = meshops.remove_components(dv, df)
    assert same[0] is dv and same[1] is df


def _check_samples(name, v, f, density, seed, colors=None):
    from patchmatchnet_amd import meshops
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    wp, wf, wc = M.sample_ref(v, f, density, seed, colors)
    gp, gf, gc = meshops.sample_surface(_up(v), _up(f), density=density, seed=seed, colors=_up(colors))
    assert gp.dtype == torch.float32 and gf.dtype == torch.int32 and gp.shape == (len(wp), 3) and gf.shape == (len(wp),)
    gp, gf = gp.cpu().numpy(), gf.cpu().numpy()
    print(f"{name}: {len(wp)} samples on {len(f)} faces; positions bit-equal {gp.tobytes() == wp.tobytes()}, faces equal "
          f"{np.array_equal(gf, wf)}")
    assert np.array_equal(gf, wf), name
    assert gp.tobytes() == wp.tobytes(), name  # bit for bit (NaN-proof)
    if colors is None:
        assert gc is None
    else:
        assert gc.dtype == torch.uint8 and np.array_equal(gc.cpu().numpy(), wc), name
    return gp, gf


def test_samples_are_bit_equal_to_the_reference(icosphere):
    from patchmatchnet_amd import meshops
    rng = np.random.default_rng(3)
    tri_v = np.array([[0.5, -1.0, 2.0], [10.25, 0.5, 3.0], [-2.0, 7.0, 1.5]], np.float32)
    tri_f = np.array([[0, 1, 2]], np.int32)
    area = float(M.face_areas_f32(tri_v, tri_f)[0])
    p, _ = _check_samples("one triangle", tri_v, tri_f, 1000.0 / area, 5, rng.integers(0, 256, (3, 3), dtype=np.uint8))
    assert abs(len(p) - 1000) <= 1
    v, f = icosphere
    col = rng.integers(0, 256, (len(v), 3), dtype=np.uint8)
    total = float(M.face_areas_f32(v, f).astype(np.float64).sum())
    for expected in (50, 20000, 300000):
        p, face = _check_samples(f"icosphere, about {expected}", v, f, expected / total, 17, col)
        assert abs(len(p) - expected) <= 3 * np.sqrt(len(f)) + 1e-5 * expected  # the count contract of test_meshops_io.py
    _check_samples("icosphere without colours", v, f, 2000 / total, 1)
    # zero-area faces and a NaN vertex: those faces get no sample
    v2 = np.concatenate([v, [[np.nan, 0.0, 0.0], [np.inf, 1.0, 1.0]]]).astype(np.float32)
    f2 = np.concatenate([[[0, 0, 1], [3, 642, 4], [5, 6, 643]], f, [[7, 7, 7], [1, 2, 642]]]).astype(np.int32)
    p, face = _check_samples("zero-area faces and non-finite vertices", v2, f2, 5000 / total, 2, np.concatenate([col, col[:2]]))
    assert np.isfinite(p).all() and face.min() >= 3 and face.max() < 3 + len(f)
    # a density so low that nothing is drawn
    p, face = _check_samples("nothing", v, f, 1e-9, 0, col)
    assert p.shape == (0, 3) and face.shape == (0,)
    # one face owns over 90 % of the samples, and it sits in the middle of the array
    big = np.array([[-40, -40, 9], [40, -40, 9], [0, 60, 9]], np.float32)
    v3 = np.concatenate([v, big])
    f3 = np.concatenate([f[:700], [[642, 643, 644]], f[700:]]).astype(np.int32)
    p, face = _check_samples("skewed", v3, f3, 20.0, 9, np.concatenate([col, col[:3]]))
    assert (face == 700).mean() > 0.9 and len(p) > 50000
    # seeds, and spacing = density^-1/2
    a = meshops.sample_surface(_up(v), _up(f), density=400.0, seed=1)
    b = meshops.sample_surface(_up(v), _up(f), density=400.0, seed=1)
    c = meshops.sample_surface(_up(v), _up(f), density=400.0, seed=2)
    d = meshops.sample_surface(_up(v), _up(f), spacing=0.05, seed=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], d[0])
    assert a[0].shape != c[0].shape or not torch.equal(a[0], c[0])
    e = meshops.sample_surface(_up(v), _up(np.zeros((0, 3), np.int32)), density=1.0)
    assert e[0].shape == (0, 3) and e[1].shape == (0,) and e[2] is None


def test_sphere_and_floater_from_the_volume():
    """tsdf_ref's 40^3 sphere and a far blob of radius 2 voxels: two components; keep_largest = 1 leaves the sphere, whose faces are
    the oracle's sphere-only mesh; sampled 0.25 voxel apart, the surface covers the analytic sphere better than its vertices do.
    Bound: a point of the sphere is within (distance to the mesh) + (distance on the mesh to a sample).  The first is at most the
    sagitta of a chord of <= sqrt(3) voxel at r = 13.4 plus the linear-interpolation error of the clipped field, together < 0.1 voxel;
    the second exceeds 0.75 voxel (three spacings: a disc that should hold 28 samples holds none) with probability e^-28 per point.
    So the largest distance to the samples is below 1 voxel, and below the vertices' (which sit about a voxel apart)."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import meshops, ops, pointcloud as PC
    centre, radius = (19.3, 20.1, 19.7), 13.4
    sphere = R.sphere_field(40, centre, radius)
    blob = R.sphere_field(40, (34.6, 35.2, 5.4), 2.0)
    field = np.minimum(sphere, blob)
    w = np.ones_like(field)
    v, f, _, _ = ops.mt_extract(_up(field), _up(w), (0.0, 0.0, 0.0), 1.0)
    label, roots, count = meshops.components(f, v.shape[0])
    print(f"sphere + blob: {v.shape[0]} vertices, {f.shape[0]} faces, components {roots.tolist()} with {count.tolist()} faces")
    assert roots.numel() == 2 and int(count.min()) > 0
    kv, kf, _, _ = meshops.remove_components(v, f, keep_largest=1)
    want = R.extract(sphere, w, (0.0, 0.0, 0.0), 1.0, normals=False)
    assert np.array_equal(kf.cpu().numpy(), want["faces"]) and kv.shape[0] == len(want["vertices"])
    t = R.topology(kv.cpu().numpy(), kf.cpu().numpy())
    assert t["closed"] and t["euler"] == 2
    pts, face, _ = meshops.sample_surface(kv, kf, spacing=0.25, seed=1)
    d = np.random.default_rng(0).standard_normal((20000, 3))
    on_sphere = _up((np.asarray(centre) + radius * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    to_samples = float(PC.nn_distance(on_sphere, PC.build_grid(pts, 1.0), 10.0).max())
    to_vertices = float(PC.nn_distance(on_sphere, PC.build_grid(kv, 1.0), 10.0).max())
    print(f"sphere r = 13.4 voxel: {pts.shape[0]} samples at spacing 0.25; largest distance from 20000 analytic points to the samples "
          f"{to_samples:.4f}, to the {kv.shape[0]} vertices {to_vertices:.4f} voxel")
    assert to_samples < to_vertices and to_samples < 1.0


# ---- command lines ---------------------------------------------------------------------------------------------------------------

def _run(script, args, cwd=ROOT):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)  # a fresh process


@pytest.fixture(scope="module")
def scan_with_floater(tmp_path_factory):
    """The rendered 5-view 96 x 128 scan of tests/test_tsdf_gpu.py with its true depth maps, plus a ball of radius 6 in front of the
    surface drawn into every map: consistent across the views, so the volume holds it as a floater."""
    from PIL import Image
    from patchmatchnet_amd import data_io
    root = tmp_path_factory.mktemp("meshops_scan")
    n, H, W = 5, 96, 128
    src = synth.write_scene_scan(str(root), "scene", n, H, W, n_src=2)
    _, intr, extr, depths = synth.render_scene(n, H, W, cameras=synth.arc_cameras(n, H, W), all_depths=True)
    res = str(root / "results")
    os.makedirs(os.path.join(res, "depth_est"))
    os.makedirs(os.path.join(res, "mask"))
    for v in range(n):
        ball = R.render_sphere(intr[0, v], extr[0, v], H, W, (10.0, -5.0, 612.0), 6.0)
        d = np.where(ball > 0, ball, depths[v].numpy().astype(np.float32)).astype(np.float32)
        assert (ball > 0).sum() > 10
        data_io.save_pfm(os.path.join(res, "depth_est/{:0>8}.pfm".format(v)), d)
        Image.fromarray(np.full((H, W), 255, np.uint8)).save(os.path.join(res, "mask/{:0>8}_final.png".format(v)))
    grid = ["--voxel", "5.0", "--trunc", "20.0", "--bounds"] + [str(b) for b in (-120.0, -90.0, 580.0, 120.0, 90.0, 720.0)]
    return src, res, grid


@pytest.mark.parametrize("volume", ["dense", "sparse"])
def test_mesh_py_removes_the_floater(scan_with_floater, tmp_path, volume):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import tsdf
    src, res, grid = scan_with_floater
    base = ["--input_folder", src, "--results_folder", res, "--volume", volume] + grid
    outs = {}
    for name, extra in (("plain", []), ("off", ["--min_component_faces", "0"]), ("one", ["--keep_components", "1"]),
                        ("min", ["--min_component_faces", "400", "--keep_components", "3"])):
        p = _run("mesh.py", base + ["--output_folder", str(tmp_path / name)] + extra)
        print(p.stdout)
        assert p.returncode == 0, p.stdout
        outs[name] = (p.stdout, os.path.join(str(tmp_path / name), "mesh.ply"))
    assert open(outs["plain"][1], "rb").read() == open(outs["off"][1], "rb").read()
    assert "components" not in outs["plain"][0] and "components" not in outs["off"][0]
    v, f, c, nrm = tsdf.read_ply_mesh(outs["plain"][1])
    label, roots, count = M.component_sizes_ref(f, len(v))
    print(f"--volume {volume}: {len(v)} vertices, {len(f)} faces, components with {sorted(count.tolist(), reverse=True)[:5]} ... faces")
    assert len(roots) >= 2 and np.sort(count)[-2] >= 20  # the floater is there
    for name, kw in (("one", dict(keep_largest=1)), ("min", dict(min_faces=400, keep_largest=3))):
        wv, wf, wc, wn, found, kept = M.remove_components_ref(v, f, c, nrm, **kw)
        gv, gf, gc, gn = tsdf.read_ply_mesh(outs[name][1])
        assert np.array_equal(gf, wf) and gv.tobytes() == wv.tobytes() and np.array_equal(gc, wc) and gn.tobytes() == wn.tobytes()
        line = ": {} components, {} kept; {} vertices and {} faces dropped".format(found, kept, len(v) - len(wv), len(f) - len(wf))
        assert line in outs[name][0], (line, outs[name][0])
        assert "-> {} vertices, {} faces; load".format(len(wv), len(wf)) in outs[name][0]  # the report line keeps its format
        assert len(wf) < len(f)


def test_eval_tnt_scores_the_sampled_surface(tmp_path):
    """A coarse mesh (320 faces) of a sphere whose ground truth is a dense cloud: scored by its 162 vertices it recalls next to
    nothing at tau = 0.04; sampled at a quarter of its mean edge it recalls more."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import fusion, tsdf
    v, f = M.icosphere(2)
    fine_v, fine_f = M.icosphere(5)
    gt = M.sample_ref(fine_v, fine_f, 40000 / (4 * np.pi), seed=3)[0]
    data = tmp_path / "Ball"
    os.makedirs(data)
    fusion.write_ply(str(data / "Ball.ply"), gt, np.full((len(gt), 3), 128, np.uint8))
    tsdf.write_ply_mesh(str(tmp_path / "mesh.ply"), v, f)
    fusion.write_ply(str(tmp_path / "cloud.ply"), v, np.full((len(v), 3), 128, np.uint8))
    edges = np.concatenate([v[f[:, 0]] - v[f[:, 1]], v[f[:, 1]] - v[f[:, 2]], v[f[:, 2]] - v[f[:, 0]]])
    spacing = float(np.linalg.norm(edges, axis=1).mean()) / 4
    base = ["--dataset_dir", str(data), "--tau", "0.04", "--no_registration", "--no_crop"]
    plain = _run("eval_tnt.py", base + ["--ply_path", str(tmp_path / "mesh.ply"), "--results_path", str(tmp_path / "plain")])
    assert plain.returncode == 0, plain.stdout
    sampled = _run("eval_tnt.py", base + ["--ply_path", str(tmp_path / "mesh.ply"), "--results_path", str(tmp_path / "sampled"),
                                          "--sample_spacing", str(spacing), "--sample_seed", "4"])
    assert sampled.returncode == 0, sampled.stdout
    a = json.load(open(tmp_path / "plain" / "tnt_scores.json"))
    b = json.load(open(tmp_path / "sampled" / "tnt_scores.json"))
    print(f"coarse sphere, tau 0.04: recall by vertices {a['recall']:.2f}, by {b['sampled_points']} samples at spacing {spacing:.4f} "
          f"{b['recall']:.2f}; precision {a['precision']:.2f} / {b['precision']:.2f}")
    assert b["recall"] > a["recall"]
    assert b["sample_spacing"] == spacing and b["sample_seed"] == 4
    assert b["sampled_points"] == len(M.sample_ref(v, f, 1.0 / spacing ** 2, seed=4)[0])
    assert set(b) - set(a) == {"sample_spacing", "sample_seed", "sampled_points"} and not set(a) - set(b)
    cloud = _run("eval_tnt.py", base + ["--ply_path", str(tmp_path / "cloud.ply"), "--results_path", str(tmp_path / "cloud"),
                                        "--sample_spacing", str(spacing)])
    assert cloud.returncode != 0 and "Traceback" not in cloud.stdout
    assert "eval_tnt.py: " in cloud.stdout and "cloud.ply: --sample_spacing needs a mesh" in cloud.stdout


def test_eval_dtu_scores_the_sampled_surface(tmp_path):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import fusion, meshops, pointcloud as PC, tsdf
    s = dtu_ref.synthetic_scan(11, n_stl=3000, n_data=5000)
    data, ply = tmp_path / "data", tmp_path / "ply"
    os.makedirs(data / "ObsMask")
    gx, gy = np.meshgrid(np.arange(0.0, 100.1, 5.0), np.arange(0.0, 100.1, 5.0), indexing="ij")
    mv = np.stack([gx.ravel(), gy.ravel(), dtu_ref.height(gx.ravel(), gy.ravel())], 1).astype(np.float32)
    idx = np.arange(21 * 21).reshape(21, 21)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    mf = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)
    fusion.write_ply(str(ply / "scan1" / "fused.ply"), s["data"], np.full((len(s["data"]), 3), 128, np.uint8))
    tsdf.write_ply_mesh(str(ply / "scan1" / "mesh.ply"), mv, mf)
    fusion.write_ply(str(data / "Points" / "stl" / "stl001_total.ply"), s["stl"], np.zeros((len(s["stl"]), 3), np.uint8))
    np.savez(str(data / "ObsMask" / "ObsMask1_10.npz"), ObsMask=s["ObsMask"], BB=s["BB"], Res=s["Res"])
    np.savez(str(data / "ObsMask" / "Plane1.npz"), P=s["P"])
    argv = ["--data_path", str(data), "--ply_path", str(ply), "--results_path", str(tmp_path / "out"), "--scans", "1"]
    r = _run("eval_dtu.py", argv)
    assert r.returncode == 0, r.stdout
    js = json.load(open(tmp_path / "out" / "dtu_scores.json"))
    direct = PC.dtu_score_scan(_up(s["data"]), _up(s["stl"]), s["ObsMask"], s["BB"], s["Res"], s["P"])
    assert set(js) == {"dst", "max_dist", "seed", "abi", "method", "light", "scans", "scans_scored", "total"}  # a plain run: today's keys
    assert set(js["scans"]["1"]) == set(direct) | {"ply"} and js["scans"]["1"]["ply"].endswith("fused.ply")
    # the mesh, sampled; into the SAME results folder: the plain scores are not taken for it
    r2 = _run("eval_dtu.py", argv + ["--ply_name", "mesh.ply", "--sample_spacing", "0.8", "--sample_seed", "6"])
    assert r2.returncode == 0 and "already in" not in r2.stdout, r2.stdout
    js2 = json.load(open(tmp_path / "out" / "dtu_scores.json"))
    pts = meshops.sample_surface(_up(mv), _up(mf), spacing=0.8, seed=6)[0]
    want = PC.dtu_score_scan(pts, _up(s["stl"]), s["ObsMask"], s["BB"], s["Res"], s["P"])
    got = js2["scans"]["1"]
    print(f"eval_dtu.py on mesh.ply: {got['sampled_points']} samples, acc {got['acc_mean']:.4f}, comp {got['comp_mean']:.4f}; "
          f"fused.ply: acc {js['scans']['1']['acc_mean']:.4f}, comp {js['scans']['1']['comp_mean']:.4f}")
    assert js2["sample_spacing"] == 0.8 and js2["sample_seed"] == 6 and got["ply"].endswith("mesh.ply")
    assert got["sampled_points"] == pts.shape[0] == len(M.sample_ref(mv, mf, 1.0 / 0.8 ** 2, seed=6)[0])
    for k, val in want.items():
        if k not in ("seconds", "reduce_rounds"):
            assert got[k] == val, k
    # and back: a plain run does not take the sampled scores for its own
    r3 = _run("eval_dtu.py", argv)
    assert r3.returncode == 0 and "already in" not in r3.stdout, r3.stdout
    assert set(json.load(open(tmp_path / "out" / "dtu_scores.json"))) == set(js)
