"""GPU checks of mesh simplification by vertex clustering: pmn_mesh_remap_faces, pmn_mesh_cluster_place and
meshops.simplify_clustering against the numpy restatement tests/simplify_ref.py, then through simplify_mesh.py and mesh.py --simplify.

Gates.  Faces, vertex_map, counts and colour bytes follow integer definitions: array_equal.  A position is held to
|out - ref_longdouble| <= ulp32(ref) / 2 + 4 * max |ref_float64 - ref_longdouble| -- the one rounding to float32 plus four times what
the float64 arithmetic itself loses against the 64-bit-mantissa restatement, measured per case and printed; no coordinate is exempt.
A normal is the float32 rounding of a float64 quotient whose error (a few 2^-53) can only move that rounding across a tie: one ulp32."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshops_ref as M
import simplify_ref as S
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEV = "cuda:0"
_REFS = {}


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _simplify(*args, **kw):
    from patchmatchnet_amd import _lib, meshops
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    assert S.LONG_RUN == _lib.MESH_PLACE_LONG_RUN
    return meshops.simplify_clustering(*args, **kw)


def _attributes(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 3), dtype=np.uint8), rng.standard_normal((n, 3)).astype(np.float32)


def _refs(name, v, f, cell, col=None, nrm=None, origin=None):
    """The float64 and the longdouble restatement of one case, computed once."""
    if name not in _REFS:
        _REFS[name] = tuple(S.simplify(v, f, cell, col, nrm, origin=origin, dtype=t) for t in (np.float64, np.longdouble))
    return _REFS[name]


def _check(name, v, f, cell, col=None, nrm=None, origin=None):
    r64, rld = _refs(name, v, f, cell, col, nrm, origin)
    gv, gf, gc, gn, gm = _simplify(_up(v), _up(f), cell, colors=_up(col), normals=_up(nrm), origin=origin, return_map=True)
    assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and gm.dtype == torch.int32
    gv, gf, gm = gv.cpu().numpy(), gf.cpu().numpy(), gm.cpu().numpy()
    assert gv.shape == r64["vertices"].shape and gf.shape == r64["faces"].shape and gm.shape == (len(v),)
    assert np.array_equal(gf, r64["faces"]) and np.array_equal(gf, rld["faces"]), name
    assert np.array_equal(gm, r64["vertex_map"]), name
    ref = rld["exact"]
    loss = float(np.abs(r64["exact"].astype(np.longdouble) - ref).max()) if len(ref) else 0.0
    err = np.abs(gv.astype(np.longdouble) - ref)
    bound = np.spacing(np.abs(ref).astype(np.float32)).astype(np.longdouble) / 2 + 4 * loss
    worst = float((err / bound).max()) if len(ref) else 0.0
    print(f"{name}: {len(v)} vertices, {len(f)} faces -> {len(gv)} vertices, {len(gf)} faces; max |float64 - longdouble| {loss:.3e}, "
          f"largest error / bound {worst:.4f}, bit-equal to the float64 restatement {gv.tobytes() == r64['vertices'].tobytes()}")
    assert (err <= bound).all(), name
    if col is None:
        assert gc is None
    else:
        assert gc.dtype == torch.uint8 and np.array_equal(gc.cpu().numpy(), r64["colors"]), name
    if nrm is None:
        assert gn is None
    else:
        got, want = gn.cpu().numpy(), r64["normals"]
        assert gn.dtype == torch.float32 and (np.abs(got - want) <= np.spacing(np.abs(want))).all(), name
    return gv, gf, gm


@pytest.fixture(scope="module")
def icosphere():
    return M.icosphere(3)  # 642 vertices, 1280 faces


@pytest.mark.parametrize("cell", [0.11, 0.35, 4.0])
def test_icosphere_matches_the_reference(icosphere, cell):
    v, f = icosphere
    col, nrm = _attributes(len(v), 1)
    gv, gf, gm = _check(f"icosphere, cell {cell}", v, f, cell, col, nrm)
    if cell == 4.0:  # one cell swallows the sphere: nothing is left, and that is no error
        assert gv.shape == (0, 3) and gf.shape == (0, 3) and (gm == -1).all()
        out = _simplify(_up(v), _up(f), cell, colors=_up(col))
        assert len(out) == 4 and out[2].shape == (0, 3) and out[2].dtype == torch.uint8 and out[3] is None
    else:
        assert 0 < len(gf) < len(f)
        d = np.linalg.norm(v.astype(np.float64) - gv[np.maximum(gm, 0)].astype(np.float64), axis=1)[gm >= 0]
        assert d.max() <= math.sqrt(3.0) * cell


def test_icosphere_far_from_the_origin(icosphere):
    """Translated by 10^4 the coordinates carry 2^-10 of rounding; relative to the cell centres the planes keep their offsets."""
    v, f = icosphere
    far = (v.astype(np.float64) + 1.0e4).astype(np.float32)
    _check("icosphere at 1e4, cell 0.35", far, f, 0.35)


@pytest.mark.parametrize("n", [S.LONG_RUN, S.LONG_RUN + 1, 300])
def test_fan_across_the_long_run_constant(n):
    v, f = S.fan(n)
    cluster = S.clusters(v, 0.5)[0]
    runs = np.bincount(cluster[f].reshape(-1))
    assert runs.max() == n and runs[cluster[0]] == n  # the hub is alone in its cell: its run holds one corner of every face
    assert (runs > S.LONG_RUN).any() == (n > S.LONG_RUN) and (runs <= S.LONG_RUN).any()
    _check(f"fan of {n}", v, f, 0.5)


def test_clamp_and_cube_corners():
    v, f, cell, origin = S.two_sheets()
    _check("two sheets", v, f, cell, origin=origin)
    v, f = S.cube(8)
    gv, gf, gm = _check("cube", v, f, 0.3)
    mv = _simplify(_up(v), _up(f), 0.3, placement="mean")[0].cpu().numpy()
    for corner in np.ndindex(2, 2, 2):  # the inequality tests/test_simplify_ref.py shows on the reference
        k = gm[int(np.flatnonzero((v == np.float32(corner)).all(1))[0])]
        assert np.linalg.norm(gv[k].astype(np.float64) - corner) < np.linalg.norm(mv[k].astype(np.float64) - corner)


def test_degenerate_duplicate_and_opposite_faces(icosphere):
    v, f = icosphere
    v2 = np.concatenate([v, [[0.0, 0.0, 0.0]]]).astype(np.float32)  # a vertex no face names
    f2 = np.concatenate([f[:40], f, f[100:130, ::-1], [[3, 3, 9], [5, 5, 5], [7, 8, 7]]]).astype(np.int32)
    zero = np.array([[10, 10, 11]], np.int32)  # a repeated index; below, a zero-area face over three distinct, collinear vertices
    v3 = np.concatenate([v2, [[2.0, 0.0, 0.0], [2.5, 0.0, 0.0], [3.0, 0.0, 0.0]]]).astype(np.float32)
    f3 = np.concatenate([f2, zero, [[643, 644, 645]]]).astype(np.int32)
    col, nrm = _attributes(len(v3), 2)
    gv, gf, gm = _check("duplicates, opposite pairs, degenerate faces", v3, f3, 0.35, col, nrm)
    assert gm[642] == -1
    plain = S.face_set(_refs("icosphere, cell 0.35 plain", v, f, 0.35)[0]["faces"])
    assert len(S.face_set(gf)) == len(gf) and len(gf) > len(plain)  # the opposite orientations stayed, the duplicates did not


def test_face_order_and_repetition_do_not_change_a_bit(icosphere):
    v, f = icosphere
    col, nrm = _attributes(len(v), 3)
    dv, dc, dn = _up(v), _up(col), _up(nrm)
    base = _simplify(dv, _up(f), 0.35, colors=dc, normals=dn, return_map=True)
    again = _simplify(dv, _up(f), 0.35, colors=dc, normals=dn, return_map=True)
    assert all(torch.equal(a, b) for a, b in zip(base, again))
    for g in (np.ascontiguousarray(f[::-1]), M.permute_faces(f, 5)):
        out = _simplify(dv, _up(g), 0.35, colors=dc, normals=dn, return_map=True)
        assert torch.equal(out[0], base[0]) and torch.equal(out[2], base[2]) and torch.equal(out[3], base[3])
        assert torch.equal(out[4], base[4])
        assert S.face_set(out[1].cpu().numpy()) == S.face_set(base[1].cpu().numpy())


def test_mean_placement_is_the_voxel_mean(icosphere):
    from patchmatchnet_amd import registration
    v, f = icosphere
    r64 = _refs("icosphere, cell 0.35 plain", v, f, 0.35)[0]
    out = _simplify(_up(v), _up(f), 0.35, placement="mean", return_map=True)
    means = registration.voxel_downsample(_up(v), 0.35)
    assert torch.equal(out[0], means[torch.from_numpy(r64["kept_clusters"]).to(DEV)])
    assert np.array_equal(out[1].cpu().numpy(), r64["faces"]) and np.array_equal(out[4].cpu().numpy(), r64["vertex_map"])


def test_refusals(icosphere):
    from patchmatchnet_amd import PmnError
    v, f = icosphere
    bad = f.copy()
    bad[10, 1], bad[700, 0], bad[-1, 2] = -1, len(v), 2 ** 31 - 1  # skipped and counted, never dereferenced
    for placement in ("quadric", "mean"):
        with pytest.raises(PmnError, match=r"\b3 faces"):
            _simplify(_up(v), _up(bad), 0.35, placement=placement)
    nan = v.copy()
    nan[17, 1] = np.nan
    with pytest.raises(PmnError, match="1 vertices have non-finite"):
        _simplify(_up(nan), _up(f), 0.35)
    with pytest.raises(PmnError, match="63-bit key"):
        _simplify(_up(v), _up(f), 1e-10)
    with pytest.raises(PmnError, match="origin"):
        _simplify(_up(v), _up(f), 0.35, origin=(0.0, 0.0, 0.0))
    with pytest.raises(PmnError):
        _simplify(_up(v), torch.from_numpy(f), 0.35)
    # no faces, no vertices
    out = _simplify(_up(v), _up(np.zeros((0, 3), np.int32)), 0.35, return_map=True)
    assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and (out[4] == -1).all()
    out = _simplify(_up(np.zeros((0, 3), np.float32)), _up(np.zeros((0, 3), np.int32)), 0.35)
    assert out[0].shape == (0, 3) and out[1].shape == (0, 3)
    # the good faces afterwards
    _check("icosphere after the refusals", v, f, 0.35)


# ---- command lines ---------------------------------------------------------------------------------------------------------------

def _run(script, args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, script)] + args, cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)  # a fresh process


def test_simplify_mesh_py(tmp_path):
    """An icosphere of 5120 faces with a floater through simplify_mesh.py: the output reads back, has fewer faces, and the two surfaces
    stay within sqrt(3) * cell of each other's vertices (meshops.point_mesh_distance, as compare_mesh.py measures)."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import meshops, ply
    ball = M.icosphere(4)
    v, f = M.join(ball, (M.tetrahedra(1)[0] * np.float32(0.05) + np.float32([3, 0, 0]), M.tetrahedra(1)[1]))
    col, nrm = _attributes(len(v), 4)
    src, dst, rep = str(tmp_path / "in.ply"), str(tmp_path / "out" / "small.ply"), str(tmp_path / "report.json")
    ply.write_ply_mesh(src, v, f, col, nrm)
    cell = 0.2
    p = _run("simplify_mesh.py", ["--input", src, "--output", dst, "--cell", str(cell), "--keep_components", "1", "--report", rep])
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    ov, of, oc, on = ply.read_ply_mesh(dst)
    js = json.load(open(rep))
    assert js["faces_in"] == len(f) and js["faces_out"] == len(of) and js["components"] == 2 and js["components_kept"] == 1
    assert 0 < len(of) < len(ball[1]) / 4 and oc is not None and on is not None
    kept = meshops.remove_components(_up(v), _up(f), _up(col), _up(nrm), keep_largest=1)
    want = meshops.simplify_clustering(*kept[:2], cell, colors=kept[2], normals=kept[3])
    assert ov.tobytes() == want[0].cpu().numpy().tobytes() and np.array_equal(of, want[1].cpu().numpy())
    assert np.array_equal(oc, want[2].cpu().numpy()) and on.tobytes() == want[3].cpu().numpy().tobytes()
    a = float(meshops.point_mesh_distance(kept[0], meshops.build_face_grid(_up(ov), _up(of)), 10.0).max())
    b = float(meshops.point_mesh_distance(_up(ov), meshops.build_face_grid(kept[0], kept[1]), 10.0).max())
    print(f"cell {cell}: {len(f)} -> {len(of)} faces; largest distance input vertices -> output {a:.4f}, output vertices -> input {b:.4f}, "
          f"bound {math.sqrt(3.0) * cell:.4f}")
    assert max(a, b) < math.sqrt(3.0) * cell
    # --target_faces: at most 12 calls, the cell and the faces it reached are reported
    t = _run("simplify_mesh.py", ["--input", src, "--output", str(tmp_path / "t.ply"), "--target_faces", "500", "--report", rep])
    print(t.stdout)
    assert t.returncode == 0, t.stdout
    js = json.load(open(rep))
    assert 1 <= len(js["calls"]) <= 12 and {"cell": js["cell"], "faces": js["faces_out"]} in js["calls"]
    assert len(ply.read_ply_mesh(str(tmp_path / "t.ply"))[1]) == js["faces_out"] < len(f)
    over = [c["faces"] for c in js["calls"] if c["faces"] <= 500]
    assert js["faces_out"] == (max(over) if over else min(c["faces"] for c in js["calls"]))
    # nothing to do, and a cloud: refused without a traceback
    for args in (["--input", src, "--output", dst], ["--input", src, "--output", dst, "--cell", "0"]):
        bad = _run("simplify_mesh.py", args)
        assert bad.returncode == 2 and "Traceback" not in bad.stdout and "simplify_mesh.py: " in bad.stdout


def test_mesh_py_simplify(tmp_path):
    """mesh.py on the rendered 5-view scan of tests/synth.py: --simplify 0 writes the bytes and the report line of a run without the
    flag; --simplify 2 writes what simplify_clustering makes of that mesh at a cell of two voxels, and says so."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import data_io, meshops, ply
    from PIL import Image
    n, H, W = 5, 96, 128
    src = synth.write_scene_scan(str(tmp_path), "scene", n, H, W, n_src=2)
    _, intr, extr, depths = synth.render_scene(n, H, W, cameras=synth.arc_cameras(n, H, W), all_depths=True)
    res = str(tmp_path / "results")
    os.makedirs(os.path.join(res, "depth_est"))
    os.makedirs(os.path.join(res, "mask"))
    for k in range(n):
        data_io.save_pfm(os.path.join(res, "depth_est/{:0>8}.pfm".format(k)), depths[k].numpy().astype(np.float32))
        Image.fromarray(np.full((H, W), 255, np.uint8)).save(os.path.join(res, "mask/{:0>8}_final.png".format(k)))
    base = ["--input_folder", src, "--results_folder", res, "--voxel", "5.0", "--trunc", "20.0", "--bounds"] + \
        [str(b) for b in (-120.0, -90.0, 580.0, 120.0, 90.0, 720.0)]
    outs = {}
    for name, extra in (("plain", []), ("off", ["--simplify", "0"]), ("two", ["--simplify", "2"])):
        p = _run("mesh.py", base + ["--output_folder", str(tmp_path / name)] + extra)
        assert p.returncode == 0, p.stdout
        outs[name] = (p.stdout, os.path.join(str(tmp_path / name), "mesh.ply"))
    strip = lambda text, name: [ln.split("; load")[0] for ln in text.replace(str(tmp_path / name), "OUT").splitlines()]
    assert open(outs["plain"][1], "rb").read() == open(outs["off"][1], "rb").read()
    assert strip(outs["plain"][0], "plain") == strip(outs["off"][0], "off") and "simplified" not in outs["off"][0]
    v, f, c, nrm = ply.read_ply_mesh(outs["plain"][1])
    want = meshops.simplify_clustering(_up(v), _up(f), 10.0, colors=_up(c), normals=_up(nrm))
    gv, gf, gc, gn = ply.read_ply_mesh(outs["two"][1])
    print(outs["two"][0])
    assert gv.tobytes() == want[0].cpu().numpy().tobytes() and np.array_equal(gf, want[1].cpu().numpy())
    assert np.array_equal(gc, want[2].cpu().numpy()) and gn.tobytes() == want[3].cpu().numpy().tobytes()
    assert 0 < len(gf) < len(f) / 2
    assert "simplified at cell 10 (2 voxels): {} vertices, {} faces -> {} vertices, {} faces".format(len(v), len(f), len(gv), len(gf)) \
        in outs["two"][0]
    bad = _run("mesh.py", base + ["--output_folder", str(tmp_path / "bad"), "--simplify", "0.5"])
    assert bad.returncode != 0 and "--simplify must be 0" in bad.stdout
