"""GPU checks of mesh smoothing and vertex normals: meshops.vertex_adjacency, pmn_mesh_smooth and
pmn_mesh_vertex_normals against the numpy restatement tests/smooth_ref.py, then through mesh.py --smooth and smooth_mesh.py.

Gates.  The adjacency follows an integer definition: array_equal.  A position after ONE step from identical inputs is held to
|out - ref_longdouble| <= ulp32(ref) / 2 + 4 * max |ref_float64 - ref_longdouble| -- the one rounding to float32 plus four times what
the float64 arithmetic itself loses against the 64-bit-mantissa restatement, measured per case and printed; no coordinate is exempt.
Several steps are held to single steps bit for bit.  A normal is the float32 rounding of a float64 quotient whose error (a few 2^-53)
can only move that rounding across a tie: one ulp32."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshops_ref as M
import simplify_ref as S
import smooth_ref as R
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEV = "cuda:0"
LAM, MU = 0.5, -0.53
_ADJ = {}


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _meshops():
    from patchmatchnet_amd import _lib, meshops
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    assert R.LONG_ROW == _lib.MESH_SMOOTH_LONG_ROW
    return meshops


def _adjacency(name, f, nv):
    if name not in _ADJ:
        _ADJ[name] = R.adjacency(f, nv)
    return _ADJ[name]


def _ico_noisy():
    v, f = M.icosphere(3)  # 642 vertices, 1280 faces
    return R.noisy_sphere(v), f


def _fan(n):
    v, f = S.fan(n)
    return v, f


def _meshes():
    v, f = _ico_noisy()
    return {"icosphere(2)": M.icosphere(2), "grid 5 x 4": R.plane_grid(5, 4), "odd": R.odd_mesh(), "noisy icosphere(3)": (v, f)}


# ---- integers --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["icosphere(2)", "grid 5 x 4", "odd"])
def test_adjacency_matches_the_reference(name):
    mo = _meshops()
    v, f = _meshes()[name]
    starts, nbrs, boundary = _adjacency(name, f, len(v))
    for g in (f, M.permute_faces(f, 7), np.ascontiguousarray(f[::-1])):
        adj = mo.vertex_adjacency(_up(g), len(v))
        assert adj.starts.dtype == torch.int64 and adj.neighbours.dtype == torch.int32 and adj.boundary.dtype == torch.bool
        assert np.array_equal(adj.starts.cpu().numpy(), starts), name
        assert np.array_equal(adj.neighbours.cpu().numpy(), nbrs), name
        assert np.array_equal(adj.boundary.cpu().numpy(), boundary), name
    empty = mo.vertex_adjacency(_up(np.zeros((0, 3), np.int32)), 3)
    assert empty.starts.tolist() == [0, 0, 0, 0] and empty.neighbours.shape == (0,) and not empty.boundary.any()


# ---- one step from identical inputs ------------------------------------------------------------------------------------------------

def _gate(name, got, r64, rld):
    loss = float(np.abs(r64.astype(np.longdouble) - rld).max())
    err = np.abs(got.astype(np.longdouble) - rld)
    bound = np.spacing(np.abs(rld).astype(np.float32)).astype(np.longdouble) / 2 + 4 * loss
    worst = float((err / bound).max())
    print(f"{name}: {len(got)} vertices; max |float64 - longdouble| {loss:.3e}, largest error / bound {worst:.4f}, bit-equal to the "
          f"float64 restatement {got.tobytes() == r64.astype(np.float32).tobytes()}")
    assert (err <= bound).all(), name


def _one_step(name, v, f, factor, boundary="fixed", pinned=None):
    mo = _meshops()
    starts, nbrs, rim = _adjacency(name, f, len(v))
    pin = rim.copy() if boundary == "fixed" else np.zeros(len(v), bool)
    if pinned is not None:
        pin |= pinned
    r64, rld = (R.step(v, starts, nbrs, factor, pin, t) for t in (np.float64, np.longdouble))
    dv = _up(v)
    got = mo.smooth_steps(dv, _up(f), [factor], boundary=boundary, pinned=_up(pinned))
    assert got.dtype == torch.float32 and got.shape == dv.shape and got.data_ptr() != dv.data_ptr()
    assert dv.cpu().numpy().tobytes() == v.tobytes()  # the caller's vertices are not written
    got = got.cpu().numpy()
    _gate(f"{name}, factor {factor}, boundary {boundary}", got, r64, rld)
    still = pin | (np.diff(starts) == 0)
    assert got[still].tobytes() == v[still].tobytes()  # pinned or without neighbours: the input bit for bit
    return got


@pytest.mark.parametrize("factor", [LAM, MU])
def test_icosphere_step(factor):
    v, f = _ico_noisy()
    got = _one_step("noisy icosphere(3)", v, f, factor)
    assert (got != v).any(1).all()  # closed: every vertex moves
    far = (v.astype(np.float64) + 1.0e4).astype(np.float32)
    _one_step("noisy icosphere(3) at 1e4", far, f, factor)


@pytest.mark.parametrize("n", [255, 256, 257, 1000])
@pytest.mark.parametrize("factor", [LAM, MU])
def test_fan_rows_across_the_long_row_constant(n, factor):
    """The hub's row has n entries: the lane path, its edge, and the wave path with a ragged tail (257 = 4 * 64 + 1, 1000 = 15 * 64 + 40)."""
    v, f = _fan(n)
    starts, _, rim = _adjacency(f"fan of {n}", f, len(v))
    assert np.diff(starts)[0] == n == np.diff(starts).max() and (np.diff(starts)[1:] == 3).all() and rim[1:].all() and not rim[0]
    got = _one_step(f"fan of {n}", v, f, factor, boundary="free")
    assert (got[0] != v[0]).any()
    _one_step(f"fan of {n}", v, f, factor, boundary="fixed")


@pytest.mark.parametrize("factor", [LAM, MU])
def test_open_grid_pinned_mask_and_odd_meshes(factor):
    v, f = R.plane_grid(5, 4)
    v = (v + np.random.default_rng(3).standard_normal(v.shape) * 0.02).astype(np.float32)
    fixed = _one_step("grid 5 x 4", v, f, factor, boundary="fixed")
    free = _one_step("grid 5 x 4", v, f, factor, boundary="free")
    rim = R.grid_rim(5, 4)
    assert fixed[rim].tobytes() == v[rim].tobytes() and (free[rim] != v[rim]).any(1).all()
    assert fixed[~rim].tobytes() == free[~rim].tobytes()  # pinned vertices still feed their neighbours
    iv, jf = _ico_noisy()
    pinned = np.random.default_rng(4).random(len(iv)) < 0.3
    got = _one_step("noisy icosphere(3)", iv, jf, factor, pinned=pinned)
    assert got[pinned].tobytes() == iv[pinned].tobytes() and (got[~pinned] != iv[~pinned]).any(1).all()
    ov, of = R.odd_mesh()
    _one_step("odd", ov, of, factor, boundary="fixed")
    got = _one_step("odd", ov, of, factor, boundary="free")
    assert got[5].tobytes() == ov[5].tobytes() and (got[4] != ov[4]).any()
    one = np.array([[1.0, -2.0, 3.5]], np.float32)
    for faces in (np.zeros((0, 3), np.int32), np.zeros((1, 3), np.int32)):  # no faces: no launch; the face (0, 0, 0): no neighbours
        got = _meshops().smooth_steps(_up(one), _up(faces), [factor])
        assert got.cpu().numpy().tobytes() == one.tobytes()
    none = _meshops().smooth_taubin(_up(np.zeros((0, 3), np.float32)), _up(np.zeros((0, 3), np.int32)))
    assert none.shape == (0, 3) and none.dtype == torch.float32


# ---- several steps ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 5])
def test_taubin_is_its_single_steps(k):
    mo = _meshops()
    v, f = _ico_noisy()
    dv, df = _up(v), _up(f)
    adj = mo.vertex_adjacency(df, len(v))
    whole = mo.smooth_taubin(dv, df, iterations=k)
    assert torch.equal(mo.smooth_taubin(dv, df, iterations=k, adjacency=adj), whole)
    cur = dv
    for factor in [LAM, MU] * k:
        cur = mo.smooth_steps(cur, df, [factor], adjacency=adj)
    assert torch.equal(cur, whole)  # 2 k steps: both parities of the ping-pong end in the output
    lap = mo.smooth_laplacian(dv, df, iterations=2 * k - 1, lam=LAM)  # an odd number of steps
    cur = dv
    for _ in range(2 * k - 1):
        cur = mo.smooth_laplacian(cur, df, iterations=1, lam=LAM)
    assert torch.equal(cur, lap)
    assert dv.cpu().numpy().tobytes() == v.tobytes()
    if k == 1:
        zero = mo.smooth_taubin(dv, df, iterations=0)
        assert zero.data_ptr() != dv.data_ptr() and zero.cpu().numpy().tobytes() == v.tobytes()
        assert mo.smooth_laplacian(dv, df, iterations=0).cpu().numpy().tobytes() == v.tobytes()


# ---- order independence ----------------------------------------------------------------------------------------------------------

def test_face_order_changes_no_bit_and_vertex_labels_stay_in_the_gate():
    mo = _meshops()
    v, f = _ico_noisy()
    base = mo.smooth_taubin(_up(v), _up(f), iterations=3)
    for g in (np.ascontiguousarray(f[::-1]), M.permute_faces(f, 5), np.concatenate([f, f[:50]])):
        assert torch.equal(mo.smooth_taubin(_up(v), _up(g), iterations=3), base)
    starts, nbrs, rim = _adjacency("noisy icosphere(3)", f, len(v))
    v2, f2, new_of_old = M.relabel_vertices(v, f, 6)
    for factor in (LAM, MU):
        r64, rld = (R.step(v, starts, nbrs, factor, rim, t) for t in (np.float64, np.longdouble))
        got = mo.smooth_steps(_up(v2), _up(f2), [factor]).cpu().numpy()[new_of_old]
        _gate(f"relabelled icosphere, factor {factor}", got, r64, rld)


# ---- what the filter is for --------------------------------------------------------------------------------------------------------

def test_taubin_removes_noise_and_keeps_the_radius():
    mo = _meshops()
    v, f = _ico_noisy()
    rms0, mean0 = R.radius_stats(v)
    rms1, mean1 = R.radius_stats(mo.smooth_taubin(_up(v), _up(f), iterations=10).cpu().numpy())
    rms2, mean2 = R.radius_stats(mo.smooth_laplacian(_up(v), _up(f), iterations=10, lam=0.5).cpu().numpy())
    print(f"radius RMS {rms0:.4f} -> {rms1:.4f} (Taubin, mean radius {mean1:.4f}); Laplacian: RMS {rms2:.4f}, mean radius {mean2:.4f}")
    assert rms1 <= rms0 / 2 and abs(mean1 - 1.0) <= 0.01
    assert mean2 < 0.96


# ---- normals ---------------------------------------------------------------------------------------------------------------------

def _check_normals(name, v, f):
    mo = _meshops()
    want = R.normals(v, f).astype(np.float32)
    got = mo.vertex_normals(_up(v), _up(f))
    assert got.dtype == torch.float32 and got.shape == (len(v), 3)
    g = got.cpu().numpy()
    worst = float((np.abs(g - want) / np.spacing(np.abs(want))).max())
    print(f"{name}: {len(v)} normals, largest |got - float64 reference| {worst:.2f} ulp32, bit-equal {g.tobytes() == want.tobytes()}")
    assert (np.abs(g - want) <= np.spacing(np.abs(want))).all(), name
    length = np.linalg.norm(g.astype(np.float64), axis=1)
    zero = (g == 0).all(1)
    assert np.array_equal(zero, (want == 0).all(1)) and (np.abs(length[~zero] - 1.0) <= 3 * 2.0 ** -24).all(), name
    flipped = mo.vertex_normals(_up(v), _up(f), flip=True).cpu().numpy()
    assert np.array_equal(flipped, -g), name
    for h in (np.ascontiguousarray(f[::-1]), M.permute_faces(f, 8)):
        assert torch.equal(mo.vertex_normals(_up(v), _up(h)), got), name
    return g


def test_vertex_normals_match_the_reference():
    v, f = _ico_noisy()
    g = _check_normals("noisy icosphere(3)", v, f)
    assert (np.einsum("ij,ij->i", g, v) > 0.9).all()  # outward winding, outward normals
    for n in (256, 257, 1000):  # the hub is a corner of every face: corner runs on both sides of the constant
        fv, ff = _fan(n)
        g = _check_normals(f"fan of {n}", fv, ff)
        assert g[0, 2] > 0.9
    ov, of = R.odd_mesh()
    g = _check_normals("odd", ov, of)
    assert (g[4] == 0).all() and (g[5] == 0).all() and not (g[:4] == 0).all(1).any()


def test_mesher_winding_against_its_normals():
    """A sphere of radius 10.2 voxels meshed by pmn_mt_emit: which way the faces wind relative to the TSDF-gradient normals is
    measured here, and mesh.MESHER_WINDING_FLIP is what makes the recomputed normals agree with them, before and after smoothing."""
    import mesh
    from patchmatchnet_amd import ops
    mo = _meshops()
    n = 32
    ax = torch.arange(n, dtype=torch.float32, device=DEV)
    k, j, i = torch.meshgrid(ax, ax, ax, indexing="ij")
    d = torch.sqrt((i - 15.3) ** 2 + (j - 16.1) ** 2 + (k - 15.7) ** 2) - 10.2
    t = torch.clamp(d / 3.0, -1, 1).contiguous()
    v, f, _, grad = ops.mt_extract(t, torch.ones_like(t), (0.0, 0.0, 0.0), 1.0, normals=True)
    own = grad.norm(dim=1) > 0
    assert int(own.sum()) > 1000
    raw = (mo.vertex_normals(v, f) * grad).sum(1)[own]
    agree = int((raw > 0).sum()) / int(own.sum())
    print(f"meshed sphere: {v.shape[0]} vertices, {f.shape[0]} faces; (B - A) x (C - A) agrees with the mesher's normal at "
          f"{100 * agree:.2f} % of the vertices that have one: MESHER_WINDING_FLIP = {mesh.MESHER_WINDING_FLIP}")
    assert agree in (0.0, 1.0) and mesh.MESHER_WINDING_FLIP == (agree == 0.0)
    smooth = mo.smooth_taubin(v, f, iterations=5)
    after = mo.vertex_normals(smooth, f, flip=mesh.MESHER_WINDING_FLIP)
    assert bool(((after * grad).sum(1)[own] > 0).all())


# ---- errors ----------------------------------------------------------------------------------------------------------------------

def test_refusals():
    from patchmatchnet_amd import PmnError
    mo = _meshops()
    v, f = _ico_noisy()
    dv, df = _up(v), _up(f)
    for call in (lambda: mo.smooth_taubin(torch.from_numpy(v), df), lambda: mo.smooth_taubin(dv, torch.from_numpy(f)),
                 lambda: mo.vertex_normals(torch.from_numpy(v), df), lambda: mo.vertex_adjacency(torch.from_numpy(f), len(v))):
        with pytest.raises(PmnError, match="ROCm GPU"):
            call()
    nan = v.copy()
    nan[17, 1] = np.nan
    with pytest.raises(PmnError, match="1 vertices have non-finite"):
        mo.smooth_taubin(_up(nan), df)
    with pytest.raises(PmnError, match="lam must be in"):
        mo.smooth_taubin(dv, df, lam=0.0)
    with pytest.raises(PmnError, match="mu must be finite and < -lam"):
        mo.smooth_taubin(dv, df, lam=0.5, mu=-0.5)
    bad = f.copy()
    bad[10, 1], bad[700, 0] = len(v), -1
    for call in (lambda: mo.smooth_taubin(dv, _up(bad)), lambda: mo.smooth_laplacian(dv, _up(bad)), lambda: mo.vertex_normals(dv, _up(bad)),
                 lambda: mo.vertex_adjacency(_up(bad), len(v)), lambda: mo.smooth_taubin(dv, _up(bad), iterations=0)):
        with pytest.raises(PmnError, match=r"\b2 faces have a vertex index outside 0\.\.641"):
            call()
    # an adjacency that is not this mesh's: refused by its shape, or its bad entries skipped, counted and reported
    with pytest.raises(PmnError, match="adjacency"):
        mo.smooth_taubin(dv, df, adjacency=mo.vertex_adjacency(df, len(v) + 1))
    adj = mo.vertex_adjacency(df, len(v))
    nb = adj.neighbours.clone()
    nb[5], nb[77], nb[-1] = len(v), -3, 2 ** 31 - 1
    with pytest.raises(PmnError, match="3 entries of the adjacency"):
        mo.smooth_taubin(dv, df, adjacency=adj._replace(neighbours=nb))
    # the good mesh afterwards
    assert torch.equal(mo.smooth_taubin(dv, df, iterations=1, adjacency=adj), mo.smooth_taubin(dv, df, iterations=1))


# ---- command lines ---------------------------------------------------------------------------------------------------------------

def _run(script, args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, script)] + args, cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)  # a fresh process


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """The rendered 5-view scan of tests/synth.py that tests/test_simplify_gpu.py uses, and mesh.py's output without any new flag and
    with --smooth 5: (folder, run, plain, five), each run (stdout, its lines without the times, the file)."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import data_io
    from PIL import Image
    tmp = tmp_path_factory.mktemp("smooth_scan")
    n, H, W = 5, 96, 128
    src = synth.write_scene_scan(str(tmp), "scene", n, H, W, n_src=2)
    _, intr, extr, depths = synth.render_scene(n, H, W, cameras=synth.arc_cameras(n, H, W), all_depths=True)
    res = str(tmp / "results")
    os.makedirs(os.path.join(res, "depth_est"))
    os.makedirs(os.path.join(res, "mask"))
    for k in range(n):
        data_io.save_pfm(os.path.join(res, "depth_est/{:0>8}.pfm".format(k)), depths[k].numpy().astype(np.float32))
        Image.fromarray(np.full((H, W), 255, np.uint8)).save(os.path.join(res, "mask/{:0>8}_final.png".format(k)))
    base = ["--input_folder", src, "--results_folder", res, "--voxel", "5.0", "--trunc", "20.0", "--bounds"] + \
        [str(b) for b in (-120.0, -90.0, 580.0, 120.0, 90.0, 720.0)]

    def run(name, extra):
        p = _run("mesh.py", base + ["--output_folder", str(tmp / name)] + extra)
        assert p.returncode == 0, p.stdout
        text = [ln.split("; load")[0] for ln in p.stdout.replace(str(tmp / name), "OUT").splitlines()]
        return p.stdout, text, os.path.join(str(tmp / name), "mesh.ply")

    return tmp, run, run("plain", []), run("five", ["--smooth", "5"])


def test_mesh_py_smooth(scan):
    from patchmatchnet_amd import meshops, ply
    tmp, run, (_, plain_text, plain), (out5, _, five) = scan
    out0, text0, off = run("off", ["--smooth", "0"])
    assert open(plain, "rb").read() == open(off, "rb").read() and text0 == plain_text and "smoothed" not in out0
    print(out5)
    v, f, c, nrm = ply.read_ply_mesh(plain)
    gv, gf, gc, gn = ply.read_ply_mesh(five)
    assert np.array_equal(gf, f) and np.array_equal(gc, c) and gv.shape == v.shape
    assert np.isfinite(gv).all() and (gv != v).any()
    length = np.linalg.norm(gn.astype(np.float64), axis=1)
    assert ((np.abs(length - 1.0) <= 3 * 2.0 ** -24) | (gn == 0).all(1)).all()
    want = meshops.smooth_taubin(_up(v), _up(f), iterations=5)
    assert gv.tobytes() == want.cpu().numpy().tobytes()
    adj = meshops.vertex_adjacency(_up(f), len(v))
    assert "smoothed by 5 Taubin iterations (lambda 0.5, mu -0.53, boundary fixed): {} vertices, {} on the boundary; displacement mean".format(
        len(v), int(adj.boundary.sum())) in out5
    rim = adj.boundary.cpu().numpy()
    assert gv[rim].tobytes() == v[rim].tobytes()


def test_mesh_py_smooth_then_simplify_and_no_normals(scan):
    """With --simplify the smoothing comes first: the quadrics see the smoothed mesh and its normals."""
    from patchmatchnet_amd import meshops, ply
    tmp, run, _, (_, _, five) = scan
    gv, gf, gc, gn = ply.read_ply_mesh(five)
    out52, _, both = run("both", ["--smooth", "5", "--simplify", "2"])
    sv, sf, sc, sn = ply.read_ply_mesh(both)
    want = meshops.simplify_clustering(_up(gv), _up(gf), 10.0, colors=_up(gc), normals=_up(gn))
    assert sv.tobytes() == want[0].cpu().numpy().tobytes() and np.array_equal(sf, want[1].cpu().numpy())
    assert np.array_equal(sc, want[2].cpu().numpy()) and sn.tobytes() == want[3].cpu().numpy().tobytes()
    assert out52.index("smoothed by 5") < out52.index("simplified at cell 10")
    # --no_normals: none are computed or written
    _, _, bare = run("bare", ["--smooth", "5", "--no_normals"])
    bv, bf, bc, bn = ply.read_ply_mesh(bare)
    assert bn is None and bv.tobytes() == gv.tobytes()


def test_smooth_mesh_py(scan):
    from patchmatchnet_amd import _lib, meshops, ply
    tmp, run, (_, _, plain), _ = scan
    v, f, c, nrm = ply.read_ply_mesh(plain)
    dst, rep = str(tmp / "tool" / "smooth.ply"), str(tmp / "tool" / "report.json")
    p = _run("smooth_mesh.py", ["--input", plain, "--output", dst, "--iterations", "4", "--report", rep])
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    gv, gf, gc, gn = ply.read_ply_mesh(dst)
    want = meshops.smooth_taubin(_up(v), _up(f), iterations=4)
    assert gv.tobytes() == want.cpu().numpy().tobytes() and np.array_equal(gf, f) and np.array_equal(gc, c)
    assert gn.tobytes() == meshops.vertex_normals(want, _up(f)).cpu().numpy().tobytes()
    js = json.load(open(rep))
    moved = np.linalg.norm(gv.astype(np.float64) - v.astype(np.float64), axis=1)
    assert js["abi"] == _lib.ABI_VERSION == 25 and js["method"] == "taubin" and js["iterations"] == 4
    assert (js["lambda"], js["mu"], js["boundary"], js["normals"]) == (0.5, -0.53, "fixed", "recompute")
    assert js["vertices"] == len(v) and js["faces"] == len(f)
    assert js["boundary_vertices"] == int(meshops.vertex_adjacency(_up(f), len(v)).boundary.sum()) > 0
    assert abs(js["displacement_mean"] - moved.mean()) <= 1e-9 and abs(js["displacement_max"] - moved.max()) <= 1e-9
    bad = _run("smooth_mesh.py", ["--input", plain, "--output", dst, "--lambda", "0"])
    assert bad.returncode == 2 and "Traceback" not in bad.stdout and "smooth_mesh.py: " in bad.stdout


def test_smooth_mesh_py_only_normals_and_laplacian(scan):
    """--iterations 0 --normals recompute: positions bit-equal, normals those of the faces; --method laplacian --normals keep."""
    from patchmatchnet_amd import meshops, ply
    tmp, run, (_, _, plain), _ = scan
    v, f, c, nrm = ply.read_ply_mesh(plain)
    dst, bare = str(tmp / "tool2" / "out.ply"), str(tmp / "tool2" / "bare.ply")
    ply.write_ply_mesh(bare, v, f, c, None)
    q = _run("smooth_mesh.py", ["--input", bare, "--output", dst, "--iterations", "0", "--normals", "recompute"])
    assert q.returncode == 0, q.stdout
    gv, gf, gc, gn = ply.read_ply_mesh(dst)
    assert gv.tobytes() == v.tobytes() and np.array_equal(gf, f) and np.array_equal(gc, c)
    assert gn is not None and gn.tobytes() == meshops.vertex_normals(_up(v), _up(f)).cpu().numpy().tobytes()
    q = _run("smooth_mesh.py", ["--input", plain, "--output", dst, "--method", "laplacian", "--iterations", "2", "--normals", "keep"])
    assert q.returncode == 0, q.stdout
    gv, gf, gc, gn = ply.read_ply_mesh(dst)
    assert gv.tobytes() == meshops.smooth_laplacian(_up(v), _up(f), iterations=2).cpu().numpy().tobytes() and gn.tobytes() == nrm.tobytes()
