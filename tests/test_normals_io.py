"""CPU checks of the surface-normal feature: the numpy oracle of the estimator (tests/normals_ref.py) against
analytic scenes, the oriented PLY and COLMAP normal-map file layouts, and the command lines / argument checks that need no GPU.  The
kernel itself is checked on the device in tests/test_normals_gpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import normals_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((64, 64), (250, 333))

# measured maxima (radians) of the angle between the float64 oracle's normal and the plane's, over r = 1, 2, 3 and both SIZES -- what
# rounding the rendered depth to float32 leaves of the plane (largest at r = 1: nine samples, shortest baseline)
PLANE_ANGLE = {"dtu_fronto": 0.0, "dtu_tilt_x": 4.593e-05, "dtu_tilt_xy": 4.679e-05, "small_fronto": 0.0, "small_tilt": 6.739e-05}


@pytest.mark.parametrize("name", sorted(NR.PLANES))
def test_oracle_recovers_analytic_planes(name):
    """Exact planes nu . X = d rendered in float64 through cameras with skew, fx != fy and an off-centre principal point (DTU-like f ~
    2900 at z 400-900; f ~ 200 at z ~ 2), rounded to float32.  Measured on the CPU before this assertion was written (max over r =
    1, 2, 3 and 64x64, 250x333; radians): dtu_fronto 0, dtu_tilt_x 4.593e-05, dtu_tilt_xy 4.679e-05, small_fronto 0, small_tilt
    6.739e-05 (fronto-parallel planes have constant depth: every difference is exactly 0 and so is the angle).  The oracle is
    deterministic; the bound is 2 x the measured maximum, the margin covering numpy build differences only."""
    worst = 0.0
    for H, W in SIZES:
        z, K, truth = NR.plane_scene(name, H, W)
        for r in (1, 2, 3):
            n = NR.depth_normals_ref(z, K, r)
            assert not (n == 0).all(0).any()  # a full plane has a normal everywhere, image corners included
            worst = max(worst, float(NR.angle(n, truth).max()))
    print(f"{name}: max angle to the plane normal {worst:.3e} rad")
    assert worst <= 2 * PLANE_ANGLE[name]


def _scenes(H, W):
    yield "sphere", NR.sphere_scene(H, W)[:2]
    yield "step", NR.step_scene(H, W)[:2]
    yield "random", NR.random_scene(H, W, seed=7)
    yield "plane", NR.plane_scene("small_tilt", H, W)[:2]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_oracle_normals_are_unit_or_zero_and_face_the_camera(dtype):
    for H, W in ((17, 19), (64, 64)):
        for name, (z, K) in _scenes(H, W):
            ray = NR.rays(K, H, W)
            for r in (1, 2, 3):
                n = NR.depth_normals_ref(z, K, r, fit_dtype=dtype).astype(np.float64)
                zero = (n == 0).all(0)
                length = np.sqrt((n * n).sum(0))
                assert np.abs(length[~zero] - 1).max(initial=0) <= 4 * np.finfo(dtype).eps, (name, r)
                assert ((n * ray).sum(0)[~zero] < 0).all(), (name, r)
                bad = ~(np.isfinite(z) & (z > 0))
                assert zero[bad].all(), (name, r)


def test_oracle_does_not_fit_across_a_depth_step():
    """Two planes more than rel_thres apart in depth: every pixel's normal is bit-equal to the normal obtained with the other side
    removed (set to 0), so nothing leaks across the edge."""
    H, W = 40, 52
    z, K, left = NR.step_scene(H, W)
    rel = np.abs(z[:, W // 2 - 1] - z[:, W // 2]) / np.minimum(z[:, W // 2 - 1], z[:, W // 2])
    assert rel.min() > 0.02
    for r in (1, 2, 3):
        both = NR.depth_normals_ref(z, K, r)
        only_l = NR.depth_normals_ref(np.where(left, z, 0).astype(np.float32), K, r)
        only_r = NR.depth_normals_ref(np.where(left, 0, z).astype(np.float32), K, r)
        np.testing.assert_array_equal(both[:, left], only_l[:, left])
        np.testing.assert_array_equal(both[:, ~left], only_r[:, ~left])
        assert not (both == 0).all(0).any()


@pytest.mark.parametrize("bad", [0.0, -3.0, np.nan, np.inf, -np.inf])
def test_oracle_invalid_depth_gives_zero_and_contaminates_nobody(bad):
    H, W = 24, 31
    z, K, _ = NR.plane_scene("small_tilt", H, W)
    holes = np.zeros((H, W), bool)
    holes[5, 7] = holes[12, 12] = holes[12, 13] = holes[0, 0] = holes[H - 1, W - 2] = True
    zb = z.copy()
    zb[holes] = bad
    z0 = z.copy()
    z0[holes] = 0
    for r in (1, 2, 3):
        n = NR.depth_normals_ref(zb, K, r)
        assert np.isfinite(n).all()
        assert (n[:, holes] == 0).all()
        assert not (n[:, ~holes] == 0).all(0).any()
        np.testing.assert_array_equal(n, NR.depth_normals_ref(z0, K, r))  # every invalid value acts like 0


def test_oracle_collinear_and_tiny_supports_give_zero():
    K = NR.camera("small", 9, 9)
    for r in (1, 2, 3):
        z = np.zeros((9, 9), np.float32)
        z[4, 4] = 2.0  # an isolated pixel
        assert (NR.depth_normals_ref(z, K, r) == 0).all()
        z = np.zeros((9, 9), np.float32)
        z[4, :] = 2.0 + 0.001 * np.arange(9)  # one valid row
        assert (NR.depth_normals_ref(z, K, r) == 0).all()
        assert (NR.depth_normals_ref(np.ascontiguousarray(z.T), K, r) == 0).all()  # one valid column
        z = np.zeros((9, 9), np.float32)
        z[np.arange(9), np.arange(9)] = 2.0  # a diagonal: collinear as well
        assert (NR.depth_normals_ref(z, K, r) == 0).all()
        z[4, 5] = 2.0  # one pixel off the line: its neighbours on the line now have three non-collinear supports
        n = NR.depth_normals_ref(z, K, r)
        assert not (n[:, 4, 4] == 0).all() and not (n[:, 4, 5] == 0).all()
        # 1x1, 1xW, Hx1 images: never three non-collinear pixels
        for shape in ((1, 1), (1, 13), (11, 1)):
            assert (NR.depth_normals_ref(np.full(shape, 2.0, np.float32), K, r) == 0).all()


def test_oracle_float32_switch_stays_next_to_float64():
    """The float32 evaluation is the yardstick of the GPU tolerance: it must decide the same zero set and sit within float32 rounding
    of the float64 one on a benign scene."""
    z, K, _ = NR.plane_scene("dtu_tilt_xy", 64, 64)
    for r in (1, 2, 3):
        n64, n32 = NR.depth_normals_ref(z, K, r), NR.depth_normals_ref(z, K, r, fit_dtype=np.float32)
        assert n32.dtype == np.float32 and n64.dtype == np.float64
        np.testing.assert_array_equal((n32 == 0).all(0), (n64 == 0).all(0))
        assert NR.angle(n32, n64).max() < 1e-5


# ---- files --------------------------------------------------------------------------------------------------------------------------

def _cloud(n=37, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3)).astype(np.float32) * 100
    c = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    nr = rng.standard_normal((n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
    return v, c, nr


def test_ply_with_normals_layout_and_unchanged_default(tmp_path):
    from patchmatchnet_amd import fusion, pointcloud
    v, c, nr = _cloud()
    # the defaults write today's bytes
    assert fusion.ply_header(37) == (b"ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\nproperty float y\n"
                                     b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert fusion.ply_header(37, normals=False) == fusion.ply_header(37)
    rec = fusion.ply_records(v, c)
    assert rec.dtype == fusion.PLY_VERTEX and rec.dtype.itemsize == 15
    assert rec.tobytes() == b"".join(v[i].tobytes() + c[i].tobytes() for i in range(37))
    assert fusion.ply_records(v, c, normals=None).tobytes() == rec.tobytes()
    fusion.write_ply(str(tmp_path / "plain.ply"), v, c)
    assert open(tmp_path / "plain.ply", "rb").read() == fusion.ply_header(37) + rec.tobytes()
    # with normals: 27-byte stride, x y z nx ny nz red green blue
    assert fusion.PLY_VERTEX_NORMALS.itemsize == 27
    assert fusion.PLY_VERTEX_NORMALS.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    hdr = fusion.ply_header(37, normals=True).decode()
    props = [ln.split()[1:] for ln in hdr.splitlines() if ln.startswith("property")]
    assert props == [["float", k] for k in ("x", "y", "z", "nx", "ny", "nz")] + [["uchar", k] for k in ("red", "green", "blue")]
    assert hdr.endswith("end_header\n") and "element vertex 37\n" in hdr
    recn = fusion.ply_records(v, c, nr)
    assert recn.dtype == fusion.PLY_VERTEX_NORMALS
    assert recn.tobytes() == b"".join(v[i].tobytes() + nr[i].tobytes() + c[i].tobytes() for i in range(37))
    fusion.write_ply(str(tmp_path / "oriented.ply"), v, c, normals=nr)
    assert open(tmp_path / "oriented.ply", "rb").read() == fusion.ply_header(37, True) + recn.tobytes()
    assert fusion.ply_records(v[:0], c[:0], nr[:0]).tobytes() == b""
    with pytest.raises(ValueError):
        fusion.ply_records(v, c, nr[:5])
    # eval_dtu's reader takes both files and returns the same positions
    a, b = pointcloud.read_ply_vertices(str(tmp_path / "plain.ply")), pointcloud.read_ply_vertices(str(tmp_path / "oriented.ply"))
    np.testing.assert_array_equal(a, v)
    np.testing.assert_array_equal(b, v)


def test_normal_map_bin_round_trip_and_byte_layout(tmp_path):
    from patchmatchnet_amd import data_io
    H, W = 5, 7
    m = np.random.default_rng(1).standard_normal((H, W, 3)).astype(np.float32)
    path = str(tmp_path / "n.geometric.bin")
    data_io.save_bin(path, m)
    raw = open(path, "rb").read()
    head = b"7&5&3&"
    assert raw.startswith(head) and len(raw) == len(head) + 4 * H * W * 3
    body = np.frombuffer(raw[len(head):], "<f4").reshape(3, H, W)  # x fastest, then y, then channel: the planar [3][H][W] map
    np.testing.assert_array_equal(body, m.transpose(2, 0, 1))
    np.testing.assert_array_equal(data_io.read_bin(path), m)


# ---- command lines and argument checks -------------------------------------------------------------------------------------------------

def _help(script):
    return subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, check=True, cwd=ROOT).stdout


def test_command_lines_list_the_flags():
    h = _help("eval.py")
    for flag in ("--normals", "--normals_radius", "--normals_depth_thres"):
        assert flag in h
    h = _help("colmap_output.py")
    for flag in ("--normal_maps", "--device", "--normals_radius", "--normals_depth_thres"):
        assert flag in h
    sys.path.insert(0, ROOT)
    import eval as pm_eval
    args = pm_eval.build_parser().parse_args([])
    assert args.normals == 0 and args.normals_radius == 2 and args.normals_depth_thres == 0.01  # opt-in; tau = --geo_depth_thres's default
    assert args.normals_depth_thres == args.geo_depth_thres


def test_colmap_output_normal_maps_without_a_device_fails_before_writing(tmp_path):
    ws = tmp_path / "ws"
    ws.mkdir()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")  # the child sees no device, wherever this runs
    r = subprocess.run([sys.executable, os.path.join(ROOT, "colmap_output.py"), "--input_folder", str(ws), "--normal_maps"],
                       capture_output=True, text=True, cwd=ROOT, env=env)
    assert r.returncode != 0
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and "--normal_maps needs a ROCm GPU" in lines[0], r.stderr
    assert os.listdir(ws) == []  # nothing was created, stereo/normal_maps/ included


def test_colmap_export_refuses_a_cpu_device_before_writing(tmp_path):
    import patchmatchnet_amd as P
    from patchmatchnet_amd import colmap
    ws = tmp_path / "ws"
    ws.mkdir()
    with pytest.raises(P.PmnError, match="ROCm GPU"):
        colmap.export_workspace(str(ws), normal_maps=True, device="cpu")
    assert os.listdir(ws) == []


def test_depth_normals_wrapper_refuses_cpu_tensors():
    import patchmatchnet_amd as P
    from patchmatchnet_amd import ops
    with pytest.raises(P.PmnError):
        ops.depth_normals(torch.ones(8, 8), np.eye(3, dtype=np.float32))
    with pytest.raises(P.PmnError):
        ops.depth_normals(np.ones((8, 8), np.float32), np.eye(3, dtype=np.float32))


def test_c_boundary_rejects_bad_arguments_without_launching():
    """Null pointers, sizes, radius, threshold and intrinsics are checked on the host before any HIP call (safe without a GPU)."""
    from patchmatchnet_amd import _lib
    L = _lib.lib()
    assert L.pmn_abi_version() == 25  # additive: the two entry points were added under ABI 25
    K = (ctypes.c_float * 9)(200, 0, 32, 0, 200, 32, 0, 0, 1)
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its argument check
    assert L.pmn_depth_normals(None, 8, 8, K, 2, 0.01, p, None) == -1
    assert L.pmn_depth_normals(p, 8, 8, None, 2, 0.01, p, None) == -1
    assert L.pmn_depth_normals(p, 8, 8, K, 2, 0.01, None, None) == -1
    assert L.pmn_depth_normals(p, 0, 8, K, 2, 0.01, p, None) == -1
    assert L.pmn_depth_normals(p, 8, -1, K, 2, 0.01, p, None) == -1
    for tau in (0.0, -0.01, float("nan"), float("inf")):
        assert L.pmn_depth_normals(p, 8, 8, K, 2, tau, p, None) == -1
    Kbad = (ctypes.c_float * 9)(200, 0, float("nan"), 0, 200, 32, 0, 0, 1)
    assert L.pmn_depth_normals(p, 8, 8, Kbad, 2, 0.01, p, None) == -1
    for radius in (0, 4, -1):
        assert L.pmn_depth_normals(p, 8, 8, K, radius, 0.01, p, None) == -2
    ok = [p, p, p, p, 3, p, 0, 8, 8, p, 64, p, p, p, None]
    for i in (0, 1, 2, 3, 5, 9, 11, 12, 13):  # every pointer
        a = list(ok)
        a[i] = None
        assert L.pmn_pack_points_normals(*a) == -1, i
    for i, v in ((4, 2), (7, 0), (8, 0), (10, -1)):  # rotation stride, H, W, capacity
        a = list(ok)
        a[i] = v
        assert L.pmn_pack_points_normals(*a) == -1, i
