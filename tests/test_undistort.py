"""CPU tests of the undistortion's host geometry (patchmatchnet_amd/undistort.py): the Newton inverse, the
undistorted camera against numbers derived by hand and against the independent oracle (tests/undistort_ref.py), the refused models,
the new flags of colmap_input.py, and ops.undistort_image's refusal of CPU tensors."""
import numpy as np
import pytest
import torch

import undistort_ref as R
from patchmatchnet_amd import undistort as U
from patchmatchnet_amd.colmap import Camera


def _camera(cam, cid=1):
    return Camera(cid, cam[0], cam[1], cam[2], tuple(float(v) for v in cam[3]))


# every supported model, with the parameter sets of the GPU cases (the two FULL_OPENCV sets with a pole are not invertible)
INVERTIBLE = [n for n in R.CASES if n not in ("full_opencv_inf", "full_opencv_nan")]


def test_every_supported_model_has_a_case():
    assert {R.CASES[n]["cam"][0] for n in INVERTIBLE} == set(R.SUPPORTED)


@pytest.mark.parametrize("name", INVERTIBLE)
def test_inverse_inverts(name):
    cam = R.CASES[name]["cam"]
    c = _camera(cam)
    W, H = cam[1], cam[2]
    # the border pixels the bounds use, and an interior grid
    bx = np.concatenate([np.full(H, 0.5), np.full(H, W - 0.5), np.arange(W) + 0.5, np.arange(W) + 0.5])
    by = np.concatenate([np.arange(H) + 0.5, np.arange(H) + 0.5, np.full(W, 0.5), np.full(W, H - 0.5)])
    gx, gy = np.meshgrid(np.linspace(1.0, W - 1.0, 9), np.linspace(1.0, H - 1.0, 7))
    px, py = np.concatenate([bx, gx.ravel()]), np.concatenate([by, gy.ravel()])
    u, v, ok = U.pixel_to_world(c, px, py)
    assert ok.all()
    qx, qy = U.world_to_pixel(c, u, v)
    assert max(np.abs(qx - px).max(), np.abs(qy - py).max()) < 1e-9
    # ... and the product's forward model is the oracle's
    ox, oy = R.project(cam, u, v)
    np.testing.assert_array_equal(qx, ox)
    np.testing.assert_array_equal(qy, oy)


# The hand-derived camera.  SIMPLE_RADIAL, W x H = 65 x 49, f = 64, principal point (32.5, 24.5) = the centre of pixel (32, 24), and
# k = -0.32768, chosen so that the corners come out exactly:
#   the border pixel centres are at x_d = (0.5 - 32.5) / 64 = -0.5 and (64.5 - 32.5) / 64 = +0.5, y_d = -+ 24 / 64 = -+ 0.375;
#   a corner has r_d = sqrt(0.25 + 0.140625) = 0.625.  Undistorting scales the point by s with s r_d (1 + k s^2 r_d^2) = r_d; s = 1.25
#   gives 1 + k * 0.78125^2 = 1 - 0.32768 * 0.6103515625 = 0.8 = 1 / 1.25: the corners undistort to (-+0.625, -+0.46875), i.e. to the
#   pixels x = 32.5 -+ 40 = -7.5 / 72.5 and y = 24.5 -+ 30 = -5.5 / 54.5.  |x| grows with r_d along a side, so these are the extremes:
#   left_min_x = -7.5, right_max_x = 72.5, top_min_y = -5.5, bottom_max_y = 54.5.
#   blank_pixels = 1:  min_scale_x = min(32.5 / 40, 32 / 40) = 0.8, scale_x = 1.25, W' = int(81.25) = 81, cx' = 32.5 * 81 / 65 = 40.5;
#                      min_scale_y = min(24.5 / 30, 24 / 30) = 0.8, scale_y = 1.25, H' = int(61.25) = 61, cy' = 24.5 * 61 / 49 = 30.5.
#   The other extremes are on the axes (row 24, column 32), where u (1 + k u^2) = 0.5 has the root u = 0.556463 (0.55646 - 0.32768 *
#   0.172307 = 0.499998) and v (1 + k v^2) = 0.375 the root v = 0.39523: left_max_x = 32.5 - 64 * 0.556463 = -3.1136, top_max_y = 24.5
#   - 64 * 0.39523 = -0.7947.
#   blank_pixels = 0:  max_scale_x = max(32.5 / 35.6136, 32 / 35.6136) = 0.91257, scale_x = 1.09580, W' = int(71.23) = 71, cx' = 35.5;
#                      max_scale_y = max(24.5 / 25.2947, 24 / 25.2947) = 0.96858, scale_y = 1.03244, H' = int(50.59) = 50, cy' = 25.0.
HAND = Camera(7, "SIMPLE_RADIAL", 65, 49, (64.0, 32.5, 24.5, -0.32768))


@pytest.mark.parametrize("blank,want", [(1.0, (81, 61, 40.5, 30.5)), (0.0, (71, 50, 35.5, 25.0))])
def test_simple_radial_camera_derived_by_hand(blank, want):
    got = U.undistorted_camera(HAND, blank_pixels=blank)
    assert got.model == "PINHOLE" and got.id == 7
    assert (got.width, got.height) == want[:2]
    assert got.params[:2] == (64.0, 64.0)
    np.testing.assert_allclose(got.params[2:], want[2:], rtol=1e-12)


def test_the_bounds_of_the_hand_derived_camera():
    u, v, ok = U.pixel_to_world(HAND, np.array([0.5, 64.5, 0.5, 32.5]), np.array([0.5, 48.5, 24.5, 0.5]))
    assert ok.all()
    np.testing.assert_allclose(u[:2], [-0.625, 0.625], atol=1e-11)
    np.testing.assert_allclose(v[:2], [-0.46875, 0.46875], atol=1e-11)
    assert abs(u[2] + 0.556463) < 1e-5 and abs(v[3] + 0.39523) < 1e-5


@pytest.mark.parametrize("cam", [Camera(3, "PINHOLE", 53, 37, (50.0, 51.0, 26.3, 18.6)), Camera(4, "SIMPLE_PINHOLE", 64, 48, (60.0, 31.0, 24.5))])
def test_pinhole_gives_the_identical_camera(cam):
    assert U.undistorted_camera(cam) == cam
    assert U.undistorted_camera(cam, blank_pixels=1.0, min_scale=0.5, max_scale=1.5) == cam
    assert not U.has_distortion(cam)


def test_scale_clamps_are_reached():
    # a 100-degree fisheye with every source pixel kept wants 2.1x (tan(1.2) / 1.2 on the axis, more in the corners): max_scale = 2
    wide = Camera(1, "OPENCV_FISHEYE", 64, 48, (26.0, 26.0, 32.5, 24.5, 0.0, 0.0, 0.0, 0.0))
    got = U.undistorted_camera(wide, blank_pixels=1.0)
    assert (got.width, got.height) == (128, 96) and got.params == (26.0, 26.0, 65.0, 49.0)
    assert U.undistorted_camera(wide, blank_pixels=1.0, max_scale=8.0).width > 128
    # a violent pincushion (k = 400) pulls the border in to a sixth: min_scale = 0.2
    pinc = Camera(2, "SIMPLE_RADIAL", 65, 49, (64.0, 32.5, 24.5, 400.0))
    got = U.undistorted_camera(pinc)
    assert (got.width, got.height) == (int(0.2 * 65), int(0.2 * 49)) == (13, 9)
    free = U.undistorted_camera(pinc, min_scale=0.01)
    assert free.width < 13 and free.height < 9
    # the same clamps through the oracle
    assert R.undistorted_camera(("SIMPLE_RADIAL", 65, 49, pinc.params))[1:3] == (13, 9)


def test_max_image_size():
    # 81 x 61 (above) limited to 40: the factor is 40 / 81, W' = int(81 * 40 / 81) = 40, H' = int(61 * 40 / 81) = int(30.12) = 30;
    # fx, cx scale by 40 / 81 and fy, cy by 30 / 61
    got = U.undistorted_camera(HAND, blank_pixels=1.0, max_image_size=40)
    assert (got.width, got.height) == (40, 30)
    np.testing.assert_allclose(got.params, (64.0 * 40 / 81, 64.0 * 30 / 61, 40.5 * 40 / 81, 30.5 * 30 / 61), rtol=1e-14)
    # no effect when the image is small enough already, and -1 / 0 mean no limit
    assert U.undistorted_camera(HAND, blank_pixels=1.0, max_image_size=81) == U.undistorted_camera(HAND, blank_pixels=1.0)
    assert U.undistorted_camera(HAND, blank_pixels=1.0, max_image_size=0) == U.undistorted_camera(HAND, blank_pixels=1.0)
    # a pinhole is resized too, and only then changes
    pin = Camera(3, "SIMPLE_PINHOLE", 64, 48, (60.0, 31.0, 24.5))
    got = U.undistorted_camera(pin, max_image_size=32)
    assert got.model == "PINHOLE" and (got.width, got.height) == (32, 24) and got.params == (30.0, 30.0, 15.5, 12.25)


@pytest.mark.parametrize("name", [n for n in INVERTIBLE if "kw" in R.CASES[n]])  # (the others name their output camera themselves)
def test_product_camera_equals_the_oracle(name):
    case = R.CASES[name]
    want = R.undistorted_camera(case["cam"], **case["kw"])
    got = U.undistorted_camera(_camera(case["cam"]), **case["kw"])
    assert (got.width, got.height) == (want[1], want[2])
    np.testing.assert_allclose(U.focal_and_center(got), R.split(want)[:4], rtol=1e-12)


@pytest.mark.parametrize("model,n", [("FOV", 5), ("THIN_PRISM_FISHEYE", 12)])
def test_fov_and_thin_prism_are_refused(model, n):
    cam = Camera(41, model, 64, 48, (60.0, 60.0, 32.0, 24.0) + (0.01,) * (n - 4))
    for call in (lambda: U.undistorted_camera(cam), lambda: U.distort(cam, 0.1, 0.1)):
        with pytest.raises(U.UndistortError) as e:
            call()
        assert "41" in str(e.value) and model in str(e.value)


def test_a_border_that_cannot_be_undistorted_is_an_error():
    # border points whose Newton iteration leaves the finite numbers are dropped from the bounds; a side that loses all of them is an
    # error that names the camera (here: every step is NaN)
    with pytest.raises(U.UndistortError) as e:
        U.undistorted_camera(Camera(5, "SIMPLE_RADIAL", 64, 48, (30.0, 32.0, 24.0, float("nan"))))
    assert "camera 5" in str(e.value)
    u, v, ok = U.pixel_to_world(Camera(5, "SIMPLE_RADIAL", 64, 48, (30.0, 32.0, 24.0, float("nan"))), np.array([0.5]), np.array([0.5]))
    assert not ok.any()


def test_cli_parses_the_new_flags():
    colmap_input = R.load_cli()
    a = colmap_input.build_parser().parse_args(["--input_folder", "x"])
    assert (a.undistort, a.blank_pixels, a.min_scale, a.max_scale, a.max_image_size) == (False, 0.0, 0.2, 2.0, -1)
    a = colmap_input.build_parser().parse_args(["--input_folder", "x", "--undistort", "--blank_pixels", "0.5", "--min_scale", "0.3",
                                                "--max_scale", "1.5", "--max_image_size", "2000"])
    assert (a.undistort, a.blank_pixels, a.min_scale, a.max_scale, a.max_image_size) == (True, 0.5, 0.3, 1.5, 2000)


def test_ops_refuses_a_cpu_tensor():
    from patchmatchnet_amd import ops
    cam = _camera(R.CASES["radial_barrel"]["cam"])
    with pytest.raises(ops.PmnError):
        ops.undistort_image(torch.zeros((48, 64, 3), dtype=torch.uint8), cam, U.undistorted_camera(cam))


def test_argument_checks_do_not_launch():
    """Bad arguments of pmn_undistort_image are rejected on the host before any HIP call (safe without a GPU)."""
    import ctypes
    from patchmatchnet_amd import _lib
    L = _lib.lib()
    par = (ctypes.c_double * 12)(60.0, 60.0, 32.0, 24.0)
    pin = (ctypes.c_double * 4)(60.0, 60.0, 32.0, 24.0)
    pp, pn, buf = ctypes.cast(par, ctypes.c_void_p), ctypes.cast(pin, ctypes.c_void_p), 4096  # (never dereferenced on these paths)
    call = lambda src=buf, Hs=48, Ws=64, ch=3, model=4, p=pp, d=pn, Hd=48, Wd=64, dst=buf: L.pmn_undistort_image(
        src, Hs, Ws, ch, model, p, d, Hd, Wd, dst, None, None, None)
    assert call(src=None) == -1 and call(dst=None) == -1 and call(p=None) == -1 and call(d=None) == -1
    assert call(ch=2) == -1 and call(ch=4) == -1 and call(ch=0) == -1
    assert call(model=7) == -1 and call(model=10) == -1 and call(model=11) == -1 and call(model=-1) == -1
    assert call(Hs=0) == -1 and call(Ws=-3) == -1 and call(Hd=0) == -1 and call(Wd=0) == -1
    assert call(Hs=32768, Ws=21846) == -1   # 2^31 + 2^11 bytes of RGB
    assert call(Hd=32768, Wd=21846) == -1
    assert call(ch=1, Hs=65536, Ws=32768) == -1  # exactly 2^31 bytes of grey
