"""GPU tests of the image undistortion: pmn_undistort_image through ops.undistort_image against the float64
numpy oracle (tests/undistort_ref.py) -- sampling positions, valid mask and bytes of every case of undistort_ref.CASES --, the
pinhole copy, the every-byte-written property, argument errors, colmap_input.py --undistort against the oracle's files, and the
geometry end to end on a synthetic model's points."""
import functools
import io
import os

import numpy as np
import pytest
import torch

import undistort_ref as R
from patchmatchnet_amd import colmap as C
from patchmatchnet_amd import ops
from patchmatchnet_amd import undistort as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIE_BAND = 1e-6   # a sample whose value before rounding is this close to a .5 tie may differ by one level ...
MAX_TIES = 4      # ... on at most this many samples of a case


def _camera(cam, cid=1):
    return C.Camera(cid, cam[0], cam[1], cam[2], tuple(float(v) for v in cam[3]))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(image, output camera, oracle image, valid, coords, values): computed once per case and only read afterwards."""
    case = R.CASES[name]
    img, dst = R.case_image(case), R.case_dst(case)
    got = R.warp(img, case["cam"], dst)
    for a in (img,) + got:
        a.setflags(write=False)
    return (img, dst) + got


def _run(name, **kw):
    img, dst = _oracle(name)[:2]
    return ops.undistort_image(torch.from_numpy(img.copy()).to(DEV), _camera(R.CASES[name]["cam"]), _camera(dst), **kw)


def _check_pixels(got, want, valid, values):
    """Equal bytes, except that at most MAX_TIES samples within TIE_BAND of a tie may differ by one level."""
    tie = R.near_tie(values, TIE_BAND) & (valid if values.ndim == 2 else valid[..., None])
    assert int(tie.sum()) <= MAX_TIES, f"the oracle alone has {int(tie.sum())} samples in the tie band: pick another seed"
    diff = got.astype(np.int16) - want.astype(np.int16)
    bad = diff != 0
    assert not (bad & ~tie).any(), f"{int((bad & ~tie).sum())} samples differ away from a tie, max |diff| {int(np.abs(diff).max())}"
    assert int(bad.sum()) <= MAX_TIES and (np.abs(diff[bad]) <= 1).all()


def test_the_case_list_covers_what_it_must():
    assert {c["cam"][0] for c in R.CASES.values()} == set(R.SUPPORTED)
    shapes = {(c["cam"][2], c["cam"][1], c["channels"]) for c in R.CASES.values()}
    assert {(48, 64, 3), (37, 53, 3), (37, 53, 1)} <= shapes
    # NaN and infinity inside the output, blank borders, an output larger and one smaller than its source
    assert np.isnan(_oracle("full_opencv_nan")[4]).any() and np.isinf(_oracle("full_opencv_inf")[4]).any()
    assert 0.10 < 1 - _oracle("simple_radial_blank")[3].mean() < 0.16
    assert _oracle("fisheye_max_scale")[1][1:3] == (128, 96) and _oracle("radial_max_image_size")[1][1:3] == (40, 29)
    x0 = _oracle("fisheye_centre")[4][18, 26]
    assert tuple(x0) == (26.0, 18.0)  # r = 0 exactly: the position is the pixel itself


@pytest.mark.parametrize("name", list(R.CASES))
def test_coordinates_mask_and_bytes_match_the_oracle(name):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    img, dst, want, valid, coords, values = _oracle(name)
    out, got_valid, got_coords = (t.cpu().numpy() for t in _run(name, want_valid=True, want_coords=True))
    assert out.shape == want.shape and out.dtype == np.uint8
    # positions: non-finite exactly where the oracle's are, within 1e-9 px elsewhere (fp64 epsilon 2.2e-16 x coordinates below 1e4
    # x a chain of about a hundred operations)
    fin = np.isfinite(coords)
    np.testing.assert_array_equal(np.isfinite(got_coords), fin)
    err = float(np.abs(got_coords[fin] - coords[fin]).max())
    print(f"{name}: max |coords - oracle| = {err:.3e} px, {int((~fin).sum())} non-finite, valid {valid.mean():.3f}")
    assert err <= 1e-9
    np.testing.assert_array_equal(got_valid, valid.astype(np.uint8))
    assert not out[~valid].any()
    _check_pixels(out, want, valid, values)
    # without the optional outputs: the same bytes; and again into a buffer full of 0xFF: every byte is written
    np.testing.assert_array_equal(_run(name).cpu().numpy(), out)
    buf = torch.full(out.shape, 0xFF, dtype=torch.uint8, device=DEV)
    again = _run(name, out=buf)
    assert again is buf
    np.testing.assert_array_equal(buf.cpu().numpy(), out)


@pytest.mark.parametrize("cam", [("PINHOLE", 53, 37, (50.0, 51.0, 26.3, 18.6)), ("SIMPLE_PINHOLE", 64, 48, (60.0, 31.0, 24.5))])
@pytest.mark.parametrize("channels", [1, 3])
def test_pinhole_returns_the_input_bytes(cam, channels):
    c = _camera(cam)
    img = np.random.default_rng(5).integers(0, 256, (cam[2], cam[1]) + ((3,) if channels == 3 else ()), dtype=np.uint8)
    t = torch.from_numpy(img).to(DEV)
    out, valid, coords = ops.undistort_image(t, c, U.undistorted_camera(c), want_valid=True, want_coords=True)
    assert out.data_ptr() != t.data_ptr()
    np.testing.assert_array_equal(out.cpu().numpy(), img)
    assert bool((valid == 1).all())
    np.testing.assert_array_equal(coords[3, 5].cpu().numpy(), [5.0, 3.0])


def test_wrapper_refuses_bad_arguments():
    cam = _camera(R.CASES["radial_barrel"]["cam"])
    dst = U.undistorted_camera(cam)
    img = torch.zeros((48, 64, 3), dtype=torch.uint8, device=DEV)
    for bad in (img.cpu(), img.float(), img[:, :60], img[:, ::2], torch.zeros((48, 64, 2), dtype=torch.uint8, device=DEV),
                torch.zeros((47, 64, 3), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ops.PmnError):
            ops.undistort_image(bad, cam, dst)
    with pytest.raises(ops.PmnError):  # the output camera must be a pinhole
        ops.undistort_image(img, cam, cam)
    with pytest.raises(ops.PmnError):  # a refused model names itself
        ops.undistort_image(img, C.Camera(9, "FOV", 64, 48, (60.0, 60.0, 32.0, 24.0, 0.5)), dst)
    with pytest.raises(ops.PmnError):  # out of the wrong shape
        ops.undistort_image(img, cam, dst, out=torch.zeros((dst.height, dst.width + 1, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(ops.PmnError):  # out on top of the input
        ops.undistort_image(img, cam, C.Camera(1, "PINHOLE", 64, 48, (60.0, 60.0, 31.0, 24.0)), out=img)


def test_argument_errors_return_without_launching():
    import ctypes
    from patchmatchnet_amd import _lib
    L = _lib.lib()
    src = torch.zeros((48, 64, 3), dtype=torch.uint8, device=DEV)
    dst = torch.full((48, 64, 3), 7, dtype=torch.uint8, device=DEV)
    par = (ctypes.c_double * 12)(60.0, 60.0, 32.0, 24.0)
    pin = (ctypes.c_double * 4)(60.0, 60.0, 32.0, 24.0)
    pp, pn = ctypes.cast(par, ctypes.c_void_p), ctypes.cast(pin, ctypes.c_void_p)
    for kw in (dict(ch=2), dict(model=7), dict(model=10), dict(model=42), dict(Hs=0), dict(Wd=-1), dict(Hd=32768, Wd=21846),
               dict(Hs=32768, Ws=21846)):
        a = dict(Hs=48, Ws=64, ch=3, model=4, Hd=48, Wd=64)
        a.update(kw)
        assert L.pmn_undistort_image(src.data_ptr(), a["Hs"], a["Ws"], a["ch"], a["model"], pp, pn, a["Hd"], a["Wd"], dst.data_ptr(),
                                     None, None, None) == -1, kw
    for nul in range(4):
        args = [src.data_ptr(), pp, pn, dst.data_ptr()]
        args[nul] = None
        assert L.pmn_undistort_image(args[0], 48, 64, 3, 4, args[1], args[2], 48, 64, args[3], None, None, None) == -1
    torch.cuda.synchronize()
    assert bool((dst == 7).all())  # nothing ran


# ---- colmap_input.py --undistort ------------------------------------------------------------------------------------------------

def _cam_file(path):
    lines = open(path).read().split("\n")
    i = lines.index("intrinsic")
    return lines[1:5], lines[i + 1:i + 4], lines[-2]


def _intrinsic_lines(fx, fy, cx, cy):
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    return ["".join(str(K[r, c]) + " " for c in range(3)) for r in range(3)]


@pytest.fixture(scope="module")
def imported(tmp_path_factory):
    """One synthetic raw model (SIMPLE_RADIAL, OPENCV and SIMPLE_PINHOLE cameras, pictures of their cameras' size), imported with and
    without --undistort."""
    colmap_input = R.load_cli()
    root = tmp_path_factory.mktemp("undistort_cli")
    src, und, plain = (str(root / d) for d in ("colmap", "undistorted", "plain"))
    os.makedirs(und)
    os.makedirs(plain)
    cams, imgs = R.write_case(src)
    colmap_input.main(["--input_folder", src, "--output_folder", und, "--num_src_images", "3", "--undistort"])
    colmap_input.main(["--input_folder", src, "--output_folder", plain, "--num_src_images", "3"])
    return src, und, plain, cams, imgs


def test_cli_writes_the_oracles_cameras_and_pictures(imported):
    from PIL import Image as PilImage
    src, und, plain, cams, imgs = imported
    assert {c[0] for c in cams.values()} == {"SIMPLE_RADIAL", "OPENCV", "SIMPLE_PINHOLE"}
    assert sorted(os.listdir(os.path.join(und, "images"))) == ["%08d.jpg" % i for i in range(len(imgs))]
    dsts = {cid: R.undistorted_camera(cam) for cid, cam in cams.items()}
    for i, im in enumerate(imgs):
        cam, dst = cams[im[3]], dsts[im[3]]
        extr, intr, rng = _cam_file(os.path.join(und, "cams", "%08d_cam.txt" % i))
        assert intr == _intrinsic_lines(*R.split(dst)[:4]), (i, cam[0])
        with PilImage.open(os.path.join(src, "images", im[4])) as f:
            pic = np.asarray(f.convert("RGB"), dtype=np.uint8)
        want, valid, _, values = R.warp(pic, cam, dst) if dst is not cam else (pic, np.ones(pic.shape[:2], bool), None, pic.astype(np.float64))
        ties = int((R.near_tie(values, TIE_BAND) & valid[..., None]).sum())
        assert ties <= MAX_TIES
        enc = io.BytesIO()
        PilImage.fromarray(want).save(enc, "JPEG", quality=95)
        got = open(os.path.join(und, "images", "%08d.jpg" % i), "rb").read()
        if got != enc.getvalue():
            assert ties > 0, f"view {i} ({cam[0]}): the JPEG differs from the oracle's although no sample is near a tie"
            with PilImage.open(io.BytesIO(got)) as a, PilImage.open(io.BytesIO(enc.getvalue())) as b:
                d = np.abs(np.asarray(a, np.int16) - np.asarray(b, np.int16))
            assert d.max() <= 1 and int((d != 0).sum()) <= MAX_TIES
        # what does not depend on the intrinsics is what the plain import writes
        pextr, pintr, prng = _cam_file(os.path.join(plain, "cams", "%08d_cam.txt" % i))
        assert extr == pextr and rng == prng
        # ... and the plain import is today's: the distortion ignored, the picture's bytes copied
        K = C.intrinsic_matrix(_camera(cam, im[3]))
        assert pintr == _intrinsic_lines(K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        assert open(os.path.join(plain, "images", "%08d.jpg" % i), "rb").read() == open(os.path.join(src, "images", im[4]), "rb").read()
    assert open(os.path.join(und, "pair.txt"), "rb").read() == open(os.path.join(plain, "pair.txt"), "rb").read()


def test_import_model_reports_the_device_time_and_names_a_picture_of_the_wrong_size(imported, tmp_path):
    import shutil
    from PIL import Image as PilImage
    src = imported[0]
    out = str(tmp_path / "out")
    os.makedirs(out)
    times = C.import_model(src, out, num_src_images=2, undistort=True, max_image_size=40)
    assert times["undistort"] > 0 and set(times) == {"read", "prepare", "view_scores", "undistort", "write"}
    with PilImage.open(os.path.join(out, "images", "00000000.jpg")) as f:
        assert max(f.size) <= 40
    bad = str(tmp_path / "bad")
    shutil.copytree(src, bad)
    name = imported[4][2][4]
    PilImage.fromarray(np.zeros((24, 32, 3), np.uint8)).save(os.path.join(bad, "images", name))
    with pytest.raises(C.ColmapFormatError) as e:
        C.import_model(bad, out, undistort=True)
    assert name in str(e.value)


def test_geometry_end_to_end(imported):
    """200 observations of the synthetic model: the point projected with its image's DISTORTED camera (p_d) and with the undistorted
    camera (p_u); the kernel's position map, read bilinearly at p_u - 0.5, must point at p_d - 0.5.  The 1e-3 px is the error of
    interpolating the smooth map over one pixel, at most (1/8) |d2 s / dx2| per axis: these cameras have f >= 60 px, |k1|, |k2| <= 0.08
    and |p| <= 0.02, and the model's points project to |u|, |v| <= 0.3, so |d2 sx / dx2| <= (6 |k1| |u| + 20 |k2| |u|^3 + 6 |p|) / f
    = (0.144 + 0.043 + 0.12) / 60 = 5.1e-3 px per px^2, i.e. 6.4e-4 px per axis at the worst (first measured run: 3.2e-4)."""
    src, _, _, cams, imgs = imported
    model = C.read_model(os.path.join(src, "sparse"))
    maps = {}
    for cid, cam in cams.items():
        dst = R.undistorted_camera(cam)
        zero = torch.zeros((cam[2], cam[1]), dtype=torch.uint8, device=DEV)
        maps[cid] = (dst, ops.undistort_image(zero, _camera(cam, cid), _camera(dst, cid), want_coords=True)[2].cpu().numpy())
    done, worst = 0, 0.0
    for im in model.images:
        cam = cams[im.camera_id]
        dst, cmap = maps[im.camera_id]
        e = C.extrinsic_matrix(im)
        pid = im.point3d_ids
        X = model.xyz[np.searchsorted(model.point_ids, pid[pid != -1])]
        Xc = X @ e[:3, :3].T + e[:3, 3]
        u, v = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
        pdx, pdy = R.project(cam, u, v)
        pux, puy = R.project(dst, u, v)
        for k in range(len(u)):
            x, y = pux[k] - 0.5, puy[k] - 0.5
            x0, y0 = int(np.floor(x)), int(np.floor(y))
            if not (0 <= x0 < dst[1] - 1 and 0 <= y0 < dst[2] - 1) or done == 200:
                continue
            ax, ay = x - x0, y - y0
            got = ((1 - ay) * ((1 - ax) * cmap[y0, x0] + ax * cmap[y0, x0 + 1])
                   + ay * ((1 - ax) * cmap[y0 + 1, x0] + ax * cmap[y0 + 1, x0 + 1]))
            worst = max(worst, abs(got[0] - (pdx[k] - 0.5)), abs(got[1] - (pdy[k] - 0.5)))
            done += 1
    print(f"geometry end to end: {done} points, worst |map(p_u) - p_d| = {worst:.3e} px")
    assert done == 200
    assert worst < 1e-3
