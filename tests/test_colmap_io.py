"""CPU tests of the COLMAP import / export host side (patchmatchnet_amd/colmap.py, colmap_output.py) against the reference's recorded
outputs in tests/golden/colmap_reference.npz (tests/golden/make_colmap_golden.py).  The view-selection scores themselves run on the
GPU (tests/test_colmap_gpu.py); here the writers are fed the numpy restatement of colmap_synth.oracle_scores."""
import os
import struct
import sys

import numpy as np
import pytest

import colmap_synth as CS
import goldenutil as GU
from patchmatchnet_amd import colmap as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    return np.load(os.path.join(GU.GOLDEN_DIR, "colmap_reference.npz"))


def _case(tmp_path, name):
    root = str(tmp_path / name)
    digest = CS.write_case(root, CS.CASES[name]["model"])
    assert digest == str(_golden()[f"{name}__model_sha256"]), "the synthetic model is not the one the golden was made from"
    return root


def test_reader_round_trips_the_writer(tmp_path):
    cams, imgs, pts = CS.make_model(**CS.CASES["B"]["model"])
    CS.write_model(str(tmp_path / "sparse"), cams, imgs, pts)
    m = C.read_model(str(tmp_path / "sparse"))
    assert sorted(m.cameras) == [c[0] for c in cams]
    for cid, model, w, h, params in cams:
        got = m.cameras[cid]
        assert (got.model, got.width, got.height, got.params) == (model, w, h, tuple(params))
    assert [im.id for im in m.images] == [im[0] for im in imgs]  # file order kept (ids unsorted, non-contiguous)
    for got, (iid, q, t, cid, name, pids) in zip(m.images, imgs):
        assert (got.qvec, got.tvec, got.camera_id, got.name) == (tuple(q), tuple(t), cid, name)
        np.testing.assert_array_equal(got.point3d_ids, pids)
    ids = np.array([p[0] for p in pts])
    order = np.argsort(ids)
    np.testing.assert_array_equal(m.point_ids, ids[order])
    np.testing.assert_array_equal(m.xyz, np.array([p[1] for p in pts])[order])


def _write_small(d, cameras=None, images=None, points=None):
    cameras = cameras or [(1, "PINHOLE", 8, 6, [5.0, 5.0, 4.0, 3.0])]
    images = images or [(1, [1.0, 0, 0, 0], [0.0, 0, 0], 1, "a.jpg", np.array([10, -1, 11])),
                        (2, [1.0, 0, 0, 0], [1.0, 0, 0], 1, "b.jpg", np.array([11, 10]))]
    points = points or [(10, [0.0, 0, 5], [1, 2, 3], 0.1, [(1, 0), (2, 1)]), (11, [1.0, 1, 6], [1, 2, 3], 0.1, [(1, 2), (2, 0)])]
    CS.write_model(d, cameras, images, points)
    return d


def test_malformed_models_name_file_and_record(tmp_path):
    d = _write_small(str(tmp_path / "ok"))
    C.read_model(d)
    # truncated images.bin
    t = _write_small(str(tmp_path / "trunc"))
    p = os.path.join(t, "images.bin")
    data = open(p, "rb").read()
    open(p, "wb").write(data[:-5])
    with pytest.raises(C.ColmapFormatError, match=r"images\.bin: truncated in image record 1"):
        C.read_model(t)
    t = _write_small(str(tmp_path / "trunc_pts"))
    p = os.path.join(t, "points3D.bin")
    data = open(p, "rb").read()
    open(p, "wb").write(data[:-3])
    with pytest.raises(C.ColmapFormatError, match=r"points3D\.bin: truncated in point record 1"):
        C.read_model(t)
    # unknown camera model id
    u = _write_small(str(tmp_path / "model"))
    p = os.path.join(u, "cameras.bin")
    data = bytearray(open(p, "rb").read())
    data[12:16] = struct.pack("<i", 42)
    open(p, "wb").write(bytes(data))
    with pytest.raises(C.ColmapFormatError, match=r"cameras\.bin: camera record 0 \(camera_id 1\) has unknown camera model id 42"):
        C.read_model(u)
    # an image that references a point3D_id missing from points3D.bin
    m = _write_small(str(tmp_path / "missing"), images=[(1, [1.0, 0, 0, 0], [0.0, 0, 0], 1, "a.jpg", np.array([10, 99]))])
    with pytest.raises(C.ColmapFormatError, match=r"images\.bin: image a\.jpg \(image_id 1\) references point3D_id 99"):
        C.read_model(m)


def test_intrinsics_and_extrinsics_for_every_camera_model():
    for mid, (name, pnames) in C.CAMERA_MODELS.items():
        params = tuple(10.0 + k for k in range(len(pnames)))
        K = C.intrinsic_matrix(C.Camera(1, name, 8, 6, params))
        if pnames[0] == "f":
            fx = fy = params[0]
            cx, cy = params[1], params[2]
        else:
            fx, fy, cx, cy = params[:4]
        np.testing.assert_array_equal(K, np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64))
        assert K.dtype == np.float64
    q = np.array([0.9, 0.1, -0.3, 0.2])
    q /= np.linalg.norm(q)
    im = C.Image(1, tuple(q), (1.0, 2.0, 3.0), 1, "x", np.zeros(0, C.POINT2D_DTYPE))
    E = C.extrinsic_matrix(im)
    R = E[:3, :3]
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-14)
    assert abs(np.linalg.det(R) - 1) < 1e-14
    np.testing.assert_array_equal(E[:3, 3], [1.0, 2.0, 3.0])
    np.testing.assert_array_equal(E[3], [0, 0, 0, 1])
    np.testing.assert_allclose(C.rotation_matrix_to_quaternion(R), q, atol=1e-14)


def test_depth_range_index_rule(tmp_path):
    for n in range(1, 3000):
        assert C.depth_index(n) == (int(n * .01), int(n * .99))
    # an image with 1 .. 201 observations at known depths: the (sorted) order statistics at those indices, duplicates counted
    for n in (1, 7, 100, 101, 201):
        zs = np.arange(n, dtype=np.float64)[::-1] + 2.0
        pts = [(100 + k, [0.0, 0.0, float(z)], [0, 0, 0], 0.0, [(1, k)]) for k, z in enumerate(zs)]
        pids = np.array([100 + k for k in range(n)] + [-1, 100])
        d = _write_small(str(tmp_path / f"d{n}"), images=[(1, [1.0, 0, 0, 0], [0.0, 0, 0], 1, "a.jpg", pids)], points=pts)
        m = C.read_model(d)
        got = C.depth_ranges(m, [C.extrinsic_matrix(im) for im in m.images])
        srt = np.sort(np.concatenate([zs, zs[:1]]))
        a, b = C.depth_index(n + 1)
        assert got == [(srt[a], srt[b])]
    # an image without a triangulated point is an error that names it
    d = _write_small(str(tmp_path / "empty"), images=[(5, [1.0, 0, 0, 0], [0.0, 0, 0], 1, "lonely.jpg", np.array([-1, -1]))])
    m = C.read_model(d)
    with pytest.raises(C.ColmapFormatError, match=r"image lonely\.jpg \(image_id 5\) has no triangulated point"):
        C.depth_ranges(m, [C.extrinsic_matrix(im) for im in m.images])


@pytest.mark.parametrize("name", ["A", "B"])
def test_cam_and_pair_writers_reproduce_the_reference_bytes(tmp_path, name):
    g = _golden()
    root = _case(tmp_path, name)
    a = CS.CASES[name]["args"]
    m = C.read_model(os.path.join(root, "sparse"))
    extr = [C.extrinsic_matrix(im) for im in m.images]
    ranges = C.depth_ranges(m, extr)
    for i, im in enumerate(m.images):
        p = str(tmp_path / "cam.txt")
        C.write_cam_file(p, extr[i], C.intrinsic_matrix(m.cameras[im.camera_id]), *ranges[i])
        assert open(p, "rb").read() == g[f"{name}__cams__{i:08d}"].tobytes(), (name, i)
    score = CS.oracle_scores(m, a["theta0"], a["sigma1"], a["sigma2"])
    p = str(tmp_path / "pair.txt")
    C.write_pair_file(p, C.select_views(score, a["num_src_images"]))
    assert open(p, "rb").read() == g[f"{name}__pair"].tobytes()
    if name == "B":
        assert np.isnan(score).any() and (score[1, 6] == 0.0)  # the case's point at a camera centre and its disjoint pair


@pytest.mark.parametrize("name", ["A", "B"])
def test_colmap_output_reproduces_the_reference_workspace(tmp_path, name):
    from patchmatchnet_amd.data_io import read_cam_file  # noqa: F401  (the export reads the cam files through it)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_colmap_golden as MG
    g = _golden()
    mvs, ws = str(tmp_path / "mvs"), str(tmp_path / "ws")
    os.makedirs(os.path.join(mvs, "cams"))
    os.makedirs(ws)
    n = CS.CASES[name]["model"]["n_images"]
    cams, imgs, _ = CS.make_model(**CS.CASES[name]["model"])
    CS.write_images(os.path.join(mvs, "images_src"), imgs, seed=CS.CASES[name]["model"]["seed"])
    C.copy_images(os.path.join(mvs, "images_src"), os.path.join(mvs, "images"), [im[4] for im in imgs])
    import shutil
    shutil.rmtree(os.path.join(mvs, "images_src"))
    for v in range(n):
        with open(os.path.join(mvs, "cams", "%08d_cam.txt" % v), "wb") as f:
            f.write(g[f"{name}__cams__{v:08d}"].tobytes())
    with open(os.path.join(mvs, "pair.txt"), "wb") as f:
        f.write(g[f"{name}__pair"].tobytes())
    MG.result_maps(mvs, n, CS.CASES[name]["model"]["seed"])
    import colmap_output
    colmap_output.main(["--input_folder", mvs, "--output_folder", ws])
    for rel in MG.OUTPUT_FILES:
        got = open(os.path.join(ws, rel), "rb").read()
        want = g[f"{name}__ws__{rel.replace('/', '__')}"].tobytes()
        if rel != "sparse/images.txt":
            assert got == want, rel
            continue
        gl, wl = got.decode().split("\n"), want.decode().split("\n")
        assert len(gl) == len(wl)
        for x, y in zip(gl, wl):
            if x.startswith("#") or not x:
                assert x == y
                continue
            xs, ys = x.split(), y.split()
            assert xs[0] == ys[0] and xs[5:] == ys[5:], (x, y)  # id, tvec, camera id, name: the same text
            np.testing.assert_allclose([float(v) for v in xs[1:5]], [float(v) for v in ys[1:5]], rtol=0, atol=1e-12)
    for kind in ("depth_maps", "confidence_maps"):
        for v in range(n):
            got = open(os.path.join(ws, "stereo", kind, "%08d.jpg.geometric.bin" % v), "rb").read()
            assert got == g[f"{name}__ws__{kind}__{v:08d}"].tobytes(), (kind, v)
    assert sorted(os.listdir(os.path.join(ws, "images"))) == ["%08d.jpg" % v for v in range(n)]


def test_in_place_copy_with_permuted_numbered_sources_loses_no_image(tmp_path):
    d = str(tmp_path / "images")
    os.makedirs(d)
    n = 6
    for k in range(n):
        with open(os.path.join(d, "%08d.jpg" % k), "wb") as f:
            f.write(b"image-%d" % k)
    order = [3, 0, 5, 1, 4, 2]  # images.bin order: output i is source order[i]
    C.copy_images(d, d, ["%08d.jpg" % k for k in order])
    for i, k in enumerate(order):
        assert open(os.path.join(d, "%08d.jpg" % i), "rb").read() == b"image-%d" % k
    assert sorted(os.listdir(d)) == ["%08d.jpg" % k for k in range(n)]  # no temporary left behind


def test_convert_format_reencodes_as_jpeg(tmp_path):
    from PIL import Image as PilImage
    d = str(tmp_path / "src")
    os.makedirs(d)
    PilImage.fromarray(np.full((6, 8, 4), 200, np.uint8)).save(os.path.join(d, "a.png"))
    C.copy_images(d, str(tmp_path / "out"), ["a.png"], convert_format=True)
    with PilImage.open(str(tmp_path / "out" / "00000000.jpg")) as im:
        assert im.format == "JPEG" and im.mode == "RGB" and im.size == (8, 6)
