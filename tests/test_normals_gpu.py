"""GPU checks of the surface-normal feature: pmn_depth_normals and pmn_pack_points_normals through the C ABI
against the numpy oracle (tests/normals_ref.py), then eval.py --normals 1 and colmap_output.py --normal_maps end to end.

Tolerance of the normals (gate "b" below): the angle between the kernel's normal and the float64 oracle's may be at most 4 x the
largest angle between the oracle's OWN float32 and float64 evaluations of the same case -- the yardstick is what float32 evaluation
costs the oracle, never the kernel's output; 4 x because a kernel may sum in another order, contract to FMA and divide differently, each
worth a few ulps of the same terms.  Where that angle is exactly 0 (fronto-parallel planes) the largest value over the cases of the
same size and radius is used.  Which pixels have no normal is exact: no allowance."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import goldenutil as GU
import normals_ref as NR
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = float(np.finfo(np.float32).eps)


def _cases(H, W):
    for name in sorted(NR.PLANES):
        z, K, _ = NR.plane_scene(name, H, W)
        yield name, z, K
    for kind in ("small", "dtu"):
        z, K, _ = NR.sphere_scene(H, W, kind)
        yield "sphere_" + kind, z, K
    z, K, _ = NR.step_scene(H, W)
    yield "step", z, K
    z, K = NR.random_scene(H, W, seed=H * 7 + W)
    yield "random", z, K


def _kernel(L, z_dev, K, r, tau=0.01, poison=True):
    H, W = z_dev.shape
    out = torch.full((3, H, W), float("nan"), device="cuda") if poison else torch.empty((3, H, W), device="cuda")
    k = np.ascontiguousarray(K, np.float32).reshape(9)
    rc = L.pmn_depth_normals(z_dev.data_ptr(), H, W, k.ctypes.data_as(ctypes.c_void_p), r, tau, out.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("H,W", [(17, 19), (64, 64), (250, 333), (1200, 1600)])
def test_depth_normals_kernel_against_the_oracle(H, W):
    """Planes, spheres, a depth step and a noisy map with 10 % invalid pixels at r = 1, 2, 3; sizes that are no multiple of the 64 x 16
    tile and one that is.  (a) identical zero set, (b) the angle gate of the module docstring, (c) unit length within 4 float32 ulps and
    n . ray < 0, (d) a second call gives the same bits, (e) every element of a poisoned output is written."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import _lib
    L = _lib.lib()
    for r in (1, 2, 3):
        rows = []
        for name, z, K in _cases(H, W):
            n64 = NR.depth_normals_ref(z, K, r)
            n32 = NR.depth_normals_ref(z, K, r, fit_dtype=np.float32)
            zero = (n64 == 0).all(0)
            np.testing.assert_array_equal((n32 == 0).all(0), zero)
            own = float(NR.angle(n32, n64)[~zero].max(initial=0.0))
            zd = torch.from_numpy(z).cuda()
            got = _kernel(L, zd, K, r)
            assert np.isfinite(got).all(), (name, r, "an element of the poisoned output was not written")            # (e)
            again = _kernel(L, zd, K, r, poison=False)
            assert got.tobytes() == again.tobytes(), (name, r)                                                         # (d)
            np.testing.assert_array_equal((got == 0).all(0), zero, err_msg=f"{name} r={r}: zero sets differ")          # (a)
            g = got.astype(np.float64)
            length = np.sqrt((g * g).sum(0))
            assert np.abs(length[~zero] - 1).max(initial=0) <= 4 * EPS32, (name, r)                                    # (c)
            assert ((g * NR.rays(K, H, W)).sum(0)[~zero] < 0).all(), (name, r)
            err = float(NR.angle(g, n64)[~zero].max(initial=0.0))
            rows.append((name, own, err, int((~zero).sum()), bool(np.array_equal(got, n32))))
        fallback = max(own for _, own, _, _, _ in rows)
        for name, own, err, count, same_bits in rows:
            bound = 4 * (own if own > 0 else fallback)
            print(f"{H}x{W} r={r} {name}: {count} normals, oracle f32-vs-f64 {own:.3e} rad, kernel-vs-f64 {err:.3e} rad, bound "
                  f"{bound:.3e}, bit-equal to the float32 oracle: {same_bits}")
            assert err <= bound, (name, r, err, bound)                                                                 # (b)


def test_depth_normals_wrapper_shapes_and_refusals():
    import patchmatchnet_amd as P
    from patchmatchnet_amd import ops
    z, K, _ = NR.plane_scene("small_tilt", 33, 47)
    z2, K2 = NR.random_scene(33, 47, seed=2, kind="small")
    zd = torch.from_numpy(np.stack((z, z2))).cuda()
    Ks = np.stack((K, K2))
    one = ops.depth_normals(zd[0], K)
    assert one.shape == (3, 33, 47) and one.dtype == torch.float32
    both = ops.depth_normals(zd, torch.from_numpy(Ks), radius=3, rel_thres=0.02)
    assert both.shape == (2, 3, 33, 47)
    assert torch.equal(both[1], ops.depth_normals(zd[1], K2, 3, 0.02))
    np.testing.assert_array_equal((one.cpu().numpy() == 0).all(0), (NR.depth_normals_ref(z, K, 2) == 0).all(0))
    for kw in (dict(radius=0), dict(radius=4), dict(radius=2.0), dict(rel_thres=0.0), dict(rel_thres=-1.0), dict(rel_thres=float("nan")),
               dict(rel_thres=1e-60)):
        with pytest.raises(P.PmnError):
            ops.depth_normals(zd[0], K, **kw)
    with pytest.raises(P.PmnError):
        ops.depth_normals(zd, K)  # [B,H,W] needs [B,3,3]
    with pytest.raises(P.PmnError):
        ops.depth_normals(zd[0], Ks)
    with pytest.raises(P.PmnError):
        ops.depth_normals(zd[None], Ks[None])
    with pytest.raises(P.PmnError):
        ops.depth_normals(zd[0].double(), K)
    with pytest.raises(P.PmnError):
        ops.depth_normals(zd[0], np.full((3, 3), np.nan, np.float32))


def _random_rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return (q * np.sign(np.linalg.det(q))).astype(np.float32)


@pytest.mark.parametrize("float_image,stride", [(False, 3), (True, 4)])
def test_pack_points_normals_against_pack_points(float_image, stride):
    """Same masks / points / images through pmn_pack_points and pmn_pack_points_normals, three views appended on one stream: the
    x y z red green blue columns, the counts and the cursor are identical; the normal columns are R . n as float32 numpy evaluates
    (r0 nx + r1 ny) + r2 nz, within 2 ulps per component; zero normals stay exactly zero; a view that does not fit writes nothing
    and reports -1."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(11 + stride)
    st = torch.cuda.current_stream().cuda_stream
    views = []
    for H, W in ((37, 53), (64, 64), (1, 1029)):
        mask = (rng.random((H, W)) < 0.4).astype(np.uint8)
        xyz = (rng.standard_normal((H, W, 3)) * 300).astype(np.float32)
        img = rng.random((H, W, 3)).astype(np.float32) if float_image else rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        nrm = rng.standard_normal((3, H, W))
        nrm = (nrm / np.sqrt((nrm * nrm).sum(0))).astype(np.float32)
        nrm[:, rng.random((H, W)) < 0.2] = 0
        R = _random_rotation(rng)
        Rbuf = np.zeros((4, 4), np.float32) if stride == 4 else np.zeros((3, 3), np.float32)
        Rbuf[:3, :3] = R
        if stride == 4:
            Rbuf[:, 3] = Rbuf[3, :] = 7.0  # translation / last row of a 4x4: must not be read
        views.append(dict(H=H, W=W, mask=mask, xyz=xyz, img=img, nrm=nrm, R=R,
                          dev=[torch.from_numpy(a).cuda() for a in (mask, xyz, img, nrm, Rbuf)]))
    total = sum(int(v["mask"].sum()) for v in views)
    cap = total + 5

    def run(with_normals, capacity):
        size = 27 if with_normals else 15
        records = torch.full((size * max(cap, 1),), 0xAB, dtype=torch.uint8, device="cuda")
        cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
        counts = torch.full((len(views),), -7, dtype=torch.int32, device="cuda")
        scratch = torch.zeros(64, dtype=torch.int64, device="cuda")
        for i, v in enumerate(views):
            m, x, im, n, Rd = v["dev"]
            if with_normals:
                rc = L.pmn_pack_points_normals(m.data_ptr(), x.data_ptr(), n.data_ptr(), Rd.data_ptr(), stride, im.data_ptr(),
                                               int(float_image), v["H"], v["W"], records.data_ptr(), capacity, cursor.data_ptr(),
                                               counts[i:].data_ptr(), scratch.data_ptr(), st)
            else:
                rc = L.pmn_pack_points(m.data_ptr(), x.data_ptr(), im.data_ptr(), int(float_image), v["H"], v["W"],
                                       records.data_ptr(), capacity, cursor.data_ptr(), counts[i:].data_ptr(), scratch.data_ptr(), st)
            assert rc == 0, rc
        torch.cuda.synchronize()
        return records.cpu().numpy(), int(cursor.item()), counts.cpu().numpy()

    plain, cur_p, cnt_p = run(False, cap)
    rich, cur_n, cnt_n = run(True, cap)
    assert cur_p == cur_n == total
    np.testing.assert_array_equal(cnt_p, cnt_n)
    np.testing.assert_array_equal(cnt_n, [int(v["mask"].sum()) for v in views])
    a = plain[:15 * total].reshape(total, 15)
    b = rich[:27 * total].reshape(total, 27)
    np.testing.assert_array_equal(b[:, :12], a[:, :12])
    np.testing.assert_array_equal(b[:, 24:], a[:, 12:])
    assert (rich[27 * total:] == 0xAB).all()  # nothing beyond the cursor
    got = np.ascontiguousarray(b[:, 12:24]).view("<f4").reshape(total, 3)
    want = []
    for v in views:
        keep = v["mask"].astype(bool)
        n = v["nrm"][:, keep]  # [3, k] row-major pixel order
        R = v["R"]
        want.append(np.stack([(R[k, 0] * n[0] + R[k, 1] * n[1]) + R[k, 2] * n[2] for k in range(3)], 1))
    want = np.concatenate(want).astype(np.float32)
    assert want.dtype == np.float32
    ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(np.abs(want), np.float32(1e-30)))
    print("pack normals: max deviation from float32 numpy", ulps.max(), "ulps; bit-equal:", np.array_equal(got, want))
    assert ulps.max() <= 2
    zero_in = np.concatenate([(v["nrm"][:, v["mask"].astype(bool)] == 0).all(0) for v in views])
    assert zero_in.any() and (got[zero_in] == 0).all()
    # does not fit: the third view overflows -- the first two are packed, the third writes nothing and reports -1
    small = total - 1
    rich2, cur2, cnt2 = run(True, small)
    first_two = int(cnt_n[0] + cnt_n[1])
    assert cur2 == first_two and list(cnt2) == [cnt_n[0], cnt_n[1], -1]
    np.testing.assert_array_equal(rich2[:27 * first_two], rich[:27 * first_two])
    assert (rich2[27 * first_two:] == 0xAB).all()


def _scan_truth(data, scan, out, with_r, tau):
    """Expected world normals of fused.ply's points, per view in pair-file order: inverse(E)[:3,:3] . oracle(depth_est, K) at the
    pixels of the final mask.  Returns (float64 expectation, the oracle's own float32-vs-float64 angle per point)."""
    from PIL import Image
    from patchmatchnet_amd import data_io
    exp, own = [], []
    for ref, _ in data_io.read_pair_file(os.path.join(data, scan, "pair.txt")):
        K, E, _ = data_io.read_cam_file(os.path.join(data, scan, "cams/{:0>8}_cam.txt".format(ref)))
        depth = data_io.read_map(os.path.join(out, scan, "depth_est/{:0>8}.pfm".format(ref)))[..., 0]
        final = np.array(Image.open(os.path.join(out, scan, "mask/{:0>8}_final.png".format(ref)))) > 0
        Ri = np.linalg.inv(E)[:3, :3]  # float32, as fusion.camera_block computes it
        n64 = NR.depth_normals_ref(depth, K, with_r, tau)[:, final]
        n32 = NR.depth_normals_ref(depth, K, with_r, tau, fit_dtype=np.float32)[:, final]
        w64 = Ri.astype(np.float64) @ n64
        w32 = np.stack([(Ri[k, 0] * n32[0] + Ri[k, 1] * n32[1]) + Ri[k, 2] * n32[2] for k in range(3)])
        exp.append(w64.T)
        own.append(np.where((n64 == 0).all(0), 0.0, NR.angle(w32, w64)))
    return np.concatenate(exp), np.concatenate(own)


def test_eval_normals_and_colmap_normal_maps_end_to_end(tmp_path):
    """eval.py --output_type both --normals 1 on the synthetic scan of tests/test_eval_gpu.py: 27-byte records whose x y z and colour
    columns, and every other file of the run, are byte-identical to a run without --normals; the normal columns are inverse(E)[:3,:3] .
    oracle(depth_est, K) under the angle gate; launch-plan replay and eager runs write the same file; eval_dtu's reader accepts it.  Then
    colmap_output.py --normal_maps on the results: one W&H&3& .geometric.bin per image of fusion.cfg, bit-equal to ops.depth_normals of
    the exported depth map, every other file of the workspace as without the flag."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    sys.path.insert(0, ROOT)
    import colmap_output
    import eval as pm_eval
    from patchmatchnet_amd import data_io, fusion, ops, pointcloud
    data = str(tmp_path / "data")
    synth.write_scan(data, "scan9", n_views=4, H=96, W=128, n_src=2)
    with open(os.path.join(data, "list.txt"), "w") as f:
        f.write("scan9\n")
    ckpt = os.path.join(GU.GOLDEN_DIR, "params_000007.npz")
    common = ["--input_folder", data, "--checkpoint_path", ckpt, "--scan_list", os.path.join(data, "list.txt"), "--num_views", "2",
              "--geo_mask_thres", "1", "--photo_thres", "0.1", "--num_workers", "0", "--sample_seed", "5", "--output_type", "both"]
    outs = {k: str(tmp_path / k) for k in ("plain", "normals", "eager", "r3")}
    pm_eval.main(common + ["--output_folder", outs["plain"]])
    pm_eval.main(common + ["--output_folder", outs["normals"], "--normals", "1"])
    pm_eval.main(common + ["--output_folder", outs["eager"], "--normals", "1", "--hip_graph", "0"])
    pm_eval.main(common + ["--output_folder", outs["r3"], "--normals", "1", "--normals_radius", "3", "--normals_depth_thres", "0.02"])
    n_files = 0
    for root, _, files in os.walk(outs["plain"]):
        for name in files:
            a = os.path.join(root, name)
            for other in ("normals", "eager", "r3"):
                b = os.path.join(outs[other], os.path.relpath(a, outs["plain"]))
                assert os.path.isfile(b), b
                if name != "fused.ply":
                    assert open(a, "rb").read() == open(b, "rb").read(), b
            n_files += 1
    assert n_files == 1 + 4 * 2 + 4 * 3
    plain = open(os.path.join(outs["plain"], "scan9", "fused.ply"), "rb").read()
    rich = open(os.path.join(outs["normals"], "scan9", "fused.ply"), "rb").read()
    assert rich == open(os.path.join(outs["eager"], "scan9", "fused.ply"), "rb").read()
    hp = plain.index(b"end_header\n") + 11
    hn = rich.index(b"end_header\n") + 11
    n = (len(plain) - hp) // 15
    assert n > 100 and len(plain) - hp == 15 * n and len(rich) - hn == 27 * n
    assert plain[:hp] == fusion.ply_header(n) and rich[:hn] == fusion.ply_header(n, normals=True)
    p = np.frombuffer(plain[hp:], fusion.PLY_VERTEX)
    q = np.frombuffer(rich[hn:], fusion.PLY_VERTEX_NORMALS)
    for k in ("x", "y", "z", "red", "green", "blue"):
        assert p[k].tobytes() == q[k].tobytes(), k
    xyz = pointcloud.read_ply_vertices(os.path.join(outs["normals"], "scan9", "fused.ply"))
    np.testing.assert_array_equal(xyz, np.stack((p["x"], p["y"], p["z"]), 1))
    for key, r, tau in (("normals", 2, 0.01), ("r3", 3, 0.02)):
        body = open(os.path.join(outs[key], "scan9", "fused.ply"), "rb").read()[hn:]
        q = np.frombuffer(body, fusion.PLY_VERTEX_NORMALS)
        got = np.stack((q["nx"], q["ny"], q["nz"]), 1).astype(np.float64)
        want, own = _scan_truth(data, "scan9", outs[key], r, tau)
        assert want.shape == got.shape
        zero = (want == 0).all(1)
        np.testing.assert_array_equal((got == 0).all(1), zero)
        assert (~zero).sum() > 50
        err = NR.angle(got[~zero].T, want[~zero].T)
        bound = 4 * own[~zero].max()
        print(f"fused.ply normals (r={r}, tau={tau}): {(~zero).sum()} of {len(zero)} points oriented, oracle f32-vs-f64 "
              f"{own[~zero].max():.3e} rad, file-vs-f64 {err.max():.3e} rad, bound {bound:.3e}")
        assert bound > 0 and err.max() <= bound
        assert np.abs(np.sqrt((got[~zero] ** 2).sum(1)) - 1).max() < 1e-6

    # ---- colmap_output.py --normal_maps ----
    src, res = os.path.join(data, "scan9"), os.path.join(outs["plain"], "scan9")
    ws0, ws1 = str(tmp_path / "ws_plain"), str(tmp_path / "ws_normals")
    os.makedirs(ws0)
    os.makedirs(ws1)
    colmap_output.main(["--input_folder", src, "--results_folder", res, "--output_folder", ws0])
    colmap_output.main(["--input_folder", src, "--results_folder", res, "--output_folder", ws1, "--normal_maps"])
    assert os.listdir(os.path.join(ws0, "stereo", "normal_maps")) == []
    listed = set()
    for ln in open(os.path.join(ws1, "stereo", "fusion.cfg")):
        listed |= {s.strip() for s in ln.split(",") if s.strip()}
    assert len(listed) == 4
    assert sorted(os.listdir(os.path.join(ws1, "stereo", "normal_maps"))) == sorted(im + ".geometric.bin" for im in listed)
    for im in listed:
        path = os.path.join(ws1, "stereo", "normal_maps", im + ".geometric.bin")
        assert open(path, "rb").read(8) == b"128&96&3"
        nm = data_io.read_bin(path)
        depth = data_io.read_bin(os.path.join(ws1, "stereo", "depth_maps", im + ".geometric.bin"))[..., 0]
        K, _, _ = data_io.read_cam_file(os.path.join(src, "cams", os.path.splitext(im)[0] + "_cam.txt"))
        want = ops.depth_normals(torch.from_numpy(np.ascontiguousarray(depth)).cuda(), K).permute(1, 2, 0).cpu().numpy()
        assert nm.shape == (96, 128, 3) and nm.tobytes() == want.tobytes()
        np.testing.assert_array_equal((nm == 0).all(2), (NR.depth_normals_ref(depth, K) == 0).all(0))
    for root, _, files in os.walk(ws0):
        for name in files:
            a = os.path.join(root, name)
            b = os.path.join(ws1, os.path.relpath(a, ws0))
            assert open(a, "rb").read() == open(b, "rb").read(), b
    extra = sum(len(f) for _, _, f in os.walk(ws1)) - sum(len(f) for _, _, f in os.walk(ws0))
    assert extra == 4
