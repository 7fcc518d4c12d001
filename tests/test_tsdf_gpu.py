"""GPU checks of the mesher: pmn_tsdf_integrate, pmn_mt_count and pmn_mt_emit against the numpy oracle
(tests/tsdf_ref.py) on the same inputs, the exact topological conditions on the kernels' own output at 256^3, and mesh.py end to end.

Gates.  weight and cweight count decisions: equal everywhere, no allowance.  tsdf / rgb (and the vertex normals): at most 4 x the
largest difference between the oracle's OWN float32 and float64 evaluations of the same case (the rule of section 14: the yardstick is
what float32 costs the oracle, never the kernel's output); the measured kernel-vs-float32-oracle difference is printed (0 expected).
faces, the vertex count and the colour bytes: equal; positions within 2 float32 ulps."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import goldenutil as GU
import synth
import tsdf_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _views(dims, h, w, seed):
    """Five views of a sphere in front of a tilted plane (10 % invalid pixels, NaN / inf / negative depths), one view of another size,
    one camera behind the volume looking away.  -> origin, voxel, trunc, list of (depth, cam21, mask, image)."""
    rng = np.random.default_rng(seed)
    voxel = np.float32(2.4 / max(dims))
    trunc = np.float32(4 * voxel)
    origin = np.array([-1.21, -1.13, 3.97], np.float32)
    target = origin.astype(np.float64) + np.array(dims) * float(voxel) / 2
    K, E = R.rig(6, h, w, target, 4.0)
    nrm = np.array((0.3, -0.2, 0.93))
    views = []
    for v in range(7):
        hv, wv, Kv, Ev = h, w, K[min(v, 5)].copy(), E[min(v, 5)].copy()
        if v == 5:  # a view of another size
            hv, wv = max(h // 2, 8) + 1, max(w // 2, 8) + 3
            Kv[:2] *= 0.5
        if v == 6:  # behind the volume, looking away: every sample has pc.z <= 0
            Ev[:3, :3] = np.diag([1.0, -1.0, -1.0]) @ Ev[:3, :3]
            Ev[:3, 3] = np.diag([1.0, -1.0, -1.0]) @ Ev[:3, 3]
        ds = R.render_sphere(Kv, Ev, hv, wv, target + [0.011, 0.007, 0.1], 0.6)
        dp = R.render_plane(Kv, Ev, hv, wv, nrm, nrm @ target + 0.4)
        d = np.where(ds > 0, ds, dp).astype(np.float32)
        if v == 6:
            d[:] = 4.0
        bad = rng.random((hv, wv))
        d[bad < 0.10] = 0.0
        d[(bad >= 0.10) & (bad < 0.11)] = np.nan
        d[(bad >= 0.11) & (bad < 0.12)] = np.inf
        d[(bad >= 0.12) & (bad < 0.13)] = -d[(bad >= 0.12) & (bad < 0.13)] - 1
        mask = (rng.random((hv, wv)) > 0.05).astype(np.uint8) * 255
        image = rng.integers(0, 256, (hv, wv, 3), dtype=np.uint8)
        views.append((d, R.cam21(Kv, Ev), mask, image))
    return origin, voxel, trunc, views


def _upload(views, dev):
    stride = max(v[0].size for v in views)
    maps = torch.zeros((len(views), stride))
    for n, v in enumerate(views):
        maps[n, :v[0].size] = torch.from_numpy(v[0].reshape(-1))
    return (maps.to(dev), [v[0].shape for v in views], np.stack([v[1] for v in views]), [torch.from_numpy(v[2]).to(dev) for v in views],
            [torch.from_numpy(v[3]).to(dev) for v in views])


def _oracle_volume(dims, origin, voxel, trunc, views, masks, color, dtype):
    vol = R.widen(R.new_volume(dims, color=color), dtype)
    for d, cam, mask, image in views:
        R.integrate(vol, origin, voxel, trunc, d, cam, mask if masks else None, image if color else None, dtype=dtype)
    return vol


@pytest.mark.parametrize("dims,hw", [((17, 19, 23), (64, 64)), ((64, 64, 64), (250, 333)), ((160, 128, 96), (1200, 1600))])
@pytest.mark.parametrize("masks,color", [(True, True), (False, False)])
def test_tsdf_integrate_against_the_oracle(dims, hw, masks, color):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import tsdf
    dev = torch.device("cuda")
    origin, voxel, trunc, views = _views(dims, hw[0], hw[1], seed=dims[0])
    maps, sizes, cams, dmasks, dimages = _upload(views, dev)
    vol = tsdf.TsdfVolume(origin, voxel, dims, trunc, dev, color=color)
    vol.integrate(maps, list(range(len(views))), sizes, cams, dmasks if masks else None, dimages if color else None, batch=4)
    torch.cuda.synchronize()
    o32 = _oracle_volume(dims, origin, voxel, trunc, views, masks, color, np.float32)
    o64 = _oracle_volume(dims, origin, voxel, trunc, views, masks, color, np.float64)
    got = {"tsdf": vol.tsdf.cpu().numpy(), "weight": vol.weight.cpu().numpy()}
    if color:
        got["rgb"], got["cweight"] = vol.rgb.cpu().numpy(), vol.cweight.cpu().numpy()
    w = got["weight"]
    assert w.max() >= 5 and (w == 0).any(), "the case must have well-observed and unobserved samples"
    for k in ("weight", "cweight") if color else ("weight",):
        diff = int((got[k] != o32[k]).sum())
        print(f"{dims} {hw} masks={masks} color={color}: {k} differs from the float32 oracle in {diff} samples")
        assert diff == 0, k
    for k in ("tsdf", "rgb") if color else ("tsdf",):
        own = float(np.abs(o32[k].astype(np.float64) - o64[k]).max())
        err = float(np.abs(got[k].astype(np.float64) - o64[k]).max())
        vs32 = float(np.abs(got[k].astype(np.float64) - o32[k].astype(np.float64)).max())
        print(f"{dims} {hw} masks={masks} color={color}: {k} oracle f32-vs-f64 {own:.3e}, kernel-vs-f64 {err:.3e} (gate {4 * own:.3e}), "
              f"kernel-vs-f32-oracle {vs32:.3e}, bit-equal {got[k].tobytes() == o32[k].tobytes()}")
        assert err <= 4 * own, k
        # the same rule on the samples where the float32 and float64 oracles took the same decisions (a sample whose pixel or band test
        # flips between the two precisions dominates the figure above; without those it is rounding noise alone)
        same = o32["weight"].astype(np.float64) == o64["weight"]
        if k == "rgb":
            same = np.broadcast_to((same & (o32["cweight"].astype(np.float64) == o64["cweight"]))[None], got[k].shape)
        own_s = float(np.abs(o32[k].astype(np.float64) - o64[k])[same].max())
        err_s = float(np.abs(got[k].astype(np.float64) - o64[k])[same].max())
        print(f"    same-decision samples ({int(same.sum())} of {same.size}): oracle f32-vs-f64 {own_s:.3e}, kernel-vs-f64 {err_s:.3e}")
        assert err_s <= 4 * own_s, k


@pytest.mark.parametrize("V", [1, 3, 8, 9])
def test_batched_integration_equals_sequential(V):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import tsdf
    dev = torch.device("cuda")
    dims = (70, 45, 33)
    origin, voxel, trunc, views = _views(dims, 120, 160, seed=V)
    views = (views + views[:3])[:V] if V > len(views) else views[:V]
    maps, sizes, cams, dmasks, dimages = _upload(views, dev)
    a = tsdf.TsdfVolume(origin, voxel, dims, trunc, dev)
    b = tsdf.TsdfVolume(origin, voxel, dims, trunc, dev)
    a.integrate(maps, list(range(V)), sizes, cams, dmasks, dimages, batch=V)
    b.integrate(maps, list(range(V)), sizes, cams, dmasks, dimages, batch=1)
    assert float(a.weight.max()) >= min(V, 2)
    for k in ("tsdf", "weight", "cweight"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for ch in range(3):
        assert torch.equal(a.rgb[ch], b.rgb[ch]), ch


def _field(dims, kind):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    c = (nx / 2 - 0.7, ny / 2 + 0.1, nz / 2 - 0.3)
    s = min(dims) / 40.0
    if kind == "sphere":
        d = np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - 13.4 * s
    else:
        q = np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2) - 11.2 * s
        d = np.sqrt(q ** 2 + (k - c[2]) ** 2) - 4.3 * s
    return np.clip(d / 3.0, -1, 1).astype(np.float32)


def _compare_extraction(name, tsdf_np, weight_np, origin, voxel, min_weight, rgb=None, cweight=None, oracles=None, empty=False):
    """ops.mt_extract against the oracle under this file's gates -> (vertices, faces) of the kernels.  ``oracles`` = the (float32,
    float64) results of R.extract on these inputs where the caller has them already; ``empty``: the case has no surface, and the
    kernels must return empty outputs of the right shape, type and device (tests/test_mesher_space_gpu.py)."""
    from patchmatchnet_amd import ops
    dev = torch.device("cuda")
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)  # a contiguous copy: the rows' arrays are read-only
    v, f, c, n = ops.mt_extract(up(tsdf_np), up(weight_np), origin, voxel, min_weight, up(rgb), up(cweight), normals=True)
    torch.cuda.synchronize()
    o32, o64 = oracles or (R.extract(tsdf_np, weight_np, origin, voxel, min_weight, rgb, cweight, True, np.float32),
                           R.extract(tsdf_np, weight_np, origin, voxel, min_weight, rgb, cweight, True, np.float64))
    if empty:
        assert len(o32["faces"]) == 0 and len(o32["vertices"]) == 0, name
        for t, dtype in ((v, torch.float32), (f, torch.int32), (n, torch.float32)) + (((c, torch.uint8),) if rgb is not None else ()):
            assert tuple(t.shape) == (0, 3) and t.dtype == dtype and t.device.type == "cuda", (name, t.shape, t.dtype, t.device)
        assert (c is None) == (rgb is None), name
        print(f"{name}: no vertex, no face")
        return v.cpu().numpy(), f.cpu().numpy()
    v, f, n = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
    assert len(o32["faces"]) > 0, name
    assert v.shape == o32["vertices"].shape and f.shape == o32["faces"].shape, (name, v.shape, f.shape, o32["vertices"].shape)
    assert np.array_equal(f, o32["faces"]), name
    assert np.array_equal(np.isfinite(v), np.isfinite(o32["vertices"])), name
    ulp = np.spacing(np.maximum(np.abs(o32["vertices"]), np.float32(1e-30)))
    dpos = float((np.abs(v.astype(np.float64) - o32["vertices"]) / ulp).max())
    own = float(np.abs(o32["normals"].astype(np.float64) - o64["normals"]).max())
    err = float(np.abs(n.astype(np.float64) - o64["normals"]).max())
    print(f"{name}: {len(v)} vertices, {len(f)} faces equal; positions within {dpos:.2f} ulp (bit-equal "
          f"{v.tobytes() == o32['vertices'].tobytes()}); normals oracle f32-vs-f64 {own:.3e}, kernel-vs-f64 {err:.3e} (gate {4 * own:.3e}), "
          f"bit-equal {n.tobytes() == o32['normals'].tobytes()}")
    assert dpos <= 2.0, name
    assert np.array_equal((n == 0).all(1), (o32["normals"] == 0).all(1)), name
    assert err <= 4 * own, name
    if rgb is not None:
        assert np.array_equal(c.cpu().numpy(), o32["colors"]), name
    return v, f


def test_marching_tetrahedra_against_the_oracle():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    rng = np.random.default_rng(3)
    for kind in ("sphere", "torus"):
        f = R.sphere_field(40, (19.3, 20.1, 19.7), 13.4) if kind == "sphere" else R.torus_field(40, (19.3, 20.1, 19.7), 11.2, 4.3)
        v, fc = _compare_extraction(kind + " 40^3", f, np.ones_like(f), (0.0, 0.0, 0.0), 1.0, 1.0)
        t = R.topology(v, fc)
        assert t["closed"] and t["euler"] == (2 if kind == "sphere" else 0) and t["volume"] > 0
    # sides that are no multiples of the 64 x 4 block, an off-origin lattice, holes (weight below min_weight), colours with empty samples
    for dims in ((37, 41, 45), (65, 5, 9), (130, 23, 17)):
        f = _field(dims, "sphere")
        w = rng.integers(0, 4, f.shape).astype(np.float32)
        w[rng.random(f.shape) < 0.9] = 3
        rgb = rng.uniform(0, 255, (3,) + f.shape).astype(np.float32)
        cw = (rng.random(f.shape) > 0.2).astype(np.float32) * 2
        _compare_extraction(f"sphere {dims} with holes", f, w, (-3.25, 100.5, 0.125), 0.37, 2.0, rgb, cw)
    # an integrated volume
    dims = (48, 44, 40)
    origin, voxel, trunc, views = _views(dims, 96, 128, seed=9)
    vol = _oracle_volume(dims, origin, voxel, trunc, views[:5], True, True, np.float32)
    _compare_extraction("integrated volume", vol["tsdf"], vol["weight"], origin, voxel, 1.0, vol["rgb"], vol["cweight"])
    _compare_extraction("integrated volume, min_weight 3", vol["tsdf"], vol["weight"], origin, voxel, 3.0, vol["rgb"], vol["cweight"])


@pytest.mark.parametrize("kind", ["sphere", "torus"])
def test_kernel_surface_is_exactly_closed_at_256(kind):
    """The exact topological conditions on the kernels' own output, checked on the device (sort / unique, no Python loops)."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import ops
    dev = torch.device("cuda")
    n = 256
    ax = torch.arange(n, dtype=torch.float64, device=dev)
    k, j, i = torch.meshgrid(ax, ax, ax, indexing="ij")
    c = (127.3, 128.1, 126.7)
    if kind == "sphere":
        d = torch.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - 101.4
    else:
        q = torch.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2) - 80.2
        d = torch.sqrt(q ** 2 + (k - c[2]) ** 2) - 30.3
    del i, j, k
    t = torch.clamp(d / 3.0, -1, 1).float().contiguous()
    del d
    assert not bool((t == 0).any())
    v, f, _, nrm = ops.mt_extract(t, torch.ones_like(t), (0.0, 0.0, 0.0), 1.0)
    nv, nf = v.shape[0], f.shape[0]
    assert nv > 100000 and nf > 200000
    f = f.long()
    assert int(f.min()) == 0 and int(f.max()) == nv - 1
    assert torch.unique(f).numel() == nv                                                    # no unreferenced vertex
    assert not bool(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any())  # no degenerate triangle
    d = torch.cat((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    assert torch.unique(d[:, 0] * nv + d[:, 1]).numel() == d.shape[0]                       # every directed edge once
    und = torch.minimum(d[:, 0], d[:, 1]) * nv + torch.maximum(d[:, 0], d[:, 1])
    uk, cnt = torch.unique(und, return_counts=True)
    assert bool((cnt == 2).all())                                                           # every edge in exactly two triangles
    euler = nv - uk.numel() + nf
    vd = v.double()
    vol = float((vd[f[:, 0]] * torch.cross(vd[f[:, 1]], vd[f[:, 2]], dim=1)).sum() / 6.0)
    analytic = 4 / 3 * np.pi * 101.4 ** 3 if kind == "sphere" else 2 * np.pi ** 2 * 80.2 * 30.3 ** 2
    print(f"{kind} 256^3: {nv} vertices, {nf} faces, V - E + F = {euler}, volume {vol:.1f} / analytic {analytic:.1f}")
    assert euler == (2 if kind == "sphere" else 0)
    assert 0.995 * analytic < vol < analytic
    assert float((nrm.norm(dim=1) - 1).abs().max()) < 1e-5


def _run_mesh(args, cwd):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "mesh.py")] + args, cwd=cwd, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)  # a fresh process
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    return p.stdout


def _oracle_mesh(src, res, voxel, trunc, bounds, dtype, mask="final"):
    """The oracle fed the files mesh.py reads."""
    import argparse
    import eval as pm_eval
    from PIL import Image
    from patchmatchnet_amd import data_io, tsdf
    ids = [r for r, _ in data_io.read_pair_file(os.path.join(src, "pair.txt"))]
    cams, sizes = pm_eval._scan_cameras(argparse.Namespace(input_folder=src, image_max_dim=-1), "", ids)
    origin, voxel, trunc, dims, _ = tsdf.choose_grid(None, None, voxel, trunc, bounds)
    vol = R.widen(R.new_volume(dims, color=True), dtype)
    for v in ids:
        d = np.ascontiguousarray(data_io.read_map(os.path.join(res, "depth_est/{:0>8}.pfm".format(v))).squeeze(2), np.float32)
        m = np.array(Image.open(os.path.join(res, "mask/{:0>8}_final.png".format(v)))) if mask == "final" else None
        if m is not None:
            m = (m.reshape(m.shape[0], m.shape[1], -1)[..., 0] > 0).astype(np.uint8)
        img = data_io.read_image_u8(os.path.join(src, "images/{:0>8}.jpg".format(v)))
        R.integrate(vol, origin, voxel, trunc, d, tsdf.camera21(cams[v]["intrinsics"], cams[v]["extrinsics"]), m, img, dtype=dtype)
    wt = vol["weight"].astype(np.float32)
    cw = vol["cweight"].astype(np.float32)
    return R.extract(vol["tsdf"], wt, origin, voxel, 1.0, vol["rgb"], cw, True, dtype)


def _height_distance(v):
    X, Y = torch.from_numpy(v[:, 0].astype(np.float64)), torch.from_numpy(v[:, 1].astype(np.float64))
    z, fx, fy = synth.scene_height(X, Y)
    return (np.abs(v[:, 2].astype(np.float64) - z.numpy()) / np.sqrt(1 + fx.numpy() ** 2 + fy.numpy() ** 2))


def test_mesh_py_on_rendered_depth_maps(tmp_path):
    """A rendered scan with its TRUE depth maps as depth_est/*.pfm and all-ones final masks -> mesh.py in a child process: the file
    parses, faces / colours equal the oracle's on the same files, positions within 2 ulp, and the vertices lie on the analytic height
    field within 2 x what the float64 oracle reaches on those files."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from PIL import Image
    from patchmatchnet_amd import data_io, pointcloud, tsdf
    n, H, W = 5, 96, 128
    src = synth.write_scene_scan(str(tmp_path), "scene", n, H, W, n_src=2)
    _, _, _, depths = synth.render_scene(n, H, W, cameras=synth.arc_cameras(n, H, W), all_depths=True)
    res = str(tmp_path / "results")
    os.makedirs(os.path.join(res, "depth_est"))
    os.makedirs(os.path.join(res, "mask"))
    for v in range(n):
        data_io.save_pfm(os.path.join(res, "depth_est/{:0>8}.pfm".format(v)), depths[v].numpy().astype(np.float32))
        Image.fromarray(np.full((H, W), 255, np.uint8)).save(os.path.join(res, "mask/{:0>8}_final.png".format(v)))
    voxel, trunc, bounds = 5.0, 20.0, (-120.0, -90.0, 580.0, 120.0, 90.0, 720.0)
    out = _run_mesh(["--input_folder", src, "--results_folder", res, "--voxel", str(voxel), "--trunc", str(trunc), "--bounds"] +
                    [str(b) for b in bounds], str(tmp_path))
    assert "vertices" in out and "integrate" in out
    path = os.path.join(res, "mesh.ply")
    v, f, c, nrm = tsdf.read_ply_mesh(path)
    assert pointcloud.read_ply_vertices(path).tobytes() == v.tobytes()
    o32 = _oracle_mesh(src, res, voxel, trunc, bounds, np.float32)
    o64 = _oracle_mesh(src, res, voxel, trunc, bounds, np.float64)
    assert len(f) > 3000 and v.shape == o32["vertices"].shape and np.array_equal(f, o32["faces"]) and np.array_equal(c, o32["colors"])
    ulp = np.spacing(np.abs(o32["vertices"]))
    assert (np.abs(v.astype(np.float64) - o32["vertices"]) / ulp).max() <= 2
    d_k, d_64 = _height_distance(v), _height_distance(o64["vertices"])
    print(f"mesh.py on rendered maps: {len(v)} vertices, {len(f)} faces; distance to the height field: kernel max {d_k.max():.4f}, "
          f"float64 oracle max {d_64.max():.4f} (voxel {voxel})")
    assert d_k.max() <= 2 * d_64.max() and d_64.max() < voxel
    t = R.topology(v, f)
    assert t["unreferenced"] == 0 and t["degenerate"] == 0 and t["max_edge_use"] == 2 and t["directed_unique"]
    # default grid: sized from the data, the surface still comes out on the height field
    out2 = str(tmp_path / "auto")
    _run_mesh(["--input_folder", src, "--results_folder", res, "--output_folder", out2, "--no_color", "--views_per_launch", "3"],
              str(tmp_path))
    v2, f2, c2, n2 = tsdf.read_ply_mesh(os.path.join(out2, "mesh.ply"))
    assert c2 is None and n2 is not None and len(f2) > 1000
    assert np.median(_height_distance(v2)) < 1.0


def test_eval_then_mesh_py(tmp_path):
    """The real eval.py --output_type both -> mesh.py: counts, faces and colours equal the oracle fed the same result files (the engine's
    depth error is not this feature's to bound)."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    import eval as pm_eval
    from patchmatchnet_amd import tsdf
    data = str(tmp_path / "data")
    synth.write_scene_scan(data, "scan9", 5, 96, 128, n_src=2)
    with open(os.path.join(data, "list.txt"), "w") as fh:
        fh.write("scan9\n")
    out = str(tmp_path / "out")
    before = {}
    pm_eval.main(["--input_folder", data, "--checkpoint_path", os.path.join(GU.GOLDEN_DIR, "params_000007.npz"), "--scan_list",
                  os.path.join(data, "list.txt"), "--num_views", "3", "--geo_mask_thres", "1", "--photo_thres", "0.1", "--num_workers", "0",
                  "--sample_seed", "5", "--output_type", "both", "--output_folder", out])
    for root, _, files in os.walk(out):
        for name in files:
            before[os.path.join(root, name)] = open(os.path.join(root, name), "rb").read()
    voxel, trunc, bounds = 8.0, 32.0, (-120.0, -90.0, 500.0, 120.0, 90.0, 800.0)
    _run_mesh(["--input_folder", data, "--results_folder", out, "--scan_list", os.path.join(data, "list.txt"), "--voxel", str(voxel),
               "--trunc", str(trunc), "--bounds"] + [str(b) for b in bounds], str(tmp_path))
    for path, blob in before.items():
        assert open(path, "rb").read() == blob, path  # eval.py's outputs are untouched
    v, f, c, nrm = tsdf.read_ply_mesh(os.path.join(out, "scan9", "mesh.ply"))
    o32 = _oracle_mesh(os.path.join(data, "scan9"), os.path.join(out, "scan9"), voxel, trunc, bounds, np.float32)
    print(f"eval.py -> mesh.py: {len(v)} vertices, {len(f)} faces; oracle {len(o32['vertices'])}, {len(o32['faces'])}")
    assert len(f) > 0 and v.shape == o32["vertices"].shape and np.array_equal(f, o32["faces"]) and np.array_equal(c, o32["colors"])
