"""GPU checks of the renderer: pmn_raster_triangles, pmn_splat_points and pmn_raster_resolve against the numpy
oracle (tests/render_ref.py) on the same inputs, order independence and watertightness on the device, and render.py end to end.

Gates.  index and the covered set: equal to the float32 oracle on every pixel where the float32 and float64 oracles agree with each
other; the pixels left out are at most 1 % of the covered ones (a condition on the inputs, asserted).  depth and normal on those pixels:
at most 4 x the largest difference between the oracle's OWN float32 and float64 evaluations (the rule of sections 14 and 15); rgb: equal
bytes where the two oracles' bytes are equal.  Counters: equal to the oracle's counts.  The number of pixels where the kernel differs
from the float32 oracle in depth or index is printed and must be 0."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import goldenutil as GU
import render_ref as RR
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(240, 320), (600, 800), (1200, 1600)]


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check(name, got, o32, o64, r32, r64, counters, want_counters):
    """got = (depth, index, rgb, normal) host arrays of the kernels; o32 / o64 the oracles' dicts; r32 / r64 their (rgb, normal)."""
    depth, index, rgb, normal = got
    same, covered, excluded = RR.compare_oracles(o32, o64)
    differ = int(((index != o32["index"]) | (depth.view(np.uint32) != o32["depth"].astype(np.float32).view(np.uint32))).sum())
    print(f"{name}: covered {covered} px, float32 / float64 oracles disagree on {excluded} px ({100.0 * excluded / max(covered, 1):.4f} %), "
          f"kernel differs from the float32 oracle on {differ} px; counters {counters} (oracle {want_counters})")
    assert covered > 0 and excluded <= 0.01 * covered, name
    assert differ == 0, name  # section 16 states the arithmetic operation by operation: the float32 oracle's bytes on every pixel
    assert tuple(counters[:len(want_counters)]) == tuple(want_counters), name
    assert np.array_equal(index[same], o32["index"][same]), name
    hit = same & (o32["index"] >= 0)
    own = float(np.abs(o32["depth"].astype(np.float64) - o64["depth"])[hit].max())
    err = float(np.abs(depth.astype(np.float64) - o64["depth"])[hit].max())
    print(f"    depth: oracle f32-vs-f64 {own:.3e}, kernel-vs-f64 {err:.3e} (gate {4 * own:.3e}), bit-equal to the float32 oracle "
          f"{depth.tobytes() == o32['depth'].astype(np.float32).tobytes()}")
    assert err <= 4 * own, name
    if normal is not None:
        own = float(np.abs(r32[1].astype(np.float64) - r64[1])[hit].max())
        err = float(np.abs(normal.astype(np.float64) - r64[1])[hit].max())
        print(f"    normal: oracle f32-vs-f64 {own:.3e}, kernel-vs-f64 {err:.3e} (gate {4 * own:.3e}), bit-equal "
              f"{normal.tobytes() == r32[1].tobytes()}")
        assert err <= 4 * own, name
    if rgb is not None:
        eq = hit & (r32[0] == r64[0]).all(2)
        bad = int((rgb[eq] != r32[0][eq]).any(1).sum())
        print(f"    rgb: {int(eq.sum())} px with equal oracle bytes, kernel differs on {bad}; elsewhere on "
              f"{int((rgb[hit & ~eq] != r32[0][hit & ~eq]).any(1).sum())} of {int((hit & ~eq).sum())}")
        assert bad == 0, name
    assert (depth[index < 0] == 0).all() and (rgb is None or (rgb[index < 0] == 0).all())


def _mesh(kind, dev):
    from patchmatchnet_amd import ops
    if kind == "mt":
        from patchmatchnet_amd import tsdf
        field, origin, voxel = RR.mt_lattice(128)
        vol = tsdf.TsdfVolume(origin, float(voxel), field.shape[::-1], 4 * float(voxel), dev, color=False)
        vol.tsdf.copy_(_up(field, dev))  # an analytic field in place of integrated views: the triangles are the mesher's own
        vol.weight.fill_(1.0)
        v, f, _, n = vol.extract(1.0, normals=True)
        v, f, n = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
        return v, f, RR.case_attributes(v)[0], n, 4.0
    if kind == "ico":
        v, f = RR.icosphere(1, RR.TARGET, 1.2)
        return v, f, RR.case_attributes(v)[0], None, 2.4  # no vertex normals: the faces' own
    v, f = RR.icosphere(4, RR.TARGET, 1.0)
    col, n = RR.case_attributes(v)
    v2, f2 = RR.spoiled(v, f)
    col2, n2 = RR.case_attributes(v2, seed=1)
    return v2, f2, col2, n2, 4.0


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("kind", ["mt", "ico", "spoiled"])
def test_raster_triangles_against_the_oracle(kind, hw):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import render
    dev = torch.device("cuda")
    h, w = hw
    v, f, col, nrm, dist = _mesh(kind, dev)
    K, E, cam = RR.case_camera(h, w, dist)
    r = render.Renderer(dev)
    depth, index, rgb, normal, counters = r.render_mesh(_up(v, dev), _up(f, dev), K, E, h, w, _up(col, dev), _up(nrm, dev), shade=True,
                                                        rgb=True, normal=True)
    got = (depth.cpu().numpy(), index.cpu().numpy().astype(np.int64), rgb.cpu().numpy(), normal.cpu().numpy())
    counters = counters.tolist()
    o32 = RR.raster_triangles(v, f, cam, h, w, np.float32)
    o64 = RR.raster_triangles(v, f, cam, h, w, np.float64)
    r32 = RR.resolve(o32["depth"], o32["index"], cam, v, f, np.float32, col, nrm, True)
    r64 = RR.resolve(o32["depth"].astype(np.float64), o32["index"], cam, v, f, np.float64, col, nrm, True)
    _check(f"{kind} {w}x{h} ({len(f)} faces)", got, o32, o64, r32, r64, counters, o32["counters"])
    if kind == "ico":
        assert counters[3] > 0, "the coarse icosphere must take the worklist path"
    if kind == "spoiled":
        assert min(o32["counters"][0], o32["counters"][2]) > 0


@pytest.mark.parametrize("mode", ["nearest", "radius_px", "radius_world"])
def test_splat_points_against_the_oracle(mode):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import render
    dev = torch.device("cuda")
    h, w = 1200, 1600
    pts = RR.point_cloud(10 ** 7, RR.TARGET, seed=2)
    col, nrm = RR.case_attributes(pts, seed=3)
    K, E, cam = RR.case_camera(h, w)
    kw = {"nearest": {}, "radius_px": {"radius_px": 1.0}, "radius_world": {"radius_world": 0.0025}}[mode]
    r = render.Renderer(dev)
    depth, index, rgb, normal, counters = r.render_points(_up(pts, dev), K, E, h, w, _up(col, dev), _up(nrm, dev), shade=True, rgb=True,
                                                          normal=True, **kw)
    got = (depth.cpu().numpy(), index.cpu().numpy().astype(np.int64), rgb.cpu().numpy(), normal.cpu().numpy())
    counters = counters.tolist()
    o32 = RR.splat_points(pts, cam, h, w, np.float32, **kw)
    o64 = RR.splat_points(pts, cam, h, w, np.float64, **kw)
    r32 = RR.resolve(o32["depth"], o32["index"], cam, pts, None, np.float32, col, nrm, True)
    r64 = RR.resolve(o32["depth"].astype(np.float64), o32["index"], cam, pts, None, np.float64, col, nrm, True)
    assert o32["counters"][0] > 0
    _check(f"points {mode} {w}x{h}", got, o32, o64, r32, r64, counters, o32["counters"])


def test_order_independence_and_repeatability():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import render
    dev = torch.device("cuda")
    h, w = 600, 800
    g = torch.Generator().manual_seed(0)
    r = render.Renderer(dev)
    for kind in ("mt", "ico", "spoiled"):
        v, f, col, nrm, dist = _mesh(kind, dev)
        K, E, _ = RR.case_camera(h, w, dist)
        vd, fd = _up(v, dev), _up(f, dev)
        a = [t.clone() for t in r.render_mesh(vd, fd, K, E, h, w, _up(col, dev), None)[:3]]
        b = [t.clone() for t in r.render_mesh(vd, fd, K, E, h, w, _up(col, dev), None)[:3]]
        assert all(torch.equal(x, y) for x, y in zip(a, b)), kind  # two runs: identical bytes
        perm = torch.randperm(len(f), generator=g).to(dev)
        c = [t.clone() for t in r.render_mesh(vd, fd[perm].contiguous(), K, E, h, w, _up(col, dev), None)[:3]]
        assert torch.equal(a[0], c[0]) and torch.equal(a[2], c[2]), kind
        # indices mapped back: equal except among triangles of EQUAL depth at a pixel, where the lowest index wins in either order
        back = torch.where(c[1] >= 0, perm[c[1].clamp(min=0).long()].int(), c[1])
        ties = int((back != a[1]).sum())
        print(f"{kind}: permuted faces give the same depth and colour bytes; {ties} px won by another triangle of equal depth")
        assert ties <= 0.001 * int((a[1] >= 0).sum())
    pts = RR.point_cloud(10 ** 6, RR.TARGET, seed=5)
    K, E, _ = RR.case_camera(h, w)
    pd = _up(pts, dev)
    perm = torch.randperm(len(pts), generator=g).to(dev)
    for kw in ({}, {"radius_px": 2.5}):
        a = r.render_points(pd, K, E, h, w, **kw)[0].clone()
        b = r.render_points(pd, K, E, h, w, **kw)[0].clone()
        c = r.render_points(pd[perm].contiguous(), K, E, h, w, **kw)[0].clone()
        assert torch.equal(a, b) and torch.equal(a, c), kw


def _covering_grid(h, w, cells, offset, winding):
    """A fronto-parallel tessellated rectangle larger than the image, shifted by a sub-pixel offset, and its camera."""
    K = np.array([[100.0, 0, 0], [0, 100.0, 0], [0, 0, 1]], np.float32)
    E = np.eye(4, dtype=np.float32)
    z = 2.0
    x0, y0 = (-7.3 + offset[0]) * z / 100.0, (-5.9 + offset[1]) * z / 100.0
    v, f = RR.plane_grid(cells[0], cells[1], (x0, y0, z), ((w + 25.1) * z / 100.0, 0, 0.03), (0, (h + 22.7) * z / 100.0, 0.02),
                         winding, jitter=0.3, seed=cells[0])
    return v, f, K, E


@pytest.mark.parametrize("cells", [(16, 12), (200, 150)])
def test_watertightness_on_the_device(cells):
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import render, tsdf
    dev = torch.device("cuda")
    h, w = 240, 320
    r = render.Renderer(dev)
    rng = np.random.default_rng(7)
    for offset in [(0.0, 0.0)] + [tuple(rng.uniform(0, 1, 2)) for _ in range(3)]:
        for winding in (1, -1):
            v, f, K, E = _covering_grid(h, w, cells, offset, winding)
            depth, index, _, _, counters = r.render_mesh(_up(v, dev), _up(f, dev), K, E, h, w, rgb=False)
            o = RR.raster_triangles(v, f, tsdf.camera21(K, E), h, w, np.float32, count_hits=True)
            index = index.cpu().numpy()
            assert (o["hits"] == 1).all(), "the oracle must hit every pixel exactly once"
            assert (index >= 0).all() and np.array_equal(index, o["index"]), (cells, offset, winding)
            assert counters.tolist()[:3] == [0, 0, 0]
    print(f"{cells}: every pixel of {w}x{h} covered, index equal to the oracle's for 4 offsets x 2 windings")


def _run(script, args, cwd, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=timeout)  # a fresh process
    print(p.stdout[-4000:])
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout


def test_render_py_end_to_end(tmp_path):
    """synthetic scan -> its true depth maps -> mesh.py -> render.py: the rendered depth_gt agrees with the true depth within 2 x what
    the float64 oracle mesh drawn by the float64 oracle reaches; train.py --mode test accepts the files; the pictures are pictures;
    --orbit frames the model."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from PIL import Image
    from patchmatchnet_amd import data_io, render, tsdf
    from test_tsdf_gpu import _oracle_mesh
    n, H, W = 5, 96, 128
    data = str(tmp_path / "data")
    src = synth.write_scene_scan(data, "scene", n, H, W, n_src=2)
    with open(os.path.join(data, "list.txt"), "w") as fh:
        fh.write("scene\n")
    _, intr, extr, depths = synth.render_scene(n, H, W, cameras=synth.arc_cameras(n, H, W), all_depths=True)
    res = str(tmp_path / "results")
    os.makedirs(os.path.join(res, "scene", "depth_est"))
    os.makedirs(os.path.join(res, "scene", "mask"))
    for v in range(n):
        data_io.save_pfm(os.path.join(res, "scene", "depth_est/{:0>8}.pfm".format(v)), depths[v].numpy().astype(np.float32))
        Image.fromarray(np.full((H, W), 255, np.uint8)).save(os.path.join(res, "scene", "mask/{:0>8}_final.png".format(v)))
    voxel, trunc, bounds = 5.0, 20.0, (-120.0, -90.0, 580.0, 120.0, 90.0, 720.0)
    lst = os.path.join(data, "list.txt")
    _run("mesh.py", ["--input_folder", data, "--results_folder", res, "--scan_list", lst, "--voxel", str(voxel), "--trunc", str(trunc),
                     "--bounds"] + [str(b) for b in bounds], str(tmp_path))
    out = _run("render.py", ["--input_folder", data, "--scan_list", lst, "--model", os.path.join(res, "{scan}", "mesh.ply"),
                             "--output_folder", data, "--write", "depth_gt,masks,images,normals"], str(tmp_path))
    assert "kept" in out and "skipped" in out and "render" in out
    # (a) the bound: the float64 oracle mesh drawn by the float64 oracle, against the true depth
    o64 = _oracle_mesh(src, os.path.join(res, "scene"), voxel, trunc, bounds, np.float64)
    worst_oracle = worst = 0.0
    for v in range(n):
        true = depths[v].numpy().astype(np.float64)
        cam = tsdf.camera21(intr[0, v], extr[0, v])
        d64 = RR.raster_triangles(o64["vertices"].astype(np.float32), o64["faces"], cam, H, W, np.float64)["depth"]
        got = data_io.read_pfm(os.path.join(src, "depth_gt/{:0>8}.pfm".format(v)))[0].squeeze(2).astype(np.float64)
        assert (got > 0).mean() > 0.25 and ((got > 0) == (d64 > 0)).mean() > 0.995
        worst_oracle = max(worst_oracle, float(np.abs(d64 - true)[d64 > 0].max()))
        worst = max(worst, float(np.abs(got - true)[got > 0].max()))
        mask = np.array(Image.open(os.path.join(src, "masks/{:0>8}.png".format(v))))
        assert mask.shape == (H, W) and np.array_equal(mask > 0, got > 0)
        img = np.array(Image.open(os.path.join(src, "render/{:0>8}.png".format(v))))
        assert img.shape == (H, W, 3) and img.std() > 5
        nrm = data_io.read_bin(os.path.join(src, "normal_maps/{:0>8}.geometric.bin".format(v)))
        ln = np.linalg.norm(nrm[got > 0], axis=1)  # unit, or zero where the mesh's own vertex normals are zero (the volume's rim)
        assert nrm.shape == (H, W, 3) and (ln > 0).mean() > 0.9 and np.abs(ln[ln > 0] - 1).max() < 1e-5
        assert (nrm[got > 0][ln > 0][:, 2] < 0).all() and (nrm[got == 0] == 0).all()
    print(f"render.py depth_gt vs the true depth: kernel max {worst:.4f}, float64 oracle mesh + float64 oracle max {worst_oracle:.4f} "
          f"(voxel {voxel})")
    assert worst <= 2 * worst_oracle
    # (b) the validator accepts what this tool wrote
    out = _run("train.py", ["--mode", "test", "--input_folder", data, "--test_list", lst, "--checkpoint_path",
                            os.path.join(GU.GOLDEN_DIR, "params_000007.npz"), "--num_views", "3", "--batch_size", "2", "--num_workers", "0"],
               ROOT)
    assert any(ln.startswith("final {") for ln in out.splitlines()), out
    # --orbit
    orbit = str(tmp_path / "orbit")
    mesh_path = os.path.join(res, "scene", "mesh.ply")
    _run("render.py", ["--model", mesh_path, "--output_folder", orbit, "--orbit", "8", "--size", "120", "160", "--fov", "40"], str(tmp_path))
    v = tsdf.read_ply_mesh(mesh_path)[0]
    lo, hi = v.min(0), v.max(0)
    Ks, Es = render.orbit_cameras(np.concatenate((lo, hi)), 8, 120, 160, 40.0)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float64)
    for i in range(8):
        img = np.array(Image.open(os.path.join(orbit, "orbit/{:04d}.png".format(i))))
        assert img.shape == (120, 160, 3) and img.std() > 5
        pc = corners @ Es[i][:3, :3].astype(np.float64).T + Es[i][:3, 3]
        q = pc @ Ks[i].astype(np.float64).T
        u, vv = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        assert (pc[:, 2] > 0).all() and u.min() >= 0 and u.max() <= 159 and vv.min() >= 0 and vv.max() <= 119, i
        drawn = img.any(2)
        assert not (drawn[0].any() or drawn[-1].any() or drawn[:, 0].any() or drawn[:, -1].any()), i
    assert sorted(os.listdir(os.path.join(orbit, "orbit"))) == ["{:04d}.png".format(i) for i in range(8)]


def test_wrappers_refuse_what_the_library_would():
    """The checks of ops.py that need device tensors to be reached: each call has one bad argument and must raise before any launch."""
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    from patchmatchnet_amd import PmnError, _lib, ops, render
    dev = torch.device("cuda")
    v, f = RR.icosphere(0, RR.TARGET, 1.0)
    vd, fd = _up(v, dev), _up(f, dev)
    _, _, cam = RR.case_camera(8, 8)
    keys = torch.full((8, 8), -1, dtype=torch.int64, device=dev)
    cnt, wl = torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(len(f), dtype=torch.int32, device=dev)
    depth, index = torch.zeros((8, 8), device=dev), torch.zeros((8, 8), dtype=torch.int32, device=dev)
    ops.raster_triangles(vd, fd, cam, keys, cnt, wl)  # the good call passes
    ops.raster_resolve(keys, cam, vd, fd, depth, index)
    bad_cam = cam.copy()
    bad_cam[5] = np.nan
    for call in (lambda: ops.raster_triangles(vd, fd, cam, keys, cnt, wl[:-1]),                      # a short worklist
                 lambda: ops.raster_triangles(vd, fd, cam, keys, cnt, wl, max_box=-1),
                 lambda: ops.raster_triangles(vd, fd, bad_cam, keys, cnt, wl),
                 lambda: ops.raster_triangles(vd, fd.long(), cam, keys, cnt, wl),
                 lambda: ops.raster_triangles(vd, fd, cam, keys.int(), cnt, wl),
                 lambda: ops.raster_triangles(vd, fd, cam, keys, cnt[:3], wl),
                 lambda: ops.raster_triangles(vd, fd, cam, torch.zeros((_lib.RASTER_MAX_DIM + 1, 1), dtype=torch.int64, device=dev), cnt, wl),
                 lambda: ops.splat_points(vd, cam, keys, cnt, radius_px=_lib.SPLAT_MAX_RADIUS + 1),
                 lambda: ops.splat_points(vd, cam, keys, cnt, radius_px=1.0, radius_world=1.0),
                 lambda: ops.splat_points(vd, cam, keys, cnt, radius_world=-1.0),
                 lambda: ops.splat_points(vd.cpu(), cam, keys, cnt),
                 lambda: ops.raster_resolve(keys, cam, vd, fd, depth[:4], index),
                 lambda: ops.raster_resolve(keys, cam, vd, fd, depth, index, colors=torch.zeros((len(v) + 1, 3), dtype=torch.uint8, device=dev)),
                 lambda: ops.raster_resolve(keys, cam, vd, fd, depth, index, rgb=torch.zeros((8, 8, 3), device=dev)),
                 lambda: render.Renderer(dev).render_mesh(vd, f, np.eye(3), np.eye(4), 8, 8),      # faces on the host
                 lambda: render.Renderer(dev).render_mesh(vd, fd, np.eye(3), np.eye(4), 0, 8)):
        with pytest.raises(PmnError):
            call()
