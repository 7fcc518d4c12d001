"""CPU checks of the mesher: the numpy oracle (tests/tsdf_ref.py) against analytic shapes -- exact topological
conditions, measured distance figures asserted at 2 x -- the integration oracle against rendered planes and a sphere, the PLY mesh files,
choose_grid, and mesh.py's argument errors.  The kernels themselves are compared with the same oracle in tests/test_tsdf_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

import synth
import tsdf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from patchmatchnet_amd import PmnError, fusion, tsdf  # noqa: E402
from patchmatchnet_amd.pointcloud import read_ply_vertices  # noqa: E402

CENTRE = (19.3, 20.1, 19.7)
# max vertex-to-surface distance (voxels) of linear interpolation of the clipped distance field on the 40^3 lattice, measured with this
# oracle: sphere 0.0276, torus 0.0856.  Asserted at 2 x.
SPHERE_DIST, TORUS_DIST = 0.0276, 0.0856


def _sphere_dist(v, c=CENTRE, r=13.4):
    return np.abs(np.linalg.norm(v.astype(np.float64) - c, axis=1) - r)


def _torus_dist(v):
    v = v.astype(np.float64)
    q = np.sqrt((v[:, 0] - CENTRE[0]) ** 2 + (v[:, 1] - CENTRE[1]) ** 2) - 11.2
    return np.abs(np.sqrt(q * q + (v[:, 2] - CENTRE[2]) ** 2) - 4.3)


@pytest.mark.parametrize("shape", ["sphere", "torus"])
def test_oracle_closed_surfaces_are_exactly_closed(shape):
    if shape == "sphere":
        f, euler, dist, bound, analytic = R.sphere_field(40, CENTRE, 13.4), 2, _sphere_dist, SPHERE_DIST, 4 / 3 * np.pi * 13.4 ** 3
        counts = (10148, 20292)
    else:
        f, euler, dist, bound, analytic = R.torus_field(40, CENTRE, 11.2, 4.3), 0, _torus_dist, TORUS_DIST, 2 * np.pi ** 2 * 11.2 * 4.3 ** 2
        counts = (8266, 16532)
    m = R.extract(f, np.ones_like(f), (0, 0, 0), 1.0)
    t = R.topology(m["vertices"], m["faces"])
    print(shape, len(m["vertices"]), len(m["faces"]), t["euler"], t["volume"], analytic, dist(m["vertices"]).max())
    assert (len(m["vertices"]), len(m["faces"])) == counts
    assert t["closed"] and t["euler"] == euler and t["degenerate"] == 0 and t["unreferenced"] == 0
    assert 0.98 * analytic < t["volume"] < analytic  # outward winding; a chordal surface of a convex-ish body lies inside it
    assert dist(m["vertices"]).max() <= 2 * bound
    # the scan the kernels are given: popcount(vmask) and ntri sum to the element counts
    assert int(np.unpackbits(m["vmask"]).sum()) == len(m["vertices"]) and int(m["ntri"].sum()) == len(m["faces"])
    # normals: the normalised gradient points outward, along the radius for the sphere
    n = m["normals"].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
    if shape == "sphere":
        radial = (m["vertices"] - np.asarray(CENTRE)) / np.linalg.norm(m["vertices"] - np.asarray(CENTRE), axis=1)[:, None]
        assert (n * radial).sum(1).min() > 0.99


def test_oracle_zero_samples_still_close_the_surface():
    f = R.sphere_field(24, (12.0, 12.0, 12.0), 5.0)  # lattice-centred, integer radius: samples at exactly 0
    assert (f == 0).any()
    m = R.extract(f, np.ones_like(f), (0, 0, 0), 1.0, normals=False)
    t = R.topology(m["vertices"], m["faces"])
    assert t["closed"] and t["euler"] == 2 and t["unreferenced"] == 0


def test_oracle_half_observed_volume_is_open_only_at_dead_cells():
    f = R.sphere_field(40, CENTRE, 13.4)
    w = np.ones_like(f)
    w[:, :, 21:] = 0  # nothing observed beyond the plane x = 20
    m = R.extract(f, w, (0, 0, 0), 1.0, min_weight=1.0)
    t = R.topology(m["vertices"], m["faces"])
    assert not t["closed"] and len(t["boundary"]) > 0 and t["unreferenced"] == 0 and t["degenerate"] == 0 and t["max_edge_use"] == 2
    assert m["vertices"][:, 0].max() <= 20.0
    b = m["vertices"][np.unique(t["boundary"])]
    assert b[:, 0].min() >= 19.0  # every boundary vertex lies in the last live layer of cells, next to the dead ones
    # normals are zero exactly where a neighbour is unobserved or outside
    zero = (m["normals"] == 0).all(1)
    assert zero.any() and not zero.all()


def _scene(kind, dtype, colour=False):
    dims, voxel, trunc = (48, 44, 40), np.float32(0.05), np.float32(0.2)
    origin = np.array([-1.21, -1.13, 3.97], np.float32)
    target = origin.astype(np.float64) + np.array(dims) * float(voxel) / 2
    h, w = 96, 128
    K, E = R.rig(6, h, w, target, 4.0)
    if kind == "fronto":
        K, E = K[:1].repeat(4, 0), E[:1].repeat(4, 0).copy()
        E[:, :3, :3] = np.eye(3)
        E[:, :3, 3] = [0.1, -0.05, 0.0]
        E[:, 0, 3] += 0.07 * np.arange(4)
    nrm = np.array((0.3, -0.2, 0.93))
    centre = target + [0.011, 0.007, 0.4]
    vol = R.widen(R.new_volume(dims, color=colour), dtype)
    rng = np.random.default_rng(1)
    for v in range(len(K)):
        if kind == "fronto":
            d = R.render_plane(K[v], E[v], h, w, (0, 0, 1), target[2] + 0.013)
        elif kind == "tilted":
            d = R.render_plane(K[v], E[v], h, w, nrm, nrm @ target + 0.013)
        else:
            d = R.render_sphere(K[v], E[v], h, w, centre, 0.62)
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if colour else None
        R.integrate(vol, origin, voxel, trunc, d, R.cam21(K[v], E[v]), image=img, dtype=dtype)
    m = R.extract(vol["tsdf"], vol["weight"].astype(np.float32), origin, voxel, 1.0, normals=False, dtype=dtype)
    v = m["vertices"].astype(np.float64)
    if kind == "fronto":
        dist = np.abs(v[:, 2] - (target[2] + 0.013))
    elif kind == "tilted":
        dist = np.abs(v @ nrm - (nrm @ target + 0.013)) / np.linalg.norm(nrm)
    else:
        dist = np.abs(np.linalg.norm(v - centre, axis=1) - 0.62)
    return m, dist, vol


# measured with the float64 oracle on these scenes (voxel 0.05, trunc 0.2, 96 x 128 maps): the nearest-pixel
# lookup puts up to half a pixel of depth gradient into every sample.  Asserted at 2 x.
TILTED_DIST, SPHERE_SCENE_DIST = 0.00563, 0.0233


def test_integration_oracle_recovers_rendered_surfaces():
    m, dist, _ = _scene("fronto", np.float32)
    print("fronto-parallel plane: max distance", dist.max())
    assert len(m["faces"]) > 10000 and dist.max() <= 4 * np.spacing(np.float32(5.0))  # a linear field interpolates exactly
    for kind, bound in (("tilted", TILTED_DIST), ("sphere", SPHERE_SCENE_DIST)):
        m64, d64, _ = _scene(kind, np.float64)
        m32, d32, _ = _scene(kind, np.float32)
        print(kind, "max distance float64", d64.max(), "float32", d32.max())
        assert len(m64["faces"]) > 5000 and d64.max() <= 2 * bound and d32.max() <= 2 * bound
        assert np.array_equal(m32["faces"], m64["faces"])


def test_integration_oracle_counts_and_colour():
    _, _, vol = _scene("sphere", np.float32, colour=True)
    w, cw = vol["weight"], vol["cweight"]
    assert w.max() == 6 and (w == np.round(w)).all() and (cw <= w).all() and (cw < w).any() and cw.max() == 6
    assert (vol["tsdf"] <= 1).all() and (vol["tsdf"] >= -1).all() and ((vol["tsdf"] == 1) | (w > 0)).all()
    assert vol["rgb"].min() >= 0 and vol["rgb"].max() <= 255 and (vol["rgb"][:, cw == 0] == 0).all()


def test_ply_mesh_round_trip(tmp_path):
    f = R.sphere_field(16, (7.3, 8.1, 7.7), 4.4)
    m = R.extract(f, np.ones_like(f), (0.5, -1, 2), 0.25)
    rng = np.random.default_rng(0)
    col = rng.integers(0, 256, (len(m["vertices"]), 3), dtype=np.uint8)
    for colors, normals, size in ((col, m["normals"], 27), (col, None, 15), (None, m["normals"], 24), (None, None, 12)):
        path = str(tmp_path / "m.ply")
        tsdf.write_ply_mesh(path, m["vertices"], m["faces"], colors, normals)
        blob = open(path, "rb").read()
        head = tsdf.mesh_header(len(m["vertices"]), len(m["faces"]), colors is not None, normals is not None)
        assert blob.startswith(head) and len(blob) == len(head) + size * len(m["vertices"]) + 13 * len(m["faces"])
        assert b"element face %d\nproperty list uchar int vertex_indices\n" % len(m["faces"]) in head
        v, fc, c, n = tsdf.read_ply_mesh(path)
        assert v.tobytes() == m["vertices"].tobytes() and fc.dtype == np.int32 and np.array_equal(fc, m["faces"])
        assert (c is None) == (colors is None) and (n is None) == (normals is None)
        assert c is None or np.array_equal(c, colors)
        assert n is None or n.tobytes() == normals.tobytes()
        path2 = str(tmp_path / "m2.ply")
        tsdf.write_ply_mesh(path2, v, fc, c, n)
        assert open(path2, "rb").read() == blob  # byte for byte
        # the vertex block is what the cloud tools already read (eval_dtu.py scores a mesh's vertices); the reader is unchanged
        assert read_ply_vertices(path).tobytes() == m["vertices"].tobytes()
    # the vertex records are fusion's
    body = blob[len(head):len(head) + 12 * len(m["vertices"])]
    assert np.frombuffer(body, "<f4").reshape(-1, 3).tobytes() == m["vertices"].tobytes()
    tsdf.write_ply_mesh(path, m["vertices"], m["faces"], col, m["normals"])
    h27 = tsdf.mesh_header(len(col), len(m["faces"]), True, True)
    rec = np.frombuffer(open(path, "rb").read()[len(h27):len(h27) + 27 * len(col)], fusion.PLY_VERTEX_NORMALS)
    assert np.array_equal(rec["red"], col[:, 0]) and rec["nz"].tobytes() == np.ascontiguousarray(m["normals"][:, 2]).tobytes()
    with pytest.raises(ValueError):
        tsdf.write_ply_mesh(path, m["vertices"], m["faces"] + len(m["vertices"]))
    fusion.write_ply(path, m["vertices"], col)
    with pytest.raises(ValueError):
        tsdf.read_ply_mesh(path)  # a cloud is not a mesh


def test_choose_grid():
    g = torch.Generator().manual_seed(0)
    pts = torch.rand(20001, 3, generator=g) * torch.tensor([10.0, 20.0, 5.0]) + torch.tensor([-3.0, 100.0, 7.0])
    pts[:50] = 1e6  # outliers: the percentile box ignores them
    foot = torch.full((20001,), 0.05)
    origin, voxel, trunc, dims, note = tsdf.choose_grid(pts, foot)
    assert note is None and abs(voxel - 0.1) < 1e-6 and abs(trunc - 0.4) < 1e-6
    srt = torch.sort(pts, 0).values
    lo, hi = srt[200].numpy(), srt[19800].numpy()
    np.testing.assert_allclose(origin, lo - trunc, rtol=1e-6)
    for c in range(3):
        far = origin[c] + (dims[c] - 1) * voxel
        assert hi[c] + trunc <= far + 1e-4 < hi[c] + trunc + voxel + 1e-4
    # given voxel / trunc / bounds are taken as they are
    origin, voxel, trunc, dims, note = tsdf.choose_grid(None, None, voxel=0.5, trunc=1.0, bounds=(0, 0, 0, 10, 5, 2.2))
    assert note is None and tuple(origin) == (0, 0, 0) and (voxel, trunc) == (0.5, 1.0) and dims == (21, 11, 6)
    # --max_voxels: the voxel grows, trunc with it, and a line says so
    o2, v2, t2, d2, note = tsdf.choose_grid(pts, foot, max_voxels=100000)
    assert note is not None and "max_voxels" in note and v2 > 0.1 and abs(t2 - 4 * v2) < 1e-9 and d2[0] * d2[1] * d2[2] <= 100000
    assert d2[0] * d2[1] * d2[2] > 40000  # and no further than needed
    _, v3, t3, _, _ = tsdf.choose_grid(pts, foot, trunc=0.3, max_voxels=100000)
    assert t3 == 0.3 and v3 > 0.1  # a given trunc stays
    with pytest.raises(PmnError):
        tsdf.choose_grid(torch.zeros(0, 3), torch.zeros(0))
    with pytest.raises(PmnError):
        tsdf.choose_grid(pts, foot, bounds=(0, 0, 0, 1, 1, 0))


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    from patchmatchnet_amd import ops
    with pytest.raises(PmnError):
        tsdf.TsdfVolume((0, 0, 0), 1.0, (8, 8, 8), 4.0, "cpu")
    t, w = torch.ones(4, 4, 4), torch.zeros(4, 4, 4)
    with pytest.raises(PmnError):
        ops.mt_extract(t, w, (0, 0, 0), 1.0)
    with pytest.raises(PmnError):
        ops.tsdf_integrate(t, w, None, None, (0, 0, 0), 1.0, 4.0, torch.zeros(1, 16), [0], [(4, 4)], np.zeros((1, 21)))
    assert torch.equal(ops._popcount_u8(torch.arange(128, dtype=torch.uint8)),
                       torch.tensor([bin(i).count("1") for i in range(128)], dtype=torch.uint8))
    # the C entry points reject bad arguments before any HIP call
    from patchmatchnet_amd import _lib
    L = _lib.lib()
    assert L.pmn_tsdf_integrate(None, None, None, None, None, None, 1.0, 1.0, None, 1, None, None, None, None, None, 1, None) == -1
    assert L.pmn_mt_count(None, None, None, 1.0, None, None, None) == -1
    assert L.pmn_mt_emit(*([None] * 6), 1.0, 1.0, *([None] * 9)) == -1
    assert _lib.TSDF_MAX_VIEWS == 16 and "#define PMN_TSDF_MAX_VIEWS 16" in open(os.path.join(ROOT, "include", "pmn_hip.h")).read()


def test_mesh_py_argument_errors(tmp_path, monkeypatch, capsys):
    import mesh
    scan = synth.write_scan(str(tmp_path), "scanA", 3, 48, 64)
    with pytest.raises(PmnError, match="ROCm GPU"):
        mesh.main(["--input_folder", scan, "--device", "cpu"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert mesh.main(["--input_folder", scan]) == 2
    assert "torchrun" in capsys.readouterr().err and "torchrun" in mesh.build_parser().format_help()
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(Exception, match="Invalid input folder"):
        mesh.main(["--input_folder", str(tmp_path / "nope")])
    args = mesh.build_parser().parse_args(["--input_folder", str(tmp_path), "--results_folder", str(tmp_path)])
    with pytest.raises(PmnError, match=r"00000000_final\.png"):  # the missing masks are named before anything is read
        mesh._load_scan(args, "scanA", "cpu")
    args.mask = "none"
    with pytest.raises(PmnError, match="no depth map"):
        mesh._load_scan(args, "scanA", "cpu")
    with pytest.raises(PmnError, match="views_per_launch"):
        mesh.main(["--input_folder", scan, "--views_per_launch", "17"])
