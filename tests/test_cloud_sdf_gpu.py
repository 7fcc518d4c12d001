"""GPU checks of the signed distance from an oriented cloud (pmn_cloud_sdf_blocks, SparseTsdfVolume.allocate_points,
pointcloud.cloud_sdf / mesh_from_cloud, mesh_cloud.py) against tests/cloud_sdf_ref.py.

The pool planes tsdf, weight, rgb and cweight, read through to_dense, are compared BIT FOR BIT with the numpy model on every cloud and
every k: the kernel is float64 from float32 data in a stated order, so a difference is a contraction, an ordering or a search bug.
The meshes of mesh_from_cloud are compared with tsdf_ref.extract on the model's planes as sets of triangles with bit-equal vertex
records (tsdf_sparse_ref.assert_same_mesh: the pool's order of vertices and faces is not the dense lattice's),
and held to the distance bounds that tests/test_cloud_sdf_ref.py measured on the model (2 x its figures)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_sdf_ref as C
import knn_ref as K
import tsdf_ref as T
import tsdf_sparse_ref as S
from test_cloud_sdf_ref import BOUNDARY, PATCH_VERTEX_BOUND, SPHERE_POINT_BOUND, SPHERE_VERTEX_BOUND

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
KS = (1, 2, 8, 9, 16, 17, 32)  # across every capacity (8, 16, 32) and their edges


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _small(m, seed=31):
    """m points inside one block of the 65 x 5 x 9 lattice, with random normals and colours."""
    rng = np.random.default_rng(seed)
    return C.with_normals((rng.uniform(1.0, 4.0, (33, 3)) * [1.0, 0.9, 1.4] + [9.0, 0.0, 0.5]).astype(np.float32)[:m], seed + m)


def _clouds():
    """name -> (points, normals, colours, lattice origin, voxel, dims, trunc, radius, boundary)"""
    rng = np.random.default_rng(1)
    o = np.zeros(3, np.float32)
    lat = K.lattice_cloud()
    out = {"sphere": C.sphere()[:3] + (o, 1.0, (40, 40, 40), 3.0, 3.0, 1.5),
           # 37 x 41 x 45: blocks overhang the lattice on every axis; the 40 outliers are mostly alone in their neighbourhood
           "sheet": C.sheet() + (np.array([-2.0, -3.0, -30.0], np.float32), 1.7, (37, 41, 45), 2.5, 4.0, 2.0),
           # integer points, samples at half-integers: exact ties in d2 at every rank, samples that coincide with points (d2 = 0),
           # and points at exactly radius = 1.5 from a sample (no neighbours)
           "lattice": C.with_normals(lat, 41) + (np.array([-2.0, -2.0, -2.0], np.float32), 0.5, (23, 21, 19), 1.0, 1.5, 1.0),
           "duplicates": C.with_normals(K.duplicate_cloud(), 43) + (np.array([-4.0, -4.0, -4.0], np.float32), 0.4, (21, 21, 21), 0.9,
                                                                    0.8, 0.5),
           "one_block": C.with_normals((rng.uniform(0.0, 2.5, (90, 3)) + 9.5).astype(np.float32), 45) + (o + 8.0, 0.5, (9, 9, 9), 1.0,
                                                                                                        1.2, 0.8)}
    for m in (1, 2):  # 65 x 5 x 9: a lattice thinner than a block
        out[f"points_{m}"] = _small(m) + (o, 1.0, (65, 5, 9), 2.0, 3.0, 2.0)
    return out


def _case(PC, TS, name, spec, cell=None, grid_origin=None):
    pts, nrm, col, origin, voxel, dims, trunc, radius, boundary = spec
    grid = PC.build_grid(_dev(pts), radius if cell is None else cell, grid_origin)
    pos = np.empty(len(pts), np.int64)
    pos[grid.perm.cpu().numpy()] = np.arange(len(pts))  # original index -> sorted position: the tie order
    return {"name": name, "spec": spec, "grid": grid, "pos": pos, "points": _dev(pts), "normals": _dev(nrm), "colors": _dev(col, np.uint8)}


def _volume(TS, case, color=True):
    pts, nrm, col, origin, voxel, dims, trunc, radius, boundary = case["spec"]
    vol = TS.SparseTsdfVolume(origin, voxel, dims, trunc, DEV, color=color)
    vol.allocate_points(case["points"], radius)
    return vol


def _run(PC, TS, case, k, color=True):
    vol = _volume(TS, case, color)
    radius, boundary = case["spec"][7:9]
    PC.cloud_sdf(vol, case["grid"], case["normals"], case["colors"] if color else None, k=k, radius=radius, boundary=boundary)
    return vol


def _dense(vol):
    return [None if t is None else t.cpu().numpy() for t in vol.to_dense()]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_planes(got, ref, tag):
    for name, g, r in zip(("tsdf", "weight", "rgb", "cweight"), got, (ref["tsdf"], ref["weight"], ref["rgb"], ref["cweight"])):
        if g is None:
            continue
        diff = _bits(g) != _bits(r)
        assert not diff.any(), (tag, name, int(diff.sum()), g[diff][:4], r[diff][:4])


@pytest.fixture(scope="module")
def cases():
    """name -> case with the reference's 32 nearest of every lattice position, ties in the grid's sorted order: computed once, read by
    every k."""
    from patchmatchnet_amd import pointcloud as PC, tsdf as TS
    out = {}
    for name, spec in _clouds().items():
        c = _case(PC, TS, name, spec)
        pts, _, _, origin, voxel, dims, _, radius, _ = spec
        c["lists"] = C.neighbours(C.positions(origin, voxel, dims).reshape(-1, 3), pts, 32, radius, rank=c["pos"])
        out[name] = c
    return out


def _ref(case, k):
    pts, nrm, col, origin, voxel, dims, trunc, radius, boundary = case["spec"]
    return C.planes(pts, nrm, col, origin, voxel, dims, trunc, k, radius, boundary, lists=case["lists"])


@pytest.mark.parametrize("k", KS)
def test_planes_match_the_model_bit_for_bit(cases, k):
    from patchmatchnet_amd import pointcloud as PC, tsdf as TS
    seen = {}
    for name, case in cases.items():
        ref = _ref(case, k)
        vol = _run(PC, TS, case, k)
        got = _dense(vol)
        _assert_planes(got, ref, (name, k, "colour"))
        plain = _dense(_run(PC, TS, case, k, color=False))
        assert plain[2] is None and plain[3] is None
        _assert_planes(plain, ref, (name, k, "no colour"))
        # the blocks are the model's, and they hold every observed sample with a block to spare
        pts, _, _, origin, voxel, dims, _, radius, _ = case["spec"]
        have = C.allocated(pts, origin, voxel, dims, radius)
        assert np.array_equal(vol.blocks.cpu().numpy(), np.nonzero(have.reshape(-1))[0])
        assert not (S.dilate(S.block_any(ref["observed"])) & ~have).any()
        # pool planes of blocks without an observed sample, and the overhang of border blocks, stay as allocated
        w, t = vol.weight.cpu().numpy(), vol.tsdf.cpu().numpy()
        empty = ~(w > 0).any((1, 2, 3))
        assert (t[empty] == 1).all() and (w[empty] == 0).all() and (vol.cweight.cpu().numpy()[empty] == 0).all()
        assert (t[w == 0] == 1).all()
        seen[name] = (int(ref["observed"].sum()), int(ref["count"].max()))
    assert seen["sphere"][0] > 10000 and seen["sphere"][1] == k and seen["points_1"][1] == 1 and seen["points_2"][1] <= 2


@pytest.mark.parametrize("k", KS)
def test_clouds_of_k_and_k_plus_one_points(k):
    """k and k + 1 points in one neighbourhood: the list exactly full, and one point displaced."""
    from patchmatchnet_amd import pointcloud as PC, tsdf as TS
    for m in (k, k + 1):
        spec = _small(m) + (np.zeros(3, np.float32), 1.0, (65, 5, 9), 2.0, 7.0, 7.0)  # radius 7: every point in reach of the middle
        case = _case(PC, TS, f"points_{m}", spec)
        ref = C.planes(*spec[:3], *spec[3:7], k, spec[7], spec[8], rank=case["pos"])
        _assert_planes(_dense(_run(PC, TS, case, k)), ref, (m, k))
        assert ref["count"].max() == k


def test_exact_ties_coincident_samples_and_the_radius_itself(cases):
    """What the lattice cloud is for, shown on the model so that the bit comparison above is known to cover it."""
    case = cases["lattice"]
    idx, d2 = case["lists"]
    assert (d2[:, 0][idx[:, 0] >= 0] == 0).any()                      # a sample on a point
    full = idx[:, 7] >= 0
    assert (d2[full, 1] == d2[full, 2]).any() and (d2[full, 6] == d2[full, 7]).any()  # ties inside the list and at its end (k = 7 + 1)
    pts, _, _, origin, voxel, dims, _, radius, _ = case["spec"]
    x = C.positions(origin, voxel, dims).reshape(-1, 3)
    all_d2 = K.pair_d2(x.astype(np.float32), pts)
    assert (all_d2 == radius * radius).any() and not (d2[idx >= 0] >= radius * radius).any()  # at exactly radius: not a neighbour
    dup = cases["duplicates"]["lists"]
    assert ((dup[1][:, :-1] == dup[1][:, 1:]) & (dup[0][:, 1:] >= 0)).any()  # exact duplicates: equal d2, both kept


def test_bits_do_not_depend_on_the_search_grid_or_the_run(cases):
    """Clouds without exact ties (with ties the tie order is the grid's sorted order, by definition): another cell and another grid
    origin give the same bits, and so does a second run."""
    from patchmatchnet_amd import pointcloud as PC, tsdf as TS
    for name in ("sphere", "sheet"):
        base = cases[name]
        pts = base["spec"][0]
        first = _dense(_run(PC, TS, base, 16))
        again = _dense(_run(PC, TS, base, 16))
        lo = pts.min(0).astype(np.float64)
        for cell, origin in ((base["spec"][7] * 0.37, None), (base["spec"][7] * 1.9, (lo - [0.3, 0.7, 1.1]).tolist())):
            other = _dense(_run(PC, TS, _case(PC, TS, name, base["spec"], cell, origin), 16))
            for a, b in zip(first, other):
                assert np.array_equal(_bits(a), _bits(b)), (name, cell)
        for a, b in zip(first, again):
            assert np.array_equal(_bits(a), _bits(b)), name


def _mesh_case(PC, pts, nrm, col, **kw):
    v, f, c, n, info = PC.mesh_from_cloud(_dev(pts), _dev(nrm), _dev(col, np.uint8), voxel=1.0, radius=3.0, trunc=3.0, k=16,
                                          boundary=BOUNDARY, min_neighbors=3, **kw)
    got = (v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy(), n.cpu().numpy())
    grid = PC.build_grid(_dev(pts), 3.0)
    pos = np.empty(len(pts), np.int64)
    pos[grid.perm.cpu().numpy()] = np.arange(len(pts))
    pl = C.planes(pts, nrm, col, np.asarray(info["origin"], np.float32), info["voxel"], info["dims"], info["trunc"], 16, 3.0, BOUNDARY,
                  rank=pos)
    return got, C.mesh(pl, np.asarray(info["origin"], np.float32), info["voxel"], 3), info, pl


def test_mesh_of_the_sphere():
    from patchmatchnet_amd import pointcloud as PC
    pts, nrm, col, centre = C.sphere()
    got, want, info, pl = _mesh_case(PC, pts, nrm, col)
    S.assert_same_mesh(got, want, "sphere")
    v, f = got[:2]
    topo = T.topology(v, f)
    assert topo["closed"] and topo["euler"] == 2 and topo["degenerate"] == 0 and topo["volume"] > 0
    d = np.abs(np.linalg.norm(v.astype(np.float64) - centre, axis=1) - C.SPHERE_RADIUS)
    print(f"sphere: {len(v)} vertices, {len(f)} faces, largest vertex distance to the sphere {d.max():.4g} voxels; {info}")
    assert d.max() <= SPHERE_VERTEX_BOUND
    assert info["points"] == len(pts) and info["dropped"] == 0 and info["observed"] == int(pl["observed"].sum())
    assert info["vertices"] == len(v) and info["faces"] == len(f) and info["s"] is None and info["note"] is None


def test_mesh_of_the_patch_and_dropped_points():
    from patchmatchnet_amd import pointcloud as PC
    pts, nrm, col = C.patch()
    got, want, info, _ = _mesh_case(PC, pts, nrm, col)
    S.assert_same_mesh(got, want, "patch")
    v, f, _, n = got
    topo = T.topology(v, f)
    assert len(f) > 0 and not topo["closed"] and len(topo["boundary"]) > 0 and topo["degenerate"] == 0
    assert np.abs(C.patch_distance(v)).max() <= PATCH_VERTEX_BOUND
    assert np.maximum(np.maximum(C.PATCH_LO - v[:, :2], v[:, :2] - C.PATCH_HI), 0.0).max() <= BOUNDARY + 1.0
    vv = v.astype(np.float64)
    assert (np.cross(vv[f[:, 1]] - vv[f[:, 0]], vv[f[:, 2]] - vv[f[:, 0]]) @ C.PATCH_NORMAL > 0).all()
    assert (n[(n != 0).any(1)].astype(np.float64) @ C.PATCH_NORMAL > 0.99).all()
    # flipped normals: the mirrored winding
    flipped = PC.mesh_from_cloud(_dev(pts), _dev(-nrm), None, voxel=1.0, radius=3.0, k=16, boundary=BOUNDARY)
    fv, ff = flipped[0].cpu().numpy().astype(np.float64), flipped[1].cpu().numpy()
    assert flipped[2] is None and len(ff) == len(f) and (np.cross(fv[ff[:, 1]] - fv[ff[:, 0]], fv[ff[:, 2]] - fv[ff[:, 0]]) @ C.PATCH_NORMAL < 0).all()
    # degenerate points (zero or non-finite normals) are dropped and counted; what is left gives the same mesh
    extra = np.array([[15.0, 15.0, 12.0], [16.0, 15.0, 12.0], [17.0, 15.0, 12.0]], np.float32)
    bad = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [0.0, np.inf, 0.0]], np.float32)
    more = PC.mesh_from_cloud(_dev(np.concatenate([pts, extra])), _dev(np.concatenate([nrm, bad])),
                              _dev(np.concatenate([col, col[:3]]), np.uint8), voxel=1.0, radius=3.0, trunc=3.0, k=16, boundary=BOUNDARY)
    assert more[4]["dropped"] == 3 and more[4]["points"] == len(pts) + 3
    S.assert_same_mesh(tuple(t.cpu().numpy() for t in more[:4]), got, "dropped")
    # the defaults: s from the cloud, everything else from s
    auto = PC.mesh_from_cloud(_dev(pts), _dev(nrm), None, normals_out=False)[4]
    assert auto["s"] > 0 and auto["voxel"] == float(np.float32(auto["s"])) and auto["radius"] == 3.0 * auto["s"]
    assert auto["trunc"] == float(np.float32(auto["radius"])) and auto["boundary"] == auto["radius"] / 2 and auto["faces"] > 0


def test_argument_checks_raise_without_a_launch(cases):
    from patchmatchnet_amd import pointcloud as PC, tsdf as TS
    from patchmatchnet_amd._lib import PmnError
    case = cases["one_block"]
    grid, nrm, col = case["grid"], case["normals"], case["colors"]
    vol = _volume(TS, case)
    before = [t.clone() for t in (vol.tsdf, vol.weight, vol.rgb, vol.cweight)]
    n = nrm.shape[0]
    bad_calls = [dict(k=0), dict(k=33), dict(k=2.0), dict(k=True), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")),
                 dict(radius=float("nan")), dict(radius=1e200), dict(radius=1e-200), dict(boundary=0.0), dict(boundary=float("nan")),
                 dict(boundary=1e200), dict(normals=nrm.cpu()), dict(normals=nrm.double()), dict(normals=nrm[:-1]),
                 dict(normals=nrm[:, :2]), dict(normals=torch.full_like(nrm, float("nan"))), dict(colors=None), dict(colors=col.cpu()),
                 dict(colors=col.float()), dict(colors=col[:-1]), dict(grid=grid._replace(xyz=grid.xyz.cpu())), dict(volume=None),
                 dict(volume=TS.SparseTsdfVolume(np.zeros(3), 1.0, (9, 9, 9), 1.0, DEV))]  # not allocated
    for kw in bad_calls:
        args = dict(volume=vol, grid=grid, normals=nrm, colors=col, k=4, radius=1.2, boundary=0.8)
        args.update(kw)
        with pytest.raises(PmnError):
            PC.cloud_sdf(**args)
    with pytest.raises(PmnError):
        PC.cloud_sdf(_volume(TS, case, color=False), grid, nrm, col, k=4, radius=1.2, boundary=0.8)  # colours without planes
    for t, b in zip((vol.tsdf, vol.weight, vol.rgb, vol.cweight), before):
        assert torch.equal(t, b)
    # allocate_points
    fresh = TS.SparseTsdfVolume(np.zeros(3, np.float32) + 8.0, 0.5, (9, 9, 9), 1.0, DEV)
    for pts, reach in ((case["points"].cpu(), 1.0), (case["points"].double(), 1.0), (case["points"][:, :2], 1.0), (case["points"], 0.0),
                       (case["points"], 4.01), (case["points"], float("nan")), (case["points"] + 500.0, 1.0),
                       (torch.full_like(case["points"], float("inf")), 1.0)):
        with pytest.raises(PmnError):
            fresh.allocate_points(pts, reach)
    assert fresh.blocks is None or fresh.needed == 0
    with pytest.raises(PmnError, match="max_blocks"):
        TS.SparseTsdfVolume(np.zeros(3, np.float32) + 8.0, 0.5, (9, 9, 9), 1.0, DEV, max_blocks=1).allocate_points(case["points"], 1.0)
    # mesh_from_cloud
    p = case["points"]
    for kw in (dict(k=0), dict(min_neighbors=0), dict(min_neighbors=17), dict(voxel=0.0), dict(radius=float("nan")), dict(trunc=-1.0),
               dict(boundary=float("inf")), dict(normals=torch.zeros_like(nrm)), dict(normals=nrm[:-1]), dict(colors=col.float()),
               dict(voxel=0.1, radius=1.0)):  # radius > 8 voxels
        args = dict(points=p, normals=nrm, colors=col, voxel=0.5, radius=1.2)
        args.update(kw)
        with pytest.raises(PmnError):
            PC.mesh_from_cloud(**args)
    assert n == p.shape[0]


def _cli(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "mesh_cloud.py"), *argv], capture_output=True, text=True, cwd=ROOT,
                          timeout=600)


def test_command_line(tmp_path):
    from patchmatchnet_amd import meshops, ply, pointcloud as PC
    pts, nrm, col, centre = C.sphere()
    src = str(tmp_path / "cloud.ply")
    ply.write_ply(src, pts, col, nrm)
    dst, report = str(tmp_path / "out" / "mesh.ply"), str(tmp_path / "out" / "report.json")
    flags = ["--voxel", "1", "--radius", "3", "--trunc", "3", "--k", "16", "--boundary", str(BOUNDARY), "--min_neighbors", "3"]
    r = _cli("--input", src, "--output", dst, "--report", report, *flags)
    assert r.returncode == 0, r.stderr
    assert "3000 points read, 0 dropped" in r.stdout and "samples observed" in r.stdout and "faces ->" in r.stdout
    want = PC.mesh_from_cloud(_dev(pts), _dev(nrm), _dev(col, np.uint8), voxel=1.0, radius=3.0, trunc=3.0, k=16, boundary=BOUNDARY)
    got = ply.read_ply_mesh(dst)
    for g, w in zip(got, want[:4]):
        assert np.array_equal(g, w.cpu().numpy())
    rep = json.load(open(report))["files"][0]
    info = want[4]
    for key in ("points", "dropped", "s", "voxel", "radius", "trunc", "k", "blocks", "block_share", "observed", "vertices", "faces"):
        assert rep[key] == info[key], key
    # the true points of the sphere lie within the recorded bound of the written surface
    d = meshops.point_mesh_distance(_dev(pts), meshops.build_face_grid(_dev(got[0]), _dev(got[1], np.int32)), 5.0)
    print(f"written mesh: largest distance from a point of the cloud {float(d.max()):.4g} voxels")
    assert float(d.max()) <= SPHERE_POINT_BOUND
    # no colours, no normals, components
    r = _cli("--input", src, "--output", str(tmp_path / "bare.ply"), "--no_color", "--no_normals", "--keep_components", "1", *flags)
    assert r.returncode == 0, r.stderr
    bare = ply.read_ply_mesh(str(tmp_path / "bare.ply"))
    assert bare[2] is None and bare[3] is None and np.array_equal(bare[0], got[0]) and np.array_equal(bare[1], got[1])
    # a file without normals names cloud_normals.py
    plain = str(tmp_path / "plain.ply")
    ply.write_ply(plain, pts, col)
    r = _cli("--input", plain, "--output", str(tmp_path / "no.ply"))
    assert r.returncode == 2 and "cloud_normals.py" in r.stderr and not os.path.exists(tmp_path / "no.ply")
    # --scan_list: one file per scan
    for scan in ("scan1", "scan9"):
        ply.write_ply(str(tmp_path / "scans" / scan / "fused_normals.ply"), pts, col, nrm)
    (tmp_path / "list.txt").write_text("scan1\nscan9\n")
    r = _cli("--input", str(tmp_path / "scans"), "--scan_list", str(tmp_path / "list.txt"), *flags)
    assert r.returncode == 0, r.stderr
    for scan in ("scan1", "scan9"):
        one = ply.read_ply_mesh(str(tmp_path / "scans" / scan / "mesh_cloud.ply"))
        assert np.array_equal(one[0], got[0]) and np.array_equal(one[1], got[1])
