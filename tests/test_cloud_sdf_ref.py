"""CPU checks of tests/cloud_sdf_ref.py, the numpy statement of the signed distance from an oriented cloud (pmn_cloud_sdf_blocks), on
analytic shapes, and of the parts of the feature that need no GPU: the declaration, the block marking and mesh_cloud.py's arguments.

The distances the model reaches here are what tests/test_cloud_sdf_gpu.py bounds the kernel's own meshes by: the bounds there are the
constants below, 2 x what this model measures (DESIGN.md section 15's rule), and this file asserts that the model stays inside them."""
import os
import sys

import numpy as np
import pytest

import cloud_sdf_ref as C
import tsdf_ref as T
import tsdf_sparse_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS = (40, 40, 40)
VOXEL, RADIUS, TRUNC, BOUNDARY, KNN, MIN_NEIGHBORS = 1.0, 3.0, 3.0, 1.5, 16, 3
PATCH_DIMS = (37, 41, 24)  # not multiples of 8: blocks overhang the lattice

# Bounds on distances, in voxels: 2 x the model's own figures, printed by the tests below (pytest -s).
SPHERE_VERTEX_BOUND = 2 * 0.0997   # measured: the largest |distance of a vertex to the sphere| is 0.09935 (lattice at 0 and shifted), 0.09969 (chosen lattice); mean 0.043
SPHERE_POINT_BOUND = 2 * 0.0673    # measured: the largest exact distance from a point of the cloud to the mesh is 0.06584 / 0.06724 (mean 0.031)
PATCH_VERTEX_BOUND = 2 * 6.48e-7   # measured: the largest distance of a vertex to the patch's plane is 6.47e-7 / 6.27e-7: float32 rounding of positions near 28


def _chosen_lattice(pts):
    """(origin, dims) of the lattice pointcloud.mesh_from_cloud picks for this cloud at voxel 1, radius 3: tsdf.choose_grid, which is
    plain torch and runs on the host.  The GPU test meshes on it, so the bounds are measured on it too."""
    import torch
    from patchmatchnet_amd import ops, tsdf
    origin, voxel, _, dims, note = tsdf.choose_grid(torch.from_numpy(np.ascontiguousarray(pts)), voxel=VOXEL, trunc=RADIUS,
                                                    max_voxels=tsdf.MAX_VIRTUAL_VOXELS, limit_name="the virtual lattice's",
                                                    max_axis=ops.SPARSE_MAX_AXIS - 1)
    assert note is None and voxel == VOXEL
    return origin, dims


def _sphere_planes(shift, chosen=False):
    pts, nrm, col, centre = C.sphere(shift=tuple(shift))
    origin, dims = _chosen_lattice(pts) if chosen else (np.asarray(shift, np.float32), DIMS)
    pl = C.planes(pts, nrm, col, origin, VOXEL, dims, TRUNC, KNN, RADIUS, BOUNDARY)
    return pts, centre, origin, pl


@pytest.fixture(scope="module")
def sphere_meshes():
    out = {}
    for name, shift in (("origin", (0.0, 0.0, 0.0)), ("shifted", tuple(C.FAR)), ("chosen", (0.0, 0.0, 0.0))):
        pts, centre, origin, pl = _sphere_planes(shift, name == "chosen")
        out[name] = (pts, centre, origin, pl, C.mesh(pl, origin, VOXEL, MIN_NEIGHBORS))
    return out


@pytest.mark.parametrize("name", ["origin", "shifted", "chosen"])
def test_sphere_is_closed_and_on_the_sphere(sphere_meshes, name):
    pts, centre, origin, pl, (v, f, col, nrm) = sphere_meshes[name]
    topo = T.topology(v, f)
    assert topo["closed"] and topo["euler"] == 2 and topo["degenerate"] == 0 and topo["unreferenced"] == 0
    assert topo["volume"] > 0  # wound outwards: the side the normals point to
    d = np.abs(np.linalg.norm(v.astype(np.float64) - centre, axis=1) - C.SPHERE_RADIUS)
    print(f"sphere ({name}): {len(v)} vertices, {len(f)} faces, {int(pl['observed'].sum())} samples observed, "
          f"largest vertex distance to the sphere {d.max():.4g} voxels, mean {d.mean():.4g}")
    assert d.max() <= SPHERE_VERTEX_BOUND
    # the mesher's normals point outwards; colours are blends of the points' colours
    out = (v.astype(np.float64) - centre) / np.linalg.norm(v.astype(np.float64) - centre, axis=1, keepdims=True)
    has = (nrm != 0).any(1)  # no normal where a neighbour of the edge's ends is unobserved
    assert has.mean() > 0.99 and ((nrm.astype(np.float64) * out).sum(1)[has] > 0.99).all()
    assert col is not None and col.shape == v.shape


def test_shifted_sphere_has_the_same_topology(sphere_meshes):
    a, b = (T.topology(*sphere_meshes[n][4][:2]) for n in ("origin", "shifted"))
    assert (a["closed"], a["euler"], a["degenerate"]) == (b["closed"], b["euler"], b["degenerate"]) == (True, 2, 0)


def _patch_mesh(flip, chosen=False):
    pts, nrm, col = C.patch()
    origin, dims = _chosen_lattice(pts) if chosen else (np.zeros(3, np.float32), PATCH_DIMS)
    pl = C.planes(pts, -nrm if flip else nrm, col, origin, VOXEL, dims, TRUNC, KNN, RADIUS, BOUNDARY)
    return pts, pl, C.mesh(pl, origin, VOXEL, MIN_NEIGHBORS)


def _face_normals(v, f):
    v = v.astype(np.float64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


@pytest.mark.parametrize("chosen", [False, True])
def test_patch_is_one_open_sheet(chosen):
    pts, pl, (v, f, col, nrm) = _patch_mesh(False, chosen)
    topo = T.topology(v, f)
    assert len(f) > 0 and not topo["closed"] and len(topo["boundary"]) > 0 and topo["degenerate"] == 0
    assert topo["max_edge_use"] <= 2 and topo["directed_unique"]
    dz = np.abs(C.patch_distance(v))
    outside = np.maximum(np.maximum(C.PATCH_LO - v[:, :2], v[:, :2] - C.PATCH_HI), 0.0).max()
    print(f"patch (chosen lattice {chosen}): {len(v)} vertices, {len(f)} faces, {len(topo['boundary'])} boundary edges, largest distance to the plane {dz.max():.3g}, "
          f"furthest vertex outside the square {outside:.4g} voxels")
    assert dz.max() <= VOXEL and dz.max() <= PATCH_VERTEX_BOUND  # one sheet, not two
    assert outside <= BOUNDARY + VOXEL
    assert (_face_normals(v, f) @ C.PATCH_NORMAL > 0).all()
    assert (nrm[(nrm != 0).any(1)].astype(np.float64) @ C.PATCH_NORMAL > 0.99).all()
    # the sheet covers the square's inside: every lattice column well inside it crosses the mesh
    assert v[:, 0].min() < C.PATCH_LO + VOXEL and v[:, 0].max() > C.PATCH_HI - VOXEL


def test_flipped_normals_mirror_the_winding():
    _, _, (v, f, _, _) = _patch_mesh(False)
    _, _, (vf, ff, _, nf) = _patch_mesh(True)
    assert (_face_normals(vf, ff) @ C.PATCH_NORMAL < 0).all() and (nf[(nf != 0).any(1)].astype(np.float64) @ C.PATCH_NORMAL < -0.99).all()
    # the same surface: the vertices agree as sets (f is negated exactly, so the crossings are the same edges at the same parameter)
    assert len(vf) == len(v) and len(ff) == len(f)
    key = lambda a: a[np.lexsort(a.T[::-1])]
    assert np.allclose(key(v), key(vf), rtol=0, atol=1e-5)


def test_point_to_mesh_bound_of_the_model(sphere_meshes):
    """The figure behind SPHERE_POINT_BOUND: the exact distance from every point of the cloud (they lie on the sphere) to the
    model's mesh, the quantity meshops.point_mesh_distance reports for the written file in the GPU test."""
    for name in ("origin", "chosen"):
        pts, centre, origin, pl, (v, f, _, _) = sphere_meshes[name]
        d = _point_mesh(pts.astype(np.float64), v.astype(np.float64), f)
        print(f"sphere ({name}): largest distance from a true point to the mesh {d.max():.4g} voxels, mean {d.mean():.4g}")
        assert d.max() <= SPHERE_POINT_BOUND


def _point_mesh(p, v, f, near=64):
    """Exact distance from points to a triangle mesh, brute force over the ``near`` triangles with the nearest centroids (Ericson's
    closest point on a triangle, vectorised)."""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cen = (a + b + c) / 3.0
    out = np.empty(len(p))
    for s in range(0, len(p), 256):
        q = p[s:s + 256]
        idx = np.argsort(((q[:, None] - cen[None]) ** 2).sum(-1), axis=1)[:, :near]
        A, B, Cc = a[idx], b[idx], c[idx]
        Q = q[:, None]
        ab, ac, ap = B - A, Cc - A, Q - A
        d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
        bp = Q - B
        d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
        cp = Q - Cc
        d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        with np.errstate(all="ignore"):
            den = 1.0 / (va + vb + vc)
            vv, ww = vb * den, vc * den
            inside = A + ab * vv[..., None] + ac * ww[..., None]
            t_ab = (d1 / (d1 - d3))[..., None]
            t_ac = (d2 / (d2 - d6))[..., None]
            t_bc = ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None]
        cl = inside
        cl = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], B + (Cc - B) * t_bc, cl)
        cl = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], A + ac * t_ac, cl)
        cl = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], A + ab * t_ab, cl)
        cl = np.where(((d6 >= 0) & (d5 <= d6))[..., None], Cc, cl)
        cl = np.where(((d3 >= 0) & (d4 <= d3))[..., None], B, cl)
        cl = np.where(((d1 <= 0) & (d2 <= 0))[..., None], A, cl)
        out[s:s + 256] = np.sqrt(((Q - cl) ** 2).sum(-1)).min(1)
    return out


def test_allocated_blocks_cover_the_observed_samples(sphere_meshes):
    """allocate_points' rule (cloud_sdf_ref.mark_points + the dilation; the GPU test holds the product to it) against the brute-force
    set: the blocks that hold an observed sample, dilated."""
    cases = [(sphere_meshes["origin"][0], np.zeros(3, np.float32), DIMS, sphere_meshes["origin"][3]),
             (sphere_meshes["shifted"][0], C.FAR.astype(np.float32), DIMS, sphere_meshes["shifted"][3])]
    pts, pl, _ = _patch_mesh(False)
    cases.append((pts, np.zeros(3, np.float32), PATCH_DIMS, pl))
    for pts, origin, dims, pl in cases:
        need = S.dilate(S.block_any(pl["observed"]))
        have = C.allocated(pts, origin, VOXEL, dims, RADIUS)
        assert have.shape == need.shape and not (need & ~have).any()
    # a cloud outside the lattice marks nothing; a reach of 8 voxels spans three blocks and the dilation closes the gap
    assert not C.mark_points(np.array([[500.0, 0.0, 0.0]], np.float32), np.zeros(3), VOXEL, DIMS, RADIUS).any()
    wide = C.allocated(np.array([[20.0, 20.0, 20.0]], np.float32), np.zeros(3), VOXEL, DIMS, 8.0)
    assert wide[1:4, 1:4, 1:4].all()


def test_weights_and_boundary_rule_on_hand_made_samples():
    """One point at the origin with normal +z, voxel 1, radius 3: the values follow from the definition by hand."""
    pts = np.array([[4.0, 4.0, 4.0]], np.float32)
    nrm = np.array([[0.0, 0.0, 1.0]], np.float32)
    col = np.array([[10, 20, 30]], np.uint8)
    pl = C.planes(pts, nrm, col, np.zeros(3, np.float32), 1.0, (9, 9, 9), 2.0, 4, 3.0, 1.5)
    assert pl["observed"][4, 4, 4] and pl["tsdf"][4, 4, 4] == 0 and pl["weight"][4, 4, 4] == 1   # the point itself: d2 = 0, f = 0
    assert pl["tsdf"][5, 4, 4] == np.float32(0.5) and pl["tsdf"][2, 4, 4] == np.float32(-1.0)     # one above: 1 / trunc; two below: clamped
    assert not pl["observed"][4, 4, 7] and not pl["observed"][7, 4, 4]                            # at exactly radius: no neighbour
    assert pl["observed"][4, 4, 5] and not pl["observed"][4, 4, 6]                                # along the plane: 1 <= 1.5 < 2
    assert pl["observed"][6, 4, 5] and not pl["observed"][6, 4, 6]                                # two above: t2 = 1, and t2 = 4 > 2.25
    assert (pl["rgb"][:, 5, 4, 4] == [10, 20, 30]).all() and pl["cweight"][5, 4, 4] == 1
    assert pl["tsdf"][~pl["observed"]].min() == 1 and pl["weight"][~pl["observed"]].max() == 0


def test_header_and_table_declare_the_entry():
    from patchmatchnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pmn_hip.h")).read()
    assert "int pmn_cloud_sdf_blocks(" in hdr and len(_lib.SIGNATURES["pmn_cloud_sdf_blocks"]) == 22
    assert _lib.ABI_VERSION == 25


def test_entry_refuses_bad_arguments_without_a_launch():
    """Host-side checks only: every call below returns before any HIP call (safe without a GPU).  Pointers are never dereferenced."""
    import ctypes
    from patchmatchnet_amd import _lib
    L = _lib.lib()
    org, dims = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_int * 3)(4, 4, 4)
    vorg, vdims = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_int * 3)(16, 16, 16)
    P = 4096  # a non-null address that no check reads

    def call(xyz=P, keys=P, n=10, cell=1.0, normals=P, colors=None, blocks=P, nb=2, vd=vdims, vo=vorg, voxel=1.0, trunc=3.0, k=16,
             radius=3.0, boundary=1.5, tsdf=P, weight=P, rgb=None, cweight=None):
        return L.pmn_cloud_sdf_blocks(xyz, keys, n, org, cell, dims, normals, colors, blocks, nb, vd, vo, voxel, trunc, k, radius,
                                      boundary, tsdf, weight, rgb, cweight, None)
    inf, nan = float("inf"), float("nan")
    for kw in (dict(xyz=None), dict(keys=None), dict(n=0), dict(cell=0.0), dict(normals=None), dict(blocks=None), dict(tsdf=None),
               dict(weight=None), dict(vd=None), dict(vo=None), dict(k=0), dict(k=33), dict(radius=0.0), dict(radius=-1.0),
               dict(radius=inf), dict(radius=nan), dict(radius=1e200), dict(radius=1e-200), dict(boundary=0.0), dict(boundary=inf),
               dict(boundary=nan), dict(boundary=1e200), dict(voxel=0.0), dict(voxel=inf), dict(trunc=0.0), dict(trunc=nan),
               dict(colors=P), dict(rgb=P), dict(cweight=P), dict(colors=P, rgb=P), dict(rgb=P, cweight=P),
               dict(vo=(ctypes.c_float * 3)(0, nan, 0))):
        assert call(**kw) == -1, kw
    for kw in (dict(nb=0), dict(nb=2 ** 22), dict(vd=(ctypes.c_int * 3)(1, 16, 16)), dict(vd=(ctypes.c_int * 3)(16, 2 ** 19, 16))):
        assert call(**kw) == -2, kw


def test_command_line_arguments():
    import mesh_cloud as M
    p = M.build_parser()
    a = p.parse_args(["--input", "a.ply", "--output", "m.ply"])
    assert (a.k, a.min_neighbors, a.voxel, a.radius, a.trunc, a.boundary, a.max_blocks) == (16, 3, None, None, None, None, None)
    assert a.ply_name == "fused_normals.ply" and not a.no_color and not a.no_normals and a.device == "cuda:0"
    M.check_args(a)
    a = p.parse_args(["--input", "o", "--scan_list", "l.txt", "--ply_name", "fused_clean.ply", "--voxel", "0.5", "--radius", "2",
                      "--trunc", "1.5", "--k", "9", "--boundary", "0.7", "--min_neighbors", "2", "--max_blocks", "4096", "--no_color",
                      "--no_normals", "--min_component_faces", "50", "--keep_components", "1", "--device", "cuda:1", "--report", "r.json"])
    assert (a.voxel, a.radius, a.trunc, a.k, a.boundary, a.min_neighbors, a.max_blocks) == (0.5, 2.0, 1.5, 9, 0.7, 2, 4096)
    assert a.no_color and a.no_normals and (a.min_component_faces, a.keep_components, a.report) == (50, 1, "r.json")
    M.check_args(a)
    for bad in (["--k", "0"], ["--k", "33"], ["--min_neighbors", "0"], ["--k", "4", "--min_neighbors", "5"], ["--voxel", "0"],
                ["--radius", "-1"], ["--trunc", "inf"], ["--boundary", "nan"], ["--max_blocks", "0"], ["--keep_components", "-1"]):
        with pytest.raises(ValueError):
            M.check_args(p.parse_args(["--input", "a.ply", "--output", "m.ply"] + bad))
    assert M.main(["--input", "a.ply", "--output", "m.ply", "--k", "0"]) == 2
    assert M.main(["--input", os.path.join(ROOT, "no_such_file.ply"), "--output", "m.ply"]) == 2
    assert M.main(["--input", os.path.join(ROOT, "no_such_file.ply")]) == 2  # a single file needs --output


def test_a_cloud_without_normals_is_refused_by_name(tmp_path):
    """Refused while reading the file, before the device is touched, with the message that names cloud_normals.py."""
    import mesh_cloud as M
    from patchmatchnet_amd import ply
    from patchmatchnet_amd._lib import PmnError
    src = str(tmp_path / "bare.ply")
    ply.write_ply(src, np.zeros((5, 3), np.float32), np.zeros((5, 3), np.uint8))
    args = M.build_parser().parse_args(["--input", src, "--output", str(tmp_path / "m.ply")])
    with pytest.raises(PmnError, match="cloud_normals.py"):
        M.mesh_file(src, args.output, args, None)
    assert M.main(["--input", src, "--output", str(tmp_path / "m.ply")]) == 2 and not os.path.exists(tmp_path / "m.ply")
