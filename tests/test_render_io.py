"""CPU checks of the renderer: the numpy oracle (tests/render_ref.py) against analytic truth and against the
exact conditions of the fill rule, the oracle's own float32-vs-float64 disagreement on the GPU tests' inputs at a reduced size, the
argument checks of the entry points, the PLY reader, orbit_cameras and render.py's refusals.  The kernels themselves are compared with
the same oracle in tests/test_render_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_ref as RR
import tsdf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from patchmatchnet_amd import PmnError, fusion, render, tsdf  # noqa: E402


def _grid_on_pixels(K, E, h, w, normal, offset, step=8):
    """A tessellation of the plane normal . X = offset whose vertices project EXACTLY onto points of the 1/256-px lattice of this
    camera (every ``step`` px, beyond the image on all sides): snapping then moves no vertex and the interpolation is exact."""
    us = np.arange(-step, w + step + 1, step, dtype=np.float64) + 3 / 256.0
    vs = np.arange(-step, h + step + 1, step, dtype=np.float64) + 5 / 256.0
    K64, E64 = K.astype(np.float64), E.astype(np.float64)
    Rm, t = E64[:3, :3], E64[:3, 3]
    C = -(Rm.T @ t)
    uu, vv = np.meshgrid(us, vs, indexing="xy")
    d = np.einsum("ij,jn->in", Rm.T @ np.linalg.inv(K64), np.stack((uu.ravel(), vv.ravel(), np.ones(uu.size))))
    s = (offset - np.asarray(normal) @ C) / (np.asarray(normal) @ d)
    verts = (C[:, None] + s * d).T
    nu, nv = len(us) - 1, len(vs) - 1
    f = []
    for j in range(nv):
        for i in range(nu):
            p, q, r, s_ = j * (nu + 1) + i, j * (nu + 1) + i + 1, (j + 1) * (nu + 1) + i + 1, (j + 1) * (nu + 1) + i
            f += [(p, q, r), (p, r, s_)]
    return verts, np.asarray(f, np.int32)


def test_oracle_against_analytic_plane_and_sphere():
    h, w = 120, 160
    nrm = np.array((0.3, -0.2, 0.93))
    offset = nrm @ np.asarray(RR.TARGET) + 0.4
    for view in range(3):
        K, E, cam = RR.case_camera(h, w, view=view)
        truth = R.render_plane(K, E, h, w, nrm, offset).astype(np.float64)
        # the vertices are kept in float64 here (project() takes float32 input): feed the oracle the exact plane through a float64 cast
        v64, f = _grid_on_pixels(K, E, h, w, nrm, offset)
        for T, ulps in ((np.float64, 4), (np.float32, 16)):
            o = RR.raster_triangles(v64.astype(np.float32), f, cam, h, w, T, count_hits=True)
            assert (o["hits"] == 1).all()
            err = float(np.abs(o["depth"].astype(np.float64) - truth).max())
            print(f"plane view {view} {T.__name__}: max |depth - analytic| {err:.3e}")
            # float rounding: the float32 vertices sit within half an ulp of the plane per coordinate, the analytic map is float32
            assert err <= ulps * np.spacing(np.float32(truth.max())), (view, T)
    # a general tessellation: snapping moves every vertex by up to sqrt(2) / 512 px while its depth stays, so the surface is off by at
    # most that times the depth gradient per pixel (measured on the analytic map), plus the rounding above; asserted at 2 x
    K, E, cam = RR.case_camera(h, w)
    truth = R.render_plane(K, E, h, w, nrm, offset).astype(np.float64)
    e1, e2 = np.cross(nrm, (0, 0, 1.0)), np.cross(nrm, np.cross(nrm, (0, 0, 1.0)))
    e1, e2 = e1 / np.linalg.norm(e1), e2 / np.linalg.norm(e2)
    p0 = np.asarray(RR.TARGET) + nrm * (offset - nrm @ np.asarray(RR.TARGET)) / (nrm @ nrm)
    v, f = RR.plane_grid(40, 40, p0 - 3 * e1 - 3 * e2, 6 * e1, 6 * e2, jitter=0.3)
    o = RR.raster_triangles(v, f, cam, h, w, np.float64, count_hits=True)
    grad = max(np.abs(np.diff(truth, axis=0)).max(), np.abs(np.diff(truth, axis=1)).max())
    bound = np.sqrt(2) / 512 * np.sqrt(2) * grad + 16 * np.spacing(np.float32(truth.max()))
    hit = o["hits"] > 0
    err = float(np.abs(o["depth"] - truth)[hit].max())
    print(f"general plane: max |depth - analytic| {err:.3e}, snapping bound {bound:.3e}")
    assert o["hits"].max() == 1 and hit.mean() > 0.5 and err <= 2 * bound
    # sphere.  The closed chordal mesh lies in the shell between the spheres of radius r - sag and r (sag: RR.chord_sag, exact for the
    # subdivision level), so along a ray that passes the centre at distance b the first mesh hit lies between the entry into the outer
    # sphere and the entry into the inner one: at most sqrt(r^2 - b^2) - sqrt((r - sag)^2 - b^2) behind the analytic hit, or, where
    # the ray misses the inner sphere, anywhere on its chord of length 2 sqrt(r^2 - b^2).  That is sag / cos(incidence) away from
    # the rim and grows towards it; camera depth changes by no more than ray length.  Asserted at 2 x per pixel, no pixel left out.
    centre, radius = np.asarray(RR.TARGET), 1.0
    C, d = R._rays(K, E, h, w)
    dn = d / np.linalg.norm(d, axis=0)
    oc = (C - centre)[:, None, None]
    b2 = (oc * oc).sum(0) - ((oc * dn).sum(0)) ** 2  # squared distance of the ray from the centre
    truth = R.render_sphere(K, E, h, w, centre, radius).astype(np.float64)
    previous = None
    for level in (2, 3, 4):
        v, f = RR.icosphere(level, centre, radius)
        sag = RR.chord_sag(v, f, centre, radius)
        assert previous is None or 3.5 < previous / sag < 4.0  # a subdivision step halves the arcs: a quarter of the sag
        previous = sag
        o = RR.raster_triangles(v, f, cam, h, w, np.float64)
        outer = np.sqrt(np.maximum(radius ** 2 - b2, 0))
        inner2 = (radius - sag) ** 2 - b2
        bound = np.where(inner2 > 0, outer - np.sqrt(np.maximum(inner2, 0)), 2 * outer)
        sel = (truth > 0) & (o["depth"] > 0)
        err = np.abs(o["depth"] - truth)
        centre_px = sel & (bound < 1.01 * sag / 0.6)
        print(f"icosphere level {level}: chord sag {sag:.3e}; max depth error {err[sel].max():.3e} over {int(sel.sum())} px (largest "
              f"per-pixel bound {bound[sel].max():.3e}); where the bound is below sag / 0.6: error {err[centre_px].max():.3e}; "
              f"worst error / bound {float((err[sel] / bound[sel]).max()):.3f}")
        assert sel.sum() > 4000 and (err[sel] <= 2 * bound[sel]).all()
        assert (o["depth"] > 0)[truth == 0].sum() == 0  # a chordal mesh never reaches outside the sphere's outline


def _cover(h, w, cells, offset, winding):
    K = np.array([[100.0, 0, 0], [0, 100.0, 0], [0, 0, 1]], np.float32)
    E = np.eye(4, dtype=np.float32)
    z = 2.0
    v, f = RR.plane_grid(cells[0], cells[1], ((-7.3 + offset[0]) * z / 100, (-5.9 + offset[1]) * z / 100, z),
                         ((w + 25.1) * z / 100, 0, 0.03), (0, (h + 22.7) * z / 100, 0.02), winding, jitter=0.3, seed=cells[0])
    return v, f, tsdf.camera21(K, E)


def test_oracle_exact_coverage_and_order_independence():
    h, w = 60, 80
    rng = np.random.default_rng(1)
    for offset in [(0.0, 0.0)] + [tuple(rng.uniform(0, 1, 2)) for _ in range(3)]:
        for winding in (1, -1):
            for cells in ((5, 4), (50, 40)):
                v, f, cam = _cover(h, w, cells, offset, winding)
                o = RR.raster_triangles(v, f, cam, h, w, np.float32, count_hits=True)
                assert (o["hits"] == 1).all(), (offset, winding, cells)  # hits, not winners: no crack, no double hit
    v, f, cam = _cover(h, w, (50, 40), (0.3, 0.7), 1)
    v2, f2 = RR.icosphere(3, (0.4, 0.3, 1.5), 0.3)
    v, f = np.concatenate((v, v2)), np.concatenate((f, f2 + len(v)))
    a = RR.raster_triangles(v, f, cam, h, w)
    perm = rng.permutation(len(f))
    b = RR.raster_triangles(v, f[perm], cam, h, w)
    assert a["depth"].tobytes() == b["depth"].tobytes()
    assert np.array_equal(np.where(b["index"] >= 0, perm[np.maximum(b["index"], 0)], -1), a["index"])


def test_oracle_top_left_rule():
    K = np.eye(3, dtype=np.float32)
    cam = tsdf.camera21(K, np.eye(4, dtype=np.float32))
    # at z = 1 and K = I a vertex (x, y, 1) lands on pixel position (x, y): a square with corners ON the pixel centres 2 and 6
    sq = np.array([[2, 2, 1], [6, 2, 1], [6, 6, 1], [2, 6, 1]], np.float32)
    for faces in ([[0, 1, 2], [0, 2, 3]], [[2, 1, 0], [3, 2, 0]], [[0, 1, 3], [1, 2, 3]]):
        o = RR.raster_triangles(sq, np.asarray(faces, np.int32), cam, 9, 9, count_hits=True)
        want = np.zeros((9, 9), int)
        want[2:6, 2:6] = 1  # the top and left edges and the top-left vertex are in, the bottom and right edges are out
        assert np.array_equal(o["hits"], want), faces
    # a diagonal edge exactly through pixel centres belongs to the triangle on its right (it is that triangle's left edge)
    o = RR.raster_triangles(sq, np.asarray([[0, 1, 2], [0, 2, 3]], np.int32), cam, 9, 9)
    assert all(o["index"][k, k] == 0 for k in range(2, 6))  # triangle 0 is the half with x > y: to the right of the diagonal


@pytest.mark.parametrize("kind", ["mt", "ico", "spoiled"])
def test_oracle_precisions_agree_on_the_gpu_cases(kind):
    """The condition of tests/test_render_gpu.py on its inputs, at a reduced size of the same generators: the float32 and float64
    oracles disagree on at most 1 % of the covered pixels."""
    h, w = 240, 320
    if kind == "mt":
        field, origin, voxel = RR.mt_lattice(32)
        m = R.extract(field, np.ones_like(field), origin, voxel, normals=False)
        v, f, dist = m["vertices"], m["faces"], 4.0
    elif kind == "ico":
        (v, f), dist = RR.icosphere(1, RR.TARGET, 1.2), 2.4
    else:
        (v, f), dist = RR.spoiled(*RR.icosphere(4, RR.TARGET, 1.0)), 4.0
    _, _, cam = RR.case_camera(h, w, dist)
    o32, o64 = RR.raster_triangles(v, f, cam, h, w, np.float32), RR.raster_triangles(v, f, cam, h, w, np.float64)
    same, covered, excluded = RR.compare_oracles(o32, o64)
    own = float(np.abs(o32["depth"] - o64["depth"])[same].max())
    print(f"{kind}: {len(f)} faces, covered {covered}, oracles disagree on {excluded} px, depth f32-vs-f64 {own:.3e}, counters {o32['counters']}")
    assert covered > 5000 and excluded <= 0.01 * covered and o32["counters"] == o64["counters"]
    if kind == "ico":
        assert o32["counters"][3] > 0
    if kind == "spoiled":
        assert o32["counters"][0] >= 200 and o32["counters"][2] >= 150
    pts = RR.point_cloud(200000, RR.TARGET, seed=2)
    _, _, cam = RR.case_camera(h, w)
    for kw in ({}, {"radius_px": 1.0}, {"radius_world": 0.0025 * 5}):
        a, b = RR.splat_points(pts, cam, h, w, np.float32, **kw), RR.splat_points(pts, cam, h, w, np.float64, **kw)
        same, covered, excluded = RR.compare_oracles(a, b)
        assert covered > 5000 and excluded <= 0.01 * covered and a["counters"] == b["counters"] and a["counters"][0] > 0, kw


def test_entry_points_reject_bad_arguments_before_any_launch():
    from patchmatchnet_amd import _lib, ops
    L = _lib.lib()
    assert L.pmn_raster_triangles(None, 1, None, 1, None, 8, 8, 0, None, None, None, None) == -1
    assert L.pmn_splat_points(None, 1, None, 8, 8, 0.0, 0.0, None, None, None) == -1
    assert L.pmn_raster_resolve(None, 8, 8, None, None, 1, None, 0, None, None, 0, None, None, None, None, None) == -1
    # every other check, one bad argument at a time, with dummy non-null pointers: nothing is launched, so this is safe without a GPU
    import ctypes
    buf = ctypes.create_string_buffer(4096)
    P = ctypes.addressof(buf)
    cam = (ctypes.c_float * 21)(*([1.0] * 21))
    C = ctypes.addressof(cam)
    nan_cam = (ctypes.c_float * 21)(*([1.0] * 20 + [float("nan")]))
    inf_cam = (ctypes.c_float * 21)(*([float("inf")] + [1.0] * 20))
    tri = lambda **k: L.pmn_raster_triangles(*[k.get(n, d) for n, d in (("v", P), ("nv", 3), ("f", P), ("nf", 1), ("cam", C), ("h", 8),
                                                                       ("w", 8), ("box", 0), ("keys", P), ("cnt", P), ("wl", P), ("s", None))])
    pts = lambda **k: L.pmn_splat_points(*[k.get(n, d) for n, d in (("p", P), ("n", 3), ("cam", C), ("h", 8), ("w", 8), ("rpx", 0.0),
                                                                   ("rw", 0.0), ("keys", P), ("cnt", P), ("s", None))])
    res = lambda **k: L.pmn_raster_resolve(*[k.get(n, d) for n, d in (("keys", P), ("h", 8), ("w", 8), ("cam", C), ("v", P), ("nv", 3),
                                                                     ("f", P), ("nf", 1), ("col", None), ("nrm", None), ("shade", 0),
                                                                     ("depth", P), ("index", P), ("rgb", None), ("normal", None),
                                                                     ("s", None))])
    big = _lib.RASTER_MAX_DIM + 1
    for call in (tri, pts, res):
        assert call(h=0) == -2 and call(w=0) == -2 and call(h=big) == -2 and call(w=big) == -2 and call(h=-1) == -2
        assert call(cam=ctypes.addressof(nan_cam)) == -1 and call(cam=ctypes.addressof(inf_cam)) == -1 and call(cam=None) == -1
        assert call(keys=None) == -1
    assert tri(box=-1) == -1 and tri(nv=0) == -1 and tri(nf=0) == -1 and tri(v=None) == -1 and tri(f=None) == -1
    assert tri(cnt=None) == -1 and tri(wl=None) == -1
    assert pts(rpx=float(_lib.SPLAT_MAX_RADIUS) + 0.5) == -1 and pts(rpx=-1.0) == -1 and pts(rpx=float("nan")) == -1
    assert pts(rw=-1.0) == -1 and pts(rw=float("inf")) == -1 and pts(rw=float("nan")) == -1 and pts(rpx=1.0, rw=1.0) == -1
    assert pts(n=0) == -1 and pts(n=2 ** 31) == -1 and pts(p=None) == -1 and pts(cnt=None) == -1
    assert res(f=None, nf=1) == -1 and res(nf=0) == -1 and res(nv=0) == -1 and res(nv=2 ** 31) == -1 and res(nf=2 ** 31) == -1
    assert res(depth=None) == -1 and res(index=None) == -1 and res(v=None) == -1
    hdr = open(os.path.join(ROOT, "include", "pmn_hip.h")).read()
    for name, value in (("PMN_RASTER_MAX_DIM", _lib.RASTER_MAX_DIM), ("PMN_RASTER_MAX_BOX", _lib.RASTER_MAX_BOX),
                        ("PMN_SPLAT_MAX_RADIUS", _lib.SPLAT_MAX_RADIUS)):
        assert f"#define {name} {value}" in hdr
    assert (RR.MAX_BOX, RR.SPLAT_MAX_RADIUS) == (_lib.RASTER_MAX_BOX, _lib.SPLAT_MAX_RADIUS)
    with pytest.raises(PmnError, match="ROCm GPU"):
        render.Renderer("cpu")
    keys, cnt = torch.full((4, 4), -1, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(PmnError):
        ops.raster_triangles(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), np.zeros(21), keys, cnt, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(PmnError):
        ops.splat_points(torch.zeros(3, 3), np.zeros(21), keys, cnt)
    with pytest.raises(PmnError):
        ops.raster_resolve(keys, np.zeros(21), torch.zeros(3, 3), None, torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.int32))


def test_read_ply_model(tmp_path):
    rng = np.random.default_rng(0)
    v, f = RR.icosphere(1)
    col, nrm = rng.integers(0, 256, (len(v), 3), dtype=np.uint8), rng.standard_normal((len(v), 3)).astype(np.float32)
    path = str(tmp_path / "m.ply")
    for c, n in ((col, nrm), (col, None), (None, nrm), (None, None)):
        tsdf.write_ply_mesh(path, v, f, c, n)
        m = render.read_ply_model(path)
        assert m["vertices"].tobytes() == v.tobytes() and np.array_equal(m["faces"], f)
        assert (m["colors"] is None) == (c is None) and (m["normals"] is None) == (n is None)
        assert c is None or np.array_equal(m["colors"], c)
    for n in (None, nrm):  # either kind of fused.ply
        fusion.write_ply(path, v, col, n)
        m = render.read_ply_model(path)
        assert m["faces"] is None and m["vertices"].tobytes() == v.tobytes() and np.array_equal(m["colors"], col)
        assert (m["normals"] is None) == (n is None)
    # a ground-truth style mesh: double positions, an extra scalar, colours first, uint indices and a per-face scalar
    vd = np.dtype([("red", "u1"), ("green", "u1"), ("blue", "u1"), ("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("quality", "<f4")])
    rec = np.zeros(len(v), vd)
    for k, name in enumerate("xyz"):
        rec[name] = v[:, k]
    rec["red"], rec["green"], rec["blue"] = col.T
    fd = np.dtype([("flags", "<i4"), ("n", "u1"), ("v", "<u4", (3,))])
    frec = np.zeros(len(f), fd)
    frec["n"], frec["v"] = 3, f
    head = ("ply\nformat binary_little_endian 1.0\ncomment made by a scanner\nelement vertex %d\nproperty uchar red\nproperty uchar green\n"
            "property uchar blue\nproperty double x\nproperty double y\nproperty double z\nproperty float quality\nelement face %d\n"
            "property int flags\nproperty list uchar uint vertex_indices\nend_header\n" % (len(v), len(f))).encode()
    with open(path, "wb") as fh:
        fh.write(head)
        rec.tofile(fh)
        frec.tofile(fh)
    m = render.read_ply_model(path)
    assert np.array_equal(m["vertices"], v) and np.array_equal(m["faces"], f) and np.array_equal(m["colors"], col) and m["normals"] is None
    with pytest.raises(ValueError):
        tsdf.read_ply_mesh(path)  # the existing reader is unchanged: it reads this library's meshes only
    with open(path, "wb") as fh:
        fh.write(head)
        rec.tofile(fh)
        frec[:5].tofile(fh)
    with pytest.raises(PmnError, match="m.ply"):
        render.read_ply_model(path)
    with open(path, "wb") as fh:
        fh.write(b"P6\n1 1\n255\n000")
    with pytest.raises(PmnError, match="m.ply"):
        render.read_ply_model(path)
    for bad in ("property list uchar ushort vertex_indices", "property list int int vertex_indices",
                "property list uchar int vertex_indices\nproperty list uchar float texcoord"):
        with open(path, "wb") as fh:  # a mesh whose faces this reader cannot decode is refused, never drawn as a cloud
            fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                      "element face 1\n%s\nend_header\n" % bad).encode() + bytes(36 + 32))
        with pytest.raises(PmnError, match="m.ply.*cannot be read"):
            render.read_ply_model(path)
    with open(path, "w") as fh:  # an ascii MESH likewise
        fh.write("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
                 "property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")
    with pytest.raises(PmnError, match="m.ply.*binary_little_endian"):
        render.read_ply_model(path)
    with open(path, "w") as fh:  # ascii: positions only
        fh.write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 1 2\n3 4 5\n")
    m = render.read_ply_model(path)
    assert m["faces"] is None and np.array_equal(m["vertices"], np.float32([[0, 1, 2], [3, 4, 5]]))


def test_orbit_cameras():
    bounds = (-3.0, 10.0, 100.0, 5.0, 14.0, 120.0)
    h, w = 90, 160
    K, E = render.orbit_cameras(bounds, 12, h, w, fov=35.0)
    assert K.shape == (12, 3, 3) and E.shape == (12, 4, 4) and K.dtype == np.float32
    centre = np.array([1.0, 12.0, 110.0])
    corners = np.array([[x, y, z] for x in bounds[0::3] for y in bounds[1::3] for z in bounds[2::3]])
    dists = []
    for i in range(12):
        Rm, t = E[i, :3, :3].astype(np.float64), E[i, :3, 3].astype(np.float64)
        assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-6) and np.linalg.det(Rm) > 0.999
        C = -Rm.T @ t
        dists.append(np.linalg.norm(C - centre))
        assert abs(C[1] - centre[1]) < 1e-3  # on a horizontal circle
        pc = Rm @ centre + t
        assert abs(pc[0]) < 1e-3 and abs(pc[1]) < 1e-3 and pc[2] > 0  # looking at the centre
        q = (corners @ Rm.T + t) @ K[i].astype(np.float64).T
        u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        assert u.min() >= 0 and u.max() <= w - 1 and v.min() >= 0 and v.max() <= h - 1
    assert np.ptp(dists) < 1e-3 * dists[0]
    assert abs(2 * np.degrees(np.arctan(h / 2.0 / K[0, 1, 1])) - 35.0) < 1e-3
    with pytest.raises(PmnError):
        render.orbit_cameras((0, 0, 0, -1, 1, 1), 4, 10, 10)


def test_render_py_parser_and_refusals(tmp_path):
    import render as cli  # the command line at the repository root
    args = cli.build_parser().parse_args(["--input_folder", "a", "--model", "b/{scan}/mesh.ply", "--output_folder", "c", "--orbit", "8",
                                          "--size", "120", "160", "--radius_world", "0.5"])
    assert args.orbit == 8 and tuple(args.size) == (120, 160) and args.write == "depth_gt,masks,images" and args.shade == 1
    assert "torchrun" in cli.build_parser().format_help()
    model = str(tmp_path / "m.ply")
    tsdf.write_ply_mesh(model, *RR.icosphere(0))
    junk = str(tmp_path / "junk.ply")
    with open(junk, "wb") as fh:
        fh.write(b"not a model")

    def run(argv, env=None):
        e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
        e.update(env or {})
        return subprocess.run([sys.executable, os.path.join(ROOT, "render.py")] + argv, env=e, capture_output=True, text=True, timeout=300)

    base = ["--model", model, "--output_folder", str(tmp_path / "out"), "--orbit", "2"]
    r = run(base, {"WORLD_SIZE": "2"})
    assert r.returncode == 2 and "torchrun" in r.stderr
    r = run(base + ["--device", "cpu"])
    assert r.returncode != 0 and "ROCm GPU" in r.stderr and "render.py:" in r.stderr
    r = run(["--model", junk, "--output_folder", str(tmp_path / "out"), "--orbit", "2"])
    assert r.returncode != 0 and "junk.ply" in r.stderr and "neither" in r.stderr
    r = run(["--model", model, "--output_folder", str(tmp_path / "out")])
    assert r.returncode != 0 and "--orbit" in r.stderr
    r = run(base + ["--write", "depth_gt,pictures"])
    assert r.returncode != 0 and "pictures" in r.stderr
    r = run(base + ["--radius_px", "1", "--radius_world", "1"])
    assert r.returncode != 0 and "only one" in r.stderr
    if not torch.cuda.is_available():
        r = run(base)
        assert r.returncode != 0 and "none is visible" in r.stderr
