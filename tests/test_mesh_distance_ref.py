"""CPU checks of the point-to-mesh distance: the numpy yardstick tests/mesh_distance_ref.py against closed forms,
and build_face_grid's cover property -- every point of every face lies within R of one of that face's reference points -- on host
tensors.  The kernel itself is compared with the yardstick in tests/test_mesh_distance_gpu.py."""
import numpy as np
import pytest
import torch

import mesh_distance_ref as R
from patchmatchnet_amd import PmnError, _lib, meshops

TRI_V = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], np.float32)
TRI_F = np.array([[0, 1, 2]], np.int32)
# (x, y) of a query in each of the seven Voronoi regions of the 3-4-5 triangle, its in-plane distance squared and its nearest point
REGIONS = [((1.0, 1.0), 0.0, (1.0, 1.0)),      # the face
           ((2.0, -2.0), 4.0, (2.0, 0.0)),     # edge AB
           ((-1.0, 1.0), 1.0, (0.0, 1.0)),     # edge CA
           ((5.0, 5.5), 25.0, (2.0, 1.5)),     # edge BC: the midpoint of the hypotenuse plus its normal (3, 4)
           ((-1.0, -1.0), 2.0, (0.0, 0.0)),    # vertex A
           ((6.0, -1.0), 5.0, (4.0, 0.0)),     # vertex B
           ((-1.0, 5.0), 5.0, (0.0, 3.0))]     # vertex C


def seven_regions(heights=(0.0, 2.0, -0.5)):
    """(query float32 [21, 3], distance float64 [21], closest float64 [21, 3]), hand-derived and exact in float64."""
    q = np.array([[x, y, h] for h in heights for (x, y), _, _ in REGIONS], np.float32)
    d = np.array([np.sqrt(p2 + h * h) for h in heights for _, p2, _ in REGIONS])
    c = np.array([[cx, cy, 0.0] for _ in heights for _, _, (cx, cy) in REGIONS])
    return q, d, c


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_one_triangle_all_seven_regions(dtype):
    q, d, c = seven_regions()
    for perm in ([0, 1, 2], [1, 2, 0], [2, 1, 0]):  # the vertex order of the face must not matter
        d2, face, closest, d_all = R.brute_force(TRI_V, TRI_F[:, perm], q, dtype)
        assert np.abs(np.sqrt(d2).astype(np.float64) - d).max() <= 4 * np.finfo(np.float64).eps * 8
        assert np.abs(closest.astype(np.float64) - c).max() <= 4 * np.finfo(np.float64).eps * 8
        assert (face == 0).all() and np.array_equal(d_all[:, 0], np.sqrt(d2))


def test_triangulated_plane():
    v, f = R.plane_grid(8, 8)
    rng = np.random.default_rng(1)
    q = np.concatenate([rng.uniform(0, 8, (300, 2)), rng.uniform(-3, 3, (300, 1))], 1).astype(np.float32)
    d2, face, closest, _ = R.brute_force(v, f, q)
    assert np.abs(np.sqrt(d2) - np.abs(q[:, 2].astype(np.longdouble))).max() < 1e-15
    assert np.abs(closest[:, :2] - q[:, :2]).max() < 1e-14 and np.abs(closest[:, 2]).max() == 0
    assert np.allclose(R.face_distance(v, f, q, face).astype(np.float64), np.sqrt(d2).astype(np.float64), rtol=0, atol=1e-15)
    # beside the rectangle: the nearest point is on its border
    out = np.array([[-3, 4, 4], [12, 9, 0], [4, 4, 0]], np.float32)
    assert np.allclose(np.sqrt(R.brute_force(v, f, out)[0]).astype(np.float64), [5.0, np.sqrt(17.0), 0.0], rtol=0, atol=1e-15)


def test_icosphere_outside_the_circumsphere():
    v, f = R.icosphere(3, 2.0)
    assert f.shape == (1280, 3) and v.shape == (642, 3)
    v64 = v.astype(np.float64)
    n = np.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]])
    inradius = np.abs((n * v64[f[:, 0]]).sum(1) / np.linalg.norm(n, axis=1)).min()
    sag = 2.0 - inradius
    assert 0 < sag < 0.02
    rng = np.random.default_rng(2)
    q = rng.normal(size=(400, 3))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(2.001, 50.0, (400, 1))).astype(np.float32)
    d = np.sqrt(R.brute_force(v, f, q)[0]).astype(np.float64)
    gap = np.linalg.norm(q.astype(np.float64), axis=1) - 2.0
    # the polyhedron lies between the spheres of radius 2 - sag and 2 (its vertices on the latter to float32 rounding)
    assert (d >= gap - 1e-6).all() and (d <= gap + sag + 1e-6).all()
    # along a vertex's direction the vertex itself is the nearest point of the (convex) polyhedron
    qv = (v64 * np.linspace(1.5, 30.0, len(v64))[:, None]).astype(np.float32)
    dv = np.sqrt(R.brute_force(v, f, qv)[0]).astype(np.float64)
    assert np.abs(dv - np.linalg.norm(qv.astype(np.float64) - v64, axis=1)).max() < 1e-12
    assert np.abs(dv - (np.linalg.norm(qv.astype(np.float64), axis=1) - 2.0)).max() < 1e-5


def test_screened_brute_force_is_the_full_one_and_degenerate_faces_are_segments():
    v, f = R.icosphere(1)
    v = np.concatenate([v, [[3, 0, 0], [5, 0, 0], [4, 0, 0]]]).astype(np.float32)
    f = np.concatenate([f, [[42, 42, 43], [42, 42, 42], [42, 44, 43]]]).astype(np.int32)  # a segment, a point, a collinear face
    rng = np.random.default_rng(3)
    q = np.concatenate([rng.uniform(-2, 6, (200, 3)), [[4, 1, 0], [7, 0, 0], [2.5, 0, 0]]]).astype(np.float32)
    a = R.brute_force(v, f, q, screen=True)
    b = R.brute_force(v, f, q, screen=False)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    kept = np.isfinite(a[3])
    assert np.array_equal(a[3][kept], b[3][kept]) and kept.any(1).all() and not kept.all()
    allowed, allowed_c, figures = R.gate(v, f, q, a)
    print("float64 against longdouble:", figures)
    assert np.array_equal(R.near_faces(a[3], allowed), R.near_faces(b[3], allowed))
    assert R.near_faces(a[3], allowed)[np.arange(len(q)), a[1]].all()
    assert figures["off_surface"] < 64 * R.TWO_M52 and figures["on_surface"] < 64 and figures["closest_units"] < 64
    seg = R.face_distance(v, f, q[-3:], [80, 81, 82]).astype(np.float64)
    assert np.array_equal(seg, [1.0, 4.0, 0.5])                       # (a, a, b): the segment; (a, a, a): the point; collinear
    assert np.array_equal(R.face_distance(v, f, q[-3:], [82, 82, 82]).astype(np.float64), [1.0, 2.0, 0.5])


# ---- build_face_grid on host tensors ----------------------------------------------------------------------------------------------------

def _cover_mesh():
    rng = np.random.default_rng(4)
    n = 300
    base = rng.uniform(0.5, 50.0, n)
    height = base / 10.0 ** rng.uniform(0.0, 3.0, n)  # aspect ratios 1 .. 1000
    apex = rng.uniform(-0.5, 1.5, n) * base
    local = np.zeros((n, 3, 3))
    local[:, 1, 0] = base
    local[:, 2, 0], local[:, 2, 1] = apex, height
    rot = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    tri = np.einsum("nij,nkj->nki", rot, local) + rng.uniform(-100, 100, (n, 1, 3))
    v = tri.reshape(-1, 3)
    f = np.arange(3 * n).reshape(n, 3)
    # a face 10 000 x the cell, and degenerate faces: (a, a, b), (a, a, a), collinear, and a long sliver of no area
    extra = np.array([[0, 0, 0], [10000, 0, 0], [0, 10000, 0], [7, 7, 7], [8, 9, 7], [1, 1, 1], [2, 2, 2], [300, 300, 300]], np.float64)
    k = len(v)
    f = np.concatenate([f, [[k, k + 1, k + 2], [k + 3, k + 3, k + 4], [k + 3, k + 3, k + 3], [k + 5, k + 6, k + 7], [k + 5, k + 7, k + 7]]])
    return np.concatenate([v, extra]).astype(np.float32), f.astype(np.int32)


def test_build_face_grid_cover_property_on_host_tensors():
    v, f = _cover_mesh()
    fg = meshops.build_face_grid(torch.from_numpy(v), torch.from_numpy(f), cell=1.0, cover=8.0)
    assert fg.grid.xyz.device.type == "cpu" and fg.cover == 8.0 and fg.grid.cell == 1.0
    levels = fg.levels.numpy()
    assert levels[300] == 10 and levels.max() == 10 and (levels[:300] > 0).any() and (levels[:300] == 0).any()
    assert levels[301] == 0 and levels[302] == 0 and levels[304] > 0
    ref, entry_face = fg.grid.xyz.double(), fg.entry_face.long()
    # every entry maps to a face, every face has its 4^L entries, and an entry lies ON its face (to the float32 rounding in R)
    assert np.array_equal(np.bincount(entry_face.numpy(), minlength=len(f)), 4 ** levels)
    rounding = np.sqrt(3.0) * 2.0 ** -23 * np.abs(v).max()
    assert fg.radius >= 8.0 * 0.5 and fg.radius <= 8.0 * (1 + 2.0 ** -40) + rounding
    on = R.face_distance(v, f, ref.numpy(), entry_face.numpy(), np.float64)
    assert on.max() <= rounding
    # 200 barycentric points per face (corners and edges among them), each within R of one of the face's entries
    rng = np.random.default_rng(5)
    b = rng.dirichlet((0.4, 0.4, 0.4), 200)
    b[:6] = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5]]
    tri = torch.from_numpy(v.astype(np.float64)[f])                      # [Nt, 3, 3]
    pts = torch.einsum("pk,fkc->fpc", torch.from_numpy(b), tri)          # [Nt, 200, 3]
    order = torch.argsort(entry_face, stable=True)
    start = np.concatenate([[0], np.cumsum(4 ** levels)])
    worst = 0.0
    for face in range(len(f)):
        mine = ref[order[start[face]:start[face + 1]]]
        for p0 in range(0, 200, 50):
            worst = max(worst, float(torch.cdist(pts[face, p0:p0 + 50], mine).min(1).values.max()))
    print(f"cover property: worst distance to the nearest own entry {worst:.6g}, R {fg.radius:.6g}")
    assert worst <= fg.radius


def test_build_face_grid_defaults_come_from_the_mesh():
    v, f = R.plane_grid(20, 10, step=0.25)
    fg = meshops.build_face_grid(torch.from_numpy(v), torch.from_numpy(f))
    edge = 0.25 * np.sqrt(2.0)
    assert fg.grid.cell == pytest.approx(meshops.FACE_CELL_EDGES * edge, rel=1e-6)
    assert fg.cover == pytest.approx(meshops.FACE_COVER_CELLS * fg.grid.cell)
    assert int(fg.levels.max()) == 0 and fg.grid.xyz.shape[0] == len(f)
    assert torch.equal(fg.entry_face.long(), fg.grid.perm)


def test_build_face_grid_refusals():
    v, f = torch.from_numpy(TRI_V.copy()), torch.from_numpy(TRI_F.copy())
    big = v * 1.0e9
    with pytest.raises(PmnError, match=r"face 0 .*cover"):
        meshops.build_face_grid(big, f, cell=1.0)
    bad = v.clone()
    bad[1, 2] = float("nan")
    with pytest.raises(PmnError, match="non-finite"):
        meshops.build_face_grid(bad, f)
    bad[1, 2] = float("inf")
    with pytest.raises(PmnError, match="non-finite"):
        meshops.build_face_grid(bad, f)
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(PmnError, match="cell"):
            meshops.build_face_grid(v, f, cell=cell)
    with pytest.raises(PmnError, match="cover"):
        meshops.build_face_grid(v, f, cell=1.0, cover=0.0)
    with pytest.raises(PmnError):
        meshops.build_face_grid(v.double(), f)
    with pytest.raises(PmnError):
        meshops.build_face_grid(v, f.long())
    with pytest.raises(PmnError):  # the search itself has no host path
        meshops.point_mesh_distance(torch.zeros(4, 3), meshops.build_face_grid(v, f), 1.0)


def test_entry_point_checks_its_arguments_before_any_launch():
    L = _lib.lib()
    assert L.pmn_mesh_distance(None, None, 0, None, 1.0, None, None, 0.0, None, 0, None, 0, None, None, 0, 1.0, None, None, None, None,
                               None) == -1
