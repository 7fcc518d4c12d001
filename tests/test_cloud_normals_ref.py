"""CPU checks of tests/cloud_normals_ref.py, the numpy statement of normals from neighbourhoods (pmn_knn_normals), and of the parts
of cloud_normals.py that need no GPU: the reference on shapes whose normals are known, its host model of the kernel's Jacobi sweeps
against numpy.linalg.eigh, the degenerate neighbourhoods, the viewpoint rule and the command line's argument handling."""
import os
import sys

import numpy as np
import pytest

import cloud_normals_ref as R
import knn_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
BIG = 1000.0


def test_constants_agree():
    """The sweep count is part of the definition: the header, the binding and the host model state the same one."""
    from patchmatchnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pmn_hip.h")).read()
    assert f"#define PMN_NORMAL_SWEEPS {_lib.NORMAL_SWEEPS}" in hdr and R.SWEEPS == _lib.NORMAL_SWEEPS
    assert f"#define PMN_NORMAL_MAX_VIEWPOINTS {_lib.NORMAL_MAX_VIEWPOINTS}" in hdr
    assert "HEURISTIC" in hdr[hdr.index("Normals of a point cloud"):hdr.index("int pmn_knn_normals(")]  # the viewpoint rule is one


def test_exact_plane():
    """Integer points of z = x + 2 y: every delta and every moment is an integer, so the only roundings are the division by m in C
    and the solver's own.  The normal is (1, 2, -1) / sqrt 6 (canonical sign: the largest component, y, positive) to 1e-14 rad and the
    variation 0 to 1e-14 (measured: 3.6e-16 rad and 1.2e-16 with eigh, 1.8e-16 rad and 2.8e-17 with the Jacobi model)."""
    pts = R.plane_cloud()
    want = np.tile(np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0), (len(pts), 1))
    for solver in (R.eigh, R.jacobi):
        r = R.normals(None, pts, 8, BIG, same_cloud=True, solver=solver)
        assert r["valid"].all() and (r["count"] == 8).all()
        assert R.angle(r["normal"], want).max() <= 1e-14
        assert np.abs(r["variation"]).max() <= 1e-14
        assert (r["normal"][:, 1] > 0).all()
    # the moments themselves are exact integers
    count, s, M = R.moments(pts, pts, R.neighbours(None, pts, 8, BIG, True))
    assert np.array_equal(s, np.round(s)) and np.array_equal(M, np.round(M))


def test_sphere_normals_are_radial_within_the_sampling():
    """1500 points on a sphere of radius 10, k = 16: a neighbourhood is a cap, and a plane fitted to points of a cap tilts from the
    radial direction by no more than the cap's angular radius, here 2 asin(d_k / 2R) of the point's own k-th neighbour (at most
    0.285 rad).  Measured with this reference: the largest angle is 0.0941 rad (5.4 degrees, 0.42 of that point's cap), the mean
    0.0245 rad."""
    pts, centre = R.sphere_cloud(noise=0.0)
    r = R.normals(None, pts, 16, BIG, same_cloud=True, solver=R.eigh)
    radial = pts.astype(np.float64) - centre
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    ang = R.angle(r["normal"], radial, signed=False)
    cap = 2.0 * np.arcsin(np.sqrt(K.knn_d2(None, pts, 16, BIG, True)[:, -1]) / 20.0)
    print(f"sphere: max angle {ang.max():.4f} rad, mean {ang.mean():.4f}, largest cap {cap.max():.4f}, max angle / cap {(ang / cap).max():.3f}")
    assert r["valid"].all()
    assert (ang <= cap).all() and ang.max() <= 0.095 and ang.mean() <= 0.025
    # oriented to the centre every normal points inwards, oriented to a far point on the other side of each normal outwards
    inward = R.orient(pts, r["normal"], centre[None])
    assert ((inward * radial).sum(1) < 0).all()


@pytest.mark.parametrize("k", [2, 3, 8, 16, 32])
def test_jacobi_model_agrees_with_eigh(k):
    """Six sweeps are ample for 3 x 3: wherever (l1 - l0) / l2 >= 1e-3 the model's vector is within 1e-12 rad of eigh's (measured: at
    most 1.3e-13, at k = 3), the values agree to 1e-12 of the largest, and both call the same neighbourhoods degenerate."""
    for pts, max_dist in ((R.sphere_cloud()[0], BIG), (R.sheet_cloud(), 5.0), (K.lattice_cloud(), 1.5), (K.duplicate_cloud(), 0.8)):
        e = R.normals(None, pts, k, max_dist, same_cloud=True, solver=R.eigh)
        j = R.normals(None, pts, k, max_dist, same_cloud=True, solver=R.jacobi)
        assert np.array_equal(e["C"], j["C"]) and np.array_equal(e["count"], j["count"])
        scale = np.maximum(e["values"][:, 2:], 1e-300)
        assert (np.abs(e["values"] - j["values"]) <= 1e-12 * scale).all()
        ok = e["valid"] & j["valid"] & (R.gap(e["values"]) >= 1e-3)
        if ok.any():
            assert R.angle(e["normal"][ok], j["normal"][ok], signed=False).max() <= 1e-12
        # the model's vectors are unit vectors and its normal is what the definition says: C n = l0 n
        n = j["normal"][j["valid"]]
        assert (np.abs(np.linalg.norm(n, axis=1) - 1.0) <= 1e-14).all()
        Cn = np.einsum("nab,nb->na", R.full(j["C"][j["valid"]]), n)
        assert (np.abs(Cn - j["values"][j["valid"], :1] * n) <= 1e-12 * j["values"][j["valid"], 2:]).all()


def test_jacobi_model_orders_equal_values_by_column():
    C = np.array([[2.0, 0.0, 0.0, 2.0, 0.0, 2.0], [3.0, 0.0, 0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    lam, vec = R.jacobi(C)
    assert np.array_equal(lam, [[2, 2, 2], [1, 1, 3], [0, 0, 0]])
    assert np.array_equal(vec[0], np.eye(3)) and np.array_equal(vec[2], np.eye(3))
    assert np.array_equal(vec[1], [[0, 0, 1], [1, 0, 0], [0, 1, 0]])  # columns y, z, x


def test_degenerate_neighbourhoods_have_no_normal():
    line = K.axis_cloud(61)
    r = R.normals(None, line, 8, BIG, same_cloud=True)
    assert not r["valid"].any() and not r["normal"].any() and not r["variation"].any() and (r["count"] == 8).all()
    skew = (np.arange(40, dtype=np.float64)[:, None] * np.array([1.0, 2.0, -3.0]) + 5.0).astype(np.float32)  # exact in float32
    for solver in (R.jacobi, R.eigh):
        assert not R.normals(None, skew, 6, BIG, same_cloud=True, solver=solver)["valid"].any()
    same = np.tile(np.array([[1.5, -2.0, 3.25]], np.float32), (9, 1))
    r = R.normals(None, same, 4, BIG, same_cloud=True)
    assert not r["valid"].any() and (r["count"] == 4).all() and not r["C"].any() and not r["normal"].any()
    for n in (1, 2):  # m < 3
        r = R.normals(None, R.sphere_cloud(n)[0], 4, BIG, same_cloud=True)
        assert not r["valid"].any() and (r["count"] == n - 1).all()
    r = R.normals(None, R.sphere_cloud(3)[0], 4, BIG, same_cloud=True)
    assert r["valid"].all() and (r["count"] == 2).all()
    # an outlier with fewer than two neighbours inside max_dist
    pts = np.concatenate([R.plane_cloud(), np.array([[100.0, 0.0, 0.0], [100.5, 0.0, 0.0]], np.float32)])
    r = R.normals(None, pts, 8, 3.0, same_cloud=True)
    assert r["valid"][:-2].all() and not r["valid"][-2:].any() and (r["count"][-2:] == 1).all()
    # line_ratio is the only tolerance: a thin strip is a line for a large ratio and a plane for 0
    strip = np.stack([np.arange(30.0), (np.arange(30) % 2) * 1e-3, np.zeros(30)], 1).astype(np.float32)
    assert not R.normals(None, strip, 8, BIG, same_cloud=True, line_ratio=1e-3)["valid"].any()
    assert R.normals(None, strip, 8, BIG, same_cloud=True, line_ratio=0.0)["valid"].all()


def test_neighbours_follow_the_tie_rank():
    """Equal squares go to the lower rank, whatever the index."""
    pts = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], np.float32)
    assert R.neighbours(None, pts, 2, BIG, True)[0].tolist() == [1, 2]
    assert R.neighbours(None, pts, 2, BIG, True, rank=[0, 4, 3, 2, 1])[0].tolist() == [4, 3]
    assert R.neighbours(None, pts, 6, 1.2, True)[0].tolist() == [1, 2, 3, 4, -1, -1]
    assert R.neighbours(pts[:1], pts, 2, BIG, False)[0].tolist() == [0, 1]


def test_viewpoint_rule():
    q = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 0.0, 5.0]], np.float32)
    views = np.array([[0.0, 0.0, 3.0], [0.0, 0.0, -3.0], [10.0, 4.0, 0.0]])
    j, e = R.nearest_viewpoint(q, views)
    assert j.tolist() == [0, 2, 0]  # the first query is equally far from 0 and 1: the lowest index
    assert np.array_equal(e, [[0, 0, 3], [0, 4, 0], [0, 0, -2]])
    n = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.6, 0.8]])
    out = R.orient(q, n, views)
    assert np.array_equal(out[0], n[0])        # faces it already
    assert np.array_equal(out[1], n[1])        # n . e == 0 exactly: the canonical sign stays
    assert np.array_equal(out[2], -n[2])       # the viewpoint is below
    assert np.array_equal(R.canonical(np.array([[-0.6, 0.0, 0.8], [0.5, -0.5, 0.1], [-0.5, 0.5, 0.5]])),
                          [[-0.6, 0.0, 0.8], [0.5, -0.5, 0.1], [0.5, -0.5, -0.5]])  # ties: the lowest axis decides


def test_cli_arguments(tmp_path, capsys):
    import cloud_normals as CN
    p = CN.build_parser()
    a = p.parse_args(["--input", "a.ply", "--output", "b.ply"])
    assert (a.k, a.max_dist, a.cell, a.orient, a.line_ratio, a.drop_degenerate) == (16, None, None, None, 1e-6, False)
    assert CN.resolve_orient(a) == "none"
    assert CN.resolve_orient(p.parse_args(["--input", "a", "--mvs_folder", "scan"])) == "cameras"
    a = p.parse_args(["--input", "a", "--viewpoint", "1", "2.5", "-3"])
    assert CN.resolve_orient(a) == "viewpoint" and a.viewpoint == [1.0, 2.5, -3.0]
    assert CN.resolve_orient(p.parse_args(["--input", "a", "--orient", "existing"])) == "existing"
    for bad in (["--orient", "cameras"], ["--orient", "viewpoint"], ["--orient", "none", "--mvs_folder", "s"],
                ["--orient", "existing", "--viewpoint", "0", "0", "0"], ["--mvs_folder", "s", "--viewpoint", "0", "0", "0"]):
        with pytest.raises(ValueError):
            CN.resolve_orient(p.parse_args(["--input", "a"] + bad))
    with pytest.raises(SystemExit):
        p.parse_args(["--input", "a", "--orient", "sideways"])
    # refusals that need neither the library nor a GPU
    src = str(tmp_path / "a.ply")
    open(src, "wb").close()
    for argv, word in ((["--input", src, "--output", "b.ply", "--k", "33"], "--k"),
                       (["--input", src, "--output", "b.ply", "--line_ratio", "-1"], "--line_ratio"),
                       (["--input", src, "--output", "b.ply", "--max_dist", "0"], "--max_dist"),
                       (["--input", src], "--output"),
                       (["--input", str(tmp_path / "none.ply"), "--output", "b.ply"], "no such file"),
                       (["--input", src, "--output", "b.ply", "--orient", "cameras"], "--mvs_folder"),
                       (["--input", src, "--output", "b.ply", "--mvs_folder", str(tmp_path)], "no camera files"),
                       (["--input", src, "--scan_list", "x.txt"], "folder")):
        assert CN.main(argv) == 2
        assert word in capsys.readouterr().err


def test_camera_centres(tmp_path):
    """-R^T t of the scan's camera files, in file-name order."""
    import cloud_normals as CN
    (tmp_path / "cams").mkdir()
    rng = np.random.default_rng(0)
    want = []
    for i in (3, 0):
        Rm = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        C = rng.uniform(-50.0, 50.0, 3)
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = Rm, -Rm @ C
        want.append((i, C))
        with open(tmp_path / "cams" / f"{i:08d}_cam.txt", "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(repr(float(v)) for v in row) for row in E) + "\n\nintrinsic\n"
                    "100 0 50\n0 100 40\n0 0 1\n\n1.0 2.0\n")
    got = CN.camera_centres(str(tmp_path))
    assert got.dtype == np.float64 and got.shape == (2, 3)
    for row, (_, C) in zip(got, sorted(want, key=lambda t: t[0])):
        assert np.abs(row - C).max() <= 1e-4  # the file's matrix is read as float32
    with pytest.raises(FileNotFoundError):
        CN.camera_centres(str(tmp_path / "cams"))
