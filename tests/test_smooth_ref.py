"""CPU checks of mesh smoothing and vertex normals on their numpy restatement tests/smooth_ref.py: the adjacency
against a brute-force set of edges, the boundary rule, what a step does to a regular grid, what the filters are for, and the refusals of
meshops, smooth_mesh.py and mesh.py --smooth that need no device.  tests/test_smooth_gpu.py holds the kernels to the same restatement."""
import os
import sys

import numpy as np
import pytest
import torch

import meshops_ref as M
import simplify_ref
import smooth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _product():
    from patchmatchnet_amd import _lib, meshops
    assert R.LONG_ROW == _lib.MESH_SMOOTH_LONG_ROW
    return meshops


def _meshes():
    return {"icosphere": M.icosphere(2), "grid": R.plane_grid(5, 4), "odd": R.odd_mesh()}


def _brute_edges(faces):
    """The set of directed pairs with different ends that the faces name, from sorted numpy arrays (no dictionary, no per-vertex set)."""
    f = np.asarray(faces, np.int64)
    pairs = np.concatenate([f[:, [p, q]] for p in range(3) for q in range(3) if p != q])
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    return np.unique(pairs, axis=0)  # sorted by (row, neighbour)


def test_header_table_and_constants_agree():
    from patchmatchnet_amd import _lib
    _product()
    hdr = open(os.path.join(ROOT, "include", "pmn_hip.h")).read()
    assert _lib.ABI_VERSION == 25 and "#define PMN_ABI_VERSION 25" in hdr
    assert f"#define PMN_MESH_SMOOTH_LONG_ROW {_lib.MESH_SMOOTH_LONG_ROW}" in hdr
    assert f"#define PMN_MESH_SMOOTH_MAX_STEPS {_lib.MESH_SMOOTH_MAX_STEPS}" in hdr
    assert _lib.MESH_SMOOTH_LONG_ROW == _lib.MESH_PLACE_LONG_RUN == R.LONG_ROW == simplify_ref.LONG_RUN
    for name, nargs in (("pmn_mesh_smooth", 12), ("pmn_mesh_vertex_normals", 10)):
        assert len(_lib.SIGNATURES[name]) == nargs
        decl = hdr[hdr.index(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") == nargs - 1, name
    assert "rounded once each in float64" in hdr and "never written" in hdr  # the step's arithmetic and the ping-pong are stated


@pytest.mark.parametrize("name", ["icosphere", "grid", "odd"])
def test_adjacency_is_the_set_of_edges(name):
    _product()
    v, f = _meshes()[name]
    starts, nbrs, boundary = R.adjacency(f, len(v))
    edges = _brute_edges(f)
    assert starts.dtype == np.int64 and nbrs.dtype == np.int32 and starts[0] == 0 and starts[-1] == len(nbrs) == len(edges)
    rows = np.repeat(np.arange(len(v)), np.diff(starts))
    assert np.array_equal(np.stack((rows, nbrs), 1), edges)  # distinct, ascending within a row, no self pair
    for g in (f[::-1], M.permute_faces(f, 1), np.concatenate([f, f[:3]])):  # a function of the SET of faces
        s2, n2, _ = R.adjacency(g, len(v))
        assert np.array_equal(s2, starts) and np.array_equal(n2, nbrs)
    assert np.array_equal(R.adjacency(M.permute_faces(f, 2), len(v))[2], boundary)


def test_boundary_vertices():
    _product()
    v, f = M.icosphere(2)
    assert not R.adjacency(f, len(v))[2].any()  # closed
    v, f = R.plane_grid(5, 4)
    assert np.array_equal(R.adjacency(f, len(v))[2], R.grid_rim(5, 4)) and R.grid_rim(5, 4).sum() == 18
    v, f = R.odd_mesh()
    starts, nbrs, boundary = R.adjacency(f, len(v))
    # the open tetrahedron: edge (1, 3) is named by the face that stands twice and so is no boundary edge, but 1 and 3 lie on others;
    # (4, 4, 1) makes 4 a neighbour of 1 and names no edge; 5 is isolated
    assert boundary.tolist() == [False, True, True, True, False, False]
    assert nbrs[starts[4]:starts[5]].tolist() == [1] and 4 in nbrs[starts[1]:starts[2]] and starts[5] == starts[6]


def test_a_regular_grid_interior_does_not_move():
    """Step 0.125: the six neighbours of an interior vertex are at +-x, +-y and +-(x + y), all exact, so the differences cancel exactly
    and the sum is 0.0 -- the vertex keeps its bits under any factor."""
    _product()
    v, f = R.plane_grid(9, 7)
    v = (v + np.float32([3.0, -2.0, 0.5])).astype(np.float32)
    starts, nbrs, boundary = R.adjacency(f, len(v))
    inner = ~R.grid_rim(9, 7)
    assert (np.diff(starts)[inner] == 6).all()
    for factor in (0.5, -0.53, 1.0):
        out = R.step(v, starts, nbrs, factor).astype(np.float32)
        assert out[inner].tobytes() == v[inner].tobytes()
        assert out[boundary].tobytes() != v[boundary].tobytes()  # the rim does move when it is not pinned
        pinned = R.step(v, starts, nbrs, factor, boundary).astype(np.float32)
        assert pinned.tobytes() == v.tobytes()


def test_what_the_filters_are_for():
    """icosphere(3) with radial noise of sigma 0.02: ten Taubin iterations at the defaults at least halve the RMS deviation of the radius
    and keep the mean radius within 0.01 of 1; ten Laplacian steps at 0.5 shrink the mean radius below 0.96."""
    _product()
    v, f = M.icosphere(3)
    noisy = R.noisy_sphere(v)
    rms0, mean0 = R.radius_stats(noisy)
    rms1, mean1 = R.radius_stats(R.taubin(noisy, f, 10))
    rms2, mean2 = R.radius_stats(R.laplacian(noisy, f, 10))
    print(f"radius RMS {rms0:.4f} -> {rms1:.4f} (Taubin, mean radius {mean1:.4f}); Laplacian: RMS {rms2:.4f}, mean radius {mean2:.4f}")
    assert rms1 <= rms0 / 2 and abs(mean1 - 1.0) <= 0.01
    assert mean2 < 0.96
    # zero iterations: a copy; and the input is not written
    keep = noisy.copy()
    assert R.taubin(noisy, f, 0).tobytes() == keep.tobytes() and noisy.tobytes() == keep.tobytes()


def test_reference_normals():
    _product()
    v, f = M.icosphere(3)
    n = R.normals(v, f)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-15
    assert (np.einsum("ij,ij->i", n, v.astype(np.float64)) > 0.99).all()  # outward winding: outward normals
    assert np.array_equal(R.normals(v, f, flip=True), -n)
    assert R.normals(v, M.permute_faces(f, 4)).tobytes() == n.tobytes()
    gap = np.abs(n.astype(np.longdouble) - R.normals(v, f, dtype=np.longdouble)).max()
    assert gap < 1e-15
    v, f = R.odd_mesh()
    n = R.normals(v, f)
    assert (n[4] == 0).all() and (n[5] == 0).all() and (np.linalg.norm(n[:4], axis=1) > 0.999).all()


def test_float64_agrees_with_the_extended_reference():
    _product()
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than float64 on this platform"
    v, f = M.icosphere(3)
    far = (R.noisy_sphere(v).astype(np.float64) + 1.0e4).astype(np.float32)
    starts, nbrs, _ = R.adjacency(f, len(v))
    for factor in (0.5, -0.53):
        gap = np.abs(R.step(far, starts, nbrs, factor).astype(np.longdouble) - R.step(far, starts, nbrs, factor, dtype=np.longdouble)).max()
        print(f"icosphere at 1e4, factor {factor}: max |float64 - longdouble| = {gap:.3e}")
        assert gap <= 4e-12  # two roundings at 1e4 (ulp64 1.8e-12); the differences themselves are exact


def test_refusals_that_need_no_device():
    from patchmatchnet_amd import PmnError
    mo = _product()
    v, f = M.icosphere(1)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    for lam in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(PmnError, match=r"lam must be in \(0, 1\]"):
            mo.smooth_taubin(tv, tf, lam=lam)
        with pytest.raises(PmnError, match=r"lam must be in \(0, 1\]"):
            mo.smooth_laplacian(tv, tf, lam=lam)
    for mu in (-0.5, 0.0, 0.6, float("nan"), float("-inf")):
        with pytest.raises(PmnError, match="mu must be finite and < -lam"):
            mo.smooth_taubin(tv, tf, lam=0.5, mu=mu)
    with pytest.raises(PmnError, match="iterations must be >= 0"):
        mo.smooth_taubin(tv, tf, iterations=-1)
    with pytest.raises(PmnError, match="boundary must be"):
        mo.smooth_taubin(tv, tf, boundary="mirror")
    with pytest.raises(PmnError, match="factor"):
        mo.smooth_steps(tv, tf, [0.5, float("inf")])
    for call in (lambda: mo.smooth_taubin(tv, tf), lambda: mo.smooth_laplacian(tv, tf), lambda: mo.vertex_normals(tv, tf),
                 lambda: mo.vertex_adjacency(tf, len(v)), lambda: mo.smooth_taubin(tv, tf, iterations=0)):
        with pytest.raises(PmnError, match="ROCm GPU|cuda|device"):
            call()


def test_smooth_mesh_py_arguments(tmp_path, capsys):
    import smooth_mesh
    from patchmatchnet_amd import ply
    v, f = M.icosphere(1)
    src = str(tmp_path / "in.ply")
    ply.write_ply_mesh(src, v, f)
    base = ["--input", src, "--output", str(tmp_path / "out.ply")]
    for extra, text in ((["--iterations", "-1"], "--iterations must be >= 0"), (["--lambda", "0"], "--lambda must be in (0, 1]"),
                        (["--lambda", "1.5"], "--lambda must be in (0, 1]"), (["--mu=-0.5"], "--mu must be finite and < -lambda"),
                        (["--lambda", "0.6", "--mu=-0.53"], "--mu must be finite and < -lambda")):
        assert smooth_mesh.main(base + extra) == 2
        assert "smooth_mesh.py: " + text in capsys.readouterr().err
    assert smooth_mesh.main(["--input", str(tmp_path / "none.ply"), "--output", src]) == 2
    assert "no such file" in capsys.readouterr().err
    for extra in (["--method", "median"], ["--boundary", "mirror"], ["--normals", "maybe"]):
        with pytest.raises(SystemExit):
            smooth_mesh.main(base + extra)
    capsys.readouterr()
    assert not os.path.exists(str(tmp_path / "out.ply"))
    # --method laplacian does not look at --mu
    args = smooth_mesh.build_parser().parse_args(base + ["--method", "laplacian", "--mu", "0"])
    assert (args.method, args.iterations, args.lam, args.boundary, args.normals) == ("laplacian", 10, 0.5, "fixed", "recompute")


def test_mesh_py_smooth_arguments(tmp_path):
    import mesh
    from patchmatchnet_amd import PmnError
    args = mesh.build_parser().parse_args(["--input_folder", str(tmp_path)])
    assert (args.smooth, args.smooth_lambda, args.smooth_mu, args.smooth_boundary) == (0, 0.5, -0.53, "fixed")
    for extra, text in ((["--smooth", "-1"], "--smooth must be >= 0"), (["--smooth", "3", "--smooth_lambda", "0"], "--smooth_lambda"),
                        (["--smooth", "3", "--smooth_mu=-0.5"], "--smooth_mu"), (["--smooth_mu=nan"], "--smooth_mu"),
                        (["--smooth_mu=-inf"], "--smooth_mu")):
        with pytest.raises(PmnError, match=text):
            mesh.main(["--input_folder", str(tmp_path)] + extra)
    with pytest.raises(SystemExit):
        mesh.build_parser().parse_args(["--input_folder", str(tmp_path), "--smooth_boundary", "mirror"])
    with pytest.raises(SystemExit):
        mesh.build_parser().parse_args(["--input_folder", str(tmp_path), "--smooth", "2.5"])
