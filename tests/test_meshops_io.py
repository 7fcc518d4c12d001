"""CPU checks of the mesh operations: the numpy yardstick tests/meshops_ref.py against hand-worked cases and
its own statistical contract, the new command-line flags, and what patchmatchnet_amd/meshops.py does with host tensors."""
import os
import sys

import numpy as np
import pytest
import torch

import meshops_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TET = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]


def test_components_ref_on_hand_worked_cases():
    # two tetrahedra that share vertex 3: one component
    shared = np.array(TET + [[3, 5, 4], [3, 4, 6], [3, 6, 5], [4, 5, 6]], np.int32)
    assert M.components_ref(shared, 7).tolist() == [0] * 7
    # two tetrahedra that share no vertex, and an unreferenced vertex: three components
    apart = np.array(TET + [[5, 7, 6], [5, 6, 8], [5, 8, 7], [6, 7, 8]], np.int32)
    assert M.components_ref(apart, 9).tolist() == [0, 0, 0, 0, 4, 5, 5, 5, 5]
    label, roots, count = M.component_sizes_ref(apart, 9)
    assert roots.tolist() == [0, 4, 5] and count.tolist() == [4, 0, 4]
    # degenerate faces: (a, a, b) unites, (a, a, a) does not; labels are minima whatever the face order
    assert M.components_ref(np.array([[4, 4, 2], [1, 1, 1], [3, 0, 0]], np.int32), 5).tolist() == [0, 1, 2, 0, 2]
    v, f = M.strip(50)
    assert M.components_ref(f[::-1], 52).tolist() == [0] * 52
    v2, f2, new = M.relabel_vertices(*M.join(M.tetrahedra(3), M.strip(4)), seed=1)
    lab, lab2 = M.components_ref(M.join(M.tetrahedra(3), M.strip(4))[1], 18), M.components_ref(f2, 18)
    for a in range(18):
        for b in range(18):
            assert (lab[a] == lab[b]) == (lab2[new[a]] == lab2[new[b]])
    assert all(lab2[x] == min(y for y in range(18) if lab2[y] == lab2[x]) for x in range(18))


def test_remove_components_ref():
    v, f = M.join(M.tetrahedra(2), M.strip(6), (np.zeros((1, 3), np.float32), np.zeros((0, 3), np.int32)), M.tetrahedra(1))
    col = np.arange(len(v) * 3, dtype=np.uint8).reshape(-1, 3)
    # sizes: 4, 4, 6, 0, 4 faces with roots 0, 4, 8, 16, 17
    v2, f2, c2, n2, found, kept = M.remove_components_ref(v, f, col, None, min_faces=5)
    assert (found, kept) == (5, 1) and len(v2) == 8 and np.array_equal(f2, M.strip(6)[1]) and np.array_equal(c2, col[8:16]) and n2 is None
    v2, f2, _, _, found, kept = M.remove_components_ref(v, f, keep_largest=2)  # the strip, then the tie 4 = 4 = 4 goes to root 0
    assert kept == 2 and len(v2) == 12 and np.array_equal(f2[:4], M.tetrahedra(1)[1]) and np.array_equal(f2[4:], M.strip(6)[1] + 4)
    v2, f2, _, _, _, kept = M.remove_components_ref(v, f, min_faces=5, keep_largest=1)
    assert kept == 1 and len(f2) == 6
    v2, f2, _, _, _, kept = M.remove_components_ref(v, f, min_faces=1)  # only the unreferenced vertex goes
    assert kept == 4 and len(v2) == len(v) - 1 and len(f2) == len(f) and f2.max() == len(v2) - 1


def test_hash_is_the_documented_one():
    # splitmix64's own test vector: seed 0 -> first output mix(0 + G) (Vigna's reference stream)
    assert int(M.mix64(np.uint64(M.GOLDEN))) == 0xE220A8397B1DCDAF
    r1, r2 = M.uniforms(7, np.arange(1000), np.arange(1000) % 17)
    assert r1.dtype == np.float32 and (r1 >= 0).all() and (r1 < 1).all() and (r2 >= 0).all() and (r2 < 1).all()
    assert np.array_equal(r1 * np.float32(2 ** 24), np.floor(r1 * np.float32(2 ** 24)))  # integers times 2^-24
    assert 0.45 < r1.mean() < 0.55 and 0.45 < r2.mean() < 0.55
    a, _ = M.uniforms(7, [3], [5])
    b, _ = M.uniforms(8, [3], [5])
    c, _ = M.uniforms(7, [5], [3])
    assert a[0] != b[0] and a[0] != c[0]


def test_sample_ref_properties_on_an_icosphere():
    v, f = M.icosphere(3)
    assert len(f) == 1280 and len(v) == 642
    area64 = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]].astype(np.float64) - v[f[:, 0]], v[f[:, 2]].astype(np.float64) - v[f[:, 0]]), axis=1)
    density = 20000.0 / area64.sum()
    col = np.random.default_rng(0).integers(0, 256, (len(v), 3), dtype=np.uint8)
    pts, face, c, bary = M.sample_ref(v, f, density, seed=11, colors=col, return_bary=True)
    n = len(pts)
    bound = 3 * np.sqrt(len(f)) + 1e-5 * density * area64.sum()
    print(f"icosphere 1280 faces: {n} samples, expected {density * area64.sum():.1f}, bound {bound:.1f}")
    assert abs(n - density * area64.sum()) <= bound
    assert pts.dtype == np.float32 and face.dtype == np.int32 and c.dtype == np.uint8 and c.shape == (n, 3)
    assert (bary >= 0).all()
    assert np.abs(bary.astype(np.float64).sum(1) - 1).max() <= 4 * 2.0 ** -24  # 4 ulp of float32 at 1
    assert (np.diff(face) >= 0).all()  # ordered by face
    r = np.linalg.norm(pts.astype(np.float64), axis=1)
    assert r.max() <= 1 + 1e-6 and r.min() > 0.98  # on the chords of the unit sphere
    # the same seed gives the same cloud, another seed another
    again = M.sample_ref(v, f, density, seed=11)
    other = M.sample_ref(v, f, density, seed=12)
    assert np.array_equal(again[0], pts) and not np.array_equal(other[0][:100], pts[:100])
    # zero-area and non-finite faces get nothing
    v2 = np.concatenate([v, [[np.nan, 0, 0]]]).astype(np.float32)
    f2 = np.concatenate([f, [[0, 0, 1], [0, 1, 642]]]).astype(np.int32)
    assert M.face_counts_ref(v2, f2, density, 11)[-2:].tolist() == [0, 0]


def test_command_lines_accept_the_new_flags():
    import eval_dtu
    import eval_tnt
    import mesh
    a = mesh.build_parser().parse_args(["--input_folder", "x"])
    assert a.min_component_faces == 0 and a.keep_components == 0
    a = mesh.build_parser().parse_args(["--input_folder", "x", "--min_component_faces", "50", "--keep_components", "2"])
    assert a.min_component_faces == 50 and a.keep_components == 2
    base = ["--dataset_dir", "d/Barn", "--ply_path", "p.ply", "--results_path", "r", "--no_registration"]
    a = eval_tnt.parse_args(base)
    assert a.sample_spacing == 0.0 and a.sample_seed == 0
    a = eval_tnt.parse_args(base + ["--sample_spacing", "0.004", "--sample_seed", "9"])
    assert a.sample_spacing == 0.004 and a.sample_seed == 9
    base = ["--data_path", "d", "--ply_path", "p", "--results_path", "r"]
    a = eval_dtu.parse_args(base)
    assert a.sample_spacing == 0.0 and a.sample_seed == 0 and a.ply_name == "fused.ply"
    a = eval_dtu.parse_args(base + ["--sample_spacing", "0.2", "--sample_seed", "3", "--ply_name", "mesh.ply"])
    assert a.sample_spacing == 0.2 and a.sample_seed == 3 and a.ply_name == "mesh.ply"
    a.scans = [7]
    with pytest.raises(FileNotFoundError, match="scan7/mesh.ply".replace("/", os.sep)):
        eval_dtu.scan_inputs(a, 7)


def test_host_tensors():
    """remove_components(min_faces=0, keep_largest=0) is the identity on ANY tensors (the very same objects come back, nothing is
    launched); everything else is the product's usual refusal of a tensor that is not on a ROCm GPU."""
    from patchmatchnet_amd import PmnError, meshops
    v, f = M.tetrahedra(2)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    col, nrm = torch.zeros((8, 3), dtype=torch.uint8), torch.zeros((8, 3))
    out = meshops.remove_components(tv, tf, col, nrm)
    assert out[0] is tv and out[1] is tf and out[2] is col and out[3] is nrm and len(out) == 4
    for call in (lambda: meshops.remove_components(tv, tf, min_faces=1), lambda: meshops.remove_components(tv, tf, keep_largest=1),
                 lambda: meshops.components(tf, 8), lambda: meshops.sample_surface(tv, tf, density=10.0)):
        with pytest.raises(PmnError, match="ROCm GPU"):
            call()
    with pytest.raises(PmnError, match="exactly one"):
        meshops.sample_surface(tv, tf)
    with pytest.raises(PmnError, match="exactly one"):
        meshops.sample_surface(tv, tf, density=1.0, spacing=1.0)
    with pytest.raises(PmnError, match="positive"):
        meshops.sample_surface(tv, tf, spacing=0.0)
    with pytest.raises(PmnError, match=">= 0"):
        meshops.remove_components(tv, tf, min_faces=-1)


def test_entry_points_reject_bad_arguments_without_a_launch():
    from patchmatchnet_amd import _lib
    L = _lib.lib()
    assert L.pmn_mesh_components(None, 0, 4, None, None, None) == -1
    assert L.pmn_mesh_components(None, 3, 4, 8, 8, None) == -1          # faces missing
    assert L.pmn_mesh_components(8, 3, 0, 8, 8, None) == -2             # no vertex
    assert L.pmn_mesh_face_samples(8, 4, 8, 4, -1.0, 0, 8, 8, None) == -1
    assert L.pmn_mesh_face_samples(8, 4, 8, 4, float("nan"), 0, 8, 8, None) == -1
    assert L.pmn_mesh_face_samples(8, 4, 8, 0, 1.0, 0, 8, 8, None) == -2
    assert L.pmn_mesh_sample(8, 4, 8, 4, None, 8, 0, 0, 8, 8, None, None) == -2
    assert L.pmn_mesh_sample(8, 4, 8, 4, None, 8, 5, 0, 8, 8, 8, None) == -1  # colours out without colours in
