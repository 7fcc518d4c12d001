"""CPU checks of the block-sparse volume: the marking rule restated in numpy (tests/tsdf_sparse_ref.py) covers
the exact band, the equality argument holds on the numpy oracle, and the entry points, wrappers and mesh.py refuse what they must.  The
kernels themselves are compared with the dense path in tests/test_tsdf_sparse_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

import synth
import tsdf_ref as R
import tsdf_sparse_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from patchmatchnet_amd import PmnError, _lib, ops, tsdf  # noqa: E402


@pytest.mark.parametrize("kind", ["A", "B"])
def test_numpy_marking_covers_the_band_and_the_dilated_set_gives_the_dense_mesh(kind):
    views = S.scene(kind)
    need = S.needed_views(S.DIMS, S.ORIGIN, S.VOXEL, S.TRUNC, views)
    mark, over = S.mark_views(S.DIMS, S.ORIGIN, S.VOXEL, S.TRUNC, views)
    dil = S.dilate(mark)
    print(f"scene {kind}: {int(need.sum())} blocks needed, {int(mark.sum())} marked ({mark.sum() / need.sum():.2f} x), "
          f"{int(dil.sum())} after the dilation ({dil.sum() / need.sum():.2f} x) of {need.size}")
    assert over == 0 and need.sum() > 20
    assert not (need & ~mark).any(), "the marking rule misses a block of the band"
    if kind == "B":  # the plane leaves the lattice: blocks on its border are marked and boxes are clipped
        assert mark[:, :, 0].any() and mark[:, :, -1].any()
    # the equality argument: the dense planes restricted to the dilated set give the dense mesh
    vol = S.dense_volume(S.DIMS, S.ORIGIN, S.VOXEL, S.TRUNC, views)
    dense = S.mesh_of(vol, S.ORIGIN, S.VOXEL)
    sparse = S.mesh_of(S.restrict(vol, S.block_samples(dil, S.DIMS)), S.ORIGIN, S.VOXEL)
    assert len(dense[1]) > 3000
    S.assert_same_mesh(dense, sparse, f"scene {kind}")
    # ... and the comparison does see a missing block: drop one the surface passes through
    holed = dil.copy()
    holed[tuple(np.argwhere(need)[len(np.argwhere(need)) // 2])] = False
    with pytest.raises(AssertionError):
        S.assert_same_mesh(dense, S.mesh_of(S.restrict(vol, S.block_samples(holed, S.DIMS)), S.ORIGIN, S.VOXEL))


def test_soup_is_free_of_order_and_keeps_the_winding():
    f = R.sphere_field(16, (7.3, 8.1, 7.7), 4.4)
    m = R.extract(f, np.ones_like(f), (0, 0, 0), 1.0)
    rng = np.random.default_rng(0)
    col = rng.integers(0, 256, (len(m["vertices"]), 3), dtype=np.uint8)
    a = (m["vertices"], m["faces"], col, m["normals"])
    perm = rng.permutation(len(a[0]))
    inv = np.argsort(perm)
    faces = np.roll(inv[a[1]][rng.permutation(len(a[1]))], 1, axis=1)  # vertices and faces shuffled, every triangle rotated
    S.assert_same_mesh(a, (a[0][perm], faces, col[perm], a[3][perm]))
    with pytest.raises(AssertionError):  # a flipped triangle
        S.assert_same_mesh(a, (a[0], np.concatenate((a[1][:1, ::-1], a[1][1:])), col, a[3]))
    with pytest.raises(AssertionError):  # a duplicated, unreferenced vertex
        S.assert_same_mesh(a, (np.concatenate((a[0], a[0][:1])), a[1], np.concatenate((col, col[:1])), np.concatenate((a[3], a[3][:1]))))
    with pytest.raises(AssertionError):  # one colour byte
        c2 = col.copy()
        c2[5, 1] ^= 1
        S.assert_same_mesh(a, (a[0], a[1], c2, a[3]))


def test_entry_points_reject_bad_arguments_without_launching():
    L = _lib.lib()
    assert L.pmn_tsdf_mark_blocks(None, None, None, None, 1.0, 1.0, None, 1, None, None, None, None, 1, None) == -1
    assert L.pmn_tsdf_integrate_blocks(None, None, None, None, None, 1, None, None, 1.0, 1.0, None, 1, None, None, None, None, None, 1,
                                       None) == -1
    assert L.pmn_mt_count_blocks(None, None, None, None, 1, None, 1.0, None, None, None) == -1
    assert L.pmn_mt_emit_blocks(None, None, None, None, None, None, 1, None, None, 1.0, 1.0, *([None] * 9)) == -1
    hdr = open(os.path.join(ROOT, "include", "pmn_hip.h")).read()
    assert "#define PMN_TSDF_MARK_SPAN 8" in hdr and _lib.TSDF_MARK_SPAN == 8 and S.MARK_SPAN == 8
    assert "#define PMN_ABI_VERSION 25" in hdr


def test_wrappers_and_volume_refuse_host_tensors_and_bad_arguments():
    with pytest.raises(PmnError, match="ROCm GPU"):
        tsdf.SparseTsdfVolume((0, 0, 0), 1.0, (64, 64, 64), 4.0, "cpu")
    cam = np.concatenate((np.eye(3).reshape(9), np.eye(4)[:3].reshape(12)))[None]
    maps = torch.zeros(1, 16)
    with pytest.raises(PmnError):
        ops.tsdf_mark_blocks(torch.zeros(1, 1, 1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), (8, 8, 8), (0, 0, 0), 1.0, 4.0,
                             maps, [0], [(4, 4)], cam)
    pool = torch.ones(1, 8, 8, 8)
    with pytest.raises(PmnError):
        ops.tsdf_integrate_blocks(pool, torch.zeros_like(pool), None, None, torch.zeros(1, dtype=torch.int32), (8, 8, 8), (0, 0, 0), 1.0,
                                  4.0, maps, [0], [(4, 4)], cam)
    with pytest.raises(PmnError):
        ops.mt_extract_blocks(pool, torch.zeros_like(pool), torch.zeros(1, 1, 1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                              (8, 8, 8), (0, 0, 0), 1.0)
    # the lattice limits: 2 .. 2^19 - 1 samples per axis, at most 2^28 blocks
    assert ops.sparse_blocks((40, 48, 56)) == (5, 6, 7) and ops.sparse_blocks((41, 9, 2)) == (6, 2, 1)
    for dims in ((1, 8, 8), (2 ** 19, 8, 8), (2 ** 13 * 8, 2 ** 13 * 8, 2 ** 3 * 8)):
        with pytest.raises(PmnError):
            ops.sparse_blocks(dims)
    # the cameras are inverted in float64: K^-1, then the camera-to-world 3 x 4
    K, E = R.rig(2, 48, 64, (0.1, 0.2, 4.0), 3.0)
    inv = ops.inverse_cameras(np.stack([tsdf.camera21(K[v], E[v]) for v in range(2)]))
    for v in range(2):
        np.testing.assert_allclose(inv[v, :9].reshape(3, 3) @ K[v].astype(np.float64), np.eye(3), atol=1e-5)
        np.testing.assert_allclose((E[v].astype(np.float64) @ np.vstack((inv[v, 9:].reshape(3, 4), [0, 0, 0, 1])))[:3], np.eye(4)[:3],
                                   atol=1e-5)
    with pytest.raises(PmnError):
        ops.inverse_cameras(np.zeros((1, 21)))


def test_mesh_py_sparse_arguments(tmp_path):
    import mesh
    scan = synth.write_scan(str(tmp_path), "scanA", 3, 48, 64)
    args = mesh.build_parser().parse_args(["--input_folder", scan])
    assert args.volume == "dense" and args.max_blocks == 2 ** 20 == tsdf.MAX_BLOCKS
    with pytest.raises(PmnError, match="ROCm GPU"):
        mesh.main(["--input_folder", scan, "--volume", "sparse", "--device", "cpu"])
    with pytest.raises(PmnError, match="max_blocks"):
        mesh.main(["--input_folder", scan, "--volume", "sparse", "--max_blocks", "0"])
    with pytest.raises(SystemExit):
        mesh.build_parser().parse_args(["--input_folder", scan, "--volume", "hashed"])
    # the virtual lattice is what choose_grid bounds in sparse mode: the natural voxel survives where --max_voxels would enlarge it
    pts = torch.rand(2001, 3, generator=torch.Generator().manual_seed(0)) * 40.0
    foot = torch.full((2001,), 0.005)
    _, v_dense, _, _, note = tsdf.choose_grid(pts, foot)
    _, v_sparse, _, dims, note2 = tsdf.choose_grid(pts, foot, None, None, None, tsdf.MAX_VIRTUAL_VOXELS, "the virtual lattice's",
                                                   ops.SPARSE_MAX_AXIS - 1)
    assert note is not None and v_dense > 0.04 and note2 is None and abs(v_sparse - 0.01) < 1e-7
    assert ops.sparse_blocks(dims) and dims[0] * dims[1] * dims[2] > 2 ** 29
