"""GPU checks of the mesher space (tests/mesher_space.py): every row through the kernels of csrc/tsdf.hip against
the numpy oracle tests/tsdf_ref.py.  tests/test_mesher_space.py has shown on the CPU that the rows cover what they claim and that the
oracle is sound on them, so a failure here is the kernels'.

Gates -- none of them new.  Dense extraction: those of tests/test_tsdf_gpu.py (_compare_extraction: faces, vertex count and colour bytes
equal, positions within 2 float32 ulps and finite where the oracle's are, normals' zero pattern equal and the normals within 4 x the
oracle's own float32-vs-float64 difference), and the vmask / ntri planes of pmn_mt_count equal to the oracle's.  Pool extraction: the
dense kernels on the same planes pass those gates, and the pool's mesh equals theirs as a set of triangles, bit for bit, as in
tests/test_tsdf_sparse_gpu.py.  Exact integration: the planes a row claims equal the float32 oracle bit for bit -- the CPU test has shown
that float32 and float64 coincide there, so there is no rounding to allow for; any other plane falls under the 4 x own rule."""
import numpy as np
import pytest
import torch

import mesher_space as M
import tsdf_ref as R
import tsdf_sparse_ref as S
from test_tsdf_gpu import _compare_extraction

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    return torch.device("cuda")


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _host(mesh):
    return tuple(None if a is None else a.cpu().numpy() for a in mesh)


def _count(tsdf, weight, min_weight):
    """pmn_mt_count alone -> the vmask and ntri planes."""
    from patchmatchnet_amd import _lib, ops
    _, dims_p = ops._volume_planes(tsdf, weight, None, None, "mt_count")
    vmask, ntri = torch.empty(tsdf.shape, dtype=torch.uint8, device=tsdf.device), torch.empty(tsdf.shape, dtype=torch.uint8, device=tsdf.device)
    ops.check(_lib.lib().pmn_mt_count(tsdf.data_ptr(), weight.data_ptr(), dims_p, float(np.float32(min_weight)), vmask.data_ptr(),
                                      ntri.data_ptr(), ops._stream(tsdf)), "pmn_mt_count")
    torch.cuda.synchronize()
    return vmask.cpu().numpy(), ntri.cpu().numpy()


@pytest.mark.parametrize("row", M.EXTRACT_ROWS, ids=lambda r: r.id)
def test_dense_extraction_of_every_row(row):
    dev = _dev()
    x = row.inputs()
    o32 = M.oracle(row)
    _compare_extraction(row.name, x["tsdf"], x["weight"], x["origin"], x["voxel"], x["min_weight"], x["rgb"], x["cweight"],
                        oracles=(o32, M.oracle(row, True)), empty=row.empty)
    vmask, ntri = _count(_up(x["tsdf"], dev), _up(x["weight"], dev), x["min_weight"])
    print(f"{row.name}: vmask differs in {int((vmask != o32['vmask']).sum())} samples, ntri in {int((ntri != o32['ntri']).sum())}")
    assert np.array_equal(vmask, o32["vmask"]) and np.array_equal(ntri, o32["ntri"]), row.name


@pytest.mark.parametrize("absent", [False, True], ids=["all-blocks", "a-third-absent"])
@pytest.mark.parametrize("row", [r for r in M.EXTRACT_ROWS if r.pool], ids=lambda r: r.id)
def test_pool_extraction_of_every_row(row, absent):
    """The row's planes as a pool, every block allocated or a seeded random third of them absent (their samples then read as weight 0,
    tsdf 1): the dense kernels on those planes against the oracle, then the pool's mesh against the dense kernels' as a set."""
    from patchmatchnet_amd import ops
    dev = _dev()
    x = row.inputs()
    vol = {k: x[k] for k in ("tsdf", "weight", "rgb", "cweight")}
    keep = np.ones(S.n_blocks(row.dims)[::-1], bool)
    if absent:
        keep &= np.random.default_rng(row.seed).random(keep.shape) >= 1 / 3
        keep.reshape(-1)[0] |= not keep.any()  # a pool holds at least one block
    planes = S.restrict(vol, S.block_samples(keep, row.dims))
    args = (x["origin"], x["voxel"], x["min_weight"], planes["rgb"], planes["cweight"])
    o32, o64 = (R.extract(planes["tsdf"], planes["weight"], *args, True, T) for T in (np.float32, np.float64))
    name = f"{row.name} as a pool of {int(keep.sum())} of {keep.size} blocks"
    _compare_extraction(name, planes["tsdf"], planes["weight"], *args, oracles=(o32, o64), empty=len(o32["faces"]) == 0)
    ref = ops.mt_extract(_up(planes["tsdf"], dev), _up(planes["weight"], dev), *args[:3], _up(planes["rgb"], dev), _up(planes["cweight"], dev))
    p = {k: _up(a, dev) for k, a in S.pool_of(vol, keep).items()}
    got = ops.mt_extract_blocks(p["tsdf"], p["weight"], p["table"], p["blocks"], row.dims, *args[:3], p["rgb"], p["cweight"])
    torch.cuda.synchronize()
    print(f"{name}: {got[0].shape[0]} vertices, {got[1].shape[0]} faces from the pool, {ref[0].shape[0]} and {ref[1].shape[0]} from the planes")
    assert got[1].shape[0] == len(o32["faces"]) and got[1].dtype == torch.int32 and got[0].dtype == torch.float32
    assert (got[2] is None) == (x["rgb"] is None) and got[3] is not None
    S.assert_same_mesh(_host(got), _host(ref), name)


def _upload(views, dev):
    stride = max(v[0].size for v in views)
    maps = torch.zeros((len(views), stride))
    for n, v in enumerate(views):
        maps[n, :v[0].size] = torch.from_numpy(v[0].reshape(-1).copy())
    return maps.to(dev), [v[0].shape for v in views], np.stack([v[1] for v in views]), [_up(v[2], dev) for v in views], [_up(v[3], dev) for v in views]


def _full_pool(row, dev):
    """A SparseTsdfVolume of the row's lattice with every block allocated."""
    from patchmatchnet_amd import tsdf
    vol = tsdf.SparseTsdfVolume(row.origin, row.voxel, row.dims, row.trunc, dev, color=True)
    nbx, nby, nbz = vol.nblocks
    B = nbx * nby * nbz
    vol.blocks = torch.arange(B, dtype=torch.int32, device=dev)
    vol.table = vol.blocks.clone().view(nbz, nby, nbx)
    shape = (B, 8, 8, 8)
    vol.tsdf, vol.weight = torch.ones(shape, device=dev), torch.zeros(shape, device=dev)
    vol.rgb, vol.cweight = torch.zeros((3,) + shape, device=dev), torch.zeros(shape, device=dev)
    return vol


@pytest.mark.parametrize("volume", ["dense", "blocks"])
@pytest.mark.parametrize("launches", ["view-by-view", "one-launch"])
@pytest.mark.parametrize("row", M.EXACT_ROWS, ids=lambda r: r.id)
def test_exact_integration_of_every_row(row, launches, volume):
    from patchmatchnet_amd import tsdf
    dev = _dev()
    views = row.views()
    maps, sizes, cams, masks, images = _upload(views, dev)
    vol = tsdf.TsdfVolume(row.origin, row.voxel, row.dims, row.trunc, dev, color=True) if volume == "dense" else _full_pool(row, dev)
    vol.integrate(maps, list(range(len(views))), sizes, cams, masks, images, batch=1 if launches == "view-by-view" else len(views))
    torch.cuda.synchronize()
    planes = (vol.tsdf, vol.weight, vol.rgb, vol.cweight) if volume == "dense" else vol.to_dense()
    got = {k: a.cpu().numpy() for k, a in zip(("tsdf", "weight", "rgb", "cweight"), planes)}
    o32, o64 = M.oracle_volume(row, np.float32), M.oracle_volume(row, np.float64)
    for k in M.PLANES:
        differ = int((got[k].view(np.uint32) != o32[k].view(np.uint32)).sum())
        print(f"{row.name} {volume} {launches}: {k} differs from the float32 oracle in the bits of {differ} of {got[k].size} samples")
        if k in row.claims:
            assert got[k].tobytes() == o32[k].tobytes(), k
        else:
            own = float(np.abs(o32[k].astype(np.float64) - o64[k]).max())
            err = float(np.abs(got[k].astype(np.float64) - o64[k]).max())
            print(f"    oracle f32-vs-f64 {own:.3e}, kernel-vs-f64 {err:.3e} (gate {4 * own:.3e})")
            assert err <= 4 * own, k
