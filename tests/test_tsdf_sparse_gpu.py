"""GPU checks of the block-sparse volume.  The yardstick is the dense path -- pmn_tsdf_integrate, pmn_mt_count and
pmn_mt_emit, which tests/test_tsdf_gpu.py pins to the numpy oracle: every plane of every allocated block equals the dense volume's
samples bit for bit, and the mesh equals the dense mesh as a set of triangles (tests/tsdf_sparse_ref.py: position, normal and colour
bits per corner, winding kept).  No tolerance anywhere: the kernels share the arithmetic."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import synth
import tsdf_ref as R
import tsdf_sparse_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _dev():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    return torch.device("cuda")


def _upload(views, dev):
    """-> maps [V,F], sizes, cams [V,21], masks, images (lists of device tensors or None entries)."""
    stride = max(v[0].size for v in views)
    maps = torch.zeros((len(views), stride))
    for n, v in enumerate(views):
        maps[n, :v[0].size] = torch.from_numpy(v[0].reshape(-1).copy())
    up = lambda a: None if a is None else torch.from_numpy(a.copy()).to(dev)
    return maps.to(dev), [v[0].shape for v in views], np.stack([v[1] for v in views]), [up(v[2]) for v in views], [up(v[3]) for v in views]


def _host(mesh):
    return tuple(None if a is None else a.cpu().numpy() for a in mesh)


def _blocked(plane, blocks):
    """The samples of a dense [nz,ny,nx] plane (sides multiples of 8) in pool layout: [B,8,8,8] of the listed blocks."""
    nz, ny, nx = plane.shape
    p = plane.view(nz // 8, 8, ny // 8, 8, nx // 8, 8).permute(0, 2, 4, 1, 3, 5).reshape(-1, 8, 8, 8)
    return p[blocks.long()]


def _pair(kind, color, masks, batch=4, dims=S.DIMS):
    """Scene A or B through both volumes on the lattice ``dims`` -> (sparse, dense)."""
    from patchmatchnet_amd import tsdf
    dev = _dev()
    maps, sizes, cams, dmasks, dimages = _upload(S.scene(kind), dev)
    slots = list(range(len(sizes)))
    sp = tsdf.SparseTsdfVolume(S.ORIGIN, S.VOXEL, dims, S.TRUNC, dev, color=color)
    sp.allocate(maps, slots, sizes, cams, dmasks if masks else None)
    sp.integrate(maps, slots, sizes, cams, dmasks if masks else None, dimages if color else None, batch=batch)
    de = tsdf.TsdfVolume(S.ORIGIN, S.VOXEL, dims, S.TRUNC, dev, color=color)
    de.integrate(maps, slots, sizes, cams, dmasks if masks else None, dimages if color else None, batch=batch)
    return sp, de


@pytest.mark.parametrize("kind", ["A", "B"])
def test_marked_blocks_cover_the_band_and_stay_within_the_rule(kind):
    from patchmatchnet_amd import ops
    dev = _dev()
    views = S.scene(kind)
    maps, sizes, cams, dmasks, _ = _upload(views, dev)
    nbx, nby, nbz = S.n_blocks(S.DIMS)
    flags = torch.zeros((nbz, nby, nbx), dtype=torch.uint8, device=dev)
    over = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.tsdf_mark_blocks(flags, over, S.DIMS, S.ORIGIN, S.VOXEL, S.TRUNC, maps, list(range(len(views))), sizes, cams, dmasks)
    got = flags.cpu().numpy()
    assert set(np.unique(got)) <= {0, 1} and int(over.item()) == 0
    got = got.astype(bool)
    need = S.needed_views(S.DIMS, S.ORIGIN, S.VOXEL, S.TRUNC, views)
    rule, rule_over = S.mark_views(S.DIMS, S.ORIGIN, S.VOXEL, S.TRUNC, views)
    print(f"scene {kind}: needed {int(need.sum())}, kernel {int(got.sum())}, numpy rule {int(rule.sum())}, "
          f"kernel == rule: {np.array_equal(got, rule)}")
    assert rule_over == 0 and need.sum() > 20
    assert not (need & ~got).any(), "a block of the band is not marked"
    assert not (got & ~S.dilate(rule)).any(), "a marked block is more than one block away from the rule's set"
    # marking accumulates: a second launch with one view changes nothing
    ops.tsdf_mark_blocks(flags, over, S.DIMS, S.ORIGIN, S.VOXEL, S.TRUNC, maps, [0], sizes[:1], cams[:1], dmasks[:1])
    assert np.array_equal(flags.cpu().numpy().astype(bool), got)


def test_a_section_wider_than_the_span_is_counted_and_allocate_raises():
    """One pixel of depth 3 seen through a focal length of 9 pixels covers 0.33 units = 166 voxels of 0.002 inside the user's
    1024^3 lattice: more than PMN_TSDF_MARK_SPAN blocks, so it is counted instead of marked."""
    from patchmatchnet_amd import PmnError, tsdf
    dev = _dev()
    dims, voxel, trunc = (1024, 1024, 1024), 0.002, 0.008
    origin = np.array([-1.024, -1.024, 3.0], np.float32)
    centre = origin.astype(np.float64) + 1.024
    K, E = R.rig(1, 8, 10, centre, 3.0)
    d = np.zeros((8, 10), np.float32)
    d[6, 2] = 3.0  # next to the principal point (2, 6): the ray ends near the lattice's centre
    views = [(d, R.cam21(K[0], E[0]), None, None)]
    assert S.mark_views(dims, origin, voxel, trunc, views, masks=False)[1] == 1
    maps, sizes, cams, _, _ = _upload(views, dev)
    vol = tsdf.SparseTsdfVolume(origin, voxel, dims, trunc, dev, color=False)
    with pytest.raises(PmnError, match="1 pixels"):
        vol.allocate(maps, [0], sizes, cams)
    # a depth whose section misses the lattice is nobody's business: nothing is counted, nothing is marked
    d2 = np.zeros((8, 10), np.float32)
    d2[6, 2] = 1e30
    maps, sizes, cams, _, _ = _upload([(d2, views[0][1], None, None)], dev)
    with pytest.raises(PmnError, match="0 blocks"):
        tsdf.SparseTsdfVolume(origin, voxel, dims, trunc, dev, color=False).allocate(maps, [0], sizes, cams)


@pytest.mark.parametrize("kind", ["A", "B"])
@pytest.mark.parametrize("color,masks", [(True, True), (False, False)])
def test_allocated_blocks_hold_the_dense_volume_bits(kind, color, masks):
    sp, de = _pair(kind, color, masks)
    B = sp.blocks.numel()
    assert 20 < B <= 210 and sp.needed == B and sp.marked <= B
    assert torch.equal(sp.table.view(-1)[sp.blocks.long()], torch.arange(B, dtype=torch.int32, device=sp.device))
    assert int((sp.table >= 0).sum()) == B and bool((sp.blocks[1:] > sp.blocks[:-1]).all())
    assert float(sp.weight.max()) >= 4 and bool((sp.weight == 0).any())
    for k in ("tsdf", "weight") + (("cweight",) if color else ()):
        assert torch.equal(getattr(sp, k), _blocked(getattr(de, k), sp.blocks)), k
    if color:
        assert float(sp.cweight.max()) >= 3
        for ch in range(3):
            assert torch.equal(sp.rgb[ch], _blocked(de.rgb[ch], sp.blocks)), ch
    # to_dense: the pool where allocated, tsdf 1 / weight 0 elsewhere
    t, w, rgb, cw = sp.to_dense()
    alloc = torch.from_numpy(S.block_samples((sp.table >= 0).cpu().numpy(), S.DIMS)).to(sp.device)
    assert torch.equal(t, torch.where(alloc, de.tsdf, torch.ones_like(t))) and torch.equal(w, torch.where(alloc, de.weight, torch.zeros_like(w)))
    assert (rgb is None) == (not color) and (cw is None) == (not color)
    if color:
        assert torch.equal(rgb, torch.where(alloc[None], de.rgb, torch.zeros_like(rgb)))


@pytest.mark.parametrize("V", [1, 3, 4])
def test_batched_block_integration_equals_sequential(V):
    from patchmatchnet_amd import tsdf
    dev = _dev()
    maps, sizes, cams, dmasks, dimages = _upload(S.scene("A"), dev)
    slots = list(range(len(sizes)))
    vols = []
    for batch in (V, 1):
        vol = tsdf.SparseTsdfVolume(S.ORIGIN, S.VOXEL, S.DIMS, S.TRUNC, dev)
        vol.allocate(maps, slots, sizes, cams, dmasks)
        vol.integrate(maps, slots[:V], sizes[:V], cams[:V], dmasks[:V], dimages[:V], batch=batch)
        vols.append(vol)
    a, b = vols
    assert float(a.weight.max()) >= min(V, 2) and torch.equal(a.blocks, b.blocks)
    for k in ("tsdf", "weight", "cweight", "rgb"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def _pool_volume(field, weight, rgb, cweight, keep, dev):
    """A SparseTsdfVolume whose pool holds the given dense planes in the blocks ``keep`` ([nbz,nby,nbx] bool)."""
    from patchmatchnet_amd import tsdf
    n = field.shape[0]
    vol = tsdf.SparseTsdfVolume((-3.25, 100.5, 0.125), 0.37, (n, n, n), 1.0, dev, color=rgb is not None)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vol.blocks = up(np.nonzero(keep.reshape(-1))[0].astype(np.int32))
    B = vol.blocks.numel()
    vol.table = torch.full(keep.shape, -1, dtype=torch.int32, device=dev)
    vol.table.view(-1)[vol.blocks.long()] = torch.arange(B, dtype=torch.int32, device=dev)
    vol.tsdf, vol.weight = _blocked(up(field), vol.blocks).contiguous(), _blocked(up(weight), vol.blocks).contiguous()
    if rgb is not None:
        vol.rgb = torch.stack([_blocked(up(rgb[c]), vol.blocks) for c in range(3)]).contiguous()
        vol.cweight = _blocked(up(cweight), vol.blocks).contiguous()
    return vol


@pytest.mark.parametrize("shape", ["sphere", "torus"])
@pytest.mark.parametrize("holes", [False, True])
def test_extraction_over_a_pool_equals_extraction_of_its_dense_planes(shape, holes):
    from patchmatchnet_amd import ops
    dev = _dev()
    c = (19.3, 20.1, 19.7)
    f = R.sphere_field(40, c, 13.4) if shape == "sphere" else R.torus_field(40, c, 11.2, 4.3)
    rng = np.random.default_rng(5)
    w = rng.integers(0, 4, f.shape).astype(np.float32)
    w[rng.random(f.shape) < 0.9] = 3
    rgb = rng.uniform(0, 255, (3,) + f.shape).astype(np.float32)
    cw = (rng.random(f.shape) > 0.2).astype(np.float32) * 2
    surface = S.block_any((f < 0)) & S.block_any((f >= 0))  # blocks the surface passes through
    keep = np.ones((5, 5, 5), bool)
    keep[::4, ::4, ::4] = False                               # the eight corner blocks: far from both surfaces
    assert not (surface & ~keep).any()
    if holes:
        drop = np.argwhere(surface)[::3]  # 14 of the sphere's 41 surface blocks, 7 of the torus's 20
        keep[tuple(drop.T)] = False
        assert (surface & ~keep).sum() >= 5
    vol = _pool_volume(f, w, rgb, cw, keep, dev)
    t, wt, drgb, dcw = vol.to_dense()
    for min_weight in (1.0, 3.0):
        for colour, normals in ((True, True), (False, False)):
            args = (vol.rgb, vol.cweight) if colour else (None, None)
            got = ops.mt_extract_blocks(vol.tsdf, vol.weight, vol.table, vol.blocks, vol.dims, vol.origin, vol.voxel, min_weight, *args,
                                        normals=normals)
            again = ops.mt_extract_blocks(vol.tsdf, vol.weight, vol.table, vol.blocks, vol.dims, vol.origin, vol.voxel, min_weight, *args,
                                          normals=normals)
            for x, y in zip(got, again):
                assert (x is None and y is None) or torch.equal(x, y)
            ref = ops.mt_extract(t, wt, vol.origin, vol.voxel, min_weight, drgb if colour else None, dcw if colour else None, normals)
            assert (got[2] is None) == (not colour) and (got[3] is None) == (not normals)
            assert ref[1].shape[0] > 3000
            S.assert_same_mesh(_host(got), _host(ref), f"{shape} holes={holes} min_weight={min_weight} colour={colour}")
    if not holes and shape == "sphere":  # every surface block is there: the pool's mesh is the closed one of the full field
        full = ops.mt_extract(torch.from_numpy(f).to(dev), torch.full(f.shape, 3.0, device=dev), vol.origin, vol.voxel, 1.0, normals=False)
        vol.weight.fill_(3.0)
        got = ops.mt_extract_blocks(vol.tsdf, vol.weight, vol.table, vol.blocks, vol.dims, vol.origin, vol.voxel, 1.0, normals=False)
        S.assert_same_mesh(_host(got), _host(full), "closed sphere")
        tp = R.topology(got[0].cpu().numpy(), got[1].cpu().numpy())
        assert tp["closed"] and tp["euler"] == 2


# The third case is scene A on a lattice of which no side is a multiple of 8, still 5 x 6 x 7 blocks: the last block of an axis holds
# samples outside the lattice, which the integration and the staging of the mesher must leave alone.  By the numpy oracle (tsdf_ref /
# tsdf_sparse_ref) the sphere lies inside this lattice and gives the mesh of the full one, 2 817 vertices / 5 192 faces at min_weight 1;
# the rule marks 56 blocks, 178 are allocated, 36 of them in the last block layer of x and 30 in that of y.  None is in the last layer
# of z (samples 48 ..): no view sees the sphere's far side, so the band ends before it.
@pytest.mark.parametrize("kind,dims,min_weights", [pytest.param("A", S.DIMS, (1.0, 2.0), id="A"), pytest.param("B", S.DIMS, (1.0, 2.0), id="B"),
                                                   pytest.param("A", (37, 45, 50), (1.0,), id="A-37x45x50")])
def test_whole_path_gives_the_dense_mesh(kind, dims, min_weights):
    sp, de = _pair(kind, True, True, dims=dims)
    for min_weight in min_weights:
        got, ref = _host(sp.extract(min_weight, normals=True)), _host(de.extract(min_weight, normals=True))
        print(f"scene {kind} {dims} min_weight {min_weight}: {len(ref[0])} vertices, {len(ref[1])} faces, {sp.needed} of 210 blocks")
        assert len(ref[1]) > 2000
        S.assert_same_mesh(got, ref, f"scene {kind} {dims} min_weight {min_weight}")


def test_a_lattice_the_dense_volume_cannot_hold():
    """1024^3 = 2^30 virtual samples (mesh.py's dense limit is 2^29; the planes with colour would be 25.8 GB): a sphere in one corner,
    seen from all round, comes out closed from a few hundred blocks."""
    from patchmatchnet_amd import tsdf
    dev = _dev()
    dims = (1024, 1024, 1024)
    assert dims[0] * dims[1] * dims[2] > tsdf.MAX_VOXELS
    views = S.surround_views()
    maps, sizes, cams, _, _ = _upload(views, dev)
    slots = list(range(len(views)))
    origin = np.zeros(3, np.float32)
    vol = tsdf.SparseTsdfVolume(origin, S.VOXEL, dims, S.TRUNC, dev, color=False)
    B = vol.allocate(maps, slots, sizes, cams)
    vol.integrate(maps, slots, sizes, cams, batch=7)
    v, f, c, n = _host(vol.extract(1.0, normals=True))
    table = vol.table.numel()
    print(f"1024^3: {B} blocks of {table} ({100.0 * B / table:.4f} %), {len(v)} vertices, {len(f)} faces")
    assert table == 2 ** 21 and 100 < B < 0.01 * table
    t = R.topology(v, f)
    assert t["closed"] and t["euler"] == 2 and t["directed_unique"] and t["degenerate"] == 0 and t["unreferenced"] == 0
    assert t["volume"] > 0  # wound outward
    # the same corner as a dense lattice with the same origin: the same samples, so the same mesh
    de = tsdf.TsdfVolume(origin, S.VOXEL, (56, 56, 56), S.TRUNC, dev, color=False)
    de.integrate(maps, slots, sizes, cams, batch=7)
    S.assert_same_mesh((v, f, c, n), _host(de.extract(1.0, normals=True)), "corner of the 1024^3 lattice")


def _run_mesh(args, cwd):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "mesh.py")] + args, cwd=cwd, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)  # a fresh process
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    return p.stdout


def test_mesh_py_sparse_equals_dense(tmp_path):
    """mesh.py in child processes on a rendered scan (true depth maps, all-ones masks): --volume sparse writes the default's mesh; with
    --max_blocks below the need it says so, enlarges the voxel and still writes a mesh that is closed wherever it was observed."""
    _dev()
    from PIL import Image
    from patchmatchnet_amd import data_io, tsdf
    n, H, W = 5, 96, 128
    src = synth.write_scene_scan(str(tmp_path), "scene", n, H, W, n_src=2)
    _, _, _, depths = synth.render_scene(n, H, W, cameras=synth.arc_cameras(n, H, W), all_depths=True)
    res = str(tmp_path / "results")
    os.makedirs(os.path.join(res, "depth_est"))
    os.makedirs(os.path.join(res, "mask"))
    for v in range(n):
        data_io.save_pfm(os.path.join(res, "depth_est/{:0>8}.pfm".format(v)), depths[v].numpy().astype(np.float32))
        Image.fromarray(np.full((H, W), 255, np.uint8)).save(os.path.join(res, "mask/{:0>8}_final.png".format(v)))
    # 49 x 37 x 29 samples: no multiple of 8 on any axis, so the border blocks hold samples outside the lattice
    grid = ["--voxel", "5.0", "--trunc", "20.0", "--bounds", "-120.0", "-90.0", "580.0", "120.0", "90.0", "720.0"]
    base = ["--input_folder", src, "--results_folder", res]
    out_d = _run_mesh(base + ["--output_folder", str(tmp_path / "dense")] + grid, str(tmp_path))
    out_s = _run_mesh(base + ["--output_folder", str(tmp_path / "sparse"), "--volume", "sparse"] + grid, str(tmp_path))
    assert "blocks allocated" in out_s and "blocks allocated" not in out_d and "enlarged" not in out_s
    dense = tsdf.read_ply_mesh(str(tmp_path / "dense" / "mesh.ply"))
    sparse = tsdf.read_ply_mesh(str(tmp_path / "sparse" / "mesh.ply"))
    assert len(dense[1]) > 3000 and dense[2] is not None and dense[3] is not None
    S.assert_same_mesh(sparse, dense, "mesh.py --volume sparse")
    out_l = _run_mesh(base + ["--output_folder", str(tmp_path / "low"), "--volume", "sparse", "--max_blocks", "40"] + grid, str(tmp_path))
    assert "would exceed --max_blocks 40: voxel enlarged to" in out_l
    v, f, _, _ = tsdf.read_ply_mesh(str(tmp_path / "low" / "mesh.ply"))
    t = R.topology(v, f)
    assert 200 < len(f) < len(dense[1])
    assert t["unreferenced"] == 0 and t["degenerate"] == 0 and t["max_edge_use"] == 2 and t["directed_unique"]
