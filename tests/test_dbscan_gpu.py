"""GPU checks of the order-free DBSCAN (pmn_cloud_core, pmn_cloud_dbscan, pointcloud.cluster_dbscan / select_clusters,
cluster_cloud.py) against the brute-force numpy float64 statement of tests/dbscan_ref.py.

The definition is exact -- every decision is taken on un-contracted float64 values that numpy reproduces bit for bit, and every tie is
broken by a stated rule -- so labels, core flags and sizes are compared with np.array_equal: no tolerance, no case left out.  What the
cases contain (noise, border points, several clusters, real ties) is asserted on the reference alone by tests/test_dbscan_ref.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dbscan_ref as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _cells(pts, eps):
    """eps / 8, eps, 10 eps and one cell for everything; at eps = 0, where those are no cells, the default, a small one and one cell."""
    one = 2.0 * float((pts.max(0).astype(np.float64) - pts.min(0).astype(np.float64)).max()) + 1.0
    return (eps / 8.0, eps, 10.0 * eps, one) if eps > 0.0 else (None, 0.05, one)


def _run(pts, eps, mp, cell=None):
    from patchmatchnet_amd import pointcloud as PC
    labels, core, sizes = PC.cluster_dbscan(_dev(pts), eps, mp, cell=cell)
    assert labels.dtype == torch.int64 and core.dtype == torch.bool and sizes.dtype == torch.int64
    assert labels.shape == (len(pts),) and core.shape == (len(pts),) and sizes.dim() == 1
    return labels.cpu().numpy(), core.cpu().numpy(), sizes.cpu().numpy()


@pytest.mark.parametrize("name", sorted(D.cases()))
def test_labels_core_and_sizes_are_the_reference_at_every_cell(name):
    pts, eps, mp, _ = D.cases()[name]
    want = D.expected(name)
    for cell in _cells(pts, eps):
        got = _run(pts, eps, mp, cell)
        for g, w, what in zip(got, want, ("labels", "core", "sizes")):
            assert np.array_equal(g, w), (name, cell, what, int((g != w).sum()) if g.shape == w.shape else (g.shape, w.shape))
    again = _run(pts, eps, mp, _cells(pts, eps)[-1])  # repeatability: a second run gives the same bits
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    default = _run(pts, eps, mp)
    assert all(np.array_equal(a, b) for a, b in zip(default, want))


def test_a_shuffled_cloud_gives_the_same_partition():
    pts, s = D.surface()
    shuf, perm = D.shuffled(pts)
    a, b = _run(pts, 2.0 * s, 4), _run(shuf, 2.0 * s, 4)
    assert all(np.array_equal(x, y) for x, y in zip(b, D.expected("surface_shuffled")))
    assert np.array_equal(a[1][perm], b[1])                       # the same core set
    assert np.array_equal(a[0][perm] < 0, b[0] < 0)               # the same noise set
    assert D.same_partition(a[0][perm], b[0]) and np.array_equal(a[2], b[2])
    # the chain: in order, reversed and shuffled it is one cluster of everything
    for name in ("chain", "chain_reversed", "chain_shuffled"):
        p, eps, mp, _ = D.cases()[name]
        labels, core, sizes = _run(p, eps, mp)
        assert not labels.any() and core.all() and sizes.tolist() == [len(p)]


def test_select_clusters_against_the_reference():
    from patchmatchnet_amd import pointcloud as PC
    from patchmatchnet_amd._lib import PmnError
    pts, eps, mp, _ = D.cases()["floater"]
    want_labels, _, want_sizes = D.expected("floater")
    labels, _, sizes = PC.cluster_dbscan(_dev(pts), eps, mp)
    for args in ((0, 0), (42, 0), (41, 0), (0, 1), (0, 2), (3000, 0), (10, 5)):
        keep = PC.select_clusters(labels, sizes, *args)
        assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), D.select_clusters(want_labels, want_sizes, *args)), args
    # the clump of wrong points is a cluster of its own, and the size threshold removes exactly it and the noise
    keep = PC.select_clusters(labels, sizes, min_cluster_points=42).cpu().numpy()
    assert not keep[D.floater()[1]].any() and keep.sum() == want_sizes[0]
    with pytest.raises(PmnError):
        PC.select_clusters(labels.cpu(), sizes.cpu())
    with pytest.raises(PmnError):
        PC.select_clusters(labels, sizes, keep_largest=-1)


def test_arguments_are_checked_before_any_launch():
    from patchmatchnet_amd import _lib, pointcloud as PC
    from patchmatchnet_amd._lib import PmnError
    pts = D.clump(65)
    for bad in (dict(eps=-1.0, min_points=3), dict(eps=float("nan"), min_points=3), dict(eps=float("inf"), min_points=3),
                dict(eps=1e200, min_points=3), dict(eps=0.1, min_points=0), dict(eps=0.1, min_points=True),
                dict(eps=0.1, min_points=2.0), dict(eps=0.1, min_points=3, cell=0.0)):
        with pytest.raises(PmnError):
            PC.cluster_dbscan(_dev(pts), **bad)
    with pytest.raises(PmnError):
        PC.cluster_dbscan(torch.from_numpy(pts), 0.1, 3)  # a host tensor: no CPU path
    g = PC.build_grid(_dev(pts), 0.5)
    a, n, L = PC._grid_args(g), len(pts), _lib.lib()
    core = torch.zeros(n, dtype=torch.uint8, device=DEV)
    parent = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    label = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    orig = g.perm.int()
    assert L.pmn_cloud_core(*a, -1.0, 3, core.data_ptr(), None) == -1
    assert L.pmn_cloud_core(*a, 0.1, 0, core.data_ptr(), None) == -1
    assert L.pmn_cloud_core(*a, 0.1, 3, None, None) == -1
    assert L.pmn_cloud_dbscan(*a, float("nan"), core.data_ptr(), orig.data_ptr(), parent.data_ptr(), label.data_ptr(), None) == -1
    assert L.pmn_cloud_dbscan(*a, 0.1, None, orig.data_ptr(), parent.data_ptr(), label.data_ptr(), None) == -1
    assert L.pmn_cloud_dbscan(*a, 0.1, core.data_ptr(), orig.data_ptr(), None, label.data_ptr(), None) == -1
    assert L.pmn_cloud_dbscan(*a, 0.1, core.data_ptr(), None, parent.data_ptr(), label.data_ptr(), None) == -1  # label without orig
    torch.cuda.synchronize()
    assert (parent == -7).all() and (label == -7).all() and not core.any()  # nothing ran


def test_the_link_stage_alone_names_every_cluster_by_its_lowest_sorted_index():
    """label = NULL leaves the border launch out; parent then holds, for core points, the minimum sorted index of their component, and
    the full call's parent is the same."""
    from patchmatchnet_amd import _lib, pointcloud as PC
    pts, eps, mp, _ = D.cases()["duplicates_eps_above"]
    want_labels, want_core, _ = D.expected("duplicates_eps_above")
    g = PC.build_grid(_dev(pts), 0.3)
    a, n, L = PC._grid_args(g), len(pts), _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    core = torch.empty(n, dtype=torch.uint8, device=DEV)
    parent, parent2, label = (torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(3))
    orig = g.perm.int()
    assert L.pmn_cloud_core(*a, eps, mp, core.data_ptr(), s) == 0
    assert L.pmn_cloud_dbscan(*a, eps, core.data_ptr(), None, parent.data_ptr(), None, s) == 0
    assert L.pmn_cloud_dbscan(*a, eps, core.data_ptr(), orig.data_ptr(), parent2.data_ptr(), label.data_ptr(), s) == 0
    perm = g.perm.cpu().numpy()
    core, parent, parent2, label = (t.cpu().numpy() for t in (core, parent, parent2, label))
    assert np.array_equal(parent, parent2) and np.array_equal(core.astype(bool), want_core[perm])
    assert np.array_equal(parent[core == 0], np.flatnonzero(core == 0))  # a point that is not core stays its own root
    ref = want_labels[perm]
    for c in np.unique(ref[core == 1]):
        members = np.flatnonzero((ref == c) & (core == 1))
        assert (parent[members] == members.min()).all()
    assert np.array_equal(label[core == 1], parent[core == 1]) and D.same_partition(label, ref)


def _cli(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "cluster_cloud.py")] + args, capture_output=True, text=True, timeout=600,
                          cwd=ROOT, env=env)


def test_cluster_cloud_end_to_end(tmp_path):
    from patchmatchnet_amd import ply
    import cluster_cloud
    pts, eps, mp, _ = D.cases()["floater"]
    want_labels, want_core, want_sizes = D.expected("floater")
    n = len(pts)
    rng = np.random.default_rng(4)
    colors = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    normals = rng.normal(size=(n, 3)).astype(np.float32)
    src, dst, lab, rep = (str(tmp_path / f) for f in ("fused.ply", "out/clusters.ply", "out/labels.npy", "out/report.json"))
    ply.write_ply(src, pts, colors, normals)
    r = _cli(["--input", src, "--output", dst, "--eps", repr(eps), "--min_points", str(mp), "--min_cluster_points", "42",
              "--labels", lab, "--report", rep])
    assert r.returncode == 0, r.stderr
    assert len(r.stdout.strip().splitlines()) == 1  # the report line
    keep = D.select_clusters(want_labels, want_sizes, 42)
    m = ply.read_ply_model(dst)
    assert m["faces"] is None and np.array_equal(m["vertices"], pts[keep]) and np.array_equal(m["colors"], colors[keep])
    assert np.array_equal(m["normals"], normals[keep])
    got = np.load(lab)
    assert got.dtype == np.int32 and np.array_equal(got, want_labels)
    one = json.load(open(rep))["files"][0]
    noise = int((want_labels < 0).sum())
    want = dict(points=n, core=int(want_core.sum()), border=n - noise - int(want_core.sum()), noise=noise, clusters=len(want_sizes),
                clusters_kept=1, kept=int(keep.sum()), eps=eps)
    assert {k: one[k] for k in want} == want
    for word in (f"{n} points read", f"{want['core']} core", f"{want['border']} border", f"{noise} noise", "2 clusters found, 1 kept",
                 f"{want['kept']} points kept"):
        assert word in r.stdout, (word, r.stdout)
    # every cluster and the noise, coloured by label; no normals in, none out; the default eps comes from the cloud's spacing
    from patchmatchnet_amd import pointcloud as PC
    src2, dst2, lab2 = (str(tmp_path / f) for f in ("plain.ply", "coloured.ply", "labels2.npy"))
    ply.write_ply(src2, pts, colors)
    r = _cli(["--input", src2, "--output", dst2, "--keep_noise", "--color_by_cluster", "--labels", lab2, "--report", rep])
    assert r.returncode == 0, r.stderr
    one = json.load(open(rep))["files"][0]
    assert one["spacing"] == PC.cloud_spacing(_dev(pts)) and one["eps"] == 4.0 * one["spacing"] and one["kept"] == n
    got = np.load(lab2)
    assert np.array_equal(got, PC.cluster_dbscan(_dev(pts), one["eps"], 10)[0].cpu().numpy())
    assert got.max() >= 1 and got.min() == -1  # several clusters and noise
    m = ply.read_ply_model(dst2)
    assert np.array_equal(m["vertices"], pts) and m["normals"] is None
    assert np.array_equal(m["colors"], cluster_cloud.cluster_colors(got))
    by_label = {int(v): {tuple(c) for c in m["colors"][got == v].tolist()} for v in np.unique(got)}
    assert all(len(v) == 1 for v in by_label.values()) and len(set.union(*by_label.values())) == len(by_label)
    assert by_label[-1] == {(128, 128, 128)}
