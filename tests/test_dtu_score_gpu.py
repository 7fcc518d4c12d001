"""GPU checks of the DTU score (pmn_nn_distance, pmn_reduce_round, patchmatchnet_amd/pointcloud.py, eval_dtu.py) against the
numpy float64 reference tests/dtu_ref.py.

nn_distance follows the definition (un-contracted float64), so the bound is 4 ulp of float64, relative; reduce_points is compared
bit for bit; the statistics to 1e-12 relative (float64 sums of identical values in another order)."""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import dtu_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP4 = 4 * 2.0 ** -52
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


@pytest.fixture(scope="module")
def scan():
    return R.synthetic_scan(0)


@pytest.fixture(scope="module")
def brute(scan):
    """Brute-force nearest distances of the synthetic pair, both directions."""
    return {"data_stl": R.nearest_distance(scan["data"], scan["stl"]), "stl_data": R.nearest_distance(scan["stl"], scan["data"])}


@pytest.mark.parametrize("direction", ["data_stl", "stl_data"])
def test_nn_distance_matches_brute_force(scan, brute, direction):
    from patchmatchnet_amd import pointcloud as PC
    frm, to = (scan["data"], scan["stl"]) if direction == "data_stl" else (scan["stl"], scan["data"])
    # far, out-of-block and empty-cell queries ride along in `data`; a few hand-placed ones on top
    extra = np.array([[1e4, 1e4, 1e4], [-3e3, 50, 20], [50, 50, 79.9], [50, 50, -39.0], to[0], to[-1] + np.float32(1e-3)], np.float32)
    frm = np.concatenate([frm, extra])
    rd = np.concatenate([brute[direction][0], R.nearest_distance(extra, to)[0]])
    results = []
    for cell in (0.5, 2.0, 7.3, 1000.0):  # smaller than the point spacing (1.3 units) ... larger than the cloud
        for cap in (60.0, 5.0):
            want = np.minimum(rd, cap)
            d, idx = PC.nn_distance(_dev(frm), PC.build_grid(_dev(to), cell), cap, return_index=True)
            d, idx = d.cpu().numpy(), idx.cpu().numpy()
            assert d.dtype == np.float64 and d.shape == (len(frm),)
            rel = np.abs(d - want) / want.clip(1e-300)
            rel[want == 0] = np.abs(d[want == 0])
            print(f"{direction} cell {cell} cap {cap}: max rel err {rel.max():.3e}, capped {(idx < 0).sum()} of {len(frm)}")
            assert rel.max() <= ULP4
            assert ((idx < 0) == (rd >= cap)).all()
            hit = idx >= 0
            a, b = frm[hit].astype(np.float64), to[idx[hit]].astype(np.float64)
            dd = a - b
            assert (np.sqrt(dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2]) == d[hit]).all()
            if cap == 60.0:
                results.append(d)
    assert (rd >= 60).any() and (rd < 60).any() and (rd == 0).any()
    for d in results[1:]:
        assert (d == results[0]).all()  # the cell size changes the work, not one bit of the result


def test_nn_distance_origin_and_order_do_not_matter(scan):
    from patchmatchnet_amd import pointcloud as PC
    to, frm = _dev(scan["stl"]), _dev(scan["data"])
    a = PC.nn_distance(frm, PC.build_grid(to, 3.0), 60.0)
    b = PC.nn_distance(frm, PC.build_grid(to, 3.0, origin=[-500.0, -7.25, -1e3]), 60.0)
    perm = torch.randperm(len(frm), generator=torch.Generator().manual_seed(1)).to(DEV)
    c = PC.nn_distance(frm[perm].contiguous(), PC.build_grid(to.flip(0).contiguous(), 3.0), 60.0)
    assert torch.equal(a, b) and torch.equal(a[perm], c)


def test_wrappers_reject_bad_input(scan):
    from patchmatchnet_amd import PmnError, pointcloud as PC
    pts = _dev(scan["stl"][:100])
    bad = pts.clone()
    bad[3, 1] = float("nan")
    bad[7, 0] = float("inf")
    with pytest.raises(PmnError, match="2 points have non-finite"):
        PC.build_grid(bad, 1.0)
    with pytest.raises(PmnError, match="63-bit"):
        PC.build_grid(torch.tensor([[0.0, 0, 0], [1e9, 1e9, 1e9]], device=DEV), 1e-3)
    with pytest.raises(PmnError, match="cell"):
        PC.build_grid(pts, -1.0)
    with pytest.raises(PmnError, match="permutation"):
        PC.reduce_points(pts, 0.2, order=np.zeros(100, np.int64))
    with pytest.raises(PmnError, match="float32"):
        PC.build_grid(pts.double(), 1.0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reduce_points_is_the_sequential_greedy_set(scan, seed):
    from patchmatchnet_amd import pointcloud as PC
    pts = scan["data"]
    assert len(np.unique(pts, axis=0)) < len(pts)  # duplicates present
    order = np.random.default_rng(seed).permutation(len(pts))
    for dst, cell in ((0.2, None), (0.5, 3.0), (2.0, 0.7), (1.0, 1.0), (0.0, None)):  # dst below, above and equal to the cell
        ref = R.reduce_points(pts, dst, order)
        got, rounds = PC.reduce_points(_dev(pts), dst, order=order, cell=cell, return_rounds=True)
        again = PC.reduce_points(_dev(pts), dst, order=torch.from_numpy(order).to(DEV), cell=cell)
        print(f"seed {seed} dst {dst} cell {cell}: kept {int(got.sum())} of {len(pts)} in {rounds} rounds")
        assert got.dtype == torch.bool and torch.equal(got, again)
        assert (got.cpu().numpy() == ref).all()
    # the default order is numpy's default_rng(seed) permutation
    assert torch.equal(PC.reduce_points(_dev(pts), 0.2, seed=seed), PC.reduce_points(_dev(pts), 0.2, order=order))


def test_reduce_points_identity_and_reversed_order_on_a_sorted_cloud(scan):
    from patchmatchnet_amd import pointcloud as PC
    pts = scan["data"][np.argsort(scan["data"][:, 0], kind="stable")]
    for order in (np.arange(len(pts)), np.arange(len(pts))[::-1].copy()):
        got, rounds = PC.reduce_points(_dev(pts), 2.0, order=order, return_rounds=True)
        print(f"sorted cloud, order {order[0]}..{order[-1]}: {rounds} rounds, kept {int(got.sum())}")
        assert (got.cpu().numpy() == R.reduce_points(pts, 2.0, order)).all()


def _assert_scores(got, ref):
    for k, v in ref.items():
        if isinstance(v, int):
            assert got[k] == v, (k, got[k], v)
        else:
            assert abs(got[k] - v) <= 1e-12 * abs(v), (k, got[k], v)


def test_dtu_score_scan_matches_the_reference(scan):
    from patchmatchnet_amd import pointcloud as PC
    for seed, dst in ((0, 0.2), (5, 0.6)):
        order = np.random.default_rng(seed).permutation(len(scan["data"]))
        ref = R.score_scan(scan["data"], scan["stl"], scan["ObsMask"], scan["BB"], scan["Res"], scan["P"], order, dst=dst)
        got = PC.dtu_score_scan(_dev(scan["data"]), _dev(scan["stl"]), scan["ObsMask"], scan["BB"], scan["Res"], scan["P"], dst=dst,
                                seed=seed)
        print(got)
        assert 0 < ref["acc_n"] < ref["n_data_reduced"] < ref["n_data_in"] and 0 < ref["comp_n"] < len(scan["stl"])
        _assert_scores(got, ref)
        assert set(got["seconds"]) == {"reduce", "data_to_stl", "stl_to_data", "statistics"}


def _run_cli(argv, timeout=300):
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, os.path.join(ROOT, "eval_dtu.py")] + argv,
                          capture_output=True, text=True, cwd=ROOT)


@pytest.mark.parametrize("naming", ["reference", "eval"])
def test_eval_dtu_end_to_end(tmp_path, naming):
    from patchmatchnet_amd import fusion, pointcloud as PC
    data, ply, out = tmp_path / "data", tmp_path / "ply", tmp_path / "out"
    scans = {1: R.synthetic_scan(11, n_stl=3000, n_data=5000), 114: R.synthetic_scan(12, n_stl=2500, n_data=4000)}
    os.makedirs(data / "ObsMask")
    for n, s in scans.items():
        grey = np.full((len(s["data"]), 3), 128, np.uint8)
        fusion.write_ply(str(ply / (f"patchmatchnet{n:03d}_l3.ply" if naming == "reference" else f"scan{n}/fused.ply")), s["data"], grey)
        fusion.write_ply(str(data / "Points" / "stl" / f"stl{n:03d}_total.ply"), s["stl"], np.zeros((len(s["stl"]), 3), np.uint8))
        np.savez(str(data / "ObsMask" / f"ObsMask{n}_10.npz"), ObsMask=s["ObsMask"], BB=s["BB"], Res=s["Res"])
        np.savez(str(data / "ObsMask" / f"Plane{n}.npz"), P=s["P"])
    argv = ["--data_path", str(data), "--ply_path", str(ply), "--results_path", str(out), "--scans", "1", "114", "--seed", "4"]
    r = _run_cli(argv)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.load(open(out / "dtu_scores.json"))
    direct = {}
    for n, s in scans.items():
        direct[n] = PC.dtu_score_scan(_dev(s["data"]), _dev(s["stl"]), s["ObsMask"], s["BB"], s["Res"], s["P"], seed=4)
        for k, v in direct[n].items():
            if k not in ("seconds", "reduce_rounds"):  # the in-place rounds decide the same set in a schedule-dependent number of rounds
                assert js["scans"][str(n)][k] == v, (n, k)
    total = PC.totals(list(direct.values()))
    assert js["total"] == total and js["seed"] == 4 and js["abi"] == 25
    m = re.search(r"final evaluation result on all scans: acc\.: ([\d.]+), comp\.: ([\d.]+), overall: ([\d.]+)", r.stdout)
    assert m and [float(g) for g in m.groups()] == [float("%f" % total[k]) for k in ("acc", "comp", "overall")]
    assert r.stdout.count("mean/median Data (acc.)") == 2 and r.stdout.count("mean/median Stl (comp.)") == 2
    # a second invocation recomputes nothing: the stored entries (their timings included) are untouched
    r2 = _run_cli(argv)
    assert r2.returncode == 0 and r2.stdout.count("already in") == 2
    assert json.load(open(out / "dtu_scores.json"))["scans"] == js["scans"]
    assert m.group(0) in r2.stdout


def test_realistic_size(scan):
    """5.2 M x 5.2 M points generated on the device: 2 000 random queries of each direction against brute force, and the whole
    score under this test's own time limit.  The wall time is printed, not gated."""
    from patchmatchnet_amd import pointcloud as PC
    limit = 600.0
    n = 5_200_000
    g = torch.Generator(device=DEV).manual_seed(7)

    def surface(m, noise):
        xy = torch.rand(m, 2, generator=g, device=DEV, dtype=torch.float64) * 100.0
        z = 20.0 + 8.0 * torch.sin(xy[:, 0] / 17.0) * torch.cos(xy[:, 1] / 23.0) + 0.05 * xy[:, 0]
        p = torch.cat([xy, z[:, None]], 1)
        return (p + noise * torch.randn(m, 3, generator=g, device=DEV, dtype=torch.float64)).float()

    stl = surface(n, 0.0)
    n_out = n // 50  # 2 % outliers, up to 150 units from the object
    out = (torch.rand(n_out, 3, generator=g, device=DEV) - 0.5) * 300.0 + 50.0
    data = torch.cat([surface(n - n_out, 0.1), out])[torch.randperm(n, generator=g, device=DEV)].contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = PC.dtu_score_scan(data, stl, scan["ObsMask"], scan["BB"], scan["Res"], scan["P"])
    wall = time.perf_counter() - t0
    print(f"realistic size: {n} x {n} points scored in {wall:.2f} s: {res}")
    assert wall < limit
    assert res["n_data_in"] == n and 0 < res["acc_n"] <= res["n_data_reduced"] < n and 0 < res["comp_n"] <= n
    for frm, to in ((data, stl), (stl, data)):
        d = PC.nn_distance(frm, PC.build_grid(to, PC.NN_CELL), 60.0)
        pick = torch.randint(0, n, (2000,), generator=torch.Generator().manual_seed(3)).to(DEV)
        q = frm[pick].double()
        best = torch.full((2000,), float("inf"), dtype=torch.float64, device=DEV)
        for s in range(0, n, 1 << 18):  # brute force in float64, the same expression, on the device
            t = to[s:s + (1 << 18)].double()
            dx, dy, dz = (q[:, None, a] - t[None, :, a] for a in range(3))
            best = torch.minimum(best, torch.sqrt(dx * dx + dy * dy + dz * dz).min(1).values)
        want = best.clamp_max(60.0)
        rel = ((d[pick] - want).abs() / want.clamp_min(1e-300)).max().item()
        print(f"2000 sampled queries: max rel err {rel:.3e}, capped {(want >= 60).sum().item()}")
        assert rel <= ULP4
