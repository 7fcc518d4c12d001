#!/usr/bin/env python
"""Times the DTU score (patchmatchnet_amd/pointcloud.py) at a realistic size on the GPU: a 5.2 M-point ground-truth surface and a
5.2 M-point method cloud (noisy surface + 2 % outliers up to 150 units away), generated on the device from a seed; a synthetic
ObsMask / plane (tests/dtu_ref.py).  Prints one JSON line per measurement: the phases of dtu_score_scan (warm-up first, the second
run reported), a sweep of the nearest-neighbour cell and of the reduction's cell, PLY reading, and -- where scipy is importable --
scipy.spatial.cKDTree(...).query(workers=16) on the same clouds, the only available yardstick (a CPU KD-tree as the reference's
MATLAB uses; it is NOT the MATLAB).  `--profile` runs one score only, for `rocprofv3 --kernel-trace --stats -- python
scripts/dtu_score_bench.py --profile`."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N = 5_200_000


def clouds(dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(7)

    def surface(m, noise):
        xy = torch.rand(m, 2, generator=g, device=dev, dtype=torch.float64) * 100.0
        z = 20.0 + 8.0 * torch.sin(xy[:, 0] / 17.0) * torch.cos(xy[:, 1] / 23.0) + 0.05 * xy[:, 0]
        p = torch.cat([xy, z[:, None]], 1)
        return (p + noise * torch.randn(m, 3, generator=g, device=dev, dtype=torch.float64)).float()

    stl = surface(N, 0.0)
    n_out = N // 50
    out = (torch.rand(n_out, 3, generator=g, device=dev) - 0.5) * 300.0 + 50.0
    data = torch.cat([surface(N - n_out, 0.1), out])[torch.randperm(N, generator=g, device=dev)].contiguous()
    return data, stl


def main() -> None:
    import numpy as np
    import torch

    import dtu_ref as R
    from patchmatchnet_amd import fusion, pointcloud as PC
    dev = "cuda:0"
    s = R.synthetic_scan(0, n_stl=10, n_data=60)
    data, stl = clouds(dev)

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    def score(**kw):
        return PC.dtu_score_scan(data, stl, s["ObsMask"], s["BB"], s["Res"], s["P"], **kw)

    if "--profile" in sys.argv:
        score()
        return
    score()
    t = sync()
    res = score()
    print(json.dumps({"what": "dtu_score_scan", "points": [N, N], "total_s": round(sync() - t, 4), "reduce_rounds": res["reduce_rounds"],
                      "n_data_reduced": res["n_data_reduced"], "seconds": {k: round(v, 4) for k, v in res["seconds"].items()}}), flush=True)
    keep = PC.reduce_points(data, 0.2)
    qd = data[keep].contiguous()
    for cell in (0.5, 1.0, 2.0, 4.0, 8.0):
        row = {"what": "nn_cell_sweep", "cell": cell}
        for name, frm, to in (("data_to_stl", qd, stl), ("stl_to_data", stl, qd), ("unreduced_data_to_stl", data, stl)):
            t = sync()
            grid = PC.build_grid(to, cell)
            t1 = sync()
            PC.nn_distance(frm, grid, 60.0)
            row[name] = {"grid_s": round(t1 - t, 4), "search_s": round(sync() - t1, 4)}
        print(json.dumps(row), flush=True)
    for ratio in (1.0, 2.0, 3.0, 4.0, 8.0):
        t = sync()
        _, rounds = PC.reduce_points(data, 0.2, cell=ratio * 0.2, return_rounds=True)
        print(json.dumps({"what": "reduce_cell_sweep", "cell_over_dst": ratio, "reduce_s": round(sync() - t, 4), "rounds": rounds}), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "fused.ply")
        xyz = data.cpu().numpy()
        fusion.write_ply(path, xyz, np.zeros((N, 3), np.uint8))
        t = time.perf_counter()
        PC.read_ply_vertices(path)
        print(json.dumps({"what": "read_ply_vertices", "points": N, "read_s": round(time.perf_counter() - t, 4)}), flush=True)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        print(json.dumps({"what": "ckdtree_yardstick", "skipped": "scipy is not importable"}))
        return
    a, b = qd.cpu().numpy(), stl.cpu().numpy()
    row = {"what": "ckdtree_yardstick", "workers": 16}
    for name, frm, to in (("data_to_stl", a, b), ("stl_to_data", b, a)):
        t = time.perf_counter()
        tree = cKDTree(to)
        t1 = time.perf_counter()
        d, _ = tree.query(frm, workers=16, distance_upper_bound=60.0)
        row[name] = {"build_s": round(t1 - t, 3), "query_s": round(time.perf_counter() - t1, 3)}
        got = PC.nn_distance(torch.from_numpy(frm).to(dev), PC.build_grid(torch.from_numpy(to).to(dev), PC.NN_CELL), 60.0).cpu().numpy()
        row[name]["max_abs_diff_vs_gpu"] = float(np.abs(np.minimum(d, 60.0) - got).max())
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
