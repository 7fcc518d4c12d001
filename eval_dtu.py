"""DTU accuracy / completeness / overall of fused point clouds, on the GPU: what the reference's MATLAB scripts
evaluations/dtu/BaseEvalMain_web.m + ComputeStat_web.m compute (patchmatchnet_amd/pointcloud.py).

    python eval_dtu.py --data_path <SampleSet/MVS Data> --ply_path outputs --results_path outputs

--data_path holds Points/stl/stl%03d_total.ply and ObsMask/{ObsMask<scan>_10,Plane<scan>}.mat (or .npz with the same field names).
A scan's cloud is <ply_path>/<method>%03d_<light>.ply (the reference's naming) or, failing that, <ply_path>/scan<N>/fused.ply (what
eval.py writes).  Scores go to <results_path>/dtu_scores.json; a scan already there is not recomputed unless --force.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from typing import Dict, List, Optional

USED_SETS = [1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118]  # BaseEvalMain_web.m:23


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--data_path", required=True, help="folder that holds Points/stl and ObsMask")
    p.add_argument("--ply_path", required=True, help="folder of the method's point clouds")
    p.add_argument("--results_path", required=True, help="folder dtu_scores.json is written to")
    p.add_argument("--method", default="patchmatchnet")
    p.add_argument("--light", default="l3")
    p.add_argument("--scans", type=int, nargs="+", default=USED_SETS)
    p.add_argument("--dst", type=float, default=0.2, help="minimum distance between points after the reduction")
    p.add_argument("--max_dist", type=float, default=20.0, help="outlier threshold of the statistics")
    p.add_argument("--seed", type=int, default=0, help="seed of the reduction's visiting order")
    p.add_argument("--force", action="store_true", help="recompute scans already in dtu_scores.json")
    p.add_argument("--device", default="cuda:0")
    return p.parse_args(argv)


def first_existing(paths: List[str]) -> Optional[str]:
    return next((p for p in paths if os.path.isfile(p)), None)


def scan_inputs(args, scan: int) -> Dict[str, str]:
    """The four input files of a scan; FileNotFoundError names the first one that is missing (every candidate path)."""
    obs = os.path.join(args.data_path, "ObsMask")
    want = {
        "ply": [os.path.join(args.ply_path, f"{args.method.lower()}{scan:03d}_{args.light}.ply"),
                os.path.join(args.ply_path, f"scan{scan}", "fused.ply")],
        "stl": [os.path.join(args.data_path, "Points", "stl", f"stl{scan:03d}_total.ply")],
        "obs_mask": [os.path.join(obs, f"ObsMask{scan}_10.mat"), os.path.join(obs, f"ObsMask{scan}_10.npz")],
        "plane": [os.path.join(obs, f"Plane{scan}.mat"), os.path.join(obs, f"Plane{scan}.npz")],
    }
    found = {}
    for what, paths in want.items():
        found[what] = first_existing(paths)
        if found[what] is None:
            raise FileNotFoundError(f"scan {scan}: no {what} file: " + " nor ".join(paths))
    return found


def score_scan(args, scan: int, files: Dict[str, str]) -> Dict:
    import torch

    from patchmatchnet_amd import pointcloud as PC
    t0 = time.perf_counter()
    data = torch.from_numpy(PC.read_ply_vertices(files["ply"])).to(args.device)
    stl = torch.from_numpy(PC.read_ply_vertices(files["stl"])).to(args.device)
    obs, bb, res = PC.load_obs_mask(files["obs_mask"])
    plane = PC.load_plane(files["plane"])
    t1 = time.perf_counter()
    out = PC.dtu_score_scan(data, stl, obs, bb, res, plane, dst=args.dst, max_dist=args.max_dist, seed=args.seed)
    out["seconds"]["read"] = t1 - t0
    out["ply"] = files["ply"]
    return out


def main(argv=None) -> int:
    args = parse_args(argv)
    from patchmatchnet_amd import _lib
    from patchmatchnet_amd.pointcloud import totals
    os.makedirs(args.results_path, exist_ok=True)
    out_path = os.path.join(args.results_path, "dtu_scores.json")
    settings = {"dst": args.dst, "max_dist": args.max_dist, "seed": args.seed}
    scores: Dict[str, Dict] = {}
    if os.path.isfile(out_path) and not args.force:
        with open(out_path) as f:
            old = json.load(f)
        if all(old.get(k) == v for k, v in settings.items()):
            scores = old.get("scans", {})
    failed = []
    for scan in args.scans:
        if str(scan) in scores:
            print(f"scan {scan}: already in {out_path}")
        else:
            try:
                scores[str(scan)] = score_scan(args, scan, scan_inputs(args, scan))
            except FileNotFoundError as e:
                print(f"error: {e}", file=sys.stderr)
                failed.append(scan)
                continue
        s = scores[str(scan)]
        print("mean/median Data (acc.) %f/%f" % (s["acc_mean"], s["acc_median"]))
        print("mean/median Stl (comp.) %f/%f" % (s["comp_mean"], s["comp_median"]))
    done = [scores[str(s)] for s in args.scans if str(s) in scores]
    total = totals(done)
    print("final evaluation result on all scans: acc.: %f, comp.: %f, overall: %f" % (total["acc"], total["comp"], total["overall"]))
    with open(out_path, "w") as f:
        json.dump({**settings, "abi": _lib.ABI_VERSION, "method": args.method, "light": args.light, "scans": scores,
                   "scans_scored": [s for s in args.scans if str(s) in scores], "total": total}, f, indent=1)
    if failed:
        print(f"error: {len(failed)} scans not scored: {failed}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
