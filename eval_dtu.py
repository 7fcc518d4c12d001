"""DTU accuracy / completeness / overall of fused point clouds, on the GPU: what the reference's MATLAB scripts
evaluations/dtu/BaseEvalMain_web.m + ComputeStat_web.m compute (patchmatchnet_amd/pointcloud.py).

    python eval_dtu.py --data_path <SampleSet/MVS Data> --ply_path outputs --results_path outputs

--data_path holds Points/stl/stl%03d_total.ply and ObsMask/{ObsMask<scan>_10,Plane<scan>}.mat (or .npz with the same field names).
A scan's cloud is <ply_path>/<method>%03d_<light>.ply (the reference's naming) or, failing that, <ply_path>/scan<N>/fused.ply (what
eval.py writes; --ply_name mesh.ply takes mesh.py's file instead).  With --sample_spacing S a file with faces is scored by points drawn on
its triangles S apart (meshops.sample_surface), not by its vertices.  With --mesh_distance 1 completeness is
the exact distance from the stl points to the triangles of that file.  Scores go to <results_path>/dtu_scores.json; a scan already there is not recomputed unless --force.
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
    p.add_argument("--ply_name", default="fused.ply", help="the file looked for under <ply_path>/scan<N>/ (mesh.ply: mesh.py's output)")
    p.add_argument("--sample_spacing", type=float, default=0.0,
                   help="score points drawn on the triangles of a mesh this far apart (0 = off: the file's vertices)")
    p.add_argument("--sample_seed", type=int, default=0, help="seed of --sample_spacing's points")
    p.add_argument("--mesh_distance", type=int, default=0, choices=[0, 1],
                   help="1: completeness is measured against the triangles of the method's mesh themselves (exact point-to-mesh "
                        "distance), not against its vertices or samples; accuracy is unchanged")
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
                os.path.join(args.ply_path, f"scan{scan}", args.ply_name)],
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

    from patchmatchnet_amd import ply, pointcloud as PC
    t0 = time.perf_counter()
    mesh = None
    if args.sample_spacing > 0 or args.mesh_distance:
        from patchmatchnet_amd import PmnError, meshops
        model = ply.read_ply_model(files["ply"])
        if model["faces"] is None or len(model["faces"]) == 0:
            flag = "--sample_spacing" if args.sample_spacing > 0 else "--mesh_distance"
            raise PmnError(f"{files['ply']}: {flag} needs a mesh, this file has no faces")
        vertices = torch.from_numpy(model["vertices"]).to(args.device)
        faces = torch.from_numpy(model["faces"]).to(args.device)
        if args.mesh_distance:
            mesh = (vertices.contiguous(), faces.contiguous())
    if args.sample_spacing > 0:
        data = meshops.sample_surface(vertices, faces, spacing=args.sample_spacing, seed=args.sample_seed)[0]
    else:
        data = torch.from_numpy(ply.read_ply_vertices(files["ply"])).to(args.device)
    stl = torch.from_numpy(ply.read_ply_vertices(files["stl"])).to(args.device)
    obs, bb, res = PC.load_obs_mask(files["obs_mask"])
    plane = PC.load_plane(files["plane"])
    t1 = time.perf_counter()
    out = PC.dtu_score_scan(data, stl, obs, bb, res, plane, dst=args.dst, max_dist=args.max_dist, seed=args.seed,
                            **({"mesh": mesh} if mesh else {}))
    out["seconds"]["read"] = t1 - t0
    out["ply"] = files["ply"]
    if args.sample_spacing > 0:
        out["sampled_points"] = int(data.shape[0])
    return out


def main(argv=None) -> int:
    args = parse_args(argv)
    from patchmatchnet_amd import _lib
    from patchmatchnet_amd.pointcloud import totals
    os.makedirs(args.results_path, exist_ok=True)
    out_path = os.path.join(args.results_path, "dtu_scores.json")
    settings = {"dst": args.dst, "max_dist": args.max_dist, "seed": args.seed}
    if args.sample_spacing < 0:
        raise SystemExit("eval_dtu.py: --sample_spacing must be >= 0")
    if args.sample_spacing > 0:  # only then: a plain run's file keeps its keys, and the two kinds of scores are never mixed
        settings.update({"sample_spacing": args.sample_spacing, "sample_seed": args.sample_seed})
    if args.mesh_distance:
        settings["mesh_distance"] = True
    sampling = ("sample_spacing", "sample_seed", "mesh_distance")
    scores: Dict[str, Dict] = {}
    if os.path.isfile(out_path) and not args.force:
        with open(out_path) as f:
            old = json.load(f)
        if all(old.get(k) == v for k, v in settings.items()) and all(old.get(k) == settings.get(k) for k in sampling):
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
    from patchmatchnet_amd import PmnError
    try:
        sys.exit(main())
    except PmnError as e:
        sys.exit("eval_dtu.py: " + str(e))
