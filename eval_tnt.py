"""Tanks and Temples precision / recall / F-score of a reconstruction, on the GPU: the protocol of the benchmark's evaluation toolbox
(patchmatchnet_amd/registration.py).

    python eval_tnt.py --dataset_dir <T&T>/Barn --ply_path outputs/Barn/fused.ply --mvs_folder <MVS>/Barn --scene Barn \
        --results_path outputs/Barn

--dataset_dir holds <Scene>.ply (the ground truth), <Scene>.json (the crop volume), <Scene>_COLMAP_SfM.log (the reference trajectory)
and <Scene>_trans.txt.  The reconstruction's cameras come from --trajectory LOG or from <mvs_folder>/cams/*_cam.txt; --init_transform
FILE (a 4 x 4 matrix) replaces the trajectory alignment, --no_registration scores a cloud that already is in the ground truth's frame.
With --mesh_distance 1 recall is the exact distance from the ground truth to the triangles of --ply_path.
--ply_path may be a mesh: its vertices are read as a cloud or, with --sample_spacing S, points drawn on its triangles S apart
(meshops.sample_surface) are scored: the surface, not the lattice its vertices sit on.  Scores go to
<results_path>/tnt_scores.json.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time


def parse_args(argv=None):
    from patchmatchnet_amd import registration as RG
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--dataset_dir", required=True, help="folder of the scene's ground truth: <Scene>.ply, .json, _COLMAP_SfM.log, _trans.txt")
    p.add_argument("--ply_path", required=True, help="the reconstruction: fused.ply, or a mesh whose vertices are scored")
    p.add_argument("--results_path", required=True, help="folder tnt_scores.json is written to")
    p.add_argument("--mvs_folder", default=None, help="MVS folder of the scene (cams/*_cam.txt give the reconstruction's cameras)")
    p.add_argument("--trajectory", default=None, help=".log trajectory of the reconstruction's cameras (instead of --mvs_folder)")
    p.add_argument("--init_transform", default=None, help="4 x 4 text matrix: reconstruction -> ground truth, replaces the trajectory alignment")
    p.add_argument("--scene", default=None, help="scene name: file prefix inside --dataset_dir (default: the folder's name) and tau")
    p.add_argument("--tau", type=float, default=None, help="distance threshold (default: the scene's)")
    p.add_argument("--no_registration", action="store_true", help="the cloud is in the ground truth's frame: no alignment, no ICP")
    p.add_argument("--no_crop", action="store_true", help="do not crop (no <Scene>.json needed)")
    p.add_argument("--round_a", type=float, nargs=2, default=list(RG.ROUND_A), metavar=("VOXEL", "DIST"), help="round A, in units of tau")
    p.add_argument("--round_b", type=float, nargs=2, default=list(RG.ROUND_B), metavar=("VOXEL", "DIST"), help="round B, in units of tau")
    p.add_argument("--round_c_dist", type=float, default=RG.ROUND_C_DIST, help="ICP distance of round C, in units of tau")
    p.add_argument("--icp_iterations", type=int, default=RG.ICP_ITERATIONS)
    p.add_argument("--max_points", type=int, default=RG.MAX_POINTS, help="round C thins both clouds to at most this many points")
    p.add_argument("--hist_max", type=float, default=None, help="cap of the distances and end of the histograms (default 5 tau)")
    p.add_argument("--hist_bins", type=int, default=RG.HIST_BINS)
    p.add_argument("--sample_spacing", type=float, default=0.0,
                   help="score points drawn on the triangles of --ply_path (a mesh) this far apart, in its own units (0 = off: the vertices)")
    p.add_argument("--sample_seed", type=int, default=0, help="seed of --sample_spacing's points")
    p.add_argument("--mesh_distance", type=int, default=0, choices=[0, 1],
                   help="1: recall is measured against the triangles of --ply_path themselves (exact point-to-mesh distance), not against "
                        "its vertices or samples; precision is unchanged")
    p.add_argument("--device", default="cuda:0")
    args = p.parse_args(argv)
    if args.sample_spacing < 0:
        p.error("--sample_spacing must be >= 0")
    if args.scene is None:
        args.scene = os.path.basename(os.path.normpath(args.dataset_dir))
    if args.tau is None:
        if args.scene not in RG.SCENE_TAU:
            p.error(f"no tau known for scene {args.scene!r} (known: {', '.join(sorted(RG.SCENE_TAU))}): give --tau")
        args.tau = RG.SCENE_TAU[args.scene]
    if not args.tau > 0:
        p.error("--tau must be positive")
    if not (args.no_registration or args.init_transform or args.trajectory or args.mvs_folder):
        p.error("one of --mvs_folder, --trajectory, --init_transform or --no_registration is needed")
    return args


def camera_centres_from_mvs(folder: str):
    """Camera-to-world matrices [m,4,4] of <folder>/cams/*_cam.txt, in file-name order."""
    import numpy as np

    from patchmatchnet_amd.data_io import read_cam_file
    files = sorted(glob.glob(os.path.join(folder, "cams", "*_cam.txt")))
    if not files:
        raise FileNotFoundError(os.path.join(folder, "cams", "*_cam.txt"))
    return np.stack([np.linalg.inv(np.asarray(read_cam_file(f)[1], np.float64)) for f in files])


def initial_transform(args):
    """gt_trans @ umeyama(reconstruction's camera centres -> reference trajectory's), cameras paired by index."""
    import numpy as np

    from patchmatchnet_amd import registration as RG
    if args.no_registration:
        return np.eye(4)
    if args.init_transform:
        return RG.read_transform(args.init_transform)
    own = RG.read_trajectory_log(args.trajectory) if args.trajectory else camera_centres_from_mvs(args.mvs_folder)
    ref = RG.read_trajectory_log(os.path.join(args.dataset_dir, f"{args.scene}_COLMAP_SfM.log"))
    if len(own) != len(ref):
        raise ValueError(f"{len(own)} cameras of the reconstruction against {len(ref)} of the reference trajectory: they are paired by index")
    gt_trans = RG.read_transform(os.path.join(args.dataset_dir, f"{args.scene}_trans.txt"))
    return gt_trans @ RG.umeyama(own[:, :3, 3], ref[:, :3, 3], with_scale=True)


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch

    from patchmatchnet_amd import _lib, ply, registration as RG
    t0 = time.perf_counter()
    mesh = None
    if args.sample_spacing > 0 or args.mesh_distance:
        from patchmatchnet_amd import meshops
        model = ply.read_ply_model(args.ply_path)
        if model["faces"] is None or len(model["faces"]) == 0:
            flag = "--sample_spacing" if args.sample_spacing > 0 else "--mesh_distance"
            raise _lib.PmnError(f"{args.ply_path}: {flag} needs a mesh, this file has no faces")
        vertices = torch.from_numpy(model["vertices"]).to(args.device)
        faces = torch.from_numpy(model["faces"]).to(args.device)
        if args.mesh_distance:
            mesh = (vertices.contiguous(), faces.contiguous())
    if args.sample_spacing > 0:
        est = meshops.sample_surface(vertices, faces, spacing=args.sample_spacing, seed=args.sample_seed)[0]
        print("%s: %d points sampled on %d triangles" % (args.ply_path, est.shape[0], len(model["faces"])))
    else:
        est = torch.from_numpy(ply.read_ply_vertices(args.ply_path)).to(args.device)
    gt = torch.from_numpy(ply.read_ply_vertices(os.path.join(args.dataset_dir, f"{args.scene}.ply"))).to(args.device)
    volume = None if args.no_crop else RG.read_crop_json(os.path.join(args.dataset_dir, f"{args.scene}.json"))
    init = initial_transform(args)
    t1 = time.perf_counter()
    out = RG.tnt_score(est, gt, volume, args.tau, init=init, register=not args.no_registration, round_a=tuple(args.round_a),
                       round_b=tuple(args.round_b), round_c_dist=args.round_c_dist, icp_iterations=args.icp_iterations,
                       max_points=args.max_points, hist_max=args.hist_max, bins=args.hist_bins, **({"mesh": mesh} if mesh else {}))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for r in out["rounds"]:
        print("registration round %s: fitness %f, inlier rmse %f, %d iterations" % (r["round"], r["fitness"], r["rmse"], r["iterations"]))
    print("precision : %.4f" % out["precision"])
    print("recall : %.4f" % out["recall"])
    print("f-score : %.4f" % out["fscore"])
    os.makedirs(args.results_path, exist_ok=True)
    out.update({"scene": args.scene, "ply": args.ply_path, "abi": _lib.ABI_VERSION, "init_transform": init.tolist(),
                "registration": not args.no_registration, "seconds": {"read": t1 - t0, "score": t2 - t1}})
    if args.sample_spacing > 0:
        out.update({"sample_spacing": args.sample_spacing, "sample_seed": args.sample_seed, "sampled_points": int(est.shape[0])})
    if args.mesh_distance:
        out["mesh_distance"] = True
    with open(os.path.join(args.results_path, "tnt_scores.json"), "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    from patchmatchnet_amd import PmnError
    try:
        sys.exit(main())
    except PmnError as e:
        sys.exit("eval_tnt.py: " + str(e))
