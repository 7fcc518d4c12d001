#!/usr/bin/env python
"""PatchmatchNet checkpoint validation against ground-truth depth -- the reference's ``train.py --mode test`` (reference train.py:63-76,
127-181, 200-end), as a drop-in command line:

    python train.py --mode test --input_folder DATA --output_folder CKPT_DIR --test_list lists/dtu/val.txt [--checkpoint_path X]

Every scan of the list needs <scan>/depth_gt/<view:08d>.pfm for each reference view.  Per batch it prints the reference's
``Iter i/N, test loss = ..., time = ...`` line (time = GPU seconds of the batch: upload, forward and metrics), every 100 batches the
running means, and at the end ``final {...}`` -- the per-batch scalars averaged with equal weight per batch, as DictAverageMeter does.
The lines trail the GPU by a few batches (patchmatchnet_amd/validate.py: the batch loop never waits for the device).

Training is not part of this engine (its kernels have no backward pass): ``--mode train`` exits with an error, and the training-only
flags are accepted and ignored.  Single process, single GPU: running under torchrun is not supported.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

import patchmatchnet_amd as P
from patchmatchnet_amd import validate as V
from patchmatchnet_amd.mvs import MVSDataset


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="PatchMatchNet for high-resolution multi-view stereo: checkpoint validation against "
                                            "ground-truth depth (--mode test). Single process on one GPU; torchrun is not supported.")
    p.add_argument("--mode", type=str, default="train", help="Execution mode (only test is supported)", choices=["train", "test"])
    p.add_argument("--input_folder", type=str, help="input data path")
    p.add_argument("--output_folder", type=str, default="", help="output path (where the latest *.ckpt is looked for)")
    p.add_argument("--checkpoint_path", type=str, default="", help="load a specific checkpoint for parameters (.ckpt or .npz)")
    p.add_argument("--num_views", type=int, default=5, help="number of source views for each patch-match problem")
    p.add_argument("--image_max_dim", type=int, default=640, help="max image dimension")
    p.add_argument("--train_list", type=str, help="training scan list text file (accepted, ignored)")
    p.add_argument("--test_list", type=str, help="validation scan list text file")
    p.add_argument("--num_light_idx", type=int, default=-1, help="Number of light indexes in source images")
    p.add_argument("--batch_size", type=int, default=12, help="validation batch size")
    # training options of the reference: accepted and ignored
    p.add_argument("--resume", action="store_true", default=False, help="training only (ignored)")
    p.add_argument("--epochs", type=int, default=16, help="training only (ignored)")
    p.add_argument("--learning_rate", type=float, default=0.001, help="training only (ignored)")
    p.add_argument("--lr_epochs", type=str, default="10,12,14:2", help="training only (ignored)")
    p.add_argument("--weight_decay", type=float, default=0.0, help="training only (ignored)")
    p.add_argument("--summary_freq", type=int, default=20, help="training only (ignored)")
    p.add_argument("--save_freq", type=int, default=1, help="training only (ignored)")
    p.add_argument("--rand_seed", type=int, default=1, metavar="S", help="random seed (torch.manual_seed)")
    p.add_argument("--patchmatch_interval_scale", nargs="+", type=float, default=[0.005, 0.0125, 0.025],
                   help="normalized interval in inverse depth range to generate samples in local perturbation")
    p.add_argument("--propagation_range", nargs="+", type=int, default=[6, 4, 2],
                   help="fixed offset of sampling points for propagation of patch match on stages 1,2,3")
    p.add_argument("--patchmatch_iteration", nargs="+", type=int, default=[1, 2, 2],
                   help="num of iteration of patch match on stages 1,2,3")
    p.add_argument("--patchmatch_num_sample", nargs="+", type=int, default=[8, 8, 16],
                   help="num of generated samples in local perturbation on stages 1,2,3")
    p.add_argument("--propagate_neighbors", nargs="+", type=int, default=[0, 8, 16],
                   help="num of neighbors for adaptive propagation on stages 1,2,3")
    p.add_argument("--evaluate_neighbors", nargs="+", type=int, default=[9, 9, 9],
                   help="num of neighbors for adaptive matching cost aggregation of adaptive evaluation on stages 1,2,3")
    # additions of this engine
    p.add_argument("--metrics_json", type=str, default="",
                   help="write every sample's scan, view, raw metrics row and per-image metrics, and the final dict, to this file")
    p.add_argument("--hip_graph", type=int, default=1, choices=(0, 1),
                   help="1: one launch-plan replay per batch covering the forward and the metrics; 0: eager forward")
    p.add_argument("--num_workers", type=int, default=4, help="DataLoader workers (the reference's test loader uses 4)")
    return p


def find_latest_checkpoint(path: str) -> str:
    """The reference's rule (train.py:186-192): the *.ckpt of ``path`` whose name ends in the highest number, "" if none."""
    if not path or not os.path.isdir(path):
        return ""
    saved = [fn for fn in os.listdir(path) if fn.endswith(".ckpt")]
    if not saved:
        return ""
    saved = sorted(saved, key=lambda x: int(x.split("_")[-1].split(".")[0]))
    return os.path.join(path, saved[-1])


def load_model(args, device):
    """A .ckpt ({"model": state_dict}, DataParallel's "module." prefix accepted) or an .npz of the same names, as eval.py loads them."""
    model = P.PatchmatchNet(patchmatch_interval_scale=args.patchmatch_interval_scale, propagation_range=args.propagation_range,
                            patchmatch_iteration=args.patchmatch_iteration, patchmatch_num_sample=args.patchmatch_num_sample,
                            propagate_neighbors=args.propagate_neighbors, evaluate_neighbors=args.evaluate_neighbors)
    if args.checkpoint_path.endswith(".npz"):
        with np.load(args.checkpoint_path) as z:
            state = {k: torch.from_numpy(z[k]) for k in z.files}
    else:
        state = torch.load(args.checkpoint_path, map_location="cpu")["model"]
    model.load_state_dict(state, strict=True)
    return model.to(device).eval()


def _json_row(result, i, iters, thresholds):
    return {"scan": result["scans"][i], "view": result["views"][i], "batch": result["batch"],
            "row": [V.finite_or_none(float(x)) for x in result["rows"][i]],
            "metrics": {k: V.finite_or_none(v) for k, v in V.image_metrics(result["rows"][i], iters, thresholds).items()}}


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if args.mode == "train":
        print("train.py: training is not supported by this engine (its HIP kernels have no backward pass); use --mode test",
              file=sys.stderr)
        return 2
    print("argv:", sys.argv[1:] if argv is None else argv)
    if not args.input_folder or not os.path.isdir(args.input_folder):
        raise Exception("Invalid input folder: {}".format(args.input_folder))
    if not args.test_list or not os.path.isfile(args.test_list):
        raise Exception("Invalid validation scan list file: {}".format(args.test_list))
    if not args.output_folder:
        args.output_folder = args.input_folder
    if not args.checkpoint_path:
        args.checkpoint_path = find_latest_checkpoint(args.output_folder)
    if not os.path.isfile(args.checkpoint_path):
        raise Exception("Invalid checkpoint file: {}".format(args.checkpoint_path))
    dataset = MVSDataset(data_path=args.input_folder, num_views=args.num_views, max_dim=args.image_max_dim, scan_list=args.test_list,
                         num_light_idx=args.num_light_idx, load_depth_gt=True)
    missing = dataset.missing_depth_gt()
    if missing:
        # the reference's dataset returns empty arrays for such a view, and its DataLoader then fails to collate the batch
        shown = ", ".join("{}/{}".format(s, dataset.depth_folder + "/{:0>8}.pfm".format(v)) for s, v in missing[:5])
        raise Exception("{} of {} samples have no ground-truth depth map ({}{}); validation needs one per reference view".format(
            len(missing), len(dataset), shown, ", ..." if len(missing) > 5 else ""))
    if not torch.cuda.is_available():
        raise P.PmnError("train.py --mode test runs on a ROCm GPU; none is visible")
    torch.manual_seed(args.rand_seed)
    device = torch.device("cuda", torch.cuda.current_device())
    loader = DataLoader(dataset, args.batch_size, shuffle=False, num_workers=max(args.num_workers, 0), drop_last=False,
                        pin_memory=True)

    print("Validation using checkpoint: ", args.checkpoint_path)
    model = load_model(args, device)
    iters = V.stage_iterations(model)
    validator = V.Validator(model, iters, V.THRESHOLDS, hip_graph=args.hip_graph, depth=4, device=device)
    avg = V.DictAverage()
    per_sample = []
    num_batches = len(loader)

    def report(results):
        for r in results:
            avg.update(r["scalars"])
            print("Iter {}/{}, test loss = {:.3f}, time = {:3f}".format(r["batch"] + 1, num_batches, r["scalars"]["loss"], r["time"]))
            if (r["batch"] + 1) % 100 == 0:
                print("Iter {}/{}, test results = {}".format(r["batch"] + 1, num_batches, avg.mean()))
            if args.metrics_json:
                per_sample.extend(_json_row(r, i, iters, V.THRESHOLDS) for i in range(len(r["scans"])))

    t0 = time.time()
    for batch in loader:
        report(validator.submit(batch))
    report(validator.drain())
    final = avg.mean()
    print("final", final)
    print("validated {} samples in {} batches, {:.2f} s".format(len(dataset), num_batches, time.time() - t0))
    if args.metrics_json:
        with open(args.metrics_json, "w") as f:
            json.dump({"checkpoint": args.checkpoint_path, "iters": iters, "thresholds": list(V.THRESHOLDS),
                       "samples": per_sample, "final": {k: V.finite_or_none(v) for k, v in final.items()}}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
