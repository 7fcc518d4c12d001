#!/usr/bin/env python
"""COLMAP sparse model -> MVSNet-layout input for eval.py (the reference's colmap_input.py, same flags and outputs).

    python colmap_input.py --input_folder COLMAP/dense/ [--output_folder OUT] [--num_src_images N]

Reads <input>/sparse/{cameras,images,points3D}.bin (COLMAP's binary model, as image_undistorter writes it) and <input>/images/, and
writes <output>/cams/%08d_cam.txt, <output>/pair.txt and <output>/images/%08d.jpg in images.bin order.  The output folder is
eval.py's --input_folder as it stands (no scan list).  The view-selection scores of every image pair are computed on the GPU
(pmn_view_scores); the rest is host file work (patchmatchnet_amd/colmap.py)."""
import argparse
import json
import sys


def main(argv=None) -> None:
    p = argparse.ArgumentParser(description="Convert a COLMAP sparse model into PatchmatchNet's input layout")
    p.add_argument("--input_folder", type=str, help="COLMAP dense folder: sparse/*.bin and images/")
    p.add_argument("--output_folder", type=str, default="", help="output folder (default: the input folder)")
    p.add_argument("--num_src_images", type=int, default=-1, help="source views per reference view (-1: every image)")
    p.add_argument("--theta0", type=float, default=5)
    p.add_argument("--sigma1", type=float, default=1)
    p.add_argument("--sigma2", type=float, default=10)
    p.add_argument("--convert_format", action="store_true", default=False,
                   help="re-encode the images as JPEG (quality 95, through PIL) instead of copying their bytes")
    p.add_argument("--device", type=str, default="cuda:0", help="GPU that computes the view-selection scores")
    p.add_argument("--timings", action="store_true", default=False, help="print the time of each phase as one JSON line")
    args = p.parse_args(argv)
    if args.input_folder is None:
        p.error("--input_folder is required")
    from patchmatchnet_amd import colmap
    times = colmap.import_model(args.input_folder, args.output_folder, args.num_src_images, args.theta0, args.sigma1,
                                args.sigma2, args.convert_format, args.device)
    if args.timings:
        print(json.dumps({k: round(v, 6) for k, v in times.items()}))


if __name__ == "__main__":
    main(sys.argv[1:])
