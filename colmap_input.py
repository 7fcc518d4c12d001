#!/usr/bin/env python
"""COLMAP sparse model -> MVSNet-layout input for eval.py (the reference's colmap_input.py, same flags and outputs).

    python colmap_input.py --input_folder COLMAP/dense/ [--output_folder OUT] [--num_src_images N]
    python colmap_input.py --input_folder COLMAP/ --output_folder OUT --undistort      a raw model: distorted cameras and pictures

Reads <input>/sparse/{cameras,images,points3D}.bin (COLMAP's binary model, as image_undistorter writes it) and <input>/images/, and
writes <output>/cams/%08d_cam.txt, <output>/pair.txt and <output>/images/%08d.jpg in images.bin order.  The output folder is
eval.py's --input_folder as it stands (no scan list).  The view-selection scores of every image pair are computed on the GPU
(pmn_view_scores); the rest is host file work (patchmatchnet_amd/colmap.py).

With --undistort the folder may be what structure-from-motion leaves (SIMPLE_RADIAL, OPENCV, fisheye ... cameras and the pictures as
taken): every picture is resampled into an ideal pinhole camera on the GPU (pmn_undistort_image; what COLMAP's image_undistorter
does), written as JPEG quality 95, and the cam files carry the pinhole intrinsics.  Without it the distortion
parameters are ignored, as in the reference."""
import argparse
import json
import sys


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Convert a COLMAP sparse model into PatchmatchNet's input layout")
    p.add_argument("--input_folder", type=str, help="COLMAP dense folder: sparse/*.bin and images/")
    p.add_argument("--output_folder", type=str, default="", help="output folder (default: the input folder)")
    p.add_argument("--num_src_images", type=int, default=-1, help="source views per reference view (-1: every image)")
    p.add_argument("--theta0", type=float, default=5)
    p.add_argument("--sigma1", type=float, default=1)
    p.add_argument("--sigma2", type=float, default=10)
    p.add_argument("--convert_format", action="store_true", default=False,
                   help="re-encode the images as JPEG (quality 95, through PIL) instead of copying their bytes")
    p.add_argument("--undistort", action="store_true", default=False,
                   help="resample every image into an ideal pinhole camera on the GPU and write that camera (for a model whose "
                        "cameras have distortion parameters; FOV and THIN_PRISM_FISHEYE are refused)")
    p.add_argument("--blank_pixels", type=float, default=0.0,
                   help="--undistort: 0 keeps only the part of the undistorted image that the source covers, 1 keeps every source pixel")
    p.add_argument("--min_scale", type=float, default=0.2, help="--undistort: lower bound of the image size change")
    p.add_argument("--max_scale", type=float, default=2.0, help="--undistort: upper bound of the image size change")
    p.add_argument("--max_image_size", type=int, default=-1, help="--undistort: longest side of the written images (-1: no limit)")
    p.add_argument("--device", type=str, default="cuda:0", help="GPU that computes the view-selection scores (and undistorts)")
    p.add_argument("--timings", action="store_true", default=False, help="print the time of each phase as one JSON line")
    return p


def main(argv=None) -> None:
    p = build_parser()
    args = p.parse_args(argv)
    if args.input_folder is None:
        p.error("--input_folder is required")
    from patchmatchnet_amd import colmap
    times = colmap.import_model(args.input_folder, args.output_folder, args.num_src_images, args.theta0, args.sigma1,
                                args.sigma2, args.convert_format, args.device, args.undistort, args.blank_pixels, args.min_scale,
                                args.max_scale, args.max_image_size)
    if args.timings:
        print(json.dumps({k: round(v, 6) for k, v in times.items()}))


if __name__ == "__main__":
    main(sys.argv[1:])
