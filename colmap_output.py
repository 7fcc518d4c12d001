#!/usr/bin/env python
"""PatchmatchNet results -> COLMAP dense workspace (the reference's colmap_output.py, same flags and layout).

    python colmap_output.py --input_folder MVS/ [--results_folder RESULTS] [--output_folder WORKSPACE]

<input> is the MVSNet-layout folder (cams/, images/, pair.txt; e.g. colmap_input.py's output), <results> holds eval.py's depth_est/
and confidence/ maps (.pfm or .bin).  Writes images/, stereo/{depth,confidence}_maps/<image>.geometric.bin, stereo/patch-match.cfg,
stereo/fusion.cfg and a PINHOLE text model without points in sparse/, so that COLMAP's stereo_fusion can fuse the maps.  Host-only --
unless --normal_maps asks for stereo/normal_maps/<image>.geometric.bin as well (stereo_fusion opens one per image): those are computed
from the exported depth maps on a ROCm device (pmn_depth_normals)."""
import argparse
import sys


def main(argv=None) -> None:
    p = argparse.ArgumentParser(description="Convert PatchmatchNet results into a COLMAP dense workspace")
    p.add_argument("--input_folder", type=str, help="PatchmatchNet input folder (cams/, images/, pair.txt)")
    p.add_argument("--results_folder", type=str, default="", help="eval.py output folder (default: the input folder)")
    p.add_argument("--output_folder", type=str, default="", help="COLMAP workspace (default: the input folder)")
    p.add_argument("--normal_maps", action="store_true",
                   help="also write stereo/normal_maps/<image>.geometric.bin (camera-frame normals of the exported depth maps, "
                        "computed on --device; needs a ROCm GPU)")
    p.add_argument("--device", type=str, default="cuda:0", help="--normal_maps: the device the normal maps are computed on")
    p.add_argument("--normals_radius", type=int, default=2, choices=(1, 2, 3), help="--normal_maps: window radius of the plane fit")
    p.add_argument("--normals_depth_thres", type=float, default=0.01,
                   help="--normal_maps: relative depth difference up to which a neighbour counts as the same surface")
    args = p.parse_args(argv)
    if args.input_folder is None:
        p.error("--input_folder is required")
    from patchmatchnet_amd import colmap
    if not args.normal_maps:
        colmap.export_workspace(args.input_folder, args.results_folder, args.output_folder)
        return
    from patchmatchnet_amd import PmnError
    try:
        colmap.export_workspace(args.input_folder, args.results_folder, args.output_folder, normal_maps=True, device=args.device,
                                normals_radius=args.normals_radius, normals_depth_thres=args.normals_depth_thres)
    except PmnError as e:
        sys.exit("colmap_output.py: " + str(e))


if __name__ == "__main__":
    main(sys.argv[1:])
