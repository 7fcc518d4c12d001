#!/usr/bin/env python
"""PatchmatchNet results -> COLMAP dense workspace (the reference's colmap_output.py, same flags and layout).

    python colmap_output.py --input_folder MVS/ [--results_folder RESULTS] [--output_folder WORKSPACE]

<input> is the MVSNet-layout folder (cams/, images/, pair.txt; e.g. colmap_input.py's output), <results> holds eval.py's depth_est/
and confidence/ maps (.pfm or .bin).  Writes images/, stereo/{depth,confidence}_maps/<image>.geometric.bin, stereo/patch-match.cfg,
stereo/fusion.cfg and a PINHOLE text model without points in sparse/, so that COLMAP's stereo_fusion can fuse the maps.  Host-only."""
import argparse
import sys


def main(argv=None) -> None:
    p = argparse.ArgumentParser(description="Convert PatchmatchNet results into a COLMAP dense workspace")
    p.add_argument("--input_folder", type=str, help="PatchmatchNet input folder (cams/, images/, pair.txt)")
    p.add_argument("--results_folder", type=str, default="", help="eval.py output folder (default: the input folder)")
    p.add_argument("--output_folder", type=str, default="", help="COLMAP workspace (default: the input folder)")
    args = p.parse_args(argv)
    if args.input_folder is None:
        p.error("--input_folder is required")
    from patchmatchnet_amd import colmap
    colmap.export_workspace(args.input_folder, args.results_folder, args.output_folder)


if __name__ == "__main__":
    main(sys.argv[1:])
