#!/usr/bin/env python
"""Pin the reference's COLMAP converters (colmap_input.py, colmap_output.py) on the synthetic models of tests/colmap_synth.py.

Runs only where the reference checkout exists (PMN_REFERENCE_ROOT, see tests/refutil.py):

    python tests/golden/make_colmap_golden.py        # writes tests/golden/colmap_reference.npz

For every case of colmap_synth.CASES the model and its images are generated from the case's seed, the reference's own scripts run in
a subprocess on them, and their output FILES are stored (bytes, as uint8 arrays) with the sha256 of the model files; the tests
regenerate the models from the seeds and compare.  cv2 is not installed: a stub module stands in for it (the reference calls cv2
only under --convert_format, which the cases do not use).  The reference's colmap_output.py lists directories with os.listdir,
whose order the file system decides; the runner sorts those listings, so the stored files list views in ascending id order.

colmap_output.py runs on the MVSNet-layout folder colmap_input.py wrote, with seeded depth / confidence maps as the results
(.pfm, written by patchmatchnet_amd.data_io.save_pfm; the generator of those maps is ``result_maps`` below)."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import colmap_synth as CS  # noqa: E402
import refutil  # noqa: E402

RUNNER = r"""
import os, runpy, sys, types
sys.modules["cv2"] = types.ModuleType("cv2")
_listdir = os.listdir
os.listdir = lambda p=".": sorted(_listdir(p))
script = sys.argv[1]
sys.path.insert(0, os.path.dirname(script))
sys.argv = sys.argv[1:]
runpy.run_path(script, run_name="__main__")
"""

OUTPUT_FILES = ["sparse/cameras.txt", "sparse/images.txt", "sparse/points3D.txt", "stereo/patch-match.cfg", "stereo/fusion.cfg"]


def result_maps(out_dir: str, n_images: int, seed: int) -> None:
    """depth_est/%08d.pfm and confidence/%08d.pfm of every view: seeded float32 maps of the images' size (24 x 32)."""
    from patchmatchnet_amd.data_io import save_pfm
    rng = np.random.default_rng(1000 + seed)
    for kind in ("depth_est", "confidence"):
        os.makedirs(os.path.join(out_dir, kind), exist_ok=True)
    for v in range(n_images):
        save_pfm(os.path.join(out_dir, "depth_est", "%08d.pfm" % v), rng.uniform(5, 11, (24, 32)).astype(np.float32))
        save_pfm(os.path.join(out_dir, "confidence", "%08d.pfm" % v), rng.uniform(0, 1, (24, 32)).astype(np.float32))


def run_reference(script: str, args):
    with tempfile.NamedTemporaryFile("w", suffix=".py", delete=False) as f:
        f.write(RUNNER)
        runner = f.name
    try:
        t = time.perf_counter()
        subprocess.run([sys.executable, runner, os.path.join(refutil.REFERENCE_ROOT, script)] + list(args), check=True,
                       stdout=subprocess.DEVNULL)
        return time.perf_counter() - t
    finally:
        os.unlink(runner)


def main() -> None:
    out = {}
    for name, case in CS.CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            src, mvs, ws = (os.path.join(tmp, d) for d in ("colmap", "mvs", "workspace"))
            for d in (mvs, ws):
                os.makedirs(d)
            out[f"{name}__model_sha256"] = np.array(CS.write_case(src, case["model"]))
            a = case["args"]
            secs = run_reference("colmap_input.py", ["--input_folder", src, "--output_folder", mvs, "--num_src_images",
                                                     str(a["num_src_images"]), "--theta0", str(a["theta0"]), "--sigma1",
                                                     str(a["sigma1"]), "--sigma2", str(a["sigma2"])])
            print(f"case {name}: reference colmap_input.py {secs:.2f} s (CPU)")
            n = case["model"]["n_images"]
            for v in range(n):
                with open(os.path.join(mvs, "cams", "%08d_cam.txt" % v), "rb") as f:
                    out[f"{name}__cams__{v:08d}"] = np.frombuffer(f.read(), np.uint8)
            with open(os.path.join(mvs, "pair.txt"), "rb") as f:
                out[f"{name}__pair"] = np.frombuffer(f.read(), np.uint8)
            result_maps(mvs, n, case["model"]["seed"])
            run_reference("colmap_output.py", ["--input_folder", mvs, "--output_folder", ws])
            for rel in OUTPUT_FILES:
                with open(os.path.join(ws, rel), "rb") as f:
                    out[f"{name}__ws__{rel.replace('/', '__')}"] = np.frombuffer(f.read(), np.uint8)
            for kind in ("depth_maps", "confidence_maps"):
                for v in range(n):
                    with open(os.path.join(ws, "stereo", kind, "%08d.jpg.geometric.bin" % v), "rb") as f:
                        out[f"{name}__ws__{kind}__{v:08d}"] = np.frombuffer(f.read(), np.uint8)
    path = os.path.join(HERE, "colmap_reference.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
