#!/usr/bin/env python
"""Times one COLMAP import (patchmatchnet_amd.colmap.import_model) of the ~300-image synthetic model of tests/colmap_synth.py
(large_case: ~100k points, mean track length ~6) on the GPU, split into reading, host preparation, pmn_view_scores (device events)
and writing; prints one JSON line.  A warm-up import runs first (code-object load), the second is reported.  For the kernel alone
run it under `rocprofv3 --kernel-trace --stats -- python scripts/colmap_import_bench.py`."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    import colmap_synth as CS
    from patchmatchnet_amd import colmap as C
    kw = CS.large_case()
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "colmap")
        t = time.perf_counter()
        CS.write_case(src, kw)
        gen = time.perf_counter() - t
        res = []
        for k in range(2):
            out = os.path.join(tmp, "out%d" % k)
            os.makedirs(out)
            t = time.perf_counter()
            times = C.import_model(src, out, num_src_images=10)
            times["total"] = time.perf_counter() - t
            res.append(times)
        m = C.read_model(os.path.join(src, "sparse"))
        obs = C.view_selection_inputs(m)
    print(json.dumps({"model": {"images": kw["n_images"], "points": int(len(m.point_ids)), "observations": int(obs[1].size),
                                "track_entries": int(obs[3].size)},
                      "generate_s": round(gen, 3), "warmup": {k: round(v, 6) for k, v in res[0].items()},
                      "import": {k: round(v, 6) for k, v in res[1].items()}}))


if __name__ == "__main__":
    main()
