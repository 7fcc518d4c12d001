"""A fresh child interpreter that sees NO device, for the few CPU tests whose point is what a launch answers without one
(tests/test_plan.py, tests/test_plan_branch.py): library calls made outside a recording, and pmn_plan_launch[_part], really launch
where a device is visible -- on the placeholder addresses those tests record.  Such statements therefore live in the ``body`` handed
to run() and nowhere else: the child's environment hides every device (HIP_VISIBLE_DEVICES = CUDA_VISIBLE_DEVICES = ""), and the
prologue below ends the child before the body when one is visible all the same.  Plain helper module (no tests here)."""
import json
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROLOGUE = """\
import ctypes, json, threading
import torch
assert not torch.cuda.is_available() and torch.cuda.device_count() == 0, "a device is visible: the body must not run"
from patchmatchnet_amd import _lib
L = _lib.lib()


def new_plan():
    p = ctypes.c_void_p()
    assert L.pmn_plan_create(ctypes.byref(p)) == 0 and p.value
    return p


"""


def run(body: str, timeout: float = 120.0) -> dict:
    """Runs PROLOGUE + ``body`` (which ends in ``print("NODEVICE_JSON " + json.dumps(...))``) in a child without a device -> that
    dict.  The child must return 0."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, "-c", PROLOGUE + textwrap.dedent(body)], env=env, capture_output=True, text=True, timeout=timeout,
                       cwd=ROOT)
    assert r.returncode == 0, f"child returned {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("NODEVICE_JSON ")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0][len("NODEVICE_JSON "):])
