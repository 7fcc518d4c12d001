"""The launch-plan recorder under AddressSanitizer and UBSan, on the CPU: tests/plan_host/plan_host_test.cpp includes
patchmatchnet_amd/csrc/plan.hip over host stubs for its HIP calls (tests/plan_host/hip_stubs.hpp) and has its own main -- appending,
the fork/join bookkeeping, replay order by part, destroy.  A stand-alone program with the sanitizer runtimes linked in statically:
nothing sanitized is loaded into python and nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_recorder_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "plan_host_test")
    static = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") else []
    build = subprocess.run([cxx, "-std=c++17", "-x", "c++", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            *static, "-Wall", "-o", exe, os.path.join(ROOT, "tests", "plan_host", "plan_host_test.cpp")],
                           capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and "san" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtimes to link")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "plan_host_test ok" in run.stdout, run.stdout + run.stderr
