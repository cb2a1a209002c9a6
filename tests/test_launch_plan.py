"""The schedule's arithmetic (csrc/library/launch_plan.h) on the CPU: tests/native/launch_plan_main.cpp is a stand-alone program, built
here with AddressSanitizer + UBSan and run directly.  It pins the plans of five frames derived by hand, checks every rule one step
either side of its edge, and holds the plan to its invariants over a sweep of frames and occupancies; UBSan sees every intermediate."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


def test_launch_plan_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "launch_plan_main")
    inc = os.path.join(ROOT, "raytracingincuda_amd", "csrc", "library")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + inc, "-o", exe, os.path.join(ROOT, "tests", "native", "launch_plan_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    assert "0 launch-plan failure(s)" in r.stdout
