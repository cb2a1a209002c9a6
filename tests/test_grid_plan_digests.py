"""library/grid_plan.h on the CPU.  The plans of both grids are pinned bit for bit: tests/golden/grid_plan_digests.json holds one SHA-256
per scene over everything the plan hooks return, recorded on the commit BEFORE the plans' arithmetic was stated once
(tests/golden/make_grid_plan_digests.py; the record names that commit), and the working tree has to return the same.  Then
tests/native/grid_plan_main.cpp, a stand-alone program built with AddressSanitizer + UBSan and run directly: plan_grid and
build_grid_blob in both precisions, held to the invariants that keep the kernel's reads of the LDS blob inside it."""
import json
import os
import shutil
import subprocess

import pytest

from tests import grid_plan_digests, large_scene
from tests.conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def record():
    return json.load(open(os.path.join(GOLDEN, "grid_plan_digests.json")))


def test_the_record_covers_every_scene(record):
    lds = {"reference_scene%d_f%d" % (s, p) for s in (1, 2, 3) for p in (32, 64)} | {"random_seed%d" % s for s in range(12)}
    lds |= {"declined_few", "declined_dense", "declined_bad"}
    large = {"lattice6000_f32", "lattice6000_f64", "lattice20000_f32", "line2000_f32", "line2000_f64", "ten_spheres"}
    large |= {"edge_%s_f%d" % (n, p) for n in large_scene.EDGE_SCENES for p in (32, 64)}
    large |= {"random_%s_f%d" % (c, p) for c in large_scene.RANDOM_CASES for p in (32, 64)}
    assert len(lds) == 21 and len(large) == 28 and len(large_scene.EDGE_SCENES) == 5 and len(large_scene.RANDOM_CASES) == 6
    assert set(record["grid_plan"]) == lds and set(record["large_grid_plan"]) == large
    assert len(record["commit"]) == 40 and all(len(d) == 64 for part in ("grid_plan", "large_grid_plan") for d in record[part].values())


def test_plans_are_the_recorded_ones_bit_for_bit(native, oracle, record):
    got = grid_plan_digests.all_digests(native, oracle)
    for part in ("grid_plan", "large_grid_plan"):
        assert set(got[part]) == set(record[part])
        differing = sorted(name for name in got[part] if got[part][name] != record[part][name])
        assert not differing, (part, differing)


def test_grid_plan_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "grid_plan_main")
    inc = os.path.join(ROOT, "raytracingincuda_amd", "csrc", "library")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + inc, "-o", exe, os.path.join(ROOT, "tests", "native", "grid_plan_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    assert r.stdout.splitlines()[-1] == "0 grid-plan failure(s)"
