"""The device grid's plan (csrc/library/device_grid.h) on the CPU.  tests/native/large_grid_plan_main.cpp is a stand-alone program, built
here with AddressSanitizer + UBSan and run directly: it holds plan and blob to the invariants that keep the kernel's gathers inside the
blob, on lattices of 6 000 to 100 000 spheres, a line of 2 000 and a scene the plan refuses.  Then the plan hook
(rtiow_debug_large_grid_plan: host arithmetic of the test build, no GPU) on the very scenes tests/test_render_large.py renders, so that
what those tests assume of their scenes is checked where no GPU is needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import large_scene
from tests.conftest import ROOT


def test_large_grid_plan_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "large_grid_plan_main")
    inc = os.path.join(ROOT, "raytracingincuda_amd", "csrc", "library")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + inc, "-o", exe, os.path.join(ROOT, "tests", "native", "large_grid_plan_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    assert r.stdout.splitlines()[-1] == "0 large-grid-plan failure(s)"


def _plan(native, scene, tables=False):
    return native.debug_large_grid_plan(np.asarray(scene["center_radius"], np.float64), large_scene.centre(scene), tables=tables)


@pytest.mark.parametrize("n,prec", [(6000, 32), (6000, 64), (20000, 32)])
def test_lattices_are_gridded_almost_whole(native, n, prec):
    """What test_oracle_parity_beyond_the_lds asserts of large_grid(), and that the scene is beyond the LDS at all."""
    sc = large_scene.lattice(n, prec)
    pl = _plan(native, sc, tables=True)
    assert pl["usable"] and pl["registered"] >= 0.9 * n and pl["direct"] <= 8, pl
    assert sorted(pl["direct_list"]) == [0, 1, 2, 3]                   # the ground and the three unit spheres
    m = len(sc["type"])
    padded = (m + 4) // 4 * 4
    assert (prec // 8 + 4) * 4 * padded > 160 * 1024                  # layout_lds: the default source's tables do not fit
    cells, idx = pl["cells"].reshape(-1, 2).astype(np.int64), pl["indices"]
    assert (cells[:, 0] + cells[:, 1] <= len(idx)).all() and idx.max() < m and cells[:, 1].max() == pl["longest_list"]
    assert pl["nx"] * pl["nz"] > 4096                                  # more cells than the LDS grid may have


def test_at_most_two_of_the_random_scenes_are_refused(native):
    """test_same_image_as_the_existing_paths asserts the refusal of a scene the plan does not suit: it must not pass on refusals alone."""
    refused = [(case, prec) for case in large_scene.RANDOM_CASES for prec in (32, 64) if not _plan(native, large_scene.random_case(case)[prec])["usable"]]
    assert len({case for case, _ in refused}) <= 2, refused


def test_the_line_is_longer_than_any_walk_of_the_lds_grid(native):
    for prec in (32, 64):
        pl = _plan(native, large_scene.line(2000, prec))
        assert pl["usable"] and pl["nx"] + pl["nz"] > 128, pl


def test_ten_spheres_are_refused(native):
    assert not _plan(native, large_scene.ten_spheres())["usable"]
