"""Scene edits that keep the history (rtiow_edit_scene, rtiow_read_scene_motion, surface_motion_kernel and the three motion_*_kernel): the
parts that need no GPU.  The rows of this feature live here, not in tests/abi_table.py and tests/test_kernel_inventory.py; the checks are
tests/test_abi.py's check_* functions wherever those take their row as arguments, and the two that read tests/abi_table.py (arity, NULL
handle) are restated over the table below.  The policy's share is tests/native/scene_motion_state_main.cpp, a stand-alone program over
csrc/library/preview_state.h alone, built here with AddressSanitizer + UBSan and run directly."""
import os
import re
import shutil
import subprocess

import pytest

from tests import test_abi as abi
from tests.conftest import ROOT

# symbol -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {"rtiow_edit_scene": (7, (None, 4, None, None, None, None, None)), "rtiow_read_scene_motion": (5, (None, None, None, None, 0))}
METHODS = {"edit_scene": ("scene",), "scene_motion": ()}
# counting substring of the demangled name -> instantiations: fp32 / fp64 (x LDS / scalar scene source for the plane)
KERNELS = {"surface_motion_kernel<": 4, "motion_reproject_kernel<": 2, "motion_length_kernel<": 2, "motion_clip_kernel<": 2}
FROZEN_NAMES = ("render_", "variance_", "guide_kernel<", "guide_chain_kernel<", "history_reproject_kernel<", "history_length_kernel<", "history_clip_kernel<")


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_symbol_is_declared_listed_and_exported(native, symbol):
    abi.check_symbol(symbol)
    abi.check_abi_version()                                  # functions were added, no struct moved: still 6


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_declaration_has_the_headers_arity(native, symbol):
    from raytracingincuda_amd import api
    argtypes = getattr(api.load_hip_library(), symbol).argtypes
    assert argtypes is not None and len(argtypes) == SYMBOLS[symbol][0] == len(SYMBOLS[symbol][1]), symbol
    declared = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % symbol, abi._sources()[0]).group(1)
    assert len(declared.split(",")) == SYMBOLS[symbol][0], (symbol, declared)


def test_edit_scene_takes_set_scenes_arguments(native):
    from raytracingincuda_amd import api
    assert api.HIP_ABI["rtiow_edit_scene"] == api.HIP_ABI["rtiow_set_scene"]
    header = abi._sources()[0]
    args = lambda s: re.sub(r"\s+", " ", re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, header).group(1))
    assert args("rtiow_edit_scene") == args("rtiow_set_scene")


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_null_handle_needs_no_gpu(native, symbol):
    from raytracingincuda_amd import api
    assert getattr(api.load_hip_library(), symbol)(*SYMBOLS[symbol][1]) == -1, symbol


@pytest.mark.parametrize("member", METHODS)
def test_renderer_has_the_member(native, member):
    from raytracingincuda_amd import api
    assert callable(getattr(api.Renderer, member, None)), member
    assert list(abi._parameters(member)) == ["self"] + list(METHODS[member]), member


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_count_and_resources(native, name):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata()
    ks = {k: v for k, v in meta.items() if name in k}
    assert len(ks) == KERNELS[name], (name, sorted(ks))
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        for frozen in FROZEN_NAMES:
            assert frozen not in k, (k, frozen)              # the names frozen tests count by
    for prec in ("float", "double"):
        if name == "surface_motion_kernel<":
            for src in (0, 1):
                assert [k for k in ks if "%s%s, %d>" % (name, prec, src) in k], (prec, src)
        else:
            assert [k for k in ks if "%s%s>" % (name, prec) in k], prec
    # no row of the frozen inventory counts these kernels too, and the inventory's own rows still hold with them in the library
    from tests import test_kernel_inventory as inventory
    assert not [row for row in inventory.KERNELS for k in ks if row in k]
    for family in inventory.FAMILIES:
        assert not [k for k in ks if family in k], family
    inventory.check_disjoint()
    for row in ("guide_kernel<", "history_reproject_kernel<", "history_length_kernel<", "history_clip_kernel<"):
        inventory.check_row(row)


def test_scene_motion_state_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    inc = os.path.join(ROOT, "raytracingincuda_amd", "csrc", "library")
    exe = str(tmp_path / "scene_motion_state_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + inc, "-o", exe, os.path.join(ROOT, "tests", "native", "scene_motion_state_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    assert r.stdout.splitlines()[-1] == "0 scene-motion rule failure(s)"
