"""Guided upscaling on large scenes (rtiow_upscale_large, rtiow_upscale_wide_large): the parts that need no GPU, in the manner of
tests/test_large_preview_abi.py.  The rows of this feature live here, not in tests/abi_table.py and tests/test_kernel_inventory.py; the
checks are tests/test_abi.py's check_* functions wherever those take their row as arguments, and the two that read tests/abi_table.py
(arity, NULL handle) are restated over the table below."""
import json
import os
import re
import shutil
import subprocess

import pytest

from tests import test_abi as abi
from tests.conftest import ROOT

# symbol -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {
    "rtiow_upscale_large": (9, (None, 2, 0, 0.3, 0.1, 0.5, 1, None, None)),
    "rtiow_upscale_wide_large": (9, (None, 2, 0, 0.3, 0.1, 0.5, 1, None, None)),
}
# method -> its twin: the twin's parameter names and defaults; symbol -> the twin's symbol
TWINS = {"upscale_large": "upscale", "upscale_wide_large": "upscale_wide"}
TWIN_SYMBOLS = {"rtiow_upscale_large": "rtiow_upscale", "rtiow_upscale_wide_large": "rtiow_upscale_wide"}
UNIT = "rtiow_large_upscale.hip"
OTHER_UNITS = ("rtiow_hip.hip", "rtiow_group.hip", "rtiow_upscale.hip", "rtiow_upscale_wide.hip", "rtiow_large.hip", "rtiow_large_preview.hip")
DEVICE_GRID = 4
# the unit's kernel templates, each over RTIOW_SCENE_DEVICE_GRID -> the most VGPRs it may use: the top of the waves-per-SIMD step the
# build reaches (512 VGPRs a SIMD lane, granule 8: 64 -> 8 waves, 72 -> 7, 80 -> 6, 96 -> 5, 128 -> 4).  The counts themselves are in
# profiles/large_upscale/kernel_resources.json (60 / 80 and 58 / 80): the steps the twins are held to, which the grid walk happens to meet.
KERNELS = {
    "upscale_kernel<float, 4>": 64,
    "upscale_kernel<double, 4>": 80,
    "upscale_wide_kernel<float, 4>": 64,
    "upscale_wide_kernel<double, 4>": 80,
}
STEPS = (64, 72, 80, 96, 128, 168, 256, 512)


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_symbol_is_declared_listed_and_exported(native, symbol):
    abi.check_symbol(symbol)
    abi.check_abi_version()                                  # functions were added, nothing moved: still 6


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_declaration_has_the_headers_arity(native, symbol):
    from raytracingincuda_amd import api
    lib = api.load_hip_library()
    argtypes = getattr(lib, symbol).argtypes
    assert argtypes is not None and len(argtypes) == SYMBOLS[symbol][0] == len(SYMBOLS[symbol][1]), symbol
    assert tuple(argtypes) == tuple(getattr(lib, TWIN_SYMBOLS[symbol]).argtypes), symbol         # the twin's list
    header = abi._sources()[0]
    declared = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % symbol, header).group(1)
    twin = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % TWIN_SYMBOLS[symbol], header).group(1)
    assert len(declared.split(",")) == SYMBOLS[symbol][0], (symbol, declared)
    assert declared.split() == twin.split(), (symbol, declared)                                   # "the same parameters"


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_null_handle_needs_no_gpu(native, symbol):
    from raytracingincuda_amd import api
    assert getattr(api.load_hip_library(), symbol)(*SYMBOLS[symbol][1]) == -1, symbol


@pytest.mark.parametrize("method", TWINS)
def test_renderer_method_follows_its_twin(native, method):
    from raytracingincuda_amd import api
    assert callable(getattr(api.Renderer, method, None)), method
    abi.check_same_as(method, TWINS[method], None)           # the twin's parameters in its order, every default the twin's
    assert abi._parameters(method)["sync"].default is True
    assert getattr(api.RendererGroup, method, None) is None, method      # not available on groups
    assert not [s for s in api.HIP_SYMBOLS if "group" in s and ("large" in s or "upscal" in s)]


def _kernel_name(key):
    """"upscale_kernel<" must not count "upscale_wide_kernel<": the counting substring starts the kernel's name."""
    return re.compile(r"(?<![A-Za-z0-9_])" + re.escape(key))


def test_kernel_inventory(native):
    from raytracingincuda_amd import build
    from raytracingincuda_amd.kernel_metadata import device_metadata
    assert build.HIP_UNITS == OTHER_UNITS + (UNIT,)          # the seventh unit, linked last
    meta, _ = device_metadata(source=UNIT)
    templates = sorted(k for k in meta if "<" in k)
    counted = []
    for name in KERNELS:
        ks = [k for k in templates if _kernel_name(name).search(k)]
        assert len(ks) == 1, (name, ks)
        counted += ks
    # beside the plain (non-template) kernels every unit that includes the device headers emits, the unit instantiates no other kernel template
    assert sorted(set(templates) - set(counted)) == [], "the unit instantiates no other kernel template"
    # no upscale kernel over the device grid in any other unit
    for other in OTHER_UNITS:
        names = list(device_metadata(source=other)[0])
        assert not [k for k in names if re.search(r"upscale(_wide)?_kernel<(float|double), %d[,>]" % DEVICE_GRID, k)], other


def test_kernel_resources(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata(source=UNIT)
    record = json.load(open(os.path.join(ROOT, "profiles", "large_upscale", "kernel_resources.json")))["kernels"]
    for name, most in KERNELS.items():
        (k, v), = [(k, v) for k, v in meta.items() if _kernel_name(name).search(k)]
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)         # a condition, not a measurement
        assert most in STEPS and v["vgpr"] <= most, (k, v)
        assert STEPS[STEPS.index(most) - 1] < v["vgpr"] or most == STEPS[0], (k, v)      # the step the build reaches, not a looser one
        (row,) = [r for n, r in record.items() if _kernel_name(name).search(n)]
        assert (row["vgprs"], row["vgpr_spills"], row["scratch_bytes"]) == (v["vgpr"], 0, 0), (k, v, row)


def test_lds_placement_under_asan_ubsan(tmp_path):
    """The kernels' own LDS bytes behind what layout_large lays out (csrc/library/lds_placement.h): the wide kernel's footprint, the direct
    list at offset 0, the shade records and the tally words do not overlap, for a direct list of zero, nine and 2 048 entries."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "lds_placement_main")
    inc = os.path.join(ROOT, "raytracingincuda_amd", "csrc", "library")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + inc, "-o", exe, os.path.join(ROOT, "tests", "native", "lds_placement_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    assert r.stdout.splitlines()[-1] == "0 lds-placement failure(s)"
    # the sizes the program states are the device headers'
    dev = os.path.join(ROOT, "raytracingincuda_amd", "csrc", "device")
    narrow, wide = open(os.path.join(dev, "upscale.h")).read(), open(os.path.join(dev, "upscale_wide.h")).read()
    assert "UPSCALE_WAVES = 4;" in narrow and "UPSCALE_TALLY_BYTES = UPSCALE_WAVES * (int)sizeof(unsigned);" in narrow
    assert "(size_t)UPSCALE_WIDE_MAX_SIDE * UPSCALE_WIDE_MAX_SIDE * (3 * sizeof(Vec4<T>) + sizeof(int4))" in wide and "// 12: at most 144 staged pixels" in wide
