"""Guided upscaling (rtiow_upscale, rtiow_read_upscaled, rtiow_upscaled_device_ptr): the parts that need no GPU.  The rows of this feature
live here, not in tests/abi_table.py and tests/test_kernel_inventory.py; the checks are tests/test_abi.py's check_* functions wherever
those take their row as arguments, and the two that read tests/abi_table.py (arity, NULL handle) are restated over the table below.
The policy of the new calls (csrc/library/preview_state.h) runs as a stand-alone program under ASan + UBSan, as
tests/test_preview_state.py runs the rest of it."""
import os
import re
import shutil
import subprocess

import pytest

from tests import test_abi as abi
from tests.conftest import ROOT

# symbol -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {
    "rtiow_upscale": (9, (None, 2, 0, 0.3, 0.1, 0.5, 1, None, None)),
    "rtiow_read_upscaled": (3, (None, None, 0)),
    "rtiow_upscaled_device_ptr": (3, (None, None, None)),
}
METHODS = {
    "upscale": ("factor", "source", "sigma_normal", "sigma_albedo", "sigma_depth", "use_coverage", "sync"),
    "read_upscaled": (),
    "upscaled_device_ptr": (),
}
DEFAULTS = [
    ("upscale", "factor", "UPSCALE_FACTOR"), ("upscale", "source", "UPSCALE_DENOISED"), ("upscale", "sigma_normal", "UPSCALE_SIGMA_NORMAL"),
    ("upscale", "sigma_albedo", "UPSCALE_SIGMA_ALBEDO"), ("upscale", "sigma_depth", "UPSCALE_SIGMA_DEPTH"),
    ("upscale", "use_coverage", "UPSCALE_COVERAGE"), ("upscale", "sync", True),
]
INF = float("inf")
# api constant -> (lowest value the C entry check accepts, whether that bound itself is refused, highest value)
RANGES = {"UPSCALE_FACTOR": (2, False, 4), "UPSCALE_SIGMA_NORMAL": (0, True, INF), "UPSCALE_SIGMA_ALBEDO": (0, True, INF),
          "UPSCALE_SIGMA_DEPTH": (0, True, INF), "UPSCALE_COVERAGE": (0, False, 1)}
# header define -> (value, the constant of api.py and of the package)
SOURCES = {"RTIOW_UPSCALE_DENOISED": (0, "UPSCALE_DENOISED"), "RTIOW_UPSCALE_LINEAR": (1, "UPSCALE_LINEAR"), "RTIOW_UPSCALE_HISTORY": (2, "UPSCALE_HISTORY")}
# counting substring of the demangled name -> instantiations: fp32 / fp64 x LDS / scalar scene source.  The kernel has a translation unit
# of its own, csrc/rtiow_upscale.hip: the code object of rtiow_hip.hip keeps exactly the kernels it had.
KERNELS = {"upscale_kernel<": 4}
UNIT = "rtiow_upscale.hip"


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_symbol_is_declared_listed_and_exported(native, symbol):
    abi.check_symbol(symbol)
    abi.check_abi_version()                                  # functions were added, nothing moved: still 6


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_declaration_has_the_headers_arity(native, symbol):
    from raytracingincuda_amd import api
    argtypes = getattr(api.load_hip_library(), symbol).argtypes
    assert argtypes is not None and len(argtypes) == SYMBOLS[symbol][0] == len(SYMBOLS[symbol][1]), symbol
    header = abi._sources()[0]
    declared = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % symbol, header).group(1)
    assert len(declared.split(",")) == SYMBOLS[symbol][0], (symbol, declared)


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_null_handle_needs_no_gpu(native, symbol):
    from raytracingincuda_amd import api
    assert getattr(api.load_hip_library(), symbol)(*SYMBOLS[symbol][1]) == -1, symbol


@pytest.mark.parametrize("member", METHODS)
def test_renderer_has_the_member(native, member):
    from raytracingincuda_amd import api
    assert callable(getattr(api.Renderer, member, None)), member
    assert list(abi._parameters(member)) == ["self"] + list(METHODS[member]), member
    assert getattr(api.RendererGroup, member, None) is None, member      # not available on groups


@pytest.mark.parametrize("method,parameter,value", DEFAULTS, ids=["%s-%s" % d[:2] for d in DEFAULTS])
def test_wrapper_default(native, method, parameter, value):
    abi.check_default(method, parameter, value)


def test_default_constants_and_sources(native):
    import raytracingincuda_amd as package
    from raytracingincuda_amd import api
    for constant, (lowest, lowest_refused, highest) in RANGES.items():
        v = getattr(api, constant)
        assert (lowest < v if lowest_refused else lowest <= v) and v <= highest, (constant, v)
    assert isinstance(api.UPSCALE_FACTOR, int) and api.UPSCALE_COVERAGE in (0, 1)
    header = abi._sources()[0]
    for name, (value, constant) in SOURCES.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
        assert getattr(api, constant) == getattr(package, constant) == value, constant
    assert not [s for s in api.HIP_SYMBOLS if "group" in s and "upscal" in s]


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_count_and_resources(native, name):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata(source=UNIT)
    # beside the plain (non-template) kernels every unit that includes the device headers emits, the unit instantiates no other kernel
    assert sorted(k for k in meta if "<" in k and name not in k) == [], "the unit instantiates no other kernel template"
    assert not [k for k in device_metadata()[0] if name in k], "rtiow_hip.hip's code object keeps the kernels it had"
    ks = {k: v for k, v in meta.items() if name in k}
    assert len(ks) == KERNELS[name], (name, sorted(ks))
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        assert v["vgpr"] <= (64 if "<float" in k else 80), (k, v)        # eight / six waves per SIMD (granule 8, min(8, 512 // alloc))
        assert "render_" not in k and "variance_" not in k, k      # the families other tests count by
    for prec in ("float", "double"):
        for src in (0, 1):
            assert [k for k in ks if "upscale_kernel<%s, %d>" % (prec, src) in k], (prec, src)
    # no row of the frozen inventory counts these kernels too
    from tests.test_kernel_inventory import KERNELS as frozen
    assert not [row for row in frozen for k in ks if row in k]


def test_upscale_state_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "upscale_state_main")
    inc = os.path.join(ROOT, "raytracingincuda_amd", "csrc", "library")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + inc, "-o", exe, os.path.join(ROOT, "tests", "native", "upscale_state_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    assert r.stdout.splitlines()[-1] == "0 upscale rule failure(s)"
