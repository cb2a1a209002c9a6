"""Edge resolve (rtiow_render_coverage, rtiow_read_coverage, rtiow_resolve_edges): the parts that need no GPU.  The rows of this feature
live here, not in tests/abi_table.py and tests/test_kernel_inventory.py; the checks are tests/test_abi.py's check_* functions wherever
those take their row as arguments, and the two that read tests/abi_table.py (arity, NULL handle) are restated over the table below.
The policy of the new calls (csrc/library/preview_state.h) runs as a stand-alone program under ASan + UBSan, as
tests/test_preview_state.py runs the rest of it."""
import os
import shutil
import subprocess

import pytest

from tests import test_abi as abi
from tests.conftest import ROOT

# symbol -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {
    "rtiow_render_coverage": (3, (None, 4, None)),
    "rtiow_read_coverage": (6, (None, None, None, None, None, 0)),
    "rtiow_resolve_edges": (7, (None, 2, 0.3, 0.5, 8.0, None, None)),
}
METHODS = {
    "render_coverage": ("subsamples_per_side", "sync"),
    "coverage": (),
    "resolve_edges": ("radius", "sigma_normal", "sigma_depth", "prior", "sync"),
}
DEFAULTS = [
    ("render_coverage", "subsamples_per_side", "COVERAGE_GRID"), ("render_coverage", "sync", True),
    ("resolve_edges", "radius", "EDGE_RADIUS"), ("resolve_edges", "sigma_normal", "EDGE_SIGMA_NORMAL"),
    ("resolve_edges", "sigma_depth", "EDGE_SIGMA_DEPTH"), ("resolve_edges", "prior", "EDGE_PRIOR"), ("resolve_edges", "sync", True),
]
INF = float("inf")
# api constant -> (lowest value the C entry check accepts, whether that bound itself is refused, highest value)
RANGES = {"EDGE_RADIUS": (1, False, 3), "EDGE_SIGMA_NORMAL": (0, True, INF), "EDGE_SIGMA_DEPTH": (0, True, INF), "EDGE_PRIOR": (0, True, INF)}
# counting substring of the demangled name -> instantiations: fp32 / fp64 x LDS / scalar scene source; fp32 / fp64
KERNELS = {"coverage_kernel<": 4, "edge_resolve_kernel<": 2}


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
    import re
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


@pytest.mark.parametrize("method,parameter,value", DEFAULTS, ids=["%s-%s" % d[:2] for d in DEFAULTS])
def test_wrapper_default(native, method, parameter, value):
    abi.check_default(method, parameter, value)


def test_default_constants(native):
    from raytracingincuda_amd import api
    assert api.COVERAGE_GRID in (2, 4)
    for constant, (lowest, lowest_refused, highest) in RANGES.items():
        v = getattr(api, constant)
        assert (lowest < v if lowest_refused else lowest <= v) and v <= highest, (constant, v)


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_count_and_resources(native, name):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata()
    ks = {k: v for k, v in meta.items() if name in k}
    assert len(ks) == KERNELS[name], (name, sorted(ks))
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        assert "render_" not in k and "variance_" not in k, k      # the families other tests count by
    if name == "coverage_kernel<":
        for prec in ("float", "double"):
            for src in (0, 1):
                assert [k for k in ks if "coverage_kernel<%s, %d>" % (prec, src) in k], (prec, src)
    # no row of the frozen inventory counts these kernels too
    from tests.test_kernel_inventory import KERNELS as frozen
    assert not [row for row in frozen for k in ks if row in k]


def test_edge_resolve_state_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "edge_resolve_state_main")
    inc = os.path.join(ROOT, "raytracingincuda_amd", "csrc", "library")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + inc, "-o", exe, os.path.join(ROOT, "tests", "native", "edge_resolve_state_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    assert r.stdout.splitlines()[-1] == "0 edge-resolve rule failure(s)"
