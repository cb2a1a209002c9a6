"""Wide-support guided upscaling (rtiow_upscale_wide): the parts that need no GPU, in the manner of tests/test_upscale_abi.py.  The rows of
this feature live here, not in tests/abi_table.py and tests/test_kernel_inventory.py; the checks are tests/test_abi.py's check_* functions
wherever those take their row as arguments, and the two that read tests/abi_table.py (arity, NULL handle) are restated over the table
below.  The call adds no state to csrc/library/preview_state.h: tests/test_upscale_abi.py runs that policy as it stands."""
import re

import pytest

from tests import test_abi as abi

# symbol -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {"rtiow_upscale_wide": (9, (None, 2, 0, 0.3, 0.1, 0.5, 1, None, None))}
METHODS = {"upscale_wide": ("factor", "source", "sigma_normal", "sigma_albedo", "sigma_depth", "use_coverage", "sync")}
DEFAULTS = [
    ("upscale_wide", "factor", "UPSCALE_FACTOR"), ("upscale_wide", "source", "UPSCALE_DENOISED"), ("upscale_wide", "sigma_normal", "UPSCALE_WIDE_SIGMA_NORMAL"),
    ("upscale_wide", "sigma_albedo", "UPSCALE_WIDE_SIGMA_ALBEDO"), ("upscale_wide", "sigma_depth", "UPSCALE_WIDE_SIGMA_DEPTH"),
    ("upscale_wide", "use_coverage", "UPSCALE_WIDE_COVERAGE"), ("upscale_wide", "sync", True),
]
INF = float("inf")
# api constant -> (lowest value the C entry check accepts, whether that bound itself is refused, highest value)
RANGES = {"UPSCALE_WIDE_SIGMA_NORMAL": (0, True, INF), "UPSCALE_WIDE_SIGMA_ALBEDO": (0, True, INF), "UPSCALE_WIDE_SIGMA_DEPTH": (0, True, INF),
          "UPSCALE_WIDE_COVERAGE": (0, False, 1)}
# header define -> value: the sources are rtiow_upscale's, untouched
SOURCES = {"RTIOW_UPSCALE_DENOISED": 0, "RTIOW_UPSCALE_LINEAR": 1, "RTIOW_UPSCALE_HISTORY": 2}
# counting substring of the demangled name -> instantiations: fp32 / fp64 x LDS / scalar scene source.  The kernel has a translation unit
# of its own, csrc/rtiow_upscale_wide.hip: the code objects of rtiow_hip.hip and rtiow_upscale.hip keep exactly the kernels they had.
KERNELS = {"upscale_wide_kernel<": 4}
UNIT = "rtiow_upscale_wide.hip"
OTHER_UNITS = ("rtiow_hip.hip", "rtiow_upscale.hip")


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_symbol_is_declared_listed_and_exported(native, symbol):
    abi.check_symbol(symbol)
    abi.check_abi_version()                                  # a function was added, nothing moved: still 6


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_declaration_has_the_headers_arity(native, symbol):
    from raytracingincuda_amd import api
    argtypes = getattr(api.load_hip_library(), symbol).argtypes
    assert argtypes is not None and len(argtypes) == SYMBOLS[symbol][0] == len(SYMBOLS[symbol][1]), symbol
    assert tuple(argtypes) == tuple(api.load_hip_library().rtiow_upscale.argtypes), symbol       # rtiow_upscale's list
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
    assert list(abi._parameters(member)) == list(abi._parameters("upscale")), member       # upscale()'s order, which stays
    assert getattr(api.RendererGroup, member, None) is None, member      # not available on groups


@pytest.mark.parametrize("method,parameter,value", DEFAULTS, ids=["%s-%s" % d[:2] for d in DEFAULTS])
def test_wrapper_default(native, method, parameter, value):
    abi.check_default(method, parameter, value)


def test_default_constants_and_sources(native):
    from raytracingincuda_amd import api
    for constant, (lowest, lowest_refused, highest) in RANGES.items():
        v = getattr(api, constant)
        assert (lowest < v if lowest_refused else lowest <= v) and v <= highest, (constant, v)
    assert api.UPSCALE_WIDE_COVERAGE in (0, 1)
    header = abi._sources()[0]
    for name, value in SOURCES.items():
        assert len(re.findall(r"#define\s+%s\s+%d\b" % (name, value), header)) == 1, name
    assert not re.search(r"#define\s+RTIOW_UPSCALE_WIDE", header)          # the call brings no define of its own
    assert not [s for s in api.HIP_SYMBOLS if "group" in s and "upscal" in s]


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_count_and_resources(native, name):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata(source=UNIT)
    # beside the plain (non-template) kernels every unit that includes the device headers emits, the unit instantiates no other kernel
    assert sorted(k for k in meta if "<" in k and name not in k) == [], "the unit instantiates no other kernel template"
    for other in OTHER_UNITS:
        assert not [k for k in device_metadata(source=other)[0] if "upscale_wide_kernel" in k], other
    ks = {k: v for k, v in meta.items() if name in k}
    assert len(ks) == KERNELS[name], (name, sorted(ks))
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        assert v["vgpr"] <= (64 if "<float" in k else 80), (k, v)        # eight / six waves per SIMD (granule 8, min(8, 512 // alloc))
        assert "render_" not in k and "variance_" not in k and "upscale_kernel<" not in k, k      # the families other tests count by
    for prec in ("float", "double"):
        for src in (0, 1):
            assert [k for k in ks if "upscale_wide_kernel<%s, %d>" % (prec, src) in k], (prec, src)
    # no row of the frozen inventory, nor tests/test_upscale_abi.py's, counts these kernels too
    from tests.test_kernel_inventory import KERNELS as frozen
    from tests.test_upscale_abi import KERNELS as narrow
    assert not [row for row in list(frozen) + list(narrow) for k in ks if row in k]
