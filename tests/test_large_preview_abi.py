"""The preview chain on large scenes (rtiow_accumulate_large, rtiow_accumulate_adaptive_large, rtiow_accumulate_budget_large,
rtiow_render_guides_large, rtiow_render_coverage_large): the parts that need no GPU, in the manner of tests/test_render_large_abi.py.
The rows of this feature live here, not in tests/abi_table.py and tests/test_kernel_inventory.py; the checks are tests/test_abi.py's
check_* functions wherever those take their row as arguments, and the two that read tests/abi_table.py (arity, NULL handle) are restated
over the table below."""
import re

import pytest

from tests import test_abi as abi

# symbol -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {
    "rtiow_accumulate_large": (3, (None, 1, None)),
    "rtiow_accumulate_adaptive_large": (7, (None, 1, 0, 0.0, 1, None, None)),
    "rtiow_accumulate_budget_large": (7, (None, 1, 0, 1.0, 1, None, None)),
    "rtiow_render_guides_large": (2, (None, None)),
    "rtiow_render_coverage_large": (3, (None, 2, None)),
}
# method -> its twin: the twin's parameter names and defaults, minus `threads`
TWINS = {
    "accumulate_large": "accumulate",
    "accumulate_adaptive_large": "accumulate_adaptive",
    "accumulate_budget_large": "accumulate_budget",
    "render_guides_large": "render_guides",
    "render_coverage_large": "render_coverage",
}
UNIT = "rtiow_large_preview.hip"
OTHER_UNITS = ("rtiow_hip.hip", "rtiow_upscale.hip", "rtiow_upscale_wide.hip", "rtiow_large.hip")
# counting substring of the demangled name -> instantiations.  The persistent kernels: fp32 plain and with the bounded rejection loop,
# fp64.  The tile kernels: the existing templates over RTIOW_SCENE_DEVICE_GRID (4), both precisions.
PERSISTENT = {"large_accumulate_kernel<": 3, "large_adaptive_kernel<": 3}
TILE = {"guide_kernel<": 2, "guide_chain_kernel<": 2, "guide_lens_kernel<": 2, "surface_motion_kernel<": 2, "coverage_kernel<": 2}
DEVICE_GRID = 4


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


@pytest.mark.parametrize("method", TWINS)
def test_renderer_method_follows_its_twin(native, method):
    from raytracingincuda_amd import api
    assert callable(getattr(api.Renderer, method, None)), method
    got = abi._parameters(method)
    want = [name for name in abi._parameters(TWINS[method]) if name != "threads"]
    assert list(got) == want, (method, list(got))
    abi.check_same_as(method, TWINS[method], want[1:])       # every parameter's default is the twin's (none where the twin has none)
    assert got["sync"].default is True
    assert getattr(api.RendererGroup, method, None) is None, method      # not available on groups
    assert not [s for s in api.HIP_SYMBOLS if "group" in s and "large" in s]


def _kernel_name(key):
    """"guide_kernel<" must not count "guide_chain_kernel<": the counting substring starts the kernel's name."""
    return re.compile(r"(?<![A-Za-z0-9_])" + re.escape(key))


def test_kernel_inventory(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata(source=UNIT)
    templates = sorted(k for k in meta if "<" in k)
    counted = []
    for name, count in {**PERSISTENT, **TILE}.items():
        ks = [k for k in templates if _kernel_name(name).search(k)]
        assert len(ks) == count, (name, ks)
        counted += ks
    for name in PERSISTENT:
        for inst in ("<float, false>", "<float, true>", "<double, false>"):
            assert [k for k in templates if name[:-1] + inst in k], (name, inst)
    for name in TILE:
        for inst in ("<float, %d>" % DEVICE_GRID, "<double, %d>" % DEVICE_GRID):
            assert [k for k in templates if _kernel_name(name[:-1] + inst).search(k)], (name, inst)
    # beside the plain (non-template) kernels every unit that includes the device headers emits, the unit instantiates no other kernel template
    assert sorted(set(templates) - set(counted)) == [], "the unit instantiates no other kernel template"
    # no kernel over the device grid in any other unit, and none of this unit's persistent kernels
    for other in OTHER_UNITS:
        names = list(device_metadata(source=other)[0])
        assert not [k for k in names if re.search(r"<(float|double), %d[,>]" % DEVICE_GRID, k)], other
        assert not [k for k in names if "large_accumulate_kernel" in k or "large_adaptive_kernel" in k], other


def test_kernel_resources(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata(source=UNIT)
    ours = {k: v for k, v in meta.items() if any(_kernel_name(n).search(k) for n in {**PERSISTENT, **TILE})}
    assert len(ours) == 16, sorted(ours)
    for k, v in ours.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
    for k, v in ours.items():
        if any(n in k for n in PERSISTENT):
            assert v["vgpr"] <= (96 if "<float" in k else 128), (k, v)    # five / four waves per SIMD, as the persistent kernels of rtiow_render
