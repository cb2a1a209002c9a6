"""Volume scenes (rtiow_render_volume, rtiow_read_volume_grid and the two hooks of the test build): the parts that need no GPU, in the
manner of tests/test_render_large_abi.py.  The rows of this feature live here, not in tests/abi_table.py and
tests/test_kernel_inventory.py; the checks are tests/test_abi.py's check_* functions wherever those take their row as arguments, and the
two that read tests/abi_table.py (arity, NULL handle) are restated over the table below."""
import re

import pytest

from tests import test_abi as abi

# symbol -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {
    "rtiow_render_volume": (2, (None, None)),
    "rtiow_read_volume_grid": (2, (None, None)),
}
DEBUG_SYMBOLS = {
    "rtiow_debug_volume_grid_plan": 13,
    "rtiow_debug_hit_world_volume": 6,
}
METHODS = {
    "render_volume": ("sync",),
    "volume_grid": (),
    "debug_hit_world_volume": ("rays",),
}
DEFAULTS = [("render_volume", "sync", True)]
# counting substring of the demangled name -> instantiations.  The kernels have a translation unit of their own, csrc/rtiow_volume.hip: the
# other code objects keep exactly the kernels they had.  volume_scene_kernel: fp32 plain and with the bounded rejection loop, fp64.
KERNELS = {"volume_scene_kernel<": 3}
DEBUG_KERNELS = {"volume_hit_probe_kernel<": 2}
UNIT = "rtiow_volume.hip"
OTHER_UNITS = ("rtiow_hip.hip", "rtiow_upscale.hip", "rtiow_upscale_wide.hip", "rtiow_large.hip", "rtiow_large_preview.hip", "rtiow_large_upscale.hip")


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


@pytest.mark.parametrize("symbol", DEBUG_SYMBOLS)
def test_hooks_ship_in_the_test_build_only(native, symbol):
    from raytracingincuda_amd import api
    _, _, nm = abi._sources()
    assert symbol in api.DEBUG_SYMBOLS and symbol not in api.HIP_SYMBOLS
    assert re.search(r"\bT %s\b" % symbol, nm["hip_debug"]) and not re.search(r"\b%s\b" % symbol, nm["hip"]), symbol
    assert len(getattr(api.load_hip_library(debug=True), symbol).argtypes) == DEBUG_SYMBOLS[symbol], symbol


@pytest.mark.parametrize("member", METHODS)
def test_renderer_has_the_member(native, member):
    from raytracingincuda_amd import api
    assert callable(getattr(api.Renderer, member, None)), member
    assert list(abi._parameters(member)) == ["self"] + list(METHODS[member]), member
    assert getattr(api.RendererGroup, member, None) is None, member      # not available on groups


@pytest.mark.parametrize("method,parameter,value", DEFAULTS, ids=["%s-%s" % d[:2] for d in DEFAULTS])
def test_wrapper_default(native, method, parameter, value):
    abi.check_default(method, parameter, value)


def test_scene_source_define_and_info_struct(native):
    import ctypes
    from raytracingincuda_amd import api
    header = abi._sources()[0]
    assert len(re.findall(r"#define\s+RTIOW_SCENE_VOLUME_GRID\s+5\b", header)) == 1
    assert api.SCENE_VOLUME_GRID == native.SCENE_VOLUME_GRID == 5
    assert api.SCENE_VOLUME_GRID not in (api.SCENE_LDS, api.SCENE_SCALAR, api.SCENE_LDS_EXACT, api.SCENE_GRID, api.SCENE_DEVICE_GRID)
    # rtiow_volume_grid_info, field for field: int32 x4, double x2, int32 x2, uint64 x2, int32 x2, uint64 = 72 bytes
    body = re.search(r"typedef struct \{([^}]*)\} rtiow_volume_grid_info;", header).group(1)
    names = re.findall(r"\b(\w+)\s*[;,]", body)
    assert names == [f for f, _ in api.VolumeGridInfo._fields_], names
    assert ctypes.sizeof(api.VolumeGridInfo) == 72
    assert not [s for s in api.HIP_SYMBOLS if "group" in s and "volume" in s]
    assert callable(api.debug_volume_grid_plan) and native.debug_volume_grid_plan is api.debug_volume_grid_plan


def test_the_unit_is_built_and_linked(native):
    from raytracingincuda_amd import build
    assert build.HIP_UNITS_VOLUME == (UNIT,)
    assert [p.rsplit("/", 1)[-1] for p in build.hip_units()] == list(build.HIP_UNITS) + [UNIT]     # the eighth unit, linked last


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_count_and_resources(native, name):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata(source=UNIT)
    # beside the plain (non-template) kernels every unit that includes the device headers emits, the unit instantiates no other kernel template
    assert sorted(k for k in meta if "<" in k and name not in k) == [], "the unit instantiates no other kernel template"
    for other in OTHER_UNITS:
        assert not [k for k in device_metadata(source=other)[0] if "volume_" in k], other
    ks = {k: v for k, v in meta.items() if name in k}
    assert len(ks) == KERNELS[name], (name, sorted(ks))
    for inst in ("<float, false>", "<float, true>", "<double, false>"):
        assert [k for k in ks if "volume_scene_kernel" + inst in k], inst
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        assert v["vgpr"] <= (96 if "<float" in k else 128), (k, v)        # five / four waves per SIMD, as large_scene_kernel
        assert "render_" not in k and "variance_" not in k and "upscale" not in k and "large_" not in k, k      # the families other tests count by
    from tests.test_kernel_inventory import KERNELS as frozen
    assert not [row for row in frozen for k in ks if row in k]


@pytest.mark.parametrize("name", DEBUG_KERNELS)
def test_debug_kernels_are_in_the_test_build_of_the_unit_only(native, name):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    assert not [k for k in device_metadata(source=UNIT)[0] if name in k]
    ks = {k: v for k, v in device_metadata(defines=("-DRTIOW_DEBUG_API",), source=UNIT)[0].items() if name in k}
    assert len(ks) == DEBUG_KERNELS[name], sorted(ks)
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
