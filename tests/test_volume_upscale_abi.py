"""Guided upscaling on volume scenes (rtiow_upscale_volume, rtiow_upscale_wide_volume): the parts that need no GPU, in the manner of
tests/test_large_upscale_abi.py.  The rows of this feature live here, not in tests/abi_table.py and tests/test_kernel_inventory.py; the
checks are tests/test_abi.py's check_* functions wherever those take their row as arguments, and the two that read tests/abi_table.py
(arity, NULL handle) are restated over the table below.  The LDS placement of the launches is place_large_lds, stated under ASan and UBSan
by tests/test_large_upscale_abi.py's native program."""
import json
import os
import re

import pytest

from tests import test_abi as abi
from tests.conftest import ROOT
from tests.test_volume_preview_abi import STEPS, _kernel_name, short_name

# symbol -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {
    "rtiow_upscale_volume": (9, (None, 2, 0, 0.3, 0.1, 0.5, 1, None, None)),
    "rtiow_upscale_wide_volume": (9, (None, 2, 0, 0.3, 0.1, 0.5, 1, None, None)),
}
# method -> its twin: the twin's parameter names and defaults; symbol -> the twin's symbol
TWINS = {"upscale_volume": "upscale", "upscale_wide_volume": "upscale_wide"}
TWIN_SYMBOLS = {"rtiow_upscale_volume": "rtiow_upscale", "rtiow_upscale_wide_volume": "rtiow_upscale_wide"}
UNIT = "rtiow_volume_upscale.hip"
OTHER_UNITS = ("rtiow_hip.hip", "rtiow_group.hip", "rtiow_upscale.hip", "rtiow_upscale_wide.hip", "rtiow_large.hip", "rtiow_large_preview.hip",
               "rtiow_large_upscale.hip", "rtiow_volume.hip", "rtiow_volume_preview.hip")
VOLUME_GRID = 5
KERNELS = ("upscale_kernel<float, 5>", "upscale_kernel<double, 5>", "upscale_wide_kernel<float, 5>", "upscale_wide_kernel<double, 5>")


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
    assert not [s for s in api.HIP_SYMBOLS if "group" in s and "volume" in s]


def test_kernel_inventory(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata(source=UNIT)
    templates = sorted(k for k in meta if "<" in k)
    counted = []
    for name in KERNELS:
        ks = [k for k in templates if _kernel_name(name).search(k)]
        assert len(ks) == 1, (name, ks)
        counted += ks
    # beside the plain (non-template) kernels every unit that includes the device headers emits, the unit instantiates no other kernel template
    assert sorted(set(templates) - set(counted)) == [], "the unit instantiates no other kernel template"
    # no upscale kernel over the volume grid in any other unit
    for other in OTHER_UNITS:
        names = list(device_metadata(source=other)[0])
        assert not [k for k in names if re.search(r"upscale(_wide)?_kernel<(float|double), %d[,>]" % VOLUME_GRID, k)], other


def test_kernel_resources(native):
    """No scratch, no spill; each kernel has the counts profiles/volume_preview/kernel_resources.json records, and with them the
    waves-per-SIMD step the build reaches (not the _large upscalers', which the longer walk does not meet)."""
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata(source=UNIT)
    record = json.load(open(os.path.join(ROOT, "profiles", "volume_preview", "kernel_resources.json")))["kernels"]
    for name in KERNELS:
        (k, v), = [(k, v) for k, v in meta.items() if _kernel_name(name).search(k)]
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)         # a condition, not a measurement
        row = record[short_name(k)]
        assert (row["vgprs"], row["vgpr_spills"], row["scratch_bytes"]) == (v["vgpr"], 0, 0), (k, v, row)
        step = min(s for s in STEPS if row["vgprs"] <= s)
        assert v["vgpr"] <= step, (k, v, step)


def test_the_wide_kernel_skips_its_own_barrier_for_the_volume_grid_too():
    """stage_device_grid stages both grids and ends in a barrier: the condition names both sources, at compile time."""
    wide = open(os.path.join(ROOT, "raytracingincuda_amd", "csrc", "device", "upscale_wide.h")).read()
    assert "SRC == RTIOW_SCENE_LDS || SRC == RTIOW_SCENE_DEVICE_GRID || SRC == RTIOW_SCENE_VOLUME_GRID || p.shade_in_lds" in wide
