"""The preview chain on volume scenes (rtiow_accumulate_volume, rtiow_accumulate_adaptive_volume, rtiow_accumulate_budget_volume,
rtiow_render_guides_volume, rtiow_render_coverage_volume): the parts that need no GPU, in the manner of tests/test_large_preview_abi.py.
The rows of this feature live here, not in tests/abi_table.py and tests/test_kernel_inventory.py; the checks are tests/test_abi.py's
check_* functions wherever those take their row as arguments, and the two that read tests/abi_table.py (arity, NULL handle) are restated
over the table below."""
import json
import os
import re

import pytest

from tests import test_abi as abi
from tests.conftest import ROOT

# symbol -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {
    "rtiow_accumulate_volume": (3, (None, 1, None)),
    "rtiow_accumulate_adaptive_volume": (7, (None, 1, 0, 0.0, 1, None, None)),
    "rtiow_accumulate_budget_volume": (7, (None, 1, 0, 1.0, 1, None, None)),
    "rtiow_render_guides_volume": (2, (None, None)),
    "rtiow_render_coverage_volume": (3, (None, 2, None)),
}
# method -> its twin: the twin's parameter names and defaults, minus `threads`; symbol -> the twin's symbol (the _large twin has the
# parameter list of a call without threads_per_block_row, which these have as well)
TWINS = {
    "accumulate_volume": "accumulate",
    "accumulate_adaptive_volume": "accumulate_adaptive",
    "accumulate_budget_volume": "accumulate_budget",
    "render_guides_volume": "render_guides",
    "render_coverage_volume": "render_coverage",
}
LARGE_TWIN_SYMBOLS = {s: s[:-len("volume")] + "large" for s in SYMBOLS}
UNIT = "rtiow_volume_preview.hip"
UPSCALE_UNIT = "rtiow_volume_upscale.hip"
OTHER_UNITS = ("rtiow_hip.hip", "rtiow_group.hip", "rtiow_upscale.hip", "rtiow_upscale_wide.hip", "rtiow_large.hip", "rtiow_large_preview.hip",
               "rtiow_large_upscale.hip", "rtiow_volume.hip", UPSCALE_UNIT)
# counting substring of the demangled name -> instantiations.  The persistent kernels: fp32 plain and with the bounded rejection loop,
# fp64.  The tile kernels: the existing templates over RTIOW_SCENE_VOLUME_GRID (5), both precisions.
PERSISTENT = {"volume_accumulate_kernel<": 3, "volume_adaptive_kernel<": 3}
TILE = {"guide_kernel<": 2, "guide_chain_kernel<": 2, "guide_lens_kernel<": 2, "surface_motion_kernel<": 2, "coverage_kernel<": 2}
VOLUME_GRID = 5
# 512 VGPRs a SIMD lane, granule 8: the most VGPRs of a kernel at 8, 7, 6, 5, 4, 3, 2 waves per SIMD and at one
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
    assert tuple(argtypes) == tuple(getattr(lib, LARGE_TWIN_SYMBOLS[symbol]).argtypes), symbol   # the twin's list, without the threads
    header = abi._sources()[0]
    declared = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % symbol, header).group(1)
    large = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % LARGE_TWIN_SYMBOLS[symbol], header).group(1)
    assert len(declared.split(",")) == SYMBOLS[symbol][0], (symbol, declared)
    assert declared.split() == large.split(), (symbol, declared)                                 # "the same parameters"


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
    assert not [s for s in api.HIP_SYMBOLS if "group" in s and "volume" in s]


def _kernel_name(key):
    """"guide_kernel<" must not count "guide_chain_kernel<": the counting substring starts the kernel's name."""
    return re.compile(r"(?<![A-Za-z0-9_])" + re.escape(key))


def short_name(demangled):
    """The name scripts/kernel_resources.py records a kernel under: without `void`, the namespace and the parameters."""
    return re.sub(r"^void |\(anonymous namespace\)::|\(.*$", "", demangled)


def _ours(meta):
    return {k: v for k, v in meta.items() if any(_kernel_name(n).search(k) for n in {**PERSISTENT, **TILE})}


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
        for inst in ("<float, %d>" % VOLUME_GRID, "<double, %d>" % VOLUME_GRID):
            assert [k for k in templates if _kernel_name(name[:-1] + inst).search(k)], (name, inst)
    # beside the plain (non-template) kernels every unit that includes the device headers emits, the unit instantiates no other kernel template
    assert sorted(set(templates) - set(counted)) == [], "the unit instantiates no other kernel template"
    # no kernel over the volume grid in any other unit but volume_scene_kernel (rtiow_volume.hip) and the upscalers (rtiow_volume_upscale.hip),
    # and none of this unit's persistent kernels
    for other in OTHER_UNITS:
        names = list(device_metadata(source=other)[0])
        over = [k for k in names if re.search(r"<(float|double), %d[,>]" % VOLUME_GRID, k)]
        if other == UPSCALE_UNIT:
            over = [k for k in over if not re.search(r"(?<![A-Za-z0-9_])upscale(_wide)?_kernel<", k)]
        assert not over, (other, over)
        assert not [k for k in names if "volume_accumulate_kernel" in k or "volume_adaptive_kernel" in k], other
        assert not [k for k in names if "volume_" in k and "volume_scene_kernel" not in k], other


def test_kernel_resources(native):
    """No scratch and no spill anywhere; the persistent kernels at five (fp32) / four (fp64) waves per SIMD, as the persistent kernels of
    rtiow_render; every kernel at the waves-per-SIMD step profiles/volume_preview/kernel_resources.json records for it, and with the
    record's counts."""
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata(source=UNIT)
    ours = _ours(meta)
    assert len(ours) == 16, sorted(ours)
    record = json.load(open(os.path.join(ROOT, "profiles", "volume_preview", "kernel_resources.json")))["kernels"]
    for k, v in ours.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)         # a condition, not a measurement
        if any(n in k for n in PERSISTENT):
            assert v["vgpr"] <= (96 if "<float" in k else 128), (k, v)
        row = record[short_name(k)]
        assert (row["vgprs"], row["vgpr_spills"], row["scratch_bytes"]) == (v["vgpr"], 0, 0), (k, v, row)
        step = min(s for s in STEPS if row["vgprs"] <= s)
        assert v["vgpr"] <= step, (k, v, step)                            # the step the build reaches, not the _large kernels'


def test_the_units_are_built_and_linked(native):
    from raytracingincuda_amd import build
    assert build.HIP_UNITS_VOLUME_PREVIEW == (UNIT, UPSCALE_UNIT)
    every = build.all_hip_units()
    assert every == build.hip_units() + [os.path.join(build.CSRC, u) for u in (UNIT, UPSCALE_UNIT)]      # the ninth and tenth, linked last
    assert len(every) == len(set(every)) == 10 and all(os.path.exists(p) for p in every)
    other = build.all_hip_units("/elsewhere/csrc")
    assert [p.rsplit("/", 1)[-1] for p in other] == [p.rsplit("/", 1)[-1] for p in every] and all(p.startswith("/elsewhere/csrc/") for p in other)
    # the build id hashes all ten: it is the id of the library that is loaded
    from raytracingincuda_amd import api
    assert api.build_id() == build.hip_build_id()
