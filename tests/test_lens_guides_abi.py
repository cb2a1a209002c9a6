"""Lens-sampled filter guides (rtiow_set_guide_lens, guide_lens_kernel): the parts that need no GPU.  The rows of this feature live here,
not in tests/abi_table.py and tests/test_kernel_inventory.py; the checks are tests/test_abi.py's check_* functions wherever those take
their row as arguments, and the two that read tests/abi_table.py (arity, NULL handle) are restated over the table below.  The knob adds
no rule to csrc/library/preview_state.h -- a change is an on_guide_mode_changed -- so the policy's own stand-alone programs cover it."""
import re

import pytest

from tests import test_abi as abi

# symbol -> (number of parameters, the arguments of a call with a NULL handle: it answers -1 before any device work)
SYMBOLS = {"rtiow_set_guide_lens": (2, (None, 2))}
METHODS = {"set_guide_lens": ("samples_per_side",)}
DEFAULTS = [("set_guide_lens", "samples_per_side", "GUIDE_LENS_GRID")]
# counting substring of the demangled name -> instantiations: fp32 / fp64 x LDS / scalar scene source
KERNELS = {"guide_lens_kernel<": 4}


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_symbol_is_declared_listed_and_exported(native, symbol):
    abi.check_symbol(symbol)
    abi.check_abi_version()                                  # a function was added, nothing moved: still 6


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_declaration_has_the_headers_arity(native, symbol):
    from raytracingincuda_amd import api
    argtypes = getattr(api.load_hip_library(), symbol).argtypes
    assert argtypes is not None and len(argtypes) == SYMBOLS[symbol][0] == len(SYMBOLS[symbol][1]), symbol
    declared = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % symbol, abi._sources()[0]).group(1)
    assert len(declared.split(",")) == SYMBOLS[symbol][0], (symbol, declared)


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_null_handle_needs_no_gpu(native, symbol):
    from raytracingincuda_amd import api
    for value in (0, 2, 4, 3):
        assert getattr(api.load_hip_library(), symbol)(None, value) == -1, (symbol, value)
    assert getattr(api.load_hip_library(), symbol)(*SYMBOLS[symbol][1]) == -1, symbol


@pytest.mark.parametrize("member", METHODS)
def test_renderer_has_the_member(native, member):
    from raytracingincuda_amd import api
    assert callable(getattr(api.Renderer, member, None)), member
    assert list(abi._parameters(member)) == ["self"] + list(METHODS[member]), member


@pytest.mark.parametrize("method,parameter,value", DEFAULTS, ids=["%s-%s" % d[:2] for d in DEFAULTS])
def test_wrapper_default(native, method, parameter, value):
    abi.check_default(method, parameter, value)


def test_default_constant(native):
    from raytracingincuda_amd import api
    assert api.GUIDE_LENS_GRID in (2, 4)


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_count_and_resources(native, name):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    meta, _ = device_metadata()
    ks = {k: v for k, v in meta.items() if name in k}
    assert len(ks) == KERNELS[name], (name, sorted(ks))
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        assert "render_" not in k and "variance_" not in k, k      # the families other tests count by
    for prec in ("float", "double"):
        for src in (0, 1):
            assert [k for k in ks if "guide_lens_kernel<%s, %d>" % (prec, src) in k], (prec, src)
    # no row of the frozen inventory counts these kernels too, and the inventory's own rows still hold with them in the library
    from tests import test_kernel_inventory as inventory
    assert not [row for row in inventory.KERNELS for k in ks if row in k]
    for family in inventory.FAMILIES:
        assert not [k for k in ks if family in k], family
    inventory.check_disjoint()
    inventory.check_row("guide_kernel<")
    inventory.check_row("guide_chain_kernel<")
