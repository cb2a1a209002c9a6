"""The progressive-preview calls of the C-ABI and their Python wrappers, the parts that need no GPU, one case per symbol or method
(tests/abi_table.py is the data): each symbol is declared in include/rtiow.h, let out by the version script, listed in api.HIP_SYMBOLS
and exported from both libraries; its declaration in api.py has the header's number of parameters; a NULL handle is refused before any
device work; the wrappers have the parameters and defaults the documents state; the ABI version is 6.  The whole symbol set against the
headers: tests/test_host.py.  The kernels behind the calls: tests/test_kernel_inventory.py.

Each check is a check_* function of one row, so that tests/kept_abi_ids.py can run the same statement for the earlier per-feature tests."""
import functools
import inspect
import os
import re
import subprocess

import pytest

from tests import abi_table as T
from tests.conftest import ROOT


@functools.lru_cache(maxsize=None)
def _sources():
    """The header without its comments, the version script's global patterns and `nm -D --defined-only` of both HIP libraries."""
    from raytracingincuda_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow.h")).read(), flags=re.S)
    version_script = open(os.path.join(ROOT, "raytracingincuda_amd", "csrc", "librtiow_hip.map")).read()
    globs = re.search(r"global:\s*([^;]*);", version_script).group(1).split()
    paths = api.lib_paths()
    nm = {which: subprocess.run(["nm", "-D", "--defined-only", paths[which]], capture_output=True, text=True, check=True).stdout
          for which in ("hip", "hip_debug")}
    return header, globs, nm


def _parameters(method):
    from raytracingincuda_amd import api
    return inspect.signature(getattr(api.Renderer, method)).parameters


def check_symbol(symbol):
    from raytracingincuda_amd import api
    header, globs, nm = _sources()
    assert re.search(r"\bint\s+%s\s*\(" % symbol, header), symbol
    assert any(re.fullmatch(g.replace("*", ".*"), symbol) for g in globs), symbol
    assert symbol in api.HIP_SYMBOLS, symbol
    assert "group" not in symbol, symbol                     # the preview calls are per handle
    for which, syms in nm.items():
        assert re.search(r"\bT %s\b" % symbol, syms), (which, symbol)


def check_arity(symbol):
    from raytracingincuda_amd import api
    argtypes = getattr(api.load_hip_library(), symbol).argtypes
    assert argtypes is not None and len(argtypes) == T.SYMBOLS[symbol][0], symbol
    assert len(T.SYMBOLS[symbol][1]) == T.SYMBOLS[symbol][0], symbol


def check_null_handle(symbol):
    from raytracingincuda_amd import api
    assert getattr(api.load_hip_library(), symbol)(*T.SYMBOLS[symbol][1]) == -1, symbol


def check_abi_version():
    import raytracingincuda_amd as native
    from raytracingincuda_amd import api
    header = _sources()[0]
    for name, (value, constant) in T.HEADER_DEFINES.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
        assert getattr(api, constant) == getattr(native, constant) == value, constant
    assert api.load_hip_library().rtiow_abi_version() == native.ABI_VERSION == api.ABI_VERSION == 6       # functions were added, nothing moved


def check_member(member):
    from raytracingincuda_amd import api
    got = getattr(api.Renderer, member, None)
    if member in T.PROPERTIES:
        assert isinstance(got, property), member
    else:
        assert callable(got), member
        if T.METHODS[member] is not None:
            assert list(_parameters(member)) == ["self"] + list(T.METHODS[member]), member


def check_default(method, parameter, value):
    from raytracingincuda_amd import api
    default = _parameters(method)[parameter].default
    if isinstance(value, str):
        assert default == getattr(api, value), (method, parameter, value)
    else:
        assert default is value, (method, parameter)


def check_range(constant):
    from raytracingincuda_amd import api
    v, (lowest, lowest_refused, highest) = getattr(api, constant), T.RANGES[constant]
    assert (lowest < v if lowest_refused else lowest <= v) and v <= highest, (constant, v, T.RANGES[constant])


def check_same_as(method, other, names):
    p, q = _parameters(method), _parameters(other)
    if names is None:
        assert list(p) == list(q), (method, other)
        names = list(q)[1:]
    for name in names:
        assert p[name].default == q[name].default, (method, other, name)


@pytest.mark.parametrize("symbol", T.SYMBOLS)
def test_symbol_is_declared_listed_and_exported(native, symbol):
    check_symbol(symbol)


@pytest.mark.parametrize("symbol", T.SYMBOLS)
def test_declaration_has_the_headers_arity(native, symbol):
    check_arity(symbol)


@pytest.mark.parametrize("symbol", T.SYMBOLS)
def test_null_handle_needs_no_gpu(native, symbol):
    """Argument and state checks come before any device work: a handle that never touched a GPU answers them too."""
    check_null_handle(symbol)


def test_abi_version_and_header_constants(native):
    check_abi_version()


@pytest.mark.parametrize("member", list(T.METHODS) + list(T.PROPERTIES))
def test_renderer_has_the_member(native, member):
    check_member(member)


@pytest.mark.parametrize("method,parameter,value", T.DEFAULTS, ids=["%s-%s" % d[:2] for d in T.DEFAULTS])
def test_wrapper_default(native, method, parameter, value):
    check_default(method, parameter, value)


@pytest.mark.parametrize("constant", T.RANGES)
def test_default_constant_is_in_the_range_the_call_accepts(native, constant):
    check_range(constant)


@pytest.mark.parametrize("method,other,names", T.SAME_AS, ids=["%s-%s" % s[:2] for s in T.SAME_AS])
def test_wrapper_follows_the_call_it_extends(native, method, other, names):
    check_same_as(method, other, names)
