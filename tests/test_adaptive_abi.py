"""Adaptive progressive rendering (rtiow_accumulate_adaptive), the parts that need no GPU: the C-ABI is declared, listed and exported,
the Python wrapper has it, and the adaptive kernels meet the main launch's register budget (compiler metadata; hipcc cross-compiles
gfx950)."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

ADAPT_SYMBOLS = ["rtiow_accumulate_adaptive", "rtiow_read_adaptive_state"]


def test_adaptive_symbols_are_declared_listed_and_exported(native):
    from raytracingincuda_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow.h")).read(), flags=re.S)
    version_script = open(os.path.join(ROOT, "raytracingincuda_amd", "csrc", "librtiow_hip.map")).read()
    globs = re.search(r"global:\s*([^;]*);", version_script).group(1).split()
    paths = native.lib_paths()
    for s in ADAPT_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert any(re.fullmatch(g.replace("*", ".*"), s) for g in globs), s
        assert s in api.HIP_SYMBOLS, s
    for lib in (paths["hip"], paths["hip_debug"]):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for s in ADAPT_SYMBOLS:
            assert re.search(r"\bT %s\b" % s, syms), (lib, s)


def test_abi_version_is_unchanged(native):
    assert native.load_hip_library().rtiow_abi_version() == 6


def test_renderer_has_the_adaptive_interface(native):
    from raytracingincuda_amd import api
    assert callable(getattr(api.Renderer, "accumulate_adaptive", None))
    assert callable(getattr(api.Renderer, "adaptive_state", None))
    lib = native.load_hip_library()
    assert len(lib.rtiow_accumulate_adaptive.argtypes) == 7
    assert len(lib.rtiow_read_adaptive_state.argtypes) == 4


def test_bad_arguments_need_no_gpu(native):
    """Argument and state checks come before any device work: a handle that never touched a GPU answers them too."""
    lib = native.load_hip_library()
    assert lib.rtiow_accumulate_adaptive(None, 4, 0, 0.1, 100, None, None) == -1
    assert lib.rtiow_read_adaptive_state(None, None, None, 0) == -1


@pytest.fixture(scope="module")
def metadata(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    return device_metadata()[0]


def _one(meta, part):
    hits = [k for k in meta if part in k]
    assert len(hits) == 1, (part, hits)
    return meta[hits[0]]


def test_adaptive_kernels_meet_the_main_launch_register_budget(metadata):
    meta = metadata
    render = {k: v for k, v in meta.items() if "render_adaptive_kernel<" in k}
    # the six instantiations of render_accumulate_kernel: fp32 / fp64 x LDS / scalar, plus the fp32 bounded loop
    for prec, src, bound in (("float", 0, "false"), ("float", 1, "false"), ("float", 0, "true"), ("float", 1, "true"),
                             ("double", 0, "false"), ("double", 1, "false")):
        assert [k for k in render if "render_adaptive_kernel<%s, %d, %s>" % (prec, src, bound) in k], (prec, src, bound)
    assert len(render) == 6, sorted(render)
    for k, v in render.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        if "<float" in k:
            assert v["vgpr"] <= 96, (k, v)        # five waves per SIMD
        else:
            assert v["vgpr"] <= 128, (k, v)       # four waves per SIMD
        prec, src = re.search(r"render_adaptive_kernel<(\w+), (\d)", k).groups()
        plain = _one(meta, "render_persistent_kernel<%s, %s, false, false>" % (prec, src))
        assert v["sgpr_spill"] <= plain["sgpr_spill"], (k, v, plain)
    for name in ("adaptive_select_kernel<", "adaptive_finish_kernel<"):
        ks = {k: v for k, v in meta.items() if name in k}
        assert len(ks) == 2, (name, sorted(ks))
        for k, v in ks.items():
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
