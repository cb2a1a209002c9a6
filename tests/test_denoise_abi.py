"""Denoised previews (rtiow_read_linear, rtiow_render_guides, rtiow_denoise, ...), the parts that need no GPU: the C-ABI is declared,
listed and exported, the Python wrapper has it, argument checks come before device work, and the new kernels have no scratch and no
VGPR spills (compiler metadata; hipcc cross-compiles gfx950)."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

DENOISE_SYMBOLS = ["rtiow_read_linear", "rtiow_render_guides", "rtiow_read_guides", "rtiow_denoise", "rtiow_read_denoised",
                   "rtiow_denoised_device_ptr"]


def test_denoise_symbols_are_declared_listed_and_exported(native):
    from raytracingincuda_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow.h")).read(), flags=re.S)
    version_script = open(os.path.join(ROOT, "raytracingincuda_amd", "csrc", "librtiow_hip.map")).read()
    globs = re.search(r"global:\s*([^;]*);", version_script).group(1).split()
    paths = native.lib_paths()
    for s in DENOISE_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert any(re.fullmatch(g.replace("*", ".*"), s) for g in globs), s
        assert s in api.HIP_SYMBOLS, s
    for lib in (paths["hip"], paths["hip_debug"]):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for s in DENOISE_SYMBOLS:
            assert re.search(r"\bT %s\b" % s, syms), (lib, s)


def test_renderer_has_the_denoise_interface(native):
    from raytracingincuda_amd import api
    for m in ("read_linear", "render_guides", "guides", "denoise", "read_denoised", "denoised_device_ptr"):
        assert callable(getattr(api.Renderer, m, None)), m
    lib = native.load_hip_library()
    arity = {"rtiow_read_linear": 3, "rtiow_render_guides": 2, "rtiow_read_guides": 5, "rtiow_denoise": 7, "rtiow_read_denoised": 3,
             "rtiow_denoised_device_ptr": 3}
    for s, n in arity.items():
        assert len(getattr(lib, s).argtypes) == n, s
    assert native.load_hip_library().rtiow_abi_version() == 6


def test_null_handle_needs_no_gpu(native):
    lib = native.load_hip_library()
    assert lib.rtiow_read_linear(None, None, 0) == -1
    assert lib.rtiow_render_guides(None, None) == -1
    assert lib.rtiow_read_guides(None, None, None, None, 0) == -1
    assert lib.rtiow_denoise(None, 5, 1.0, 1.0, 1.0, 1.0, None) == -1
    assert lib.rtiow_read_denoised(None, None, 0) == -1
    assert lib.rtiow_denoised_device_ptr(None, None, None) == -1


@pytest.fixture(scope="module")
def metadata(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    return device_metadata()[0]


def test_denoise_kernels_have_no_scratch_and_no_vgpr_spills(metadata):
    # guide_kernel: fp32 / fp64 x LDS / scalar scene source; the filter and the linear read: fp32 / fp64
    for name, count in (("guide_kernel<", 4), ("denoise_level_kernel<", 2), ("linear_kernel<", 2)):
        ks = {k: v for k, v in metadata.items() if name in k}
        assert len(ks) == count, (name, sorted(ks))
        for k, v in ks.items():
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
