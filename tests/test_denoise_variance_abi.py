"""Variance-guided denoising (rtiow_read_variance, rtiow_denoise_variance), the parts that need no GPU: the C-ABI is declared, listed and
exported, the Python wrapper has it, a NULL handle is refused before device work, and the new kernels have no scratch and no VGPR
spills (compiler metadata; hipcc cross-compiles gfx950)."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

VARIANCE_SYMBOLS = ["rtiow_read_variance", "rtiow_denoise_variance"]


def test_variance_symbols_are_declared_listed_and_exported(native):
    from raytracingincuda_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow.h")).read(), flags=re.S)
    version_script = open(os.path.join(ROOT, "raytracingincuda_amd", "csrc", "librtiow_hip.map")).read()
    globs = re.search(r"global:\s*([^;]*);", version_script).group(1).split()
    paths = native.lib_paths()
    for s in VARIANCE_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert any(re.fullmatch(g.replace("*", ".*"), s) for g in globs), s
        assert s in api.HIP_SYMBOLS, s
    for lib in (paths["hip"], paths["hip_debug"]):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for s in VARIANCE_SYMBOLS:
            assert re.search(r"\bT %s\b" % s, syms), (lib, s)


def test_renderer_has_the_variance_interface(native):
    import inspect
    from raytracingincuda_amd import api
    for m in ("variance", "denoise_variance", "accumulate_with_variance"):
        assert callable(getattr(api.Renderer, m, None)), m
    p = inspect.signature(api.Renderer.denoise_variance).parameters
    assert list(p)[1:] == ["levels", "sigma_variance", "sigma_normal", "sigma_albedo", "sigma_depth", "sync"]
    q = inspect.signature(api.Renderer.denoise).parameters
    for name in ("levels", "sigma_normal", "sigma_albedo", "sigma_depth", "sync"):          # the guide defaults stay
        assert p[name].default == q[name].default, name
    assert p["sigma_variance"].default == api.DENOISE_SIGMA_VARIANCE > 0
    lib = native.load_hip_library()
    assert len(lib.rtiow_read_variance.argtypes) == 3 and len(lib.rtiow_denoise_variance.argtypes) == 7
    assert lib.rtiow_abi_version() == 6


def test_null_handle_needs_no_gpu(native):
    lib = native.load_hip_library()
    assert lib.rtiow_read_variance(None, None, 0) == -1
    assert lib.rtiow_denoise_variance(None, 5, 4.0, 1.0, 1.0, 1.0, None) == -1


@pytest.fixture(scope="module")
def metadata(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    return device_metadata()[0]


def test_variance_kernels_have_no_scratch_and_no_vgpr_spills(metadata):
    for name in ("variance_plane_kernel<", "variance_filter_kernel<", "variance_tile_kernel<"):                      # fp32 and fp64 each
        ks = {k: v for k, v in metadata.items() if name in k}
        assert len(ks) == 2, (name, sorted(ks))
        for k, v in ks.items():
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
    # the committed filter's kernels keep their names apart from the new ones (tests/test_denoise_abi.py counts them by substring)
    for name, count in (("guide_kernel<", 4), ("denoise_level_kernel<", 2), ("linear_kernel<", 2)):
        assert len([k for k in metadata if name in k]) == count, name
