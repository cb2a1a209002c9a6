"""Filter guides through mirrors and glass (rtiow_set_guide_mode, rtiow_read_filter_guides), the parts that need no GPU: the C-ABI is
declared, listed and exported, the Python wrapper has it, argument checks come before device work, and guide_chain_kernel has no scratch
and no VGPR spills (compiler metadata; hipcc cross-compiles gfx950) next to the unchanged counts of the kernels it joins."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

GUIDE_SYMBOLS = ["rtiow_set_guide_mode", "rtiow_read_filter_guides"]


def test_guide_mode_symbols_are_declared_listed_and_exported(native):
    from raytracingincuda_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow.h")).read(), flags=re.S)
    version_script = open(os.path.join(ROOT, "raytracingincuda_amd", "csrc", "librtiow_hip.map")).read()
    globs = re.search(r"global:\s*([^;]*);", version_script).group(1).split()
    paths = native.lib_paths()
    for s in GUIDE_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert any(re.fullmatch(g.replace("*", ".*"), s) for g in globs), s
        assert s in api.HIP_SYMBOLS, s
    assert re.search(r"#define\s+RTIOW_GUIDES_FIRST_HIT\s+0\b", header) and re.search(r"#define\s+RTIOW_GUIDES_SPECULAR\s+1\b", header)
    assert re.search(r"#define\s+RTIOW_ABI_VERSION\s+6\b", header)
    for lib in (paths["hip"], paths["hip_debug"]):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for s in GUIDE_SYMBOLS:
            assert re.search(r"\bT %s\b" % s, syms), (lib, s)


def test_renderer_has_the_guide_mode_interface(native):
    from raytracingincuda_amd import api
    for m in ("set_guide_mode", "filter_guides"):
        assert callable(getattr(api.Renderer, m, None)), m
    assert (native.GUIDES_FIRST_HIT, native.GUIDES_SPECULAR) == (0, 1)
    assert 1 <= api.GUIDE_MAX_BOUNCES <= 16 and api.GUIDE_MAX_FUZZ >= 0
    lib = native.load_hip_library()
    assert len(lib.rtiow_set_guide_mode.argtypes) == 4
    assert len(lib.rtiow_read_filter_guides.argtypes) == 6
    assert lib.rtiow_abi_version() == 6 == api.ABI_VERSION


def test_null_handle_needs_no_gpu(native):
    lib = native.load_hip_library()
    assert lib.rtiow_set_guide_mode(None, 1, 8, 0.0) == -1
    assert lib.rtiow_read_filter_guides(None, None, None, None, None, 0) == -1


@pytest.fixture(scope="module")
def metadata(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    return device_metadata()[0]


def test_guide_chain_kernel_has_no_scratch_and_no_vgpr_spills(metadata):
    # guide_chain_kernel and guide_kernel: fp32 / fp64 x LDS / scalar scene source; the filter and the linear read: fp32 / fp64
    for name, count in (("guide_chain_kernel<", 4), ("guide_kernel<", 4), ("denoise_level_kernel<", 2), ("linear_kernel<", 2)):
        ks = {k: v for k, v in metadata.items() if name in k}
        assert len(ks) == count, (name, sorted(ks))
        for k, v in ks.items():
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
    for k in metadata:                                   # existing tests count kernels by these substrings
        if "guide_chain_kernel<" in k:
            assert "render_" not in k and "variance_" not in k, k
