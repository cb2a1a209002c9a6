"""Progressive rendering (rtiow_accumulate), the parts that need no GPU: the C-ABI is declared, listed and exported, the Python
wrapper has it, and the accumulate kernels meet the main launch's register budget (compiler metadata; hipcc cross-compiles gfx950)."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

ACC_SYMBOLS = ["rtiow_accumulate", "rtiow_accumulate_reset", "rtiow_accumulated_samples"]


def test_accumulate_symbols_are_declared_listed_and_exported(native):
    from raytracingincuda_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow.h")).read(), flags=re.S)
    paths = native.lib_paths()
    for s in ACC_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in api.HIP_SYMBOLS, s
    for lib in (paths["hip"], paths["hip_debug"]):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for s in ACC_SYMBOLS:
            assert re.search(r"\bT %s\b" % s, syms), (lib, s)


def test_renderer_has_the_progressive_interface(native):
    from raytracingincuda_amd import api
    assert callable(getattr(api.Renderer, "accumulate", None))
    assert callable(getattr(api.Renderer, "reset_accumulation", None))
    assert isinstance(getattr(api.Renderer, "accumulated_samples", None), property)
    lib = native.load_hip_library()
    assert lib.rtiow_accumulate.argtypes is not None and len(lib.rtiow_accumulate.argtypes) == 4


@pytest.fixture(scope="module")
def accumulate_metadata(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    return device_metadata()[0]


def _one(meta, part):
    hits = [k for k in meta if part in k]
    assert len(hits) == 1, (part, hits)
    return meta[hits[0]]


def test_accumulate_kernels_meet_the_main_launch_register_budget(accumulate_metadata):
    meta = accumulate_metadata
    acc = {k: v for k, v in meta.items() if "render_accumulate_kernel<" in k}
    for prec in ("float", "double"):
        for src in (0, 1):                       # RTIOW_SCENE_LDS (the screened / grid sources run this one too), RTIOW_SCENE_SCALAR
            assert [k for k in acc if "render_accumulate_kernel<%s, %d," % (prec, src) in k], (prec, src)
    for k, v in acc.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        if "<float" in k:
            assert v["vgpr"] <= 96, (k, v)        # five waves per SIMD
        else:
            assert v["vgpr"] <= 128, (k, v)       # four waves per SIMD
        prec, src = re.search(r"render_accumulate_kernel<(\w+), (\d)", k).groups()
        plain = _one(meta, "render_persistent_kernel<%s, %s, false, false>" % (prec, src))
        assert v["sgpr_spill"] <= plain["sgpr_spill"], (k, v, plain)
