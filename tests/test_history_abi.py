"""Temporal history (rtiow_history_*, rtiow_denoise_history, rtiow_host_camera_look), the parts that need no GPU: the C-ABI is declared,
listed and exported, the Python wrapper has it, a NULL handle is refused before device work, the placeable camera reproduces the
reference's fixed one byte for byte, and the new kernel has no scratch and no VGPR spills (compiler metadata; hipcc cross-compiles
gfx950)."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

HISTORY_SYMBOLS = ["rtiow_history_reset", "rtiow_history_update", "rtiow_history_commit", "rtiow_read_history", "rtiow_history_device_ptr",
                   "rtiow_denoise_history"]
# the reference's placement, main.cu:114-121
LOOKFROM, LOOKAT, VUP, VFOV, DEFOCUS, FOCUS = (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 0.6, 10.0


def _uncommented(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def test_history_symbols_are_declared_listed_and_exported(native):
    from raytracingincuda_amd import api
    header = _uncommented("rtiow.h")
    version_script = open(os.path.join(ROOT, "raytracingincuda_amd", "csrc", "librtiow_hip.map")).read()
    globs = re.search(r"global:\s*([^;]*);", version_script).group(1).split()
    paths = native.lib_paths()
    for s in HISTORY_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert any(re.fullmatch(g.replace("*", ".*"), s) for g in globs), s
        assert s in api.HIP_SYMBOLS, s
    for lib in (paths["hip"], paths["hip_debug"]):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for s in HISTORY_SYMBOLS:
            assert re.search(r"\bT %s\b" % s, syms), (lib, s)
    # the placeable camera lives in the host library
    assert re.search(r"\bint\s+rtiow_host_camera_look\s*\(", _uncommented("rtiow_host.h"))
    assert "rtiow_host_camera_look" in api.HOST_SYMBOLS
    hsyms = subprocess.run(["nm", "-D", "--defined-only", paths["host"]], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rtiow_host_camera_look\b", hsyms)
    assert not [s for s in HISTORY_SYMBOLS if "group" in s]


def test_renderer_has_the_history_interface(native):
    import inspect
    from raytracingincuda_amd import api
    for m in ("history_reset", "history_update", "history_commit", "history", "history_device_ptr", "denoise_history"):
        assert callable(getattr(api.Renderer, m, None)), m
    p = inspect.signature(api.Renderer.history_update).parameters
    assert list(p)[1:] == ["depth_tol", "normal_cos", "max_history", "sync"]
    assert p["depth_tol"].default == api.HISTORY_DEPTH_TOL >= 0
    assert -1 <= p["normal_cos"].default == api.HISTORY_NORMAL_COS <= 1
    assert p["max_history"].default == api.HISTORY_MAX > 0
    d, q = inspect.signature(api.Renderer.denoise_history).parameters, inspect.signature(api.Renderer.denoise).parameters
    assert list(d) == list(q)
    for name in list(q)[1:]:
        assert d[name].default == q[name].default, name
    lib = native.load_hip_library()
    assert [len(getattr(lib, s).argtypes) for s in HISTORY_SYMBOLS] == [1, 6, 1, 4, 3, 7]
    assert lib.rtiow_abi_version() == native.ABI_VERSION == 6
    assert callable(native.camera_look)


def test_null_handle_needs_no_gpu(native):
    lib = native.load_hip_library()
    assert lib.rtiow_history_reset(None) == -1
    assert lib.rtiow_history_update(None, 0.1, 0.9, 32.0, None, None) == -1
    assert lib.rtiow_history_commit(None) == -1
    assert lib.rtiow_read_history(None, None, None, 0) == -1
    assert lib.rtiow_history_device_ptr(None, None, None) == -1
    assert lib.rtiow_denoise_history(None, 5, 1.0, 1.0, 1.0, 1.0, None) == -1


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("size", [(320, 192), (1920, 1080)])
def test_camera_look_at_the_reference_placement_is_camera(native, prec, size):
    W, H = size
    want = native.camera(prec, W, H, 100, 50)
    got = native.camera_look(prec, W, H, 100, 50, LOOKFROM, LOOKAT, VUP, VFOV, DEFOCUS, FOCUS)
    assert type(got) is type(want)
    assert bytes(got) == bytes(want)
    assert bytes(native.camera_look(prec, W, H, 100, 50)) == bytes(want)          # the defaults are that placement


@pytest.mark.parametrize("prec", [32, 64])
def test_camera_look_moves_the_camera(native, prec):
    import numpy as np
    W, H = 320, 192
    base = native.camera(prec, W, H, 4, 10)
    moved = native.camera_look(prec, W, H, 4, 10, lookfrom=(12.0, 2.5, 4.0))
    dt = np.float32 if prec == 32 else np.float64
    assert list(moved.center) == [dt(12.0), dt(2.5), dt(4.0)]
    assert list(moved.center) != list(base.center) and list(moved.pixel00_loc) != list(base.pixel00_loc)
    assert (moved.img_width, moved.img_height, moved.samples_per_pixel, moved.max_depth) == (W, H, 4, 10)
    # the pixel grid is centred on the view axis: pixel00 + ((W-1)/2) du + ((H-1)/2) dv lies on the line lookfrom -> lookat, focus_dist away
    p00, du, dv, c = (np.array(v[:], np.float64) for v in (moved.pixel00_loc, moved.pixel_delta_u, moved.pixel_delta_v, moved.center))
    mid = p00 + (W - 1) / 2 * du + (H - 1) / 2 * dv
    axis = -c / np.linalg.norm(c)
    assert np.allclose(mid, c + 10.0 * axis, atol=1e-4 if prec == 32 else 1e-12)
    # a wider field of view widens the pixel steps; a roll turns them
    wide = native.camera_look(prec, W, H, 4, 10, vfov=40.0)
    assert np.linalg.norm(np.array(wide.pixel_delta_u[:])) > 1.9 * np.linalg.norm(np.array(base.pixel_delta_u[:]))
    rolled = native.camera_look(prec, W, H, 4, 10, vup=(0.2, 1.0, 0.0))
    assert list(rolled.center) == list(base.center) and list(rolled.pixel_delta_u) != list(base.pixel_delta_u)
    lib = native.load_host_library()
    v = (ctypes.c_double * 3)(1, 2, 3)
    assert lib.rtiow_host_camera_look(prec, W, H, 4, 10, None, v, v, 20.0, 0.6, 10.0, ctypes.addressof(moved)) == -1
    assert lib.rtiow_host_camera_look(16, W, H, 4, 10, v, v, v, 20.0, 0.6, 10.0, ctypes.addressof(moved)) == -1
    assert lib.rtiow_host_camera_look(prec, 0, H, 4, 10, v, v, v, 20.0, 0.6, 10.0, ctypes.addressof(moved)) == -1


@pytest.fixture(scope="module")
def metadata(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    return device_metadata()


def test_history_kernel_has_no_scratch_and_no_vgpr_spills(metadata):
    meta, listing = metadata
    ks = {k: v for k, v in meta.items() if "history_reproject_kernel<" in k}
    assert len(ks) == 2, sorted(ks)                                  # fp32 and fp64
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
    # the name stays apart from the kernels other tests count by substring
    for k in ks:
        for other in ("render_", "guide_kernel<", "denoise_level_kernel<", "linear_kernel<", "variance_"):
            assert other not in k, (k, other)
    for name, count in (("guide_kernel<", 4), ("denoise_level_kernel<", 2), ("linear_kernel<", 2), ("variance_plane_kernel<", 2),
                        ("variance_filter_kernel<", 2), ("variance_tile_kernel<", 2)):
        assert len([k for k in meta if name in k]) == count, name
    # fp32: every tap is two 16-byte vector loads -- the four taps' eight plus the pixel's own guides
    sym = next(v["symbol"] for k, v in ks.items() if "<float>" in k)
    body = listing[listing.index("\n%s:" % sym):]
    body = body[:body.index(".Lfunc_end")]
    assert len(re.findall(r"\bglobal_load_dwordx4\b", body)) >= 9, re.findall(r"\bglobal_load_\w+", body)
