"""Recurrent history (rtiow_history_commit_filtered, rtiow_read_history_base), the parts that need no GPU: the C-ABI is declared, listed
and exported, the Python wrappers have it, a NULL handle is refused before device work, the new kernel has no scratch and no VGPR spills
and reads its taps from LDS (compiler metadata; hipcc cross-compiles gfx950), and the frame of tests/test_history_feedback.py's
unsampled-pixel test holds both classes of pixel -- with and without history -- from the CPU oracle's guides through the numpy restatement
of section 11."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.preview_drive import moves
from tests.preview_model import as_base, guides_np, update_np

SYMBOLS = ("rtiow_history_commit_filtered", "rtiow_read_history_base")


def test_symbols_are_declared_listed_and_exported(native):
    from raytracingincuda_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow.h")).read(), flags=re.S)
    version_script = open(os.path.join(ROOT, "raytracingincuda_amd", "csrc", "librtiow_hip.map")).read()
    globs = re.search(r"global:\s*([^;]*);", version_script).group(1).split()
    paths = native.lib_paths()
    for symbol in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % symbol, header), symbol
        assert any(re.fullmatch(g.replace("*", ".*"), symbol) for g in globs), symbol
        assert symbol in api.HIP_SYMBOLS
        for lib in (paths["hip"], paths["hip_debug"]):
            syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
            assert re.search(r"\bT %s\b" % symbol, syms), (symbol, lib)


def test_renderer_has_the_calls(native):
    from raytracingincuda_amd import api
    p = inspect.signature(api.Renderer.history_commit_filtered).parameters
    assert list(p) == ["self", "sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth", "feedback", "sync"]
    assert p["sigma_color"].default == api.HISTORY_FEEDBACK_SIGMA_COLOR > 0
    assert p["feedback"].default == api.HISTORY_FEEDBACK and 0 < api.HISTORY_FEEDBACK <= 1
    assert p["sync"].default is True
    d = inspect.signature(api.Renderer.denoise_history).parameters
    for name, value in (("sigma_normal", api.DENOISE_SIGMA_NORMAL), ("sigma_albedo", api.DENOISE_SIGMA_ALBEDO), ("sigma_depth", api.DENOISE_SIGMA_DEPTH)):
        assert p[name].default == d[name].default == value, name
    assert list(inspect.signature(api.Renderer.history_base).parameters) == ["self"]
    assert list(inspect.signature(api.Renderer.history_commit).parameters) == ["self"]                # unchanged
    lib = native.load_hip_library()
    assert len(lib.rtiow_history_commit_filtered.argtypes) == 7
    assert len(lib.rtiow_read_history_base.argtypes) == 4
    assert len(lib.rtiow_history_commit.argtypes) == 1 and len(lib.rtiow_read_history.argtypes) == 4
    assert lib.rtiow_abi_version() == native.ABI_VERSION == 6       # functions were added, nothing moved


def test_null_handle_needs_no_gpu(native):
    lib = native.load_hip_library()
    assert lib.rtiow_history_commit_filtered(None, 0.1, 0.1, 0.2, 0.05, 1.0, None) == -1
    assert lib.rtiow_read_history_base(None, None, None, 0) == -1


@pytest.fixture(scope="module")
def metadata(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    return device_metadata()


def test_feedback_kernel_has_no_scratch_and_no_vgpr_spills(metadata):
    meta, listing = metadata
    ks = {k: v for k, v in meta.items() if "feedback_filter_kernel<" in k}
    assert len(ks) == 2, sorted(ks)                                  # fp32 and fp64
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        # the name stays apart from the kernels other tests count by substring
        for other in ("render_", "guide_kernel<", "guide_chain_kernel<", "denoise_level_kernel<", "linear_kernel<", "variance_",
                      "history_reproject_kernel<", "history_length_kernel<", "history_clip_kernel<", "budget_select_kernel<",
                      "adaptive_select_kernel<", "adaptive_finish_kernel<", "temporal_noise_kernel<"):
            assert other not in k, (k, other)
        body = listing[listing.index("\n%s:" % v["symbol"]):]
        body = body[:body.index(".Lfunc_end")]
        assert len(re.findall(r"\bds_(?:read|load)_\w+", body)) >= 1, (k, re.findall(r"\bds_\w+", body))      # the taps come from LDS
        assert len(re.findall(r"\bs_barrier\b", body)) == 1, k                                               # the tile is staged once
    # the existing kernels are the ones tests/test_history_variance_abi.py lists: nothing else was instantiated
    for name, count in (("guide_kernel<", 4), ("denoise_level_kernel<", 2), ("linear_kernel<", 2), ("variance_plane_kernel<", 2),
                        ("variance_filter_kernel<", 2), ("variance_tile_kernel<", 2), ("history_reproject_kernel<", 2),
                        ("history_length_kernel<", 2), ("history_clip_kernel<", 2), ("budget_select_kernel<", 2),
                        ("adaptive_select_kernel<", 2), ("adaptive_finish_kernel<", 2), ("temporal_noise_kernel<", 2)):
        assert len([k for k in meta if name in k]) == count, name


# ---- the classes of pixel in the frame of tests/test_history_feedback.py::test_unsampled_pixels_do_not_count

@pytest.mark.parametrize("scene_id", [1, 3])
def test_the_unsampled_frame_holds_pixels_with_and_without_history(native, oracle, scene_id):
    """After the move home -> orbit of tests/preview_drive.py's moves, a base of 3 samples everywhere and no sample at the new camera, M
    of the update is the gathered history length alone: 0 in at least 1 % of the 203 x 117 frame (disoccluded, or off the base's frame),
    positive in at least 50 %, and at least one pixel with history has a pixel without inside its 5 x 5 window.  The lengths depend on
    the cameras and the first-hit guides only, so the CPU oracle's guides and the default tolerances decide it."""
    from raytracingincuda_amd import api
    W, H = 203, 117
    prec, dt = 32, np.float32
    params = (api.HISTORY_DEPTH_TOL, api.HISTORY_NORMAL_COS, api.HISTORY_MAX)
    cams = moves(native, prec, W, H)
    guides = {}
    for view in ("home", "orbit"):
        normal, _, depth, _ = guides_np(native, oracle, prec, scene_id, cams[view], np.arange(H))
        guides[view] = (normal, depth)
    blank = lambda view, count: {"c": np.zeros((H, W, 3), dt), "n": np.full((H, W), count, np.int32), "N": guides[view][0], "t": guides[view][1]}
    home = blank("home", 3)
    c0, m0, _ = update_np(cams["home"], home, None, *params)
    assert (m0 == 3).all()
    _, M, carried = update_np(cams["orbit"], blank("orbit", 0), as_base(cams["home"], home, c0, m0), *params)
    empty, held = M == 0, M > 0
    print("scene %d: M == 0 in %.1f %%, M > 0 in %.1f %% of %d" % (scene_id, 100 * empty.mean(), 100 * held.mean(), W * H))
    assert carried == int(held.sum()) and (empty | held).all()
    assert empty.mean() >= 0.01 and held.mean() >= 0.5
    near = np.zeros_like(empty)
    pe = np.pad(empty, 2)
    for dy in range(5):
        for dx in range(5):
            near |= pe[dy:dy + H, dx:dx + W]
    assert (held & near).any()
