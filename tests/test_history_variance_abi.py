"""Variance-guided filtering of the temporal image (rtiow_denoise_history_variance, rtiow_read_history_variance), the parts that need no
GPU: the C-ABI is declared, listed and exported, the Python wrappers have it, a NULL handle is refused before device work, the new kernel
has no scratch and no VGPR spills and reads its window from LDS (compiler metadata; hipcc cross-compiles gfx950), and the budget frame
of tests/test_history_variance.py holds both classes of pixel -- measured and spatial -- from the CPU oracle's images and guides through
the numpy restatements of sections 11 and 15."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT, compact
from tests.preview_drive import moves
from tests.preview_model import as_base, guides_np, noise_classes, temporal_noise_np, update_np, window_np

SYMBOLS = ("rtiow_denoise_history_variance", "rtiow_read_history_variance")


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
    p = inspect.signature(api.Renderer.denoise_history_variance).parameters
    assert list(p) == ["self", "levels", "sigma_variance", "sigma_normal", "sigma_albedo", "sigma_depth", "variance_radius", "sync"]
    assert p["variance_radius"].default == api.HISTORY_VARIANCE_RADIUS and 1 <= api.HISTORY_VARIANCE_RADIUS <= 3
    assert p["sigma_variance"].default == api.HISTORY_SIGMA_VARIANCE > 0
    v = inspect.signature(api.Renderer.denoise_variance).parameters
    assert list(v) == ["self", "levels", "sigma_variance", "sigma_normal", "sigma_albedo", "sigma_depth", "sync"]      # unchanged
    assert v["sigma_variance"].default == api.DENOISE_SIGMA_VARIANCE
    for name in ("levels", "sigma_normal", "sigma_albedo", "sigma_depth", "sync"):
        assert p[name].default == v[name].default, name
    assert list(inspect.signature(api.Renderer.history_variance).parameters) == ["self"]
    lib = native.load_hip_library()
    assert len(lib.rtiow_denoise_history_variance.argtypes) == 8
    assert len(lib.rtiow_read_history_variance.argtypes) == 3
    assert len(lib.rtiow_denoise_variance.argtypes) == 7 and len(lib.rtiow_denoise_history.argtypes) == 7
    assert lib.rtiow_abi_version() == native.ABI_VERSION == 6       # functions were added, nothing moved


def test_null_handle_needs_no_gpu(native):
    lib = native.load_hip_library()
    assert lib.rtiow_denoise_history_variance(None, 5, 4.0, 0.1, 0.2, 0.05, 1, None) == -1
    assert lib.rtiow_read_history_variance(None, None, 0) == -1


@pytest.fixture(scope="module")
def metadata(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    return device_metadata()


def test_noise_kernel_has_no_scratch_and_no_vgpr_spills(metadata):
    meta, listing = metadata
    ks = {k: v for k, v in meta.items() if "temporal_noise_kernel<" in k}
    assert len(ks) == 2, sorted(ks)                                  # fp32 and fp64
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        # the name stays apart from the kernels other tests count by substring
        for other in ("render_", "guide_kernel<", "guide_chain_kernel<", "denoise_level_kernel<", "linear_kernel<", "variance_",
                      "history_reproject_kernel<", "history_length_kernel<", "history_clip_kernel<", "budget_select_kernel<",
                      "adaptive_select_kernel<", "adaptive_finish_kernel<"):
            assert other not in k, (k, other)
        body = listing[listing.index("\n%s:" % v["symbol"]):]
        body = body[:body.index(".Lfunc_end")]
        assert len(re.findall(r"\bds_(?:read|load)_\w+", body)) >= 1, (k, re.findall(r"\bds_\w+", body))      # the window comes from LDS
    # the filter levels are the existing kernels: nothing else was instantiated
    for name, count in (("guide_kernel<", 4), ("denoise_level_kernel<", 2), ("linear_kernel<", 2), ("variance_plane_kernel<", 2),
                        ("variance_filter_kernel<", 2), ("variance_tile_kernel<", 2), ("history_reproject_kernel<", 2),
                        ("history_length_kernel<", 2), ("history_clip_kernel<", 2), ("budget_select_kernel<", 2),
                        ("adaptive_select_kernel<", 2), ("adaptive_finish_kernel<", 2)):
        assert len([k for k in meta if name in k]) == count, name


# ---- the classes of pixel in the budget frame of tests/test_history_variance.py

@pytest.mark.parametrize("scene_id", [1, 3])
def test_the_budget_frame_holds_measured_and_spatial_pixels(native, oracle, scene_id):
    """After the move home -> orbit of tests/preview_drive.py's moves and the two budget chunks of tests/test_history_variance.py's
    _budget_mix (one sample where the planned history is short of 6, two more where history and count are short of 3, min_samples = 0) at
    least 1 % of the 203 x 117 frame is measured (n >= 2) and at least 1 % takes the spatial estimate with k >= 2.  The GPU tests commit
    the base after an adaptive pattern that leaves every pixel 4 or 8 samples; here the base is given 4 everywhere and 8 everywhere in turn
    (4: every covered pixel gets one sample; 8: none does).  Images of the CPU oracle (squared back to linear), seeds 1227 and 1228, its
    first-hit guides, the default tolerances."""
    from raytracingincuda_amd import api
    W, H = 203, 117
    prec, dt = 32, np.float32
    params = (api.HISTORY_DEPTH_TOL, api.HISTORY_NORMAL_COS, api.HISTORY_MAX)
    cams = moves(native, prec, W, H)
    scene = compact(native.build_scene(scene_id, prec))

    def linear(view, seed, S):
        cam = cams[view]
        cam.samples_per_pixel = S
        cam.pixel_samples_scale = dt(1) / dt(S)
        img, _ = oracle.render(prec, scene, cam, seed)
        return (img.astype(dt) * img.astype(dt)).reshape(H, W, 3)

    guides = {}
    for view in ("home", "orbit"):
        normal, _, depth, _ = guides_np(native, oracle, prec, scene_id, cams[view], np.arange(H))
        guides[view] = (normal, depth)
    orbit = {1: linear("orbit", 1228, 1), 3: linear("orbit", 1228, 3)}
    for count in (4, 8):
        home = {"c": linear("home", 1227, count), "n": np.full((H, W), count, np.int32), "N": guides["home"][0], "t": guides["home"][1]}
        c0, m0, _ = update_np(cams["home"], home, None, *params)
        base = as_base(cams["home"], home, c0, m0)
        zero = {"c": np.zeros((H, W, 3), dt), "n": np.zeros((H, W), np.int32), "N": guides["orbit"][0], "t": guides["orbit"][1]}
        _, m, _ = update_np(cams["orbit"], zero, base, *params)              # the plan: the m of the update before any sample
        n = np.zeros((H, W), np.int32)
        n = np.where(n.astype(dt) + m < dt(6.0), n + 1, n)                    # budget chunk: 1 sample, target 6
        n = np.where(n.astype(dt) + m < dt(3.0), n + 2, n)                    # budget chunk: 2 samples, target 3
        assert set(np.unique(n)) <= {0, 1, 3}
        c = np.where((n == 3)[..., None], orbit[3], np.where((n == 1)[..., None], orbit[1], dt(0))).astype(dt)
        cur = {"c": c, "n": n, "N": guides["orbit"][0], "t": guides["orbit"][1]}
        C, M, _ = update_np(cams["orbit"], cur, base, *params)
        for radius in (1, 3):
            spatial, k = window_np(C, M, radius)
            got = noise_classes(n, k)
            print("scene %d, base count %d, r = %d: %s of %d" % (scene_id, count, radius, got, W * H))
            assert got["measured"] >= 0.01 * W * H, got
            assert got["spatial with k >= 2"] >= 0.01 * W * H, got
            # the plane of this frame: finite, not negative, and a real estimate in the spatial class
            V0 = temporal_noise_np(C, M, n, np.ones((H, W), dt), radius)
            assert np.isfinite(V0).all() and (V0 >= 0).all()
            assert ((n < 2) & (spatial > 0)).sum() >= 0.01 * W * H
            assert (V0[n >= 2] <= 1).all() and (V0[n >= 2] > 0).all()        # alpha in (0, 1]
