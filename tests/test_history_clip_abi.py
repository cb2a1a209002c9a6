"""History clipped to the neighbourhood colours (rtiow_history_update_clipped), the parts that need no GPU: the C-ABI is declared,
listed and exported, the Python wrapper has it, a NULL handle is refused before device work, the new kernel has no scratch and no VGPR
spills and stages its window in LDS (compiler metadata; hipcc cross-compiles gfx950), and the views of tests/test_history_clip.py hold
both classes of carried pixel -- clipped and not -- from the CPU oracle's images through the numpy restatements of sections 11 and 14."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT, compact
from tests.preview_drive import moves
from tests.preview_model import as_base, clipped_np, guides_np, update_np

SYMBOL = "rtiow_history_update_clipped"


def test_symbol_is_declared_listed_and_exported(native):
    from raytracingincuda_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtiow.h")).read(), flags=re.S)
    version_script = open(os.path.join(ROOT, "raytracingincuda_amd", "csrc", "librtiow_hip.map")).read()
    globs = re.search(r"global:\s*([^;]*);", version_script).group(1).split()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, header)
    assert any(re.fullmatch(g.replace("*", ".*"), SYMBOL) for g in globs)
    assert SYMBOL in api.HIP_SYMBOLS
    paths = native.lib_paths()
    for lib in (paths["hip"], paths["hip_debug"]):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT %s\b" % SYMBOL, syms), lib


def test_renderer_has_the_clipped_update(native):
    from raytracingincuda_amd import api
    p = inspect.signature(api.Renderer.history_update_clipped).parameters
    assert list(p) == ["self", "clip_radius", "clip_gamma", "depth_tol", "normal_cos", "max_history", "sync"]
    assert p["clip_radius"].default == api.HISTORY_CLIP_RADIUS and 1 <= api.HISTORY_CLIP_RADIUS <= 3
    assert p["clip_gamma"].default == api.HISTORY_CLIP_GAMMA >= 0
    u = inspect.signature(api.Renderer.history_update).parameters
    assert list(u) == ["self", "depth_tol", "normal_cos", "max_history", "sync"]         # unchanged
    for name in list(u)[1:]:
        assert p[name].default == u[name].default, name
    assert (u["depth_tol"].default, u["normal_cos"].default, u["max_history"].default, u["sync"].default) == \
        (api.HISTORY_DEPTH_TOL, api.HISTORY_NORMAL_COS, api.HISTORY_MAX, True)
    lib = native.load_hip_library()
    assert len(lib.rtiow_history_update_clipped.argtypes) == 9
    assert len(lib.rtiow_history_update.argtypes) == 6
    assert lib.rtiow_abi_version() == native.ABI_VERSION == 6       # a function was added, nothing moved


def test_null_handle_needs_no_gpu(native):
    lib = native.load_hip_library()
    assert lib.rtiow_history_update_clipped(None, 0.1, 0.9, 16.0, 1, 0.75, None, None, None) == -1


@pytest.fixture(scope="module")
def metadata(native):
    from raytracingincuda_amd.kernel_metadata import device_metadata
    return device_metadata()


def test_clip_kernel_has_no_scratch_and_no_vgpr_spills(metadata):
    meta, listing = metadata
    ks = {k: v for k, v in meta.items() if "history_clip_kernel<" in k}
    assert len(ks) == 2, sorted(ks)                                  # fp32 and fp64
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        # the name stays apart from the kernels other tests count by substring
        for other in ("render_", "guide_kernel<", "guide_chain_kernel<", "denoise_level_kernel<", "linear_kernel<", "variance_",
                      "history_reproject_kernel<", "history_length_kernel<", "budget_select_kernel<", "adaptive_select_kernel<",
                      "adaptive_finish_kernel<"):
            assert other not in k, (k, other)
    for name, count in (("guide_kernel<", 4), ("denoise_level_kernel<", 2), ("linear_kernel<", 2), ("variance_plane_kernel<", 2),
                        ("variance_filter_kernel<", 2), ("variance_tile_kernel<", 2), ("history_reproject_kernel<", 2),
                        ("history_length_kernel<", 2), ("budget_select_kernel<", 2), ("adaptive_select_kernel<", 2),
                        ("adaptive_finish_kernel<", 2)):
        assert len([k for k in meta if name in k]) == count, name
    # fp32: the gather is the plain update's -- the four taps' eight 16-byte vector loads plus the pixel's own guides -- and the
    # window comes from LDS
    sym = next(v["symbol"] for k, v in ks.items() if "<float>" in k)
    body = listing[listing.index("\n%s:" % sym):]
    body = body[:body.index(".Lfunc_end")]
    assert len(re.findall(r"\bglobal_load_dwordx4\b", body)) >= 9, re.findall(r"\bglobal_load_\w+", body)
    assert len(re.findall(r"\bds_(?:read|load)_\w+", body)) >= 1, re.findall(r"\bds_\w+", body)


# ---- the classes of pixel in the views of tests/test_history_clip.py

@pytest.mark.parametrize("scene_id", [1, 3])
def test_the_orbit_holds_clipped_and_unclipped_history(native, oracle, scene_id):
    """At r = 1, gamma = 0.75 at least 1 % of the 203 x 117 frame is clipped and at least 1 % is carried and not clipped after the move
    home -> orbit of tests/preview_drive.py's moves: 6 samples a frame from the CPU oracle (its images squared back to linear), seeds
    1227 and 1228, its first-hit guides, the default tolerances."""
    from raytracingincuda_amd import api
    W, H, S = 203, 117, 6
    prec, dt = 32, np.float32
    params = (api.HISTORY_DEPTH_TOL, api.HISTORY_NORMAL_COS, api.HISTORY_MAX)
    cams = moves(native, prec, W, H)
    scene = compact(native.build_scene(scene_id, prec))
    state = {}
    for view, seed in (("home", 1227), ("orbit", 1228)):
        cam = cams[view]
        cam.samples_per_pixel = S
        cam.pixel_samples_scale = dt(1) / dt(S)
        img, _ = oracle.render(prec, scene, cam, seed)
        normal, _, depth, _ = guides_np(native, oracle, prec, scene_id, cam, np.arange(H))
        state[view] = {"c": (img.astype(dt) * img.astype(dt)).reshape(H, W, 3), "n": np.full((H, W), S, np.int32), "N": normal, "t": depth}
    c0, m0, _ = update_np(cams["home"], state["home"], None, *params)
    base = as_base(cams["home"], state["home"], c0, m0)
    want = clipped_np(cams["orbit"], state["orbit"], base, params, 1, 0.75)
    kept = int(((want["m"] > 0) & ~want["mask"]).sum())
    print("scene %d: clipped %d, carried and not clipped %d of %d" % (scene_id, want["clipped"], kept, W * H))
    assert want["clipped"] + kept == want["reprojected"]
    assert want["clipped"] >= 0.01 * W * H, want["clipped"]
    assert kept >= 0.01 * W * H, kept
