"""The table of tests/preview_refusals.py through the library on the GPU: every preview call (INTEGRATION.md sections 9 to 16) in every
state and with every bad argument returns the recorded code and leaves the recorded rtiow_last_error_string, byte for byte.  One handle
per state; after a call that went through and may have changed the state, the handle goes through the state's steps again."""
import ctypes

import numpy as np
import pytest

from tests import preview_refusals as table
from tests.preview_drive import moves

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _steps(r, rt, steps, cams, scene):
    do = {"scene_camera": lambda: (r.set_camera(cams["home"]), r.set_scene(scene)), "rng": lambda: r.init_rng(1227),
          "plain": lambda: r.accumulate(1), "adaptive": lambda: r.accumulate_adaptive(1, 0.0), "update": lambda: r.history_update(),
          "plan": lambda: r.history_plan(), "commit": lambda: r.history_commit(), "move": lambda: r.set_camera(cams["orbit"]),
          "history_variance": lambda: r.denoise_history_variance(), "shard": lambda: r.set_shard(*table.SHARD)}
    for s in steps:
        do[s]()


def _restore(r, rt, steps, cams, scene):
    """Back to the state on the same handle: the guide mode, then -- a handle that has a scene -- an unsharded handle without a base,
    and the steps, the first of which sets the scene and the camera and with them everything else."""
    r.set_guide_mode(rt.api.GUIDES_FIRST_HIT)
    if steps:
        r.set_shard(0, 1, 8)
        _steps(r, rt, steps, cams, scene)


def _call(r, call, a, out, rows):
    """The call with the arguments `a`; outputs go to `out`, counters and times are not asked for."""
    lib, h, p = r._lib, r._h, out.ctypes.data
    npix = table.W * rows
    ptr, size = ctypes.c_void_p(), ctypes.c_size_t(0)
    sig = lambda: (a["sigma_first"], a["sigma_normal"], a["sigma_albedo"], a["sigma_depth"])
    tol = lambda: (a["depth_tol"], a["normal_cos"], a["max_history"])
    return {
        "rtiow_read_linear": lambda: lib.rtiow_read_linear(h, p, npix * 12 + a["size"]),
        "rtiow_render_guides": lambda: lib.rtiow_render_guides(h, None),
        "rtiow_read_guides": lambda: lib.rtiow_read_guides(h, p, None, None, npix + a["size"]),
        "rtiow_denoise": lambda: lib.rtiow_denoise(h, a["levels"], *sig(), None),
        "rtiow_read_denoised": lambda: lib.rtiow_read_denoised(h, p, npix * 12 + a["size"]),
        "rtiow_denoised_device_ptr": lambda: lib.rtiow_denoised_device_ptr(h, ctypes.byref(ptr), ctypes.byref(size)),
        "rtiow_read_variance": lambda: lib.rtiow_read_variance(h, p, npix + a["size"]),
        "rtiow_denoise_variance": lambda: lib.rtiow_denoise_variance(h, a["levels"], *sig(), None),
        "rtiow_history_reset": lambda: lib.rtiow_history_reset(h),
        "rtiow_history_update": lambda: lib.rtiow_history_update(h, *tol(), None, None),
        "rtiow_history_commit": lambda: lib.rtiow_history_commit(h),
        "rtiow_read_history": lambda: lib.rtiow_read_history(h, p, None, npix + a["size"]),
        "rtiow_history_device_ptr": lambda: lib.rtiow_history_device_ptr(h, ctypes.byref(ptr), ctypes.byref(size)),
        "rtiow_denoise_history": lambda: lib.rtiow_denoise_history(h, a["levels"], *sig(), None),
        "rtiow_set_guide_mode": lambda: lib.rtiow_set_guide_mode(h, a["mode"], a["max_bounces"], a["max_fuzz"]),
        "rtiow_read_filter_guides": lambda: lib.rtiow_read_filter_guides(h, p, None, None, None, npix + a["size"]),
        "rtiow_history_plan": lambda: lib.rtiow_history_plan(h, *tol(), None, None),
        "rtiow_read_history_plan": lambda: lib.rtiow_read_history_plan(h, p, npix + a["size"]),
        "rtiow_accumulate_budget": lambda: lib.rtiow_accumulate_budget(h, a["samples"], a["min_samples"], a["target"], a["max_samples"], None, None),
        "rtiow_history_update_clipped": lambda: lib.rtiow_history_update_clipped(h, *tol(), a["clip_radius"], a["clip_gamma"], None, None, None),
        "rtiow_denoise_history_variance": lambda: lib.rtiow_denoise_history_variance(h, a["levels"], *sig(), a["variance_radius"], None),
        "rtiow_read_history_variance": lambda: lib.rtiow_read_history_variance(h, p, npix + a["size"]),
        "rtiow_history_commit_filtered": lambda: lib.rtiow_history_commit_filtered(h, *sig(), a["feedback"], None),
        # the base keeps the whole frame it was committed at
        "rtiow_read_history_base": lambda: lib.rtiow_read_history_base(h, p, None, table.W * table.H + a["size"]),
    }[call]()


def drive(rt):
    """[(state, call, label, code, message)] of every case of the table, the message '' where the call went through."""
    cams = moves(rt, table.PRECISION, table.W, table.H, table.MAX_DEPTH)
    scene = rt.build_scene(table.SCENE_ID, table.PRECISION)
    out = np.zeros(table.W * table.H * 4 + 16, np.float32)
    got = []
    for state, steps in table.STATES.items():
        with rt.Renderer(0, table.PRECISION) as r:
            _steps(r, rt, steps, cams, scene)
            rows = r.local_rows if "scene_camera" in steps else 0
            for call in table.CALLS:
                for varied, args in table.argument_sets(call):
                    code = _call(r, call, args, out, rows)
                    message = r._lib.rtiow_last_error_string(r._h).decode() if code else ""
                    got.append((state, call, table.label(varied, args), code, message))
                    if code == 0 and call not in table.READ_ONLY:
                        _restore(r, rt, steps, cams, scene)
            r.synchronize()
    return got


def test_every_call_in_every_state(rt):
    want = table.expected()
    got = drive(rt)
    assert len(got) == len(want) == len(table.cases())
    wrong = [(state, call, case, (code, message), want.get((state, call, case))) for state, call, case, code, message in got
             if want.get((state, call, case)) != (code, message)]
    assert not wrong, (len(wrong), wrong[:10])
    assert {code for _, _, _, code, _ in got} == {0, table.E_BADARG, table.E_STATE}
