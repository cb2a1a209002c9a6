"""Recurrent history (rtiow_history_commit_filtered, rtiow_read_history_base): the parts that need no GPU.
The checks themselves are the rows of tests/test_abi.py and tests/test_kernel_inventory.py; this module keeps its test ids and runs
its feature's rows through tests/kept_abi_ids.py.
Its own still: the unsampled frame of tests/test_history_feedback.py holds pixels with and without history (the like of
tests/test_preview_views.py)."""
import numpy as np
import pytest

from tests import kept_abi_ids as kept
from tests.preview_drive import moves
from tests.preview_model import as_base, guides_np, update_np

SYMBOLS = ("rtiow_history_commit_filtered", "rtiow_read_history_base")
MEMBERS = ("history_commit_filtered", "history_base", "history_commit", "denoise_history")


def test_symbols_are_declared_listed_and_exported(native):
    kept.symbols(SYMBOLS)


def test_renderer_has_the_calls(native):
    kept.wrappers(SYMBOLS + ("rtiow_history_commit", "rtiow_read_history"), MEMBERS)


def test_null_handle_needs_no_gpu(native):
    kept.null_handles(SYMBOLS)


def test_feedback_kernel_has_no_scratch_and_no_vgpr_spills(native):
    kept.kernels("feedback_filter_kernel<")


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
