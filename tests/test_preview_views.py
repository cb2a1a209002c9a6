"""The frames the GPU tests of the preview chain run on hold every class of pixel those tests are about -- shown on the CPU, from the
oracle's images and first-hit guides through the numpy restatements of tests/preview_model.py: the plan's three classes in the view
pairs of tests/test_history_budget.py, clipped and unclipped history in the orbit of tests/test_history_clip.py, measured and spatial
variance in the budget frame of tests/test_history_variance.py.  (Pixels with and without history in the unsampled frame of
tests/test_history_feedback.py: still in tests/test_history_feedback_abi.py.)"""
import numpy as np
import pytest

from tests.conftest import compact
from tests.preview_drive import BUDGET_PAIRS, CAP_LOW, budget_moves, moves
from tests.preview_model import as_base, clipped_np, guides_np, noise_classes, temporal_noise_np, update_np, window_np


# ---- the classes of pixel in the view pairs of tests/test_history_budget.py

@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("size", [(67, 41), (203, 117)])
def test_the_view_pairs_hold_every_class_of_pixel(native, oracle, scene_id, size):
    """The plan's three classes -- m = 0 (no history: disoccluded, or outside the base's frame), 0 < m < cap, m at the cap -- each hold at
    least 1 % of the frame for every (base view, current view) of tests/test_history_budget.py (BUDGET_PAIRS), from the CPU oracle's
    first-hit guides alone.  The GPU tests commit the base after tests/preview_drive.py's adaptive sample(), which leaves every pixel 4 or
    8 samples, so a gathered length is 0 or lies in [4, 8] whatever the mix; here the base is given 4 everywhere and 8 everywhere in
    turn.  The covered pixels are the same in both, so under CAP_LOW = 2.5 every covered pixel is at the cap and under the default cap
    of 16 every covered pixel is below it; the GPU tests use both caps (and CAP_MIX = 6, between the two counts, where all three classes
    share one plan: that mix depends on the noise and is asserted on the GPU).  Counted here, fp32, pixels with m = 0 of W x H:
                         home->orbit  home->dolly  home->roll  orbit->home  roll->home
      scene 1   67 x  41         192          278         217          185         213      of  2747
      scene 3   67 x  41         112          176         129           88         135
      scene 1  203 x 117        1372         2006        1149         1300        1130      of 23751
      scene 3  203 x 117         990         1815        1120          900        1124"""
    from raytracingincuda_amd import api
    W, H = size
    prec, dt = 32, np.float32
    cams = budget_moves(native, prec, W, H)
    rows = np.arange(H)
    guides = {}
    for view in {v for pair in BUDGET_PAIRS for v in pair}:
        normal, _, depth, _ = guides_np(native, oracle, prec, scene_id, cams[view], rows)
        guides[view] = (normal, depth)
    zero = np.zeros((H, W, 3), dt)
    floor = 0.01 * W * H
    for first, then in BUDGET_PAIRS:
        cur = {"c": zero, "n": np.zeros((H, W), np.int32), "N": guides[then][0], "t": guides[then][1]}
        covered = None
        for count in (4, 8):
            base = {"cam": cams[first], "H": zero, "M": np.full((H, W), count, dt), "N": guides[first][0], "z": guides[first][1]}
            for cap in (CAP_LOW, api.HISTORY_MAX):
                _, m, carried = update_np(cams[then], cur, base, api.HISTORY_DEPTH_TOL, api.HISTORY_NORMAL_COS, cap)
                assert carried == int((m > 0).sum())
                if covered is None:
                    covered = m > 0
                    print("scene %d %dx%d %s -> %s: m = 0 in %d" % (scene_id, W, H, first, then, int((~covered).sum())))
                assert np.array_equal(m > 0, covered), (first, then, count, cap)       # coverage is geometry alone
                if cap == CAP_LOW:
                    assert (m[covered] == dt(cap)).all(), (first, then, count)
                else:
                    assert (m[covered] < dt(cap)).all() and (m[covered] >= dt(count) * dt(1 - 1e-6)).all(), (first, then, count)
        assert (~covered).sum() >= floor, (first, then, int((~covered).sum()), floor)  # m = 0
        assert covered.sum() >= floor, (first, then, int(covered.sum()), floor)        # at CAP_LOW: at the cap; at the default cap: below it


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
