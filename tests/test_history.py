"""Temporal history for progressive previews on the GPU: rtiow_history_update reprojects every pixel of the
current camera into the frame committed from an earlier one, gathers the matching history and blends it with the accumulation by sample
count.  Every output is defined operation by operation in T with plain * + - /, so it is checked BIT FOR BIT against
tests/preview_model.py's update_np; the cameras come from camera_look."""
import ctypes

import numpy as np
import pytest

from tests.preview_drive import E_BADARG, E_STATE, INF, SLACK, begin, check_update, move, moves, orbit_walk, sample, state
from tests.preview_model import as_base, filter_np, quality, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


# ---- 1. exactness

@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_update_is_exact(rt, prec, scene_id, adaptive):
    W, H = 203, 117                                     # not a multiple of 16 in either direction
    rt_default = (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, rt.api.HISTORY_MAX)
    cams = moves(rt, prec, W, H)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, cams["home"])
        sample(r, adaptive)
        cur = state(r, adaptive)
        c0, m0, _ = check_update(r, cams["home"], cur, None, rt_default, "first frame")
        r.history_commit()
        base = as_base(cams["home"], cur, c0, m0)
        sweeps = {"orbit": [rt_default, (0.0, rt_default[1], rt_default[2]), (rt_default[0], -1.0, INF)],
                  "dolly": [rt_default, (rt_default[0], rt_default[1], 2.5), (0.0, -1.0, INF)],
                  "roll": [rt_default, (rt_default[0], -1.0, 2.5), (rt_default[0], rt_default[1], INF)]}
        for name, params_list in sweeps.items():
            move(r, cams[name], 1228)
            sample(r, adaptive)
            cur = state(r, adaptive)
            for params in params_list:
                _, m, count = check_update(r, cams[name], cur, base, params, (prec, scene_id, adaptive, name, params))
                if params == rt_default:
                    assert count > 0.5 * W * H, (name, count)        # a small move keeps most of the frame
                    assert m.max() > cur["n"].max()
                if params[2] == 2.5:
                    assert (m - cur["n"].astype(m.dtype)).max() <= 2.5


# ---- 2. no history means no change

@pytest.mark.parametrize("prec", [32, 64])
def test_no_history_means_no_change(rt, prec):
    W, H = 150, 90
    cams = moves(rt, prec, W, H)

    def unchanged(r, adaptive, where):
        lin = r.read_linear()
        n = r.adaptive_state()[0] if adaptive else np.full((r.height, r.width), r.accumulated_samples, np.int32)
        count = r.history_update()
        rgb, length = r.history()
        assert count == 0, where
        assert same_bits(rgb, lin), where
        assert same_bits(length, n.astype(r.dtype)), where

    for adaptive in (False, True):
        with rt.Renderer(0, prec) as r:
            begin(r, rt, prec, 3, cams["home"])
            sample(r, adaptive)
            unchanged(r, adaptive, "before any commit")
            r.history_commit()
            move(r, cams["orbit"]); sample(r, adaptive)
            assert r.history_update() > 0
            r.history_reset()
            unchanged(r, adaptive, "after history_reset")
            r.history_commit()
            r.set_scene(rt.build_scene(3, prec)); r.init_rng(1227); sample(r, adaptive)
            unchanged(r, adaptive, "after set_scene")
            r.history_commit()
            move(r, rt.camera_look(prec, W + 10, H, 1, 10)); sample(r, adaptive)
            unchanged(r, adaptive, "a base of another frame size")
            r.history_commit()
            # facing away from the scene: what the new camera sees lies behind the base camera or outside its frame
            away = rt.camera_look(prec, W + 10, H, 1, 10, lookfrom=(13.0, 2.0, 3.0), lookat=(26.0, 4.0, 6.0))
            move(r, away); sample(r, adaptive)
            unchanged(r, adaptive, "a camera facing away")


# ---- 3. oracle-free sanity

def test_same_camera_is_the_count_weighted_mean(rt):
    """fp64: commit, set the same camera again, accumulate: every pixel reprojects onto itself (u, v within rounding of x, y), so M is
    M_base + n and the colour the count-weighted mean of the two accumulations."""
    prec, W, H = 64, 160, 96
    cam = rt.camera_look(prec, W, H, 1, 10)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 3, cam)
        r.accumulate(6)
        c1 = r.read_linear()
        r.history_update(max_history=INF)
        r.history_commit()
        move(r, cam, 99)
        r.accumulate(2)
        c2 = r.read_linear()
        count = r.history_update(depth_tol=1e-6, normal_cos=0.999999, max_history=INF)
        rgb, length = r.history()
    assert count == W * H
    assert np.allclose(length, 8.0, rtol=1e-9, atol=0)
    # the bilinear gather lands within rounding of the pixel itself: the neighbours' share of the weight is ~1e-13
    assert np.allclose(rgb, (6.0 * c1 + 2.0 * c2) / 8.0, rtol=1e-9, atol=1e-9 * float(max(c1.max(), c2.max())))


# ---- 4. idempotence and commit

@pytest.mark.parametrize("prec", [32, 64])
def test_update_is_idempotent_and_counts_nothing_twice(rt, prec):
    W, H = 150, 90
    cams = moves(rt, prec, W, H)
    params = (0.05, 0.8, INF)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 1, cams["home"])
        r.accumulate(4)
        cur = state(r, False)
        c0, m0, _ = check_update(r, cams["home"], cur, None, params, "home")
        r.history_commit()
        base = as_base(cams["home"], cur, c0, m0)
        move(r, cams["orbit"], 5)
        r.accumulate(2)
        r.history_update(*params)
        first = r.history()
        r.history_update(*params)
        again = r.history()
        assert same_bits(first[0], again[0]) and same_bits(first[1], again[1])
        r.accumulate(3)                                   # a further chunk: the update is over the whole accumulation, n = 5
        cur = state(r, False)
        assert int(cur["n"].max()) == 5
        _, m, _ = check_update(r, cams["orbit"], cur, base, params, "after a further chunk")
        assert float(m.max()) <= 4 + 5


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("prec", [32, 64])
def test_a_chain_of_commits_is_exact(rt, prec, adaptive):
    W, H = 203, 117
    cams = moves(rt, prec, W, H)
    params = (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, 12.0)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 3, cams["home"])
        base = None
        for k, name in enumerate(("home", "orbit", "dolly")):
            if k:
                move(r, cams[name], 1227 + k)
            sample(r, adaptive)
            cur = state(r, adaptive)
            c, m, count = check_update(r, cams[name], cur, base, params, (prec, adaptive, name))
            assert (count > 0) == (k > 0)
            r.history_commit()
            base = as_base(cams[name], cur, c, m)
        assert float(base["M"].max()) > float(cur["n"].max())


# ---- 5. denoise_history

@pytest.mark.parametrize("prec", [32, 64])
def test_denoise_history_is_the_filter_of_the_temporal_image(rt, prec):
    W, H = 150, 90
    cams = moves(rt, prec, W, H)
    sig = (0.5, 0.1, 0.1, 1.0)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 3, cams["home"])
        r.accumulate(4)
        r.history_update(); r.history_commit()
        move(r, cams["orbit"], 7)
        r.accumulate(4)
        own = r.denoise(3, *sig)
        assert r.history_update() > 0
        rgb, _ = r.history()
        n, a, z = r.guides()
        assert not same_bits(rgb, r.read_linear())
        for levels in (1, 3):
            got = r.denoise_history(levels, *sig)
            assert same_bits(got, filter_np(rgb, n, a, z, levels, *sig)), (prec, levels)
            assert same_bits(r.read_denoised(), got)
        assert same_bits(r.denoise(3, *sig), own)       # rtiow_denoise still reads the accumulation
        ptr, nbytes = r.history_device_ptr()
        assert ptr and nbytes == W * H * 4 * (prec // 8)


# ---- 6. nothing else moved

@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("prec", [32, 64])
def test_history_leaves_everything_else_alone(rt, prec, adaptive):
    W, H = 128, 72
    cams = moves(rt, prec, W, H)

    def run(with_history):
        out = []
        with rt.Renderer(0, prec) as r:
            begin(r, rt, prec, 1, cams["home"])
            sample(r, adaptive)
            if with_history:
                r.history_update(); r.history_commit()
            move(r, cams["orbit"])
            sample(r, adaptive, calls=1)
            if with_history:
                r.history_update()
                r.denoise_history(2)
                r.history_update(0.0, -1.0, INF, sync=False)
                r.synchronize()
            out += [r.read_framebuffer(), r.read_linear()]
            if adaptive:
                out += list(r.adaptive_state())
            if with_history:
                r.history_commit()
                r.history_reset()
            if adaptive:
                r.accumulate_adaptive(4, 0.0, min_samples=8)
            else:
                r.accumulate(3)
            out += [r.read_framebuffer(), r.read_linear(), np.array([r.accumulated_samples])]
            if adaptive:
                out += list(r.adaptive_state())
        return out

    plain, touched = run(False), run(True)
    assert len(plain) == len(touched)
    for k, (a, b) in enumerate(zip(plain, touched)):
        assert same_bits(a, b), (prec, adaptive, k)


# ---- 7. states and error codes

def test_states_and_error_codes(rt):
    W, H = 96, 64
    npix = W * H
    cams = moves(rt, 32, W, H)
    nul = (None, None)
    with rt.Renderer(0, 32) as r:
        lib = r._lib
        p, nb = ctypes.c_void_p(), ctypes.c_size_t(0)
        stale = lambda: (lib.rtiow_history_commit(r._h), lib.rtiow_read_history(r._h, None, None, npix),
                         lib.rtiow_history_device_ptr(r._h, ctypes.byref(p), ctypes.byref(nb)),
                         lib.rtiow_denoise_history(r._h, 2, 1.0, 1.0, 1.0, 1.0, None))
        begin(r, rt, 32, 3, cams["home"])
        assert lib.rtiow_history_update(r._h, 0.1, 0.9, 8.0, *nul) == E_STATE           # no chunk since the reset
        assert stale() == (E_STATE,) * 4
        assert lib.rtiow_history_reset(r._h) == 0
        r.accumulate(2)
        for bad in ((-0.1, 0.9, 8.0), (float("nan"), 0.9, 8.0), (0.1, 1.5, 8.0), (0.1, -1.5, 8.0), (0.1, float("nan"), 8.0),
                    (0.1, 0.9, 0.0), (0.1, 0.9, -1.0), (0.1, 0.9, float("nan"))):
            assert lib.rtiow_history_update(r._h, *bad, *nul) == E_BADARG, bad
        assert stale() == (E_STATE,) * 4                                                 # the bad calls wrote nothing
        assert lib.rtiow_history_update(r._h, 0.0, -1.0, INF, *nul) == 0                 # the ends of the ranges; asynchronous
        assert lib.rtiow_history_update(r._h, 0.1, 1.0, 1e-3, *nul) == 0
        assert lib.rtiow_read_history(r._h, None, None, npix) == 0
        assert lib.rtiow_read_history(r._h, None, None, npix + 1) == E_BADARG
        assert lib.rtiow_history_device_ptr(r._h, None, ctypes.byref(nb)) == E_BADARG
        assert lib.rtiow_history_device_ptr(r._h, ctypes.byref(p), ctypes.byref(nb)) == 0 and nb.value == npix * 16
        for levels in (0, 9):
            assert lib.rtiow_denoise_history(r._h, levels, 1.0, 1.0, 1.0, 1.0, None) == E_BADARG
        assert lib.rtiow_denoise_history(r._h, 2, 0.0, 1.0, 1.0, 1.0, None) == E_BADARG
        assert lib.rtiow_denoise_history(r._h, 2, 1.0, 1.0, 1.0, 1.0, None) == 0
        # the temporal image survives a further chunk, an accumulation reset and init_rng (it is what the last update wrote) ...
        r.accumulate(2); r.reset_accumulation(); r.init_rng(3)
        assert lib.rtiow_read_history(r._h, None, None, npix) == 0
        assert lib.rtiow_history_update(r._h, 0.1, 0.9, 8.0, *nul) == E_STATE            # ... but an update needs a chunk
        # ... and goes stale on commit, set_camera, set_scene, set_shard and history_reset
        assert lib.rtiow_history_commit(r._h) == 0
        assert stale() == (E_STATE,) * 4
        for go_stale in (lambda: r.set_camera(cams["orbit"]), lambda: r.set_scene(rt.build_scene(3, 32)), lambda: r.history_reset(),
                         lambda: (r.set_shard(0, 1, 8), r.set_shard(0, 1, 8))):
            r.set_camera(cams["home"]); r.init_rng(1227); r.accumulate(1)
            r.history_update()
            assert lib.rtiow_read_history(r._h, None, None, npix) == 0
            go_stale()
            assert stale() == (E_STATE,) * 4
        # the base survives set_camera, reset_accumulation and init_rng; set_scene, set_shard and history_reset empty it
        for empties, change in ((False, lambda: r.set_camera(cams["orbit"])), (False, lambda: r.reset_accumulation()),
                                (True, lambda: r.set_scene(rt.build_scene(3, 32))), (True, lambda: r.set_shard(0, 1, 4)),
                                (True, lambda: r.history_reset())):
            r.set_camera(cams["home"]); r.init_rng(1227); r.accumulate(1)
            r.history_update(); r.history_commit()
            change()
            r.set_camera(cams["dolly"]); r.init_rng(1227); r.accumulate(1)
            assert (r.history_update() == 0) == empties, empties
    with rt.Renderer(0, 32) as r:                        # a sharded handle: none of it
        lib = r._lib
        begin(r, rt, 32, 3, cams["home"])
        r.set_shard(1, 3, 8); r.init_rng(1227)
        r.accumulate(2)
        p, nb = ctypes.c_void_p(), ctypes.c_size_t(0)
        assert lib.rtiow_history_reset(r._h) == E_STATE
        assert lib.rtiow_history_update(r._h, 0.1, 0.9, 8.0, *nul) == E_STATE
        assert lib.rtiow_history_commit(r._h) == E_STATE
        assert lib.rtiow_read_history(r._h, None, None, W * r.local_rows) == E_STATE
        assert lib.rtiow_history_device_ptr(r._h, ctypes.byref(p), ctypes.byref(nb)) == E_STATE
        assert lib.rtiow_denoise_history(r._h, 2, 1.0, 1.0, 1.0, 1.0, None) == E_STATE


# ---- 8. it helps

# scripts/history_probe.py measured, on this walk at the default parameters (profiles/history/history_probe.json, "orbit"):
#   q_t  = MSE(temporal) / MSE(noisy), q_dt = MSE(denoise_history) / MSE(denoise), per scene
# The test allows 15 % over the measured values: that covers run-to-run differences in which pixels lose their history at silhouettes.
Q_T = {1: 0.1995, 3: 0.1648}
Q_DT = {1: 0.3909, 3: 0.3713}


def test_it_helps(rt, capsys):
    got = {}
    for scene_id in (1, 3):
        got[scene_id] = quality(orbit_walk(rt, scene_id))
    with capsys.disabled():
        print("\nhistory over an 8-frame orbit, 4 spp per frame: {scene: (q_t, q_dt)} =", {k: (round(a, 4), round(b, 4)) for k, (a, b) in got.items()})
    for scene_id, (q_t, q_dt) in got.items():
        assert q_t < 1 and q_dt < 1, (scene_id, q_t, q_dt)
        assert q_t <= SLACK * Q_T[scene_id], (scene_id, q_t)
        assert q_dt <= SLACK * Q_DT[scene_id], (scene_id, q_dt)
