"""Variance-guided filtering of the temporal image on the GPU: rtiow_denoise_history_variance is
rtiow_denoise_variance with level 0 reading the temporal colour Cout and the plane V^0 -- the frame's measured variance scaled by the
update's blend weight alpha = n / Mout where the accumulation measured one, the spread of Cout's luminance over the (2r + 1)^2 window
elsewhere.  V^0 is defined operation by operation in T with plain * + - /, so the plane and the image are checked BIT FOR BIT against
tests/preview_model.py's temporal_noise_np, fed through its restatements of sections 10, 11 and 14."""
import ctypes

import numpy as np
import pytest

from tests.preview_drive import E_BADARG, E_STATE, INF, begin, history_defaults, move, moves, sample, state
from tests.preview_model import as_base, clipped_np, noise_classes, same_bits, temporal_noise_np, update_np, variance_filter_np, window_np

pytestmark = pytest.mark.gpu

RADII = (1, 2, 3)
SETTINGS = ((1, 1), (2, 3), (3, 5))                     # (variance_radius, levels): V^0 depends on the first alone, the levels on V^0 alone
CLIP = (1, 0.75)


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _sig(rt):
    a = rt.api
    return (a.HISTORY_SIGMA_VARIANCE, a.DENOISE_SIGMA_NORMAL, a.DENOISE_SIGMA_ALBEDO, a.DENOISE_SIGMA_DEPTH)


def _check(r, rt, C, M, n, adaptive, settings, where, sig=None):
    """The plane and the image of the handle's temporal image, which the caller has restated as (C, M), for every (radius, levels)."""
    sig = sig or _sig(rt)
    V = r.variance() if adaptive else None
    normal, albedo, depth = r.guides()
    planes = {}
    for radius, levels in settings:
        got = r.denoise_history_variance(levels, *sig, radius)
        v0 = r.history_variance()
        want_v0 = temporal_noise_np(C, M, n, V, radius)
        assert v0.dtype == r.dtype and np.isfinite(v0).all() and (v0 >= 0).all(), (where, radius)
        assert same_bits(v0, want_v0), (where, radius, int((v0 != want_v0).sum()))
        assert np.isfinite(got).all(), (where, radius, levels)
        assert same_bits(got, variance_filter_np(C, want_v0, normal, albedo, depth, levels, *sig)), (where, radius, levels)
        assert same_bits(r.read_denoised(), got), (where, radius, levels)
        planes[radius] = v0
    return planes


def _budget_mix(r, params):
    """Never sampled, one sample and three samples in one frame: one more sample where the planned history is short of 6, then two more
    where history and count together are short of 3 (min_samples = 0: a pixel with enough history is not sampled at all)."""
    r.history_plan(*params)
    r.accumulate_budget(1, 6.0, 0)
    r.accumulate_budget(2, 3.0, 0)


# ---- 1. exactness: moves x updates x settings

@pytest.mark.parametrize("clipped", [False, True], ids=["plain", "clipped"])
@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_plane_and_image_are_exact(rt, prec, scene_id, clipped):
    """The orbit is sampled by the budget (the three classes in one frame), the dolly in plain chunks (every pixel spatial), the roll
    adaptively (every pixel measured)."""
    W, H = 203, 117                                     # not a multiple of 16 in either direction
    params = history_defaults(rt)
    cams = moves(rt, prec, W, H)

    def update(r, cam, cur, base, where):
        if clipped:
            r.history_update_clipped(*CLIP, *params)
            want = clipped_np(cam, cur, base, params, *CLIP)
            C, M = want["C"], want["M"]
        else:
            r.history_update(*params)
            C, M, _ = update_np(cam, cur, base, *params)
        rgb, length = r.history()
        assert same_bits(rgb, C) and same_bits(length, M), where
        return C, M

    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, cams["home"])
        sample(r, True)
        cur = state(r, True)
        C, M = update(r, cams["home"], cur, None, "home")
        _check(r, rt, C, M, cur["n"], True, SETTINGS[:1], (prec, scene_id, clipped, "home"))
        r.history_commit()
        base = as_base(cams["home"], cur, C, M)
        for name in ("orbit", "dolly", "roll"):
            where = (prec, scene_id, clipped, name)
            move(r, cams[name], 1228)
            adaptive = name != "dolly"
            if name == "orbit":
                _budget_mix(r, params)
            else:
                sample(r, adaptive)
            cur = state(r, adaptive)
            C, M = update(r, cams[name], cur, base, where)
            planes = _check(r, rt, C, M, cur["n"], adaptive, SETTINGS, where)
            assert float(M.max()) > float(cur["n"].max()), where                     # history was carried: alpha < 1 somewhere
            if name == "roll":
                assert (cur["n"] >= 2).all() and same_bits(planes[1], planes[3]), where        # measured: the radius plays no part
                assert (planes[1] < r.variance()).any(), where
            if name == "dolly":
                assert not same_bits(planes[1], planes[2]) and not same_bits(planes[2], planes[3]), where
            if name == "orbit":
                got = noise_classes(cur["n"], window_np(C, M, 1)[1])
                print(where, got)
                for cls, count in got.items():
                    assert count >= 0.01 * W * H, (where, cls, got)


# ---- 2. mixed pixel classes

@pytest.mark.parametrize("prec", [32, 64])
def test_mixed_pixel_classes(rt, prec):
    W, H = 203, 117
    params = history_defaults(rt)
    cams = moves(rt, prec, W, H)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 3, cams["home"])
        sample(r, True)                                 # every pixel 4 or 8 samples
        cur = state(r, True)
        c0, m0, _ = update_np(cams["home"], cur, None, *params)
        r.history_update(*params); r.history_commit()
        base = as_base(cams["home"], cur, c0, m0)
        move(r, cams["orbit"], 1228)
        _budget_mix(r, params)
        cur = state(r, True)
        r.history_update(*params)
        C, M, _ = update_np(cams["orbit"], cur, base, *params)
        got = noise_classes(cur["n"], window_np(C, M, 1)[1])
        print(prec, got)
        for cls, count in got.items():
            assert count >= 0.01 * W * H, (prec, cls, got)
        planes = _check(r, rt, C, M, cur["n"], True, SETTINGS, (prec, "budget"))
        measured = cur["n"] >= 2
        assert same_bits(np.ascontiguousarray(planes[1][measured]), np.ascontiguousarray(planes[3][measured]))
        assert (planes[1][~measured] > 0).any() and (planes[1][measured] > 0).any()


@pytest.mark.parametrize("prec", [32, 64])
def test_nobody_sampled(rt, prec):
    """An adaptive accumulation in which no pixel was sampled: every pixel is spatial, a disoccluded one (Mout = 0) counts in no window
    and Cout is the gathered history."""
    W, H = 64, 40
    params = history_defaults(rt)
    cams = moves(rt, prec, W, H)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 3, cams["home"])
        r.accumulate(3)
        cur = state(r, False)
        c0, m0, _ = update_np(cams["home"], cur, None, *params)
        r.history_update(*params); r.history_commit()
        base = as_base(cams["home"], cur, c0, m0)
        move(r, cams["orbit"], 1228)
        _, active = r.accumulate_adaptive(4, 0.0, min_samples=0, max_samples=3)     # 4 more samples would pass max_samples
        assert active == 0
        cur = state(r, True)
        assert (cur["n"] == 0).all()
        r.history_update(*params)
        C, M, carried = update_np(cams["orbit"], cur, base, *params)
        assert 0.5 * W * H < carried < W * H             # some pixels have Mout = 0
        planes = _check(r, rt, C, M, cur["n"], True, SETTINGS, (prec, "nobody"))
        assert (planes[1] > 0).any()


# ---- 3. spatial everywhere, by two routes

@pytest.mark.parametrize("prec", [32, 64])
def test_spatial_everywhere_by_two_routes(rt, prec):
    """Plain chunks keep no second moment, and one sample measures nothing: both take the spatial estimate everywhere, and for equal
    counts both have the same temporal image, so the same plane and the same filtered image."""
    W, H = 150, 90
    params = history_defaults(rt)
    cams = moves(rt, prec, W, H)
    out = {}
    for route in ("plain", "one sample"):
        with rt.Renderer(0, prec) as r:
            begin(r, rt, prec, 1, cams["home"])
            r.accumulate(4)
            cur = state(r, False)
            c0, m0, _ = update_np(cams["home"], cur, None, *params)
            r.history_update(*params); r.history_commit()
            base = as_base(cams["home"], cur, c0, m0)
            move(r, cams["orbit"], 1228)
            adaptive = route == "one sample"
            if adaptive:
                r.accumulate_with_variance(1)
            else:
                r.accumulate(1)
            cur = state(r, adaptive)
            assert (cur["n"] == 1).all()
            r.history_update(*params)
            C, M, _ = update_np(cams["orbit"], cur, base, *params)
            planes = _check(r, rt, C, M, cur["n"], adaptive, SETTINGS, (prec, route))
            if adaptive:
                assert (r.variance() == 0).all()
            for radius in RADII:
                assert same_bits(planes[radius], window_np(C, M, radius)[0]), (prec, route, radius)
            out[route] = (C, planes, r.read_denoised())
        if not adaptive:                                 # more plain chunks: still spatial
            with rt.Renderer(0, prec) as r:
                begin(r, rt, prec, 1, cams["orbit"])
                r.accumulate(2); r.accumulate(3)
                cur = state(r, False)
                r.history_update(*params)
                C, M, _ = update_np(cams["orbit"], cur, None, *params)
                _check(r, rt, C, M, cur["n"], False, SETTINGS[1:2], (prec, "plain, no base"))
    assert same_bits(out["plain"][0], out["one sample"][0])
    for radius in RADII:
        assert same_bits(out["plain"][1][radius], out["one sample"][1][radius]), (prec, radius)
    assert same_bits(out["plain"][2], out["one sample"][2])


# ---- 4. cross-checks that need no new restatement

@pytest.mark.parametrize("prec", [32, 64])
def test_an_empty_base_gives_denoise_variance(rt, prec):
    """No base: Mout = n, alpha = 1 and Cout = c, so the plane is variance() and the image denoise_variance()'s, bit for bit."""
    W, H = 203, 117
    cams = moves(rt, prec, W, H)
    sig = (3.0, 0.1, 0.2, 0.05)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 1, cams["home"])
        sample(r, True)                                 # every pixel 4 or 8 samples: all measured
        for clipped in (False, True):
            if clipped:
                assert r.history_update_clipped() == (0, 0)
            else:
                assert r.history_update() == 0
            rgb, length = r.history()
            assert same_bits(rgb, r.read_linear()) and same_bits(length, r.adaptive_state()[0].astype(r.dtype))
            for levels in (1, 3, 5):
                got = r.denoise_history_variance(levels, *sig, 2)
                assert same_bits(r.history_variance(), r.variance()), (prec, clipped, levels)
                assert same_bits(got, r.denoise_variance(levels, *sig)), (prec, clipped, levels)


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("prec", [32, 64])
def test_infinite_sigma_variance_is_denoise_history(rt, prec, adaptive):
    W, H = 150, 90
    cams = moves(rt, prec, W, H)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 3, cams["home"])
        sample(r, adaptive)
        r.history_update(); r.history_commit()
        move(r, cams["orbit"], 7)
        sample(r, adaptive)
        assert r.history_update_clipped()[0] > 0
        for levels, guides in ((1, (0.1, 0.2, 0.05)), (3, (0.3, INF, 1.0)), (5, (0.1, 0.2, 0.05)), (5, (INF, INF, INF))):
            want = r.denoise_history(levels, INF, *guides)
            got = r.denoise_history_variance(levels, INF, *guides, 1)
            assert same_bits(got, want), (prec, adaptive, levels, guides)
        assert not same_bits(r.denoise_history_variance(5, 4.0, 0.1, 0.2, 0.05, 1), want)


# ---- 5. tile and frame edges

@pytest.mark.parametrize("frame", [(1, 1), (1, 37), (37, 1), (5, 3), (15, 17), (16, 16), (17, 16), (33, 31), (63, 65)], ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("prec", [32, 64])
def test_windows_at_tile_and_frame_edges(rt, prec, frame):
    """The same camera twice with independent noise, plain chunks: every pixel is spatial, and the windows cross the frame's edge, cross
    workgroup borders and, in the small frames, exceed the frame."""
    W, H = frame
    params = history_defaults(rt)
    cam = rt.camera_look(prec, W, H, 1, 10)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 3, cam)
        r.accumulate(3)
        cur = state(r, False)
        c0, m0, _ = update_np(cam, cur, None, *params)
        r.history_update(*params); r.history_commit()
        base = as_base(cam, cur, c0, m0)
        move(r, cam, 1228)
        r.accumulate(3)
        cur = state(r, False)
        r.history_update(*params)
        C, M, _ = update_np(cam, cur, base, *params)
        planes = _check(r, rt, C, M, cur["n"], False, ((1, 2), (2, 2), (3, 2)), (prec, frame))
        for radius in RADII:
            k = window_np(C, M, radius)[1]
            assert int(k.max()) == min(W, 2 * radius + 1) * min(H, 2 * radius + 1), (prec, frame, radius)
            if W * H == 1:
                assert (planes[radius] == 0).all()           # k = 1: no estimate
            else:
                assert int(k.min()) >= 2 and (planes[radius] > 0).any(), (prec, frame, radius)


# ---- 6. nothing else moved

@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("prec", [32, 64])
def test_the_call_leaves_everything_else_alone(rt, prec, adaptive):
    W, H = 128, 72
    cams = moves(rt, prec, W, H)

    def run(with_call):
        out = []
        with rt.Renderer(0, prec) as r:
            begin(r, rt, prec, 1, cams["home"])
            sample(r, adaptive)
            r.history_update(); r.history_commit()
            move(r, cams["orbit"])
            sample(r, adaptive, calls=1)
            r.history_plan()
            r.history_update_clipped()
            if with_call:
                r.denoise_history_variance()
                r.denoise_history_variance(3, 2.0, 0.2, 0.3, 0.4, 3, sync=False)
                r.synchronize()
                assert same_bits(r.read_denoised(), r.denoise_history_variance(3, 2.0, 0.2, 0.3, 0.4, 3))
                assert r.history_variance().shape == (H, W)
            out += [r.read_framebuffer(), r.read_linear(), r.history_plan_lengths(), *r.guides(), *r.history()]
            out += [r.denoise_history(), r.denoise()]
            if adaptive:
                out += [*r.adaptive_state(), r.variance(), r.denoise_variance()]
            if adaptive:
                r.accumulate_adaptive(4, 0.0, min_samples=8)
            else:
                r.accumulate(3)
            out += [r.read_framebuffer(), r.read_linear(), np.array([r.accumulated_samples])]
            if adaptive:
                out += list(r.adaptive_state())
            out += [np.array([r.history_update()]), *r.history()]                   # the base and the guides it is gathered by
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
    nan = float("nan")
    ok = (5, 4.0, 1.0, 1.0, 1.0, 1)
    with rt.Renderer(0, 32) as r:
        lib = r._lib
        call = lambda *a: lib.rtiow_denoise_history_variance(r._h, *a, None)
        read = lambda n=npix: lib.rtiow_read_history_variance(r._h, None, n)
        begin(r, rt, 32, 3, cams["home"])
        assert call(*ok) == E_STATE and read() == E_STATE                                # no temporal image
        r.accumulate_with_variance(2)
        assert call(*ok) == E_STATE and read() == E_STATE                                # a chunk, still no update
        r.history_update()
        assert read() == E_STATE                                                         # an update, the call has not run
        for levels in (0, 9, -1):
            assert call(levels, 4.0, 1.0, 1.0, 1.0, 1) == E_BADARG, levels
        for bad in (0.0, -1.0, nan):
            for pos in range(4):
                sig = [1.0] * 4
                sig[pos] = bad
                assert call(5, *sig, 1) == E_BADARG, (bad, pos)
        for radius in (0, 4, -1):
            assert call(5, 4.0, 1.0, 1.0, 1.0, radius) == E_BADARG, radius
        assert read() == E_STATE and lib.rtiow_read_denoised(r._h, None, 0) == E_STATE   # the refused calls wrote nothing
        ms = ctypes.c_float(-1)
        assert lib.rtiow_denoise_history_variance(r._h, 5, nan, 1.0, 1.0, 1.0, 1, ctypes.byref(ms)) == E_BADARG and ms.value == 0.0
        assert lib.rtiow_denoise_history_variance(r._h, *ok, ctypes.byref(ms)) == 0 and ms.value > 0
        assert read() == 0
        for bad in (npix + 1, npix - 1, 0):
            assert read(bad) == E_BADARG, bad
        v0 = r.history_variance()
        assert v0.shape == (H, W) and r.read_denoised().shape == (H, W, 3)
        assert call(1, INF, INF, INF, INF, 3) == 0 and call(8, 1e-3, 1e-3, 1e-3, 1e-3, 1) == 0       # the ends of the ranges; asynchronous
        # a failing call leaves the plane readable as it was
        assert call(5, 4.0, 1.0, 1.0, 1.0, 0) == E_BADARG and same_bits(r.history_variance(), v0)
        # a later update makes the plane stale, whichever update
        r.history_update()
        assert read() == E_STATE and call(*ok) == 0 and read() == 0
        r.history_update_clipped()
        assert read() == E_STATE and call(*ok) == 0 and read() == 0
        # a chunk after the update: alpha would no longer be the update's.  The temporal image itself stays readable.
        v0 = r.history_variance()
        r.accumulate_with_variance(1)
        assert call(*ok) == E_STATE
        assert lib.rtiow_read_history(r._h, None, None, npix) == 0 and read() == 0 and same_bits(r.history_variance(), v0)
        r.history_update()
        assert call(*ok) == 0
        r.reset_accumulation()                                                           # ... and a reset
        assert call(*ok) == E_STATE and lib.rtiow_read_history(r._h, None, None, npix) == 0
        r.accumulate(2)                                                                  # plain chunks now
        assert call(*ok) == E_STATE
        r.history_update()
        assert call(*ok) == 0 and read() == 0
        r.init_rng(5)                                                                    # init_rng resets the accumulation
        assert call(*ok) == E_STATE
        # the plane goes stale wherever the temporal image does
        for go_stale in (lambda: r.set_camera(cams["orbit"]), lambda: r.history_commit(), lambda: r.set_scene(rt.build_scene(3, 32)),
                         lambda: r.history_reset(), lambda: (r.set_shard(0, 1, 8), r.set_shard(0, 1, 8))):
            r.set_camera(cams["home"]); r.init_rng(1227); r.accumulate_with_variance(2)
            r.history_update()
            assert call(*ok) == 0 and read() == 0
            go_stale()
            assert call(*ok) == E_STATE and read() == E_STATE
        # stale guides are rendered first
        r.set_camera(cams["home"]); r.init_rng(1227); r.accumulate_with_variance(2)
        r.history_update()
        r.set_guide_mode(rt.api.GUIDES_SPECULAR)
        assert lib.rtiow_read_guides(r._h, None, None, None, npix) == E_STATE
        assert call(*ok) == 0 and lib.rtiow_read_guides(r._h, None, None, None, npix) == 0
    with rt.Renderer(0, 32) as r:                        # a sharded handle: not this either
        begin(r, rt, 32, 3, cams["home"])
        r.set_shard(1, 3, 8); r.init_rng(1227)
        r.accumulate_with_variance(2)
        assert r._lib.rtiow_denoise_history_variance(r._h, *ok, None) == E_STATE
        assert r._lib.rtiow_read_history_variance(r._h, None, W * r.local_rows) == E_STATE


def test_the_filter_guides_of_the_guide_mode(rt):
    """In RTIOW_GUIDES_SPECULAR mode the levels steer by the chain's guides, as rtiow_denoise_variance's do."""
    prec, W, H = 32, 150, 90
    cams = moves(rt, prec, W, H)
    sig = _sig(rt)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 1, cams["home"])
        r.set_guide_mode(rt.api.GUIDES_SPECULAR)
        r.accumulate_with_variance(4)
        r.history_update(); r.history_commit()
        move(r, cams["orbit"], 7)
        r.accumulate_with_variance(4)
        r.history_update()
        rgb, length = r.history()
        n = r.adaptive_state()[0]
        normal, albedo, depth, _ = r.filter_guides()
        assert not same_bits(normal, r.guides()[0])
        got = r.denoise_history_variance(3, *sig, 1)
        v0 = temporal_noise_np(rgb, length, n, r.variance(), 1)
        assert same_bits(r.history_variance(), v0)
        assert same_bits(got, variance_filter_np(rgb, v0, normal, albedo, depth, 3, *sig))
