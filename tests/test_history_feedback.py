"""Recurrent history on the GPU: rtiow_history_commit_filtered replaces the colour of the temporal image by
one level of the a-trous filter at step 1 -- over the pixels that hold samples, steered by the filter guides, blended by `feedback` --
before it becomes the base, and rtiow_read_history_base reads the base back.  Every value is defined operation by operation in T with
plain * + - /, so the base is checked BIT FOR BIT against tests/preview_model.py's feedback_np."""
import ctypes

import numpy as np
import pytest

from tests.preview_drive import E_BADARG, E_STATE, INF, begin, filter_state, guide_sigmas, history_defaults, move, moves, sample, state
from tests.preview_model import as_base, clipped_np, feedback_np, same_bits, update_np

pytestmark = pytest.mark.gpu

PAIRS = ((0.1, 1.0), (0.3, 0.5))                            # (sigma_color, feedback)
CLIP = (1, 0.75)


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _commit_and_check(r, rt, pair, where):
    """Commit the temporal image the handle holds through the filter at `pair` and compare the base with the restatement; returns it."""
    C, M = r.history()
    N, A, Z = filter_state(r)
    sig = (pair[0],) + guide_sigmas(rt)
    ms = r.history_commit_filtered(sig[0], *sig[1:], feedback=pair[1])
    assert ms > 0, where
    rgb, length = r.history_base()
    want, want_m = feedback_np(C, M, N, A, Z, sig, pair[1])
    assert same_bits(length, want_m) and same_bits(length, M), where
    assert same_bits(rgb, want), (where, int((rgb != want).any(axis=-1).sum()))
    return C, M, rgb


def _update(r, rt, clipped, params):
    if clipped:
        return r.history_update_clipped(*CLIP, *params)[0]
    return r.history_update(*params)


# ---- 1. exactness

def _exact(rt, prec, scene_id, adaptive, specular):
    W, H = 203, 117                                     # not a multiple of 16 in either direction
    params = history_defaults(rt)
    cams = moves(rt, prec, W, H)
    for clipped in (False, True):
        for pair in PAIRS:
            where = (prec, scene_id, adaptive, specular, clipped, pair)
            with rt.Renderer(0, prec) as r:
                if specular:
                    r.set_guide_mode(rt.GUIDES_SPECULAR, 8, INF)
                begin(r, rt, prec, scene_id, cams["home"])
                sample(r, adaptive)
                home = state(r, adaptive)
                _update(r, rt, clipped, params)
                C0, M0, H0 = _commit_and_check(r, rt, pair, where + ("home",))      # the first commit of the handle: it allocates the base
                assert same_bits(C0, home["c"])
                base = as_base(cams["home"], home, H0, M0)
                move(r, cams["orbit"], 1228)
                sample(r, adaptive)
                cur = state(r, adaptive)
                count = _update(r, rt, clipped, params)
                assert count > 0.5 * W * H, where
                # the update gathers from the filtered base by the first-hit guides the commit kept, whatever the guide mode
                want = clipped_np(cams["orbit"], cur, base, params, *CLIP) if clipped else None
                want_c, want_m = (want["C"], want["M"]) if clipped else update_np(cams["orbit"], cur, base, *params)[:2]
                C, M = r.history()
                assert same_bits(M, want_m) and same_bits(C, want_c), where
                if specular:
                    fn, fa, fz = filter_state(r)
                    assert not same_bits(fn, cur["N"]) and not same_bits(fz, cur["t"]), where
                _, _, H1 = _commit_and_check(r, rt, pair, where + ("orbit",))
                assert not same_bits(H1, C), where                                  # the filter did something


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_filtered_commit_is_exact(rt, prec, scene_id, adaptive):
    _exact(rt, prec, scene_id, adaptive, False)


@pytest.mark.parametrize("prec", [32, 64])
def test_filtered_commit_is_exact_with_specular_guides(rt, prec):
    _exact(rt, prec, 3, False, True)


# ---- 2. the existing filter

@pytest.mark.parametrize("prec", [32, 64])
def test_feedback_one_is_a_level_of_denoise_history(rt, prec):
    """Every pixel is sampled, so every tap inside the frame counts, and feedback = 1 stores the filtered colour itself: its gamma has
    the bits of denoise_history(levels=1) at the same sigmas, taken just before the commit."""
    W, H = 150, 90
    cams = moves(rt, prec, W, H)
    sig = (0.5, 0.1, 0.1, 1.0)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 3, cams["home"])
        r.accumulate(4)
        r.history_update(); r.history_commit()
        move(r, cams["orbit"], 7)
        r.accumulate(4)
        assert r.history_update() > 0
        assert (r.history()[1] > 0).all()
        shown = r.denoise_history(1, *sig)
        r.history_commit_filtered(*sig, feedback=1.0)
        rgb, _ = r.history_base()
        gamma = np.zeros_like(rgb)
        gamma[rgb > 0] = np.sqrt(rgb[rgb > 0])
        assert same_bits(gamma, shown), prec
        assert same_bits(r.read_denoised(), shown)      # the commit left the denoised buffer alone


# ---- 3. tile and frame edges

@pytest.mark.parametrize("frame", [(1, 1), (1, 37), (37, 1), (5, 3), (15, 17), (16, 16), (17, 16), (33, 31), (63, 65)], ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("prec", [32, 64])
def test_tiles_at_tile_and_frame_edges(rt, prec, frame):
    """The same camera twice with independent noise: the halo exceeds the frame, crosses workgroup borders and is cut by the frame's edge."""
    W, H = frame
    params = history_defaults(rt)
    cam = rt.camera_look(prec, W, H, 1, 10)
    for pair in PAIRS:
        with rt.Renderer(0, prec) as r:
            begin(r, rt, prec, 3, cam)
            r.accumulate(3)
            r.history_update(*params); r.history_commit()
            move(r, cam, 1228)
            r.accumulate(3)
            assert r.history_update(*params) == W * H
            _commit_and_check(r, rt, pair, (prec, frame, pair))


# ---- 4. unsampled pixels

@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_unsampled_pixels_do_not_count(rt, prec, scene_id):
    W, H = 203, 117
    cams = moves(rt, prec, W, H)
    params = history_defaults(rt)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, cams["home"])
        r.accumulate(3)
        r.history_update(*params); r.history_commit()
        move(r, cams["orbit"], 1228)
        _, active = r.accumulate_adaptive(4, 0.0, min_samples=0, max_samples=3)     # 4 more samples would pass max_samples
        assert active == 0 and (r.adaptive_state()[0] == 0).all()
        r.history_update(*params)
        _, M = r.history()
        empty, held = M == 0, M > 0
        print("scene %d: M == 0 in %.1f %%, M > 0 in %.1f %%" % (scene_id, 100 * empty.mean(), 100 * held.mean()))
        assert empty.mean() >= 0.01 and held.mean() >= 0.5
        near = np.zeros_like(empty)
        pe = np.pad(empty, 2)
        for dy in range(5):
            for dx in range(5):
                near |= pe[dy:dy + H, dx:dx + W]
        assert (held & near).any()                       # a pixel with samples has a pixel without in its window
        for pair in PAIRS[:1]:
            _, _, Hn = _commit_and_check(r, rt, pair, (prec, scene_id, pair))
            assert np.isfinite(Hn).all()
            assert not Hn[empty].any()


# ---- 5. a chain

@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("prec", [32, 64])
def test_a_chain_of_filtered_commits_is_exact(rt, prec, adaptive):
    W, H = 203, 117
    cams = moves(rt, prec, W, H)
    params = (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, 12.0)
    sig = (0.3,) + guide_sigmas(rt)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 3, cams["home"])
        base = None
        for k, name in enumerate(("home", "orbit", "dolly")):
            where = (prec, adaptive, name)
            if k:
                move(r, cams[name], 1227 + k)
            assert (r.history_plan(*params) > 0) == (k > 0)
            plan = r.history_plan_lengths()
            sample(r, adaptive)
            cur = state(r, adaptive)
            count = r.history_update(*params)
            C, M = r.history()
            want_c, want_m, want_count = update_np(cams[name], cur, base, *params)      # base: the restatement's own output
            assert same_bits(M, want_m) and same_bits(C, want_c) and count == want_count, where
            assert same_bits(M, plan + cur["n"].astype(r.dtype)), where
            N, A, Z = filter_state(r)
            r.history_commit_filtered(*sig, feedback=0.5)
            rgb, length = r.history_base()
            Hn, Mn = feedback_np(want_c, want_m, N, A, Z, sig, 0.5)
            assert same_bits(rgb, Hn) and same_bits(length, Mn) and same_bits(length, M), where
            base = as_base(cams[name], cur, Hn, Mn)
        assert float(base["M"].max()) > float(cur["n"].max())


# ---- 6. the plain commit

@pytest.mark.parametrize("prec", [32, 64])
def test_plain_commit_is_unchanged(rt, prec):
    W, H = 150, 90
    cams = moves(rt, prec, W, H)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, 1, cams["home"])
        for k, name in enumerate(("home", "orbit", "dolly")):
            if k:
                move(r, cams[name], 1227 + k)
            r.accumulate(3)
            r.history_update()
            C, M = r.history()
            if k == 1:
                r.history_commit_filtered()              # a filtered commit between two plain ones: the buffers keep their roles
                assert not same_bits(r.history_base()[0], C)
            else:
                r.history_commit()
                rgb, length = r.history_base()
                assert same_bits(rgb, C) and same_bits(length, M), (prec, name)


# ---- 7. nothing else moved

@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("prec", [32, 64])
def test_filtered_commit_leaves_everything_else_alone(rt, prec, adaptive):
    W, H = 128, 72
    cams = moves(rt, prec, W, H)

    def run(with_commit):
        out = []
        with rt.Renderer(0, prec) as r:
            begin(r, rt, prec, 1, cams["home"])
            sample(r, adaptive)
            r.history_update(); r.history_commit()
            move(r, cams["orbit"])
            sample(r, adaptive, calls=1)
            r.history_update()
            r.denoise_history(2)
            if with_commit:
                r.history_commit_filtered()
                npix = ctypes.c_size_t(W * H)
                assert r._lib.rtiow_read_history(r._h, None, None, npix) == E_STATE
                assert r._lib.rtiow_read_history_plan(r._h, None, npix) == E_STATE
            out += [r.read_framebuffer(), r.read_linear(), r.read_denoised()]
            if adaptive:
                out += list(r.adaptive_state())
            if adaptive:
                r.accumulate_adaptive(4, 0.0, min_samples=8)
            else:
                r.accumulate(3)
            out += [r.read_framebuffer(), r.read_linear(), np.array([r.accumulated_samples])]
            if adaptive:
                out += list(r.adaptive_state())
            r.init_rng(77)
            r.render()
            out += [r.read_framebuffer()]
        return out

    plain, touched = run(False), run(True)
    assert len(plain) == len(touched)
    for k, (a, b) in enumerate(zip(plain, touched)):
        assert same_bits(a, b), (prec, adaptive, k)


# ---- 8. states and error codes

def test_states_and_error_codes(rt):
    W, H = 96, 64
    npix = W * H
    cams = moves(rt, 32, W, H)
    nan = float("nan")
    good = (0.1, 0.1, 0.2, 0.05, 1.0)
    with rt.Renderer(0, 32) as r:
        lib = r._lib
        commit = lambda *a: lib.rtiow_history_commit_filtered(r._h, *a, None)
        read = lambda n=npix: lib.rtiow_read_history_base(r._h, None, None, n)
        begin(r, rt, 32, 3, cams["home"])
        assert commit(*good) == E_STATE and read() == E_STATE                            # no temporal image, no base
        r.accumulate(2)
        assert commit(*good) == E_STATE and read() == E_STATE                            # a chunk, but no update
        r.history_update()
        assert read() == E_STATE                                                         # an update alone makes no base
        r.history_commit()
        assert read() == 0 and read(npix + 1) == E_BADARG and read(0) == E_BADARG
        assert commit(*good) == E_STATE                                                  # the commit made the temporal image stale
        old = r.history_base()
        move(r, cams["orbit"], 1228)
        assert commit(*good) == E_STATE                                                  # a new camera: nothing to commit
        r.accumulate(2)
        assert commit(*good) == E_STATE
        r.history_update()
        before = r.history()
        for k in range(4):
            for bad in (0.0, -0.1, nan, -INF):
                args = list(good); args[k] = bad
                assert commit(*args) == E_BADARG, args
        for bad in (0.0, -0.5, 1.0000001, 2.0, nan, INF):
            assert commit(*good[:4], bad) == E_BADARG, bad
        ms = ctypes.c_float(-1)
        assert lib.rtiow_history_commit_filtered(r._h, *good[:4], nan, ctypes.byref(ms)) == E_BADARG and ms.value == 0.0
        # the refused calls left the temporal image readable and the old base in place ...
        after = r.history()
        assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
        kept = r.history_base()
        assert same_bits(kept[0], old[0]) and same_bits(kept[1], old[1])
        r.history_commit()                                                               # ... and a plain commit gives what it would have
        got = r.history_base()
        assert same_bits(got[0], before[0]) and same_bits(got[1], before[1])
        # the ends of the ranges, asynchronous (kernel_ms == NULL); every sigma off: the kernel of K over the pixels that count
        move(r, cams["dolly"], 1229); r.accumulate(2); r.history_update()
        C, M = r.history()
        N, A, Z = filter_state(r)
        assert commit(INF, INF, INF, INF, 1e-3) == 0
        r.synchronize()
        rgb, length = r.history_base()
        want, _ = feedback_np(C, M, N, A, Z, (INF,) * 4, 1e-3)
        assert same_bits(rgb, want) and same_bits(length, M)
        assert lib.rtiow_read_history(r._h, None, None, npix) == E_STATE                 # stale, as after a plain commit
        assert commit(*good) == E_STATE
        # stale guides are rendered by the call: a new guide mode between update and commit
        move(r, cams["roll"], 1230); r.accumulate(2); r.history_update()
        r.set_guide_mode(rt.GUIDES_SPECULAR, 8, INF)
        C, M = r.history()
        assert isinstance(r.history_commit_filtered(), float)
        rgb, _ = r.history_base()
        r.render_guides()
        N, A, Z = filter_state(r)
        a = rt.api
        sig = (a.HISTORY_FEEDBACK_SIGMA_COLOR, a.DENOISE_SIGMA_NORMAL, a.DENOISE_SIGMA_ALBEDO, a.DENOISE_SIGMA_DEPTH)
        assert same_bits(rgb, feedback_np(C, M, N, A, Z, sig, a.HISTORY_FEEDBACK)[0])
        # the base survives set_camera; set_scene, history_reset and set_shard empty it; a base of another frame size keeps its own
        r.set_camera(rt.camera_look(32, W + 10, H, 1, 10))
        assert read() == 0 and read((W + 10) * H) == E_BADARG
        r.history_reset()
        assert read() == E_STATE
    with rt.Renderer(0, 32) as r:                        # a sharded handle: neither call
        begin(r, rt, 32, 3, cams["home"])
        r.set_shard(1, 3, 8); r.init_rng(1227)
        r.accumulate(2)
        assert r._lib.rtiow_history_commit_filtered(r._h, *good, None) == E_STATE
        assert r._lib.rtiow_read_history_base(r._h, None, None, W * r.local_rows) == E_STATE


# ---- 9. the walks of scripts/history_feedback_probe.py

