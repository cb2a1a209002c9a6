"""Guided upscaling on large scenes on the GPU (-m gpu): rtiow_upscale_large and rtiow_upscale_wide_large against their twins on a second
handle set up alike, bit for bit (NaN against NaN), image and count, on scenes beyond a compute unit's LDS (tests/large_scene.py: the
twin traces every output pixel's ray through the exact loop over every sphere, the _large call through the device grid of
rtiow_render_large); on the lattice also against the numpy models with the CPU oracle's hits; on the edge scenes of the device grid,
on frames smaller than a tile, from the horizon and from beyond the grid's reach; with stale guides and layers, interchanged with the
twins on one handle, with the twins' refusals and the grid's own behind them, and with everything else of the handle left alone.
Traced frames are 48 x 32 and smaller."""
import contextlib
import ctypes
import math

import numpy as np
import pytest

from tests import large_scene
from tests.preview_model import same_bits
from tests.upscale_drive import Cpu, _bits, _everything, check_guides
from tests.upscale_drive import check as drive_check
from tests.upscale_model import DENOISED, HISTORY, INF, LINEAR, upscale_np
from tests.upscale_wide_model import upscale_wide_np

pytestmark = pytest.mark.gpu
BADARG, STATE = -1, -2
W, H, B, SEED = 48, 32, 8, 1227
SIGMAS = (0.3, 0.1, 0.5)
# method -> (C call, twin method, twin's C call)
CALLS = {
    "upscale_large": ("rtiow_upscale_large", "upscale", "rtiow_upscale"),
    "upscale_wide_large": ("rtiow_upscale_wide_large", "upscale_wide", "rtiow_upscale_wide"),
}
UNSUITED = "the device grid does not suit this scene"


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


@pytest.fixture(scope="module")
def cpu(rt, oracle):
    return Cpu(rt, oracle)


def _open(stack, rt, prec, scene, w=W, h=H, shard=None, cam=None, bounces=B):
    r = stack.enter_context(rt.Renderer(0, prec))
    r.set_camera(cam if cam is not None else rt.camera(prec, w, h, 1, bounces)); r.set_scene(scene)
    if shard:
        r.set_shard(*shard)
    r.init_rng(SEED)
    return r


def _pair(stack, rt, prec, scene, **kw):
    """(the handle of the _large calls, the handle of the twins), set up alike."""
    return _open(stack, rt, prec, scene, **kw), _open(stack, rt, prec, scene, **kw)


def _fill(r):
    """Every source of the upscalers through the existing calls: an adaptive accumulation whose counts differ (everyone 2 samples, then
    the frame's median error as the threshold), a filtered image and a temporal image."""
    r.accumulate_adaptive(2, 0.0, min_samples=2)
    r.accumulate_adaptive(2, float(np.median(r.adaptive_state()[1])), min_samples=2)
    r.denoise()
    r.history_update()


def _grid_in_stats(rt, large):
    st, grid = large.stats(), large.large_grid()
    assert st["scene_source"] == rt.SCENE_DEVICE_GRID
    assert (st["grid_nx"], st["grid_nz"], st["grid_registered"], st["grid_direct"]) == (grid["nx"], grid["nz"], grid["registered"], grid["direct"])


def _compare(rt, large, twin, F, source, flag, where, kinds=CALLS):
    """Both _large calls against their twins at one setting: the count and every pixel.  Returns the counts."""
    counts = []
    for method in kinds:
        n_large = getattr(large, method)(F, source, *SIGMAS, flag)
        _grid_in_stats(rt, large)
        n_twin = getattr(twin, CALLS[method][1])(F, source, *SIGMAS, flag)
        got, want = large.read_upscaled(), twin.read_upscaled()
        assert got.shape == want.shape == (F * twin.local_rows, F * twin.width, 3), (where, method)
        assert same_bits(got, want), (where, method, F, source, flag, int((got != want).any(axis=-1).sum()))
        assert n_large == n_twin and (n_twin == 0 or flag), (where, method, F, source, flag, n_large, n_twin)
        counts.append(n_twin)
    return counts


def _share(large, twin, G):
    """The layers of lattice G on both handles (None: the share is off).  Returns use_coverage."""
    if G is None:
        return 0
    large.render_coverage_large(G); twin.render_coverage(G)
    return 1


# ---- 1. sources and precisions

@pytest.mark.parametrize("n,prec", [(6000, 32), (6000, 64), (20000, 32)])
def test_every_source_factor_and_share_on_the_lattice(rt, n, prec):
    """F = 2, 3, 4: the wide kernel's footprint sides 12, 10 and 8."""
    sc = large_scene.lattice(n, prec)
    with contextlib.ExitStack() as stack:
        large, twin = _pair(stack, rt, prec, sc)
        _fill(large); _fill(twin)
        assert twin.stats()["scene_source"] == rt.SCENE_SCALAR               # the scene really is beyond the LDS
        assert len(np.unique(twin.adaptive_state()[0])) >= 2
        decided = 0
        for G in (None, 2, 4):
            flag = _share(large, twin, G)
            for F in (2, 3, 4):
                for source in (DENOISED, LINEAR, HISTORY):
                    decided += sum(_compare(rt, large, twin, F, source, flag, (n, prec, G)))
        assert twin.stats()["scene_source"] == rt.SCENE_SCALAR
        assert decided > 0                                                    # the share did decide pixels
        out = twin.read_upscaled()
        assert float(np.asarray(out, np.float64).std()) > 0.01               # a picture, not a constant


@pytest.mark.parametrize("prec", [32, 64])
def test_the_numpy_models_on_the_lattice(rt, cpu, prec):
    """upscale_drive.check with the oracle's hits: the output pixels', the traced pixels' guides and layers."""
    sc = dict(large_scene.lattice(6000, prec), name="large_lattice_6000")
    w, h = 24, 16
    cam = rt.camera(prec, w, h, 1, B)
    with contextlib.ExitStack() as stack:
        r = _open(stack, rt, prec, sc, cam=cam)
        r.accumulate_large(3)
        r.render_guides_large()
        check_guides(r, cpu, prec, sc, cam, (prec, "guides"))
        r.render_coverage_large(2)
        for upscale, np_model, setting in ((r.upscale_large, upscale_np, (2, 0.3, 0.1, 0.5, 1)), (r.upscale_large, upscale_np, (3, 0.1, INF, 0.1, 0)),
                                           (r.upscale_wide_large, upscale_wide_np, (2, 0.3, 0.1, 0.5, 1)),
                                           (r.upscale_wide_large, upscale_wide_np, (3, 0.1, INF, 0.1, 1))):
            drive_check(upscale, np_model, r, cpu, prec, sc, cam, LINEAR, setting, 2, (prec, upscale.__name__))
            _grid_in_stats(rt, r)
        r.denoise()
        drive_check(r.upscale_large, upscale_np, r, cpu, prec, sc, cam, DENOISED, (2, 0.3, 0.1, 0.5, 1), 2, (prec, "denoised"))
        drive_check(r.upscale_wide_large, upscale_wide_np, r, cpu, prec, sc, cam, DENOISED, (2, 0.3, 0.1, 0.5, 1), 2, (prec, "denoised, wide"))


# ---- 2. edge scenes

@pytest.mark.parametrize("name", ["equal_no_ground", "mixed_with_bad", "clusters"])
def test_edge_scenes(rt, name):
    """equal_no_ground: an empty direct list, so nothing lies in LDS in front of the kernels' own bytes; mixed_with_bad: a direct list of
    nine with NaN, inf and negative radii; clusters: long lists with exact duplicates.  These fit the LDS: the twin reads them from there.
    One bounce: mixed_with_bad is no scene for a picture, only for first hits."""
    for prec in (32, 64):
        sc = large_scene.edge_scene(name, prec)
        with contextlib.ExitStack() as stack:
            large, twin = _pair(stack, rt, prec, sc, bounces=1)
            for r in (large, twin):
                r.accumulate(2); r.denoise()
            direct = large.large_grid()["direct"]
            assert direct == {"equal_no_ground": 0, "mixed_with_bad": 9}.get(name, direct), (name, direct)
            for G in (None, 2):
                flag = _share(large, twin, G)
                for F in (2, 3, 4):
                    _compare(rt, large, twin, F, LINEAR, flag, (name, prec, G))
                _compare(rt, large, twin, 3, DENOISED, flag, (name, prec, G))
            assert (twin.guides()[2] > 0).any()
            if name == "equal_no_ground":
                assert (twin.guides()[2] == 0).any()                          # sky pixels as well


# ---- 3. frames

@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (13, 7)])
def test_frames_smaller_than_a_tile(rt, w, h):
    """Neither F W nor F H is a multiple of 8 or 16 (but 4 x 13 of 4, of neither 8 nor 16)."""
    for prec in (32, 64):
        sc = large_scene.lattice(6000, prec)
        with contextlib.ExitStack() as stack:
            large, twin = _pair(stack, rt, prec, sc, w=w, h=h)
            _fill(large); _fill(twin)
            for G in (None, 2):
                flag = _share(large, twin, G)
                for F in (2, 3, 4):
                    for source in (LINEAR, HISTORY):
                        _compare(rt, large, twin, F, source, flag, (w, h, prec, G))


def _looking(rt, prec, sc, where):
    """A camera at the horizon -- half a unit above the ground, looking level across the lattice: sky rays, slab misses and walks in one
    wave -- or one farther from the scene's centre than the grid's rfar, whose waves take the exact loop."""
    ctr = large_scene.centre(sc)
    if where == "horizon":
        return rt.camera_look(prec, W, H, 1, B, lookfrom=(ctr[0] + 30.0, 0.5, ctr[2] + 7.0), lookat=(ctr[0], 0.5, ctr[2]), vfov=40.0)
    with rt.Renderer(0, prec) as probe:
        probe.set_scene(sc)
        rfar = probe.large_grid()["rfar"]
    assert rfar > 0
    d = np.array([1.0, 0.15, 0.3]) / np.linalg.norm([1.0, 0.15, 0.3])
    dist = 1.5 * rfar
    lookfrom = tuple(float(v) for v in ctr + dist * d)
    assert np.linalg.norm(np.array(lookfrom) - ctr) > rfar
    return rt.camera_look(prec, W, H, 1, B, lookfrom=lookfrom, lookat=tuple(float(v) for v in ctr), vfov=2 * math.degrees(math.atan(40.0 / dist)),
                          focus_dist=dist)


@pytest.mark.parametrize("where", ["horizon", "beyond_rfar"])
def test_cameras_at_the_horizon_and_beyond_the_grids_reach(rt, where):
    for prec in (32, 64):
        sc = large_scene.lattice(6000, prec)
        cam = _looking(rt, prec, sc, where)
        with contextlib.ExitStack() as stack:
            large, twin = _pair(stack, rt, prec, sc, cam=cam)
            _fill(large); _fill(twin)
            depth = twin.guides()[2]
            assert (depth > 0).any(), (where, prec)
            if where == "horizon":
                assert (depth == 0).any(), prec                               # sky
            for G in (None, 4):
                flag = _share(large, twin, G)
                for F in (2, 3):
                    for source in (DENOISED, LINEAR):
                        _compare(rt, large, twin, F, source, flag, (where, prec, G))


# ---- 4. stale inputs

@pytest.mark.parametrize("method", CALLS)
def test_stale_guides_and_layers_are_rendered_through_the_grid(rt, method):
    call, _, twin_call = CALLS[method]
    for prec in (32, 64):
        sc = large_scene.lattice(6000, prec)
        for flag in (0, 1):
            with contextlib.ExitStack() as stack:
                large, twin = _pair(stack, rt, prec, sc)
                for r in (large, twin):
                    r.accumulate(1); r.render_guides(); r.render_coverage(4)
                    r.set_camera(rt.camera(prec, W, H, 1, B)); r.init_rng(SEED)      # a new camera: guides and layers are stale
                    r.accumulate(2)
                    assert r._lib.rtiow_read_guides(r._h, None, None, None, W * H) == STATE
                    assert r._lib.rtiow_read_coverage(r._h, None, None, None, None, W * H) == STATE
                assert large.stats()["scene_source"] == rt.SCENE_SCALAR
                out = {}
                for r, name in ((large, call), (twin, twin_call)):
                    ms, n = ctypes.c_float(-1), ctypes.c_uint64(7)
                    assert getattr(r._lib, name)(r._h, 2, LINEAR, *SIGMAS, flag, ctypes.byref(ms), ctypes.byref(n)) == 0
                    assert ms.value > 0
                    assert r._lib.rtiow_read_guides(r._h, None, None, None, W * H) == 0                       # rendered by the call
                    assert r._lib.rtiow_read_coverage(r._h, None, None, None, None, W * H) == (0 if flag else STATE)
                    out[name] = (n.value, r.read_upscaled())
                _grid_in_stats(rt, large)                                                                   # guides, layers and rays
                assert twin.stats()["scene_source"] == rt.SCENE_SCALAR
                assert out[call][0] == out[twin_call][0] and (out[call][0] > 0) == bool(flag), (prec, flag)
                assert same_bits(out[call][1], out[twin_call][1]), (prec, flag)
                assert all(same_bits(a, b) for a, b in zip(large.guides(), twin.guides())), (prec, flag)
                if flag:                                     # the layers at the default lattice: the C call was never told one since the camera
                    assert all(same_bits(a, b) for a, b in zip(large.coverage(), twin.coverage())), prec


# ---- 5. interchange

@pytest.mark.parametrize("prec", [32, 64])
def test_the_four_calls_interchange_on_one_handle(rt, prec):
    """upscale_large, upscale, upscale_wide_large on a handle whose chunks and guides came through the grid: read_upscaled serves the
    last each time, equal to a fresh handle's that knows the twins alone."""
    sc = large_scene.lattice(6000, prec)
    with contextlib.ExitStack() as stack:
        r, fresh = _pair(stack, rt, prec, sc)
        r.accumulate_large(2); r.render_guides_large(); r.render_coverage_large(2)
        fresh.accumulate(2); fresh.render_guides(); fresh.render_coverage(2)
        r.denoise(); fresh.denoise()
        for method, twin_method, F in (("upscale_large", "upscale", 2), ("upscale", "upscale", 3), ("upscale_wide_large", "upscale_wide", 4),
                                       ("upscale_wide", "upscale_wide", 2), ("upscale_large", "upscale", 4)):
            n = getattr(r, method)(F, DENOISED, *SIGMAS, 1)
            assert n == getattr(fresh, twin_method)(F, DENOISED, *SIGMAS, 1) > 0, (prec, method)
            got = r.read_upscaled()
            assert got.shape == (F * H, F * W, 3) and same_bits(got, fresh.read_upscaled()), (prec, method)
            ptr, nbytes = r.upscaled_device_ptr()
            assert ptr and nbytes == got.nbytes
        # the image goes stale by the existing rule
        r.set_camera(rt.camera(prec, W, H, 1, B))
        assert r._lib.rtiow_read_upscaled(r._h, None, 0) == STATE


# ---- 6. refusals

def _c_call(r, name, *args):
    ms, n = ctypes.c_float(-1), ctypes.c_uint64(7)
    code = getattr(r._lib, name)(r._h, *args, ctypes.byref(ms), ctypes.byref(n))
    return code, r._lib.rtiow_last_error_string(r._h).decode(), ms.value, n.value


def _same_refusal(large, twin, args, where, code=None):
    """Each _large call refuses `args` as its twin does on a handle set up alike: the code, and the text under the new name."""
    for method, (call, _, twin_call) in CALLS.items():
        code_l, text_l, ms, n = _c_call(large, call, *args)
        code_t, text_t, _, _ = _c_call(twin, twin_call, *args)
        assert code_l == code_t and code_l in ((BADARG, STATE) if code is None else (code,)), (where, method, code_l, code_t)
        assert call in text_l and text_l.replace(call, twin_call) == text_t and UNSUITED not in text_l, (where, method, text_l, text_t)
        assert ms == 0 and n == 0, (where, method)


def test_refusals_are_the_twins_under_the_new_name(rt):
    good = (2, DENOISED) + SIGMAS + (1,)
    nan = float("nan")
    bad = [(F,) + good[1:] for F in (-1, 0, 1, 5, 8)] + [(2, s) + good[2:] for s in (-1, 3, 9)]
    bad += [good[:k] + (v,) + good[k + 1:] for k in (2, 3, 4) for v in (0.0, -1.0, nan)] + [good[:5] + (f,) for f in (-1, 2, 3)]
    sc = large_scene.lattice(6000, 32)
    with contextlib.ExitStack() as stack:
        large, twin = stack.enter_context(rt.Renderer(0, 32)), stack.enter_context(rt.Renderer(0, 32))
        for source in (DENOISED, LINEAR, HISTORY):            # before scene and camera
            _same_refusal(large, twin, (2, source) + SIGMAS + (1,), "nothing set", STATE)
        _same_refusal(large, twin, bad[0], "arguments come first", BADARG)
        for r in (large, twin):
            r.set_camera(rt.camera(32, W, H, 1, B)); r.set_scene(sc); r.init_rng(SEED)
        _same_refusal(large, twin, good, "before a filter", STATE)
        _same_refusal(large, twin, (2, LINEAR) + SIGMAS + (1,), "before a chunk", STATE)
        _same_refusal(large, twin, (2, HISTORY) + SIGMAS + (1,), "before the history", STATE)
        assert large._lib.rtiow_read_upscaled(large._h, None, 0) == STATE    # the refused calls wrote nothing
        for r in (large, twin):
            r.accumulate(2); r.denoise()
        _same_refusal(large, twin, (2, HISTORY) + SIGMAS + (1,), "a filter, no history", STATE)
        assert large.upscale_large(3, use_coverage=1) == twin.upscale(3, use_coverage=1) > 0
        before = _bits(large)
        for args in bad:
            _same_refusal(large, twin, args, args, BADARG)
        after = _bits(large)
        for name in before:
            assert same_bits(before[name], after[name]), name
    with contextlib.ExitStack() as stack:                     # a sharded handle
        large, twin = _pair(stack, rt, 32, sc, shard=(1, 3, 8))
        for r in (large, twin):
            r.accumulate(2)
        for source in (DENOISED, LINEAR, HISTORY):
            _same_refusal(large, twin, (2, source) + SIGMAS + (1,), "sharded", STATE)
        assert "sharded" in large._lib.rtiow_last_error_string(large._h).decode()


def test_a_scene_the_grid_does_not_suit_is_refused_last_and_changes_nothing(rt):
    good = (2, DENOISED) + SIGMAS + (1,)
    with contextlib.ExitStack() as stack:
        r, twin = _pair(stack, rt, 32, large_scene.ten_spheres())
        # the twin's own checks come first, in their order: arguments, then state
        _same_refusal(r, twin, (7,) + good[1:], "arguments first", BADARG)
        _same_refusal(r, twin, good, "before a filter", STATE)
        _same_refusal(r, twin, (2, LINEAR) + SIGMAS + (1,), "before a chunk", STATE)
        for h in (r, twin):
            h.accumulate(2); h.denoise(); h.history_update(); h.render_coverage(2)
        assert r.upscale(3, use_coverage=1) > 0
        assert not r.large_grid()["usable"]
        before, guides, layers = _bits(r), r.guides(), r.coverage()
        for method, (call, twin_method, twin_call) in CALLS.items():
            for source in (DENOISED, LINEAR, HISTORY):
                code, text, ms, n = _c_call(r, call, 2, source, *SIGMAS, 1)
                assert code == BADARG and text.count(call) == 1 and text.endswith("use " + twin_call) and UNSUITED in text, (method, text)
                assert ms == 0 and n == 0
            with pytest.raises(Exception) as e:
                getattr(r, method)(2, DENOISED, *SIGMAS, 1)
            assert e.value.code == BADARG and UNSUITED in str(e.value)
            _same_refusal(r, twin, (5,) + good[1:], "arguments before the grid", BADARG)
        after = _bits(r)
        for name in before:
            assert same_bits(before[name], after[name]), name
        assert all(same_bits(a, b) for a, b in zip(guides + layers, r.guides() + r.coverage()))
        assert r.read_upscaled().shape == (3 * H, 3 * W, 3)                  # the earlier image stays readable
        assert r.upscale(2, use_coverage=1) > 0 and r.upscale_wide(2, use_coverage=1) > 0      # ... and the twins do upscale the scene


# ---- 7. nothing else moves

def _session(r, rt, prec):
    """An adaptive base at the home view, then a budget chunk at a second view, a temporal image, its plan and filter, the layers."""
    home = rt.camera(prec, W, H, 1, B)
    away = rt.camera_look(prec, W, H, 1, B, lookfrom=(13.5, 2.1, 3.1))
    r.accumulate_adaptive(2, 0.0, min_samples=2)
    r.accumulate_adaptive(2, float(np.median(r.adaptive_state()[1])), min_samples=2)
    r.history_update(); r.history_commit()
    r.set_camera(away); r.init_rng(SEED + 1)
    r.history_plan()
    r.accumulate_budget(2, 6.0, 0)
    r.history_update()
    r.history_plan()
    r.denoise_history()
    r.render_coverage(2)
    return home


@pytest.mark.parametrize("prec", [32, 64])
def test_the_calls_touch_nothing_but_the_upscaled_image(rt, prec):
    sc = large_scene.lattice(6000, prec)
    states = []
    with contextlib.ExitStack() as stack:
        fresh = _open(stack, rt, prec, sc)
        fresh.render(0)
        want_render = fresh.read_framebuffer()
        for large in (False, True):
            r = _open(stack, rt, prec, sc)
            home = _session(r, rt, prec)
            if large:
                counts = [getattr(r, method)(F, source, use_coverage=flag) for method in CALLS
                          for F, source, flag in ((2, DENOISED, 1), (4, LINEAR, 1), (3, HISTORY, 1), (2, HISTORY, 0))]
                assert min(counts[:3] + counts[4:7]) > 0 and counts[3] == counts[7] == 0
                assert r.read_upscaled().shape == (2 * H, 2 * W, 3)
                _grid_in_stats(rt, r)
            s = _everything(r)
            r.accumulate_budget(2, INF, 0)                   # the next chunk's bits
            s["next_fb"], s["next_linear"] = r.read_framebuffer(), r.read_linear()
            r.set_camera(home); r.init_rng(SEED)
            r.render(0)                                      # and a render() after them: a fresh handle's
            assert r.stats()["scene_source"] == rt.SCENE_SCALAR
            s["render"] = r.read_framebuffer()
            assert same_bits(s["render"], want_render), (prec, large)
            states.append(s)
    for name in states[0]:
        assert same_bits(states[0][name], states[1][name]), name
