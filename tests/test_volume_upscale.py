"""Guided upscaling on volume scenes on the GPU (-m gpu): rtiow_upscale_volume and rtiow_upscale_wide_volume against their twins on a second
handle set up alike, bit for bit (NaN against NaN), image and count, on scenes that fill a volume (tests/volume_scene.py: beyond a compute
unit's LDS the twin traces every output pixel's ray through the exact loop over every sphere, the _volume call through the three-axis grid
of rtiow_render_volume); on the cube also against the numpy models with the CPU oracle's hits; on frames smaller than a tile; with stale
guides and layers, interchanged with the twins and the _large twins on one handle, and with the twins' refusals and the grid's own behind
them.  In the manner of tests/test_large_upscale.py.  Traced frames are 48 x 32 and smaller."""
import contextlib
import ctypes

import numpy as np
import pytest

from tests import volume_scene
from tests.preview_model import same_bits
from tests.upscale_drive import Cpu, _bits, check_guides
from tests.upscale_drive import check as drive_check
from tests.upscale_model import DENOISED, HISTORY, INF, LINEAR, upscale_np
from tests.upscale_wide_model import upscale_wide_np

pytestmark = pytest.mark.gpu
BADARG, STATE = -1, -2
W, H, B, SEED = 48, 32, 8, 1227
SIGMAS = (0.3, 0.1, 0.5)
# method -> (C call, twin method, twin's C call)
CALLS = {
    "upscale_volume": ("rtiow_upscale_volume", "upscale", "rtiow_upscale"),
    "upscale_wide_volume": ("rtiow_upscale_wide_volume", "upscale_wide", "rtiow_upscale_wide"),
}
UNSUITED = "the volume grid does not suit this scene"


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
    """(the handle of the _volume calls, the handle of the twins), set up alike."""
    return _open(stack, rt, prec, scene, **kw), _open(stack, rt, prec, scene, **kw)


def _fill(r):
    """Every source of the upscalers through the existing calls: an adaptive accumulation whose counts differ (everyone 2 samples, then
    the frame's median error as the threshold), a filtered image and a temporal image."""
    r.accumulate_adaptive(2, 0.0, min_samples=2)
    r.accumulate_adaptive(2, float(np.median(r.adaptive_state()[1])), min_samples=2)
    r.denoise()
    r.history_update()


def _grid_in_stats(rt, volume):
    st, grid = volume.stats(), volume.volume_grid()
    assert st["scene_source"] == rt.SCENE_VOLUME_GRID
    assert (st["grid_nx"], st["grid_nz"], st["grid_registered"], st["grid_direct"]) == (grid["nx"], grid["nz"], grid["registered"], grid["direct"])


def _compare(rt, volume, twin, F, source, flag, where, kinds=CALLS):
    """Both _volume calls against their twins at one setting: the count and every pixel.  Returns the counts."""
    counts = []
    for method in kinds:
        n_volume = getattr(volume, method)(F, source, *SIGMAS, flag)
        _grid_in_stats(rt, volume)
        n_twin = getattr(twin, CALLS[method][1])(F, source, *SIGMAS, flag)
        got, want = volume.read_upscaled(), twin.read_upscaled()
        assert got.shape == want.shape == (F * twin.local_rows, F * twin.width, 3), (where, method)
        assert same_bits(got, want), (where, method, F, source, flag, int((got != want).any(axis=-1).sum()))
        assert n_volume == n_twin and (n_twin == 0 or flag), (where, method, F, source, flag, n_volume, n_twin)
        counts.append(n_twin)
    return counts


def _share(volume, twin, G):
    """The layers of lattice G on both handles (None: the share is off).  Returns use_coverage."""
    if G is None:
        return 0
    volume.render_coverage_volume(G); twin.render_coverage(G)
    return 1


# ---- 1. sources, factors, the share

@pytest.mark.parametrize("name,prec", [("cube18", 32), ("cube18", 64), ("cube_no_ground14", 32)])
def test_every_source_factor_and_share(rt, name, prec):
    """F = 2, 3, 4: the wide kernel's footprint sides 12, 10 and 8.  cube_no_ground(14): an empty direct list, so nothing lies in LDS in
    front of the kernels' own bytes, and sky pixels; it fits the LDS, so its twin reads it from there."""
    sc = volume_scene.cube(18, prec) if name == "cube18" else volume_scene.cube_no_ground(14, prec)
    with contextlib.ExitStack() as stack:
        volume, twin = _pair(stack, rt, prec, sc)
        _fill(volume); _fill(twin)
        if name == "cube18":
            assert twin.stats()["scene_source"] == rt.SCENE_SCALAR           # the scene really is beyond the LDS
        else:
            assert volume.volume_grid()["direct"] == 0 and (twin.guides()[2] == 0).any()
        assert len(np.unique(twin.adaptive_state()[0])) >= 2
        decided = 0
        for G in (None, 2, 4):
            flag = _share(volume, twin, G)
            for F in (2, 3, 4):
                for source in (DENOISED, LINEAR, HISTORY):
                    decided += sum(_compare(rt, volume, twin, F, source, flag, (name, prec, G)))
        assert decided > 0                                                    # the share did decide pixels
        out = twin.read_upscaled()
        assert float(np.asarray(out, np.float64).std()) > 0.01               # a picture, not a constant


@pytest.mark.parametrize("prec", [32, 64])
def test_the_numpy_models_on_the_cube(rt, cpu, prec):
    """upscale_drive.check with the oracle's hits: the output pixels', the traced pixels' guides and layers.  One configuration per kernel
    with the share and one without."""
    sc = dict(volume_scene.cube(18, prec), name="volume_cube_18")
    w, h = 24, 16
    cam = rt.camera(prec, w, h, 1, B)
    with contextlib.ExitStack() as stack:
        r = _open(stack, rt, prec, sc, cam=cam)
        r.accumulate_volume(3)
        r.render_guides_volume()
        check_guides(r, cpu, prec, sc, cam, (prec, "guides"))
        r.render_coverage_volume(2)
        for upscale, np_model, setting in ((r.upscale_volume, upscale_np, (2, 0.3, 0.1, 0.5, 1)), (r.upscale_volume, upscale_np, (3, 0.1, INF, 0.1, 0)),
                                           (r.upscale_wide_volume, upscale_wide_np, (2, 0.3, 0.1, 0.5, 1)),
                                           (r.upscale_wide_volume, upscale_wide_np, (3, 0.1, INF, 0.1, 0))):
            drive_check(upscale, np_model, r, cpu, prec, sc, cam, LINEAR, setting, 2, (prec, upscale.__name__))
            _grid_in_stats(rt, r)


# ---- 2. frames

@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (65, 9)])
def test_frames_smaller_than_a_tile(rt, w, h):
    for prec in (32, 64):
        sc = volume_scene.cube(18, prec)
        with contextlib.ExitStack() as stack:
            volume, twin = _pair(stack, rt, prec, sc, w=w, h=h)
            _fill(volume); _fill(twin)
            for G in (None, 2):
                flag = _share(volume, twin, G)
                for F in (2, 3, 4):
                    for source in (LINEAR, HISTORY):
                        _compare(rt, volume, twin, F, source, flag, (w, h, prec, G))


# ---- 3. stale inputs

@pytest.mark.parametrize("method", CALLS)
def test_stale_guides_and_layers_are_rendered_through_the_volume_grid(rt, method):
    call, _, twin_call = CALLS[method]
    for prec in (32, 64):
        sc = volume_scene.cube(18, prec)
        for flag in (0, 1):
            with contextlib.ExitStack() as stack:
                volume, twin = _pair(stack, rt, prec, sc)
                for r in (volume, twin):
                    r.accumulate(1); r.render_guides(); r.render_coverage(4)
                    r.set_camera(rt.camera(prec, W, H, 1, B)); r.init_rng(SEED)      # a new camera: guides and layers are stale
                    r.accumulate(2)
                    assert r._lib.rtiow_read_guides(r._h, None, None, None, W * H) == STATE
                    assert r._lib.rtiow_read_coverage(r._h, None, None, None, None, W * H) == STATE
                assert volume.stats()["scene_source"] == rt.SCENE_SCALAR
                out = {}
                for r, name in ((volume, call), (twin, twin_call)):
                    ms, n = ctypes.c_float(-1), ctypes.c_uint64(7)
                    assert getattr(r._lib, name)(r._h, 2, LINEAR, *SIGMAS, flag, ctypes.byref(ms), ctypes.byref(n)) == 0
                    assert ms.value > 0
                    assert r._lib.rtiow_read_guides(r._h, None, None, None, W * H) == 0                       # rendered by the call
                    assert r._lib.rtiow_read_coverage(r._h, None, None, None, None, W * H) == (0 if flag else STATE)
                    out[name] = (n.value, r.read_upscaled())
                _grid_in_stats(rt, volume)                                                                  # guides, layers and rays
                assert twin.stats()["scene_source"] == rt.SCENE_SCALAR
                assert out[call][0] == out[twin_call][0] and (out[call][0] > 0) == bool(flag), (prec, flag)
                assert same_bits(out[call][1], out[twin_call][1]), (prec, flag)
                assert all(same_bits(a, b) for a, b in zip(volume.guides(), twin.guides())), (prec, flag)
                if flag:                                     # the layers at the default lattice: the C call was never told one since the camera
                    assert all(same_bits(a, b) for a, b in zip(volume.coverage(), twin.coverage())), prec


# ---- 4. interchange

@pytest.mark.parametrize("prec", [32, 64])
def test_the_six_calls_interchange_on_one_handle(rt, prec):
    """The six upscale calls on a handle whose chunks and guides came through the volume grid: read_upscaled serves the last each time,
    equal to a fresh handle's that knows the twins alone."""
    sc = volume_scene.cube(18, prec)
    with contextlib.ExitStack() as stack:
        r, fresh = _pair(stack, rt, prec, sc)
        r.accumulate_volume(2); r.render_guides_volume(); r.render_coverage_volume(2)
        fresh.accumulate(2); fresh.render_guides(); fresh.render_coverage(2)
        r.denoise(); fresh.denoise()
        for method, twin_method, F in (("upscale_volume", "upscale", 2), ("upscale", "upscale", 3), ("upscale_wide_volume", "upscale_wide", 4),
                                       ("upscale_large", "upscale", 2), ("upscale_wide", "upscale_wide", 2), ("upscale_wide_large", "upscale_wide", 3),
                                       ("upscale_volume", "upscale", 4), ("upscale_wide_volume", "upscale_wide", 2)):
            n = getattr(r, method)(F, DENOISED, *SIGMAS, 1)
            assert n == getattr(fresh, twin_method)(F, DENOISED, *SIGMAS, 1) > 0, (prec, method)
            got = r.read_upscaled()
            assert got.shape == (F * H, F * W, 3) and same_bits(got, fresh.read_upscaled()), (prec, method)
            ptr, nbytes = r.upscaled_device_ptr()
            assert ptr and nbytes == got.nbytes
            if method.endswith("_volume"):
                _grid_in_stats(rt, r)
        # the image goes stale by the existing rule
        r.set_camera(rt.camera(prec, W, H, 1, B))
        assert r._lib.rtiow_read_upscaled(r._h, None, 0) == STATE


# ---- 5. refusals

def _c_call(r, name, *args):
    ms, n = ctypes.c_float(-1), ctypes.c_uint64(7)
    code = getattr(r._lib, name)(r._h, *args, ctypes.byref(ms), ctypes.byref(n))
    return code, r._lib.rtiow_last_error_string(r._h).decode(), ms.value, n.value


def _same_refusal(volume, twin, args, where, code=None):
    """Each _volume call refuses `args` as its twin does on a handle set up alike: the code, and the text under the new name."""
    for method, (call, _, twin_call) in CALLS.items():
        code_v, text_v, ms, n = _c_call(volume, call, *args)
        code_t, text_t, _, _ = _c_call(twin, twin_call, *args)
        assert code_v == code_t and code_v in ((BADARG, STATE) if code is None else (code,)), (where, method, code_v, code_t)
        assert call in text_v and text_v.replace(call, twin_call) == text_t and UNSUITED not in text_v, (where, method, text_v, text_t)
        assert ms == 0 and n == 0, (where, method)


def test_refusals_are_the_twins_under_the_new_name(rt):
    good = (2, DENOISED) + SIGMAS + (1,)
    nan = float("nan")
    bad = [(F,) + good[1:] for F in (-1, 0, 1, 5, 8)] + [(2, s) + good[2:] for s in (-1, 3, 9)]
    bad += [good[:k] + (v,) + good[k + 1:] for k in (2, 3, 4) for v in (0.0, -1.0, nan)] + [good[:5] + (f,) for f in (-1, 2, 3)]
    sc = volume_scene.cube(14, 32)
    with contextlib.ExitStack() as stack:
        volume, twin = stack.enter_context(rt.Renderer(0, 32)), stack.enter_context(rt.Renderer(0, 32))
        for source in (DENOISED, LINEAR, HISTORY):            # before scene and camera
            _same_refusal(volume, twin, (2, source) + SIGMAS + (1,), "nothing set", STATE)
        _same_refusal(volume, twin, bad[0], "arguments come first", BADARG)
        for r in (volume, twin):
            r.set_camera(rt.camera(32, W, H, 1, B)); r.set_scene(sc); r.init_rng(SEED)
        _same_refusal(volume, twin, good, "before a filter", STATE)
        _same_refusal(volume, twin, (2, LINEAR) + SIGMAS + (1,), "before a chunk", STATE)
        _same_refusal(volume, twin, (2, HISTORY) + SIGMAS + (1,), "before the history", STATE)
        assert volume._lib.rtiow_read_upscaled(volume._h, None, 0) == STATE  # the refused calls wrote nothing
        for r in (volume, twin):
            r.accumulate(2); r.denoise()
        _same_refusal(volume, twin, (2, HISTORY) + SIGMAS + (1,), "a filter, no history", STATE)
        assert volume.upscale_volume(3, use_coverage=1) == twin.upscale(3, use_coverage=1) > 0
        before = _bits(volume)
        for args in bad:
            _same_refusal(volume, twin, args, args, BADARG)
        after = _bits(volume)
        for name in before:
            assert same_bits(before[name], after[name]), name
    with contextlib.ExitStack() as stack:                     # a sharded handle
        volume, twin = _pair(stack, rt, 32, sc, shard=(1, 3, 8))
        for r in (volume, twin):
            r.accumulate(2)
        for source in (DENOISED, LINEAR, HISTORY):
            _same_refusal(volume, twin, (2, source) + SIGMAS + (1,), "sharded", STATE)
        assert "sharded" in volume._lib.rtiow_last_error_string(volume._h).decode()


def test_a_scene_the_grid_does_not_suit_is_refused_last_and_changes_nothing(rt):
    good = (2, DENOISED) + SIGMAS + (1,)
    with contextlib.ExitStack() as stack:
        r, twin = _pair(stack, rt, 32, volume_scene.ten_spheres())
        # the twin's own checks come first, in their order: arguments, then state
        _same_refusal(r, twin, (7,) + good[1:], "arguments first", BADARG)
        _same_refusal(r, twin, good, "before a filter", STATE)
        _same_refusal(r, twin, (2, LINEAR) + SIGMAS + (1,), "before a chunk", STATE)
        for h in (r, twin):
            h.accumulate(2); h.denoise(); h.history_update(); h.render_coverage(2)
        assert r.upscale(3, use_coverage=1) > 0
        assert not r.volume_grid()["usable"]
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
