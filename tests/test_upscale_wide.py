"""Wide-support guided upscaling on the GPU: rtiow_upscale_wide writes rtiow_upscale's preview with the 4 x 4
traced pixels around every output pixel gathered under the cubic B-spline.  Every value is defined operation by operation in T with
plain * + - / and sqrt, so the image is checked BIT FOR BIT, every pixel, against tests/upscale_wide_model.py, whose inputs are the CPU
oracle's hits (the output pixels' and the traced pixels' guides and layers) and the colour the handle itself reads back.  The frames are
the smallest at which the kernel can go wrong: 1 x 1 (fifteen of sixteen taps outside), 2 x 3, 7 x 5, 33 x 17 (no multiple of a
workgroup's 16 x 16 output block at any factor, so footprints straddle workgroups and the last blocks are partial) and 64 x 40 (several
whole blocks each way)."""
import ctypes

import numpy as np
import pytest

from tests.preview_drive import E_BADARG, E_STATE, begin, move, moves, sample
from tests.preview_model import LATTICE, same_bits
from tests.test_edge_resolve import _budget_frame, start, view
from tests.upscale_drive import Cpu, _bits, _everything, check_guides, colour
from tests.upscale_drive import check as drive_check, model as drive_model
from tests.upscale_model import upscale_np
from tests.upscale_wide_model import DENOISED, HISTORY, INF, LINEAR, upscale_wide_np

pytestmark = pytest.mark.gpu

FRAMES = ((1, 1), (2, 3), (7, 5), (33, 17), (64, 40))
ODD, BIG = FRAMES[3], FRAMES[4]
# (factor, sigma_normal, sigma_albedo, sigma_depth, use_coverage); the layers alternate between the two lattices
SETTINGS = ((2, 0.3, 0.1, 0.5, 1), (3, 0.1, INF, 0.1, 1), (4, 0.3, 0.1, INF, 0), (2, INF, INF, INF, 0), (4, INF, 0.1, 0.5, 1), (3, 0.3, INF, INF, 0))
GRIDS = (2, 2, 2, 4, 4, 4)


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


@pytest.fixture(scope="module")
def cpu(rt, oracle):
    return Cpu(rt, oracle)


def model(r, *args, np_model=upscale_wide_np, **kwargs):
    """The model's (image, covered) of a setting on what the handle holds (upscale_drive.model)."""
    return drive_model(np_model, r, *args, **kwargs)


def check(r, *args, **kwargs):
    """upscale_wide() against tests/upscale_wide_model.py (upscale_drive.check)."""
    return drive_check(r.upscale_wide, upscale_wide_np, r, *args, **kwargs)


# ---- 1. every source

@pytest.mark.parametrize("scene_id", [1, 3, LATTICE])
@pytest.mark.parametrize("prec", [32, 64])
def test_upscaled_accumulation_is_exact(rt, cpu, prec, scene_id):
    for W, H in FRAMES:
        cam = view(rt, prec, scene_id, W, H)
        where = (prec, scene_id, W, H)
        with rt.Renderer(0, prec) as r:
            start(r, rt, prec, scene_id, cam)
            r.accumulate(3)
            check_guides(r, cpu, prec, scene_id, cam, where)
            outs, grid = {}, 0
            for setting, G in zip(SETTINGS, GRIDS):
                if G != grid:
                    r.render_coverage(G)
                    grid = G
                outs[setting] = check(r, cpu, prec, scene_id, cam, LINEAR, setting, G, where)
            if (W, H) == BIG:                                # the edge-stop and the share both decide pixels of this frame
                first = SETTINGS[0]
                r.render_coverage(GRIDS[0])
                no_stop = check(r, cpu, prec, scene_id, cam, LINEAR, (first[0], INF, INF, INF, 1), GRIDS[0], where)
                no_share = check(r, cpu, prec, scene_id, cam, LINEAR, first[:4] + (0,), GRIDS[0], where)
                again = check(r, cpu, prec, scene_id, cam, LINEAR, first, GRIDS[0], where)
                assert same_bits(again, outs[first]) and not same_bits(again, no_stop) and not same_bits(again, no_share), where
                # the asynchronous form: the same image, read after the fact
                r.upscale_wide(3, LINEAR, sync=False)
                assert r.upscale_wide(*first[:1], LINEAR, *first[1:], sync=False) is None
                assert same_bits(r.read_upscaled(), again), where


@pytest.mark.parametrize("scene_id", [1, 3, LATTICE])
@pytest.mark.parametrize("prec", [32, 64])
def test_upscaled_denoised_image_is_exact_before_and_after_the_resolve(rt, cpu, prec, scene_id):
    for W, H in (FRAMES[1], ODD, BIG):
        cam = view(rt, prec, scene_id, W, H)
        where = (prec, scene_id, W, H)
        with rt.Renderer(0, prec) as r:
            start(r, rt, prec, scene_id, cam)
            r.accumulate(3)
            r.render_coverage(2)
            plain = r.denoise()
            for setting in SETTINGS[:3]:
                check(r, cpu, prec, scene_id, cam, DENOISED, setting, 2, where + ("denoise",))
            rewritten = r.resolve_edges()
            resolved = r.read_denoised()
            for setting in (SETTINGS[0], SETTINGS[5]):
                check(r, cpu, prec, scene_id, cam, DENOISED, setting, 2, where + ("resolve_edges",))
            assert same_bits(r.read_denoised(), resolved), where
            if (W, H) == BIG:
                assert rewritten > 0 and not same_bits(resolved, plain), where


@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_upscaled_temporal_image_is_exact(rt, cpu, prec, scene_id):
    """HISTORY after a commit at the home view and an update at the orbit view, whose disoccluded pixels carry the frame's samples alone."""
    for W, H in (FRAMES[2], ODD):
        cams = moves(rt, prec, W, H)
        where = (prec, scene_id, W, H)
        with rt.Renderer(0, prec) as r:
            begin(r, rt, prec, scene_id, cams["home"])
            sample(r, False)
            r.history_update(); r.history_commit()
            move(r, cams["orbit"], 1228)
            r.accumulate(3)
            r.history_update()
            r.render_coverage(4)
            for setting in (SETTINGS[0], SETTINGS[1], SETTINGS[2]):
                check(r, cpu, prec, scene_id, cams["orbit"], HISTORY, setting, 4, where)


@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_taps_without_a_sample_are_skipped(rt, cpu, prec, scene_id):
    """A budget chunk leaves pixels with 0 samples: LINEAR skips those taps, HISTORY takes what the base carried there."""
    for W, H in (ODD, BIG):
        where = (prec, scene_id, W, H)
        with rt.Renderer(0, prec) as r:
            cam = _budget_frame(r, rt, prec, scene_id, W, H)
            counts = r.adaptive_state()[0]
            if (W, H) == BIG:
                assert (counts == 0).any() and (counts > 0).any(), where
            r.render_coverage(2)
            for setting in (SETTINGS[0], SETTINGS[3], SETTINGS[4]):
                out = check(r, cpu, prec, scene_id, cam, LINEAR, setting, 2, where, adaptive=True)
            assert np.isfinite(out).all(), where
            r.history_update()
            check(r, cpu, prec, scene_id, cam, HISTORY, SETTINGS[0], 2, where)


# ---- 2. scene sources, shards, stale inputs

@pytest.mark.parametrize("prec", [32, 64])
def test_every_scene_source(rt, cpu, prec):
    W, H = ODD
    for scene_id in (1, 3):
        cam = view(rt, prec, scene_id, W, H)
        images = []
        for source in (rt.SCENE_LDS, rt.SCENE_SCALAR, rt.SCENE_LDS_EXACT, rt.SCENE_GRID):
            with rt.Renderer(0, prec) as r:
                start(r, rt, prec, scene_id, cam, source)
                r.accumulate(2)
                r.render_coverage(4)
                images.append(check(r, cpu, prec, scene_id, cam, LINEAR, SETTINGS[1], 4, (prec, scene_id, "scene source", source)))
        assert all(same_bits(images[0], img) for img in images[1:])


def test_a_sharded_handle_is_refused(rt):
    W, H, prec = ODD + (32,)
    with rt.Renderer(0, prec) as r:
        start(r, rt, prec, 3, rt.camera(prec, W, H, 1, 10), shard=(1, 3, 3))
        r.accumulate(2)
        for source in (DENOISED, LINEAR, HISTORY):
            assert r._lib.rtiow_upscale_wide(r._h, 2, source, 0.3, 0.1, 0.5, 1, None, None) == E_STATE, source
            text = r._lib.rtiow_last_error_string(r._h).decode()
            assert "sharded" in text and "rtiow_upscale_wide" in text
        assert r._lib.rtiow_read_upscaled(r._h, None, 0) == E_STATE


@pytest.mark.parametrize("prec", [32, 64])
def test_stale_guides_and_layers_are_rendered_inside_the_call(rt, cpu, prec):
    W, H, scene_id = ODD + (3,)
    cam = view(rt, prec, scene_id, W, H)
    _, N, A, Z = cpu.hits(prec, scene_id, cam, 1)
    for flag in (0, 1):
        with rt.Renderer(0, prec) as r:
            lib, h = r._lib, r._h
            start(r, rt, prec, scene_id, cam)
            r.set_camera(cam); r.init_rng(1227)               # a new camera: guides and layers are stale
            r.accumulate(2)
            assert lib.rtiow_read_guides(h, None, None, None, W * H) == E_STATE and lib.rtiow_read_coverage(h, None, None, None, None, W * H) == E_STATE
            c, has = colour(r, LINEAR)
            ms, n = ctypes.c_float(-1), ctypes.c_uint64(7)
            assert lib.rtiow_upscale_wide(h, 2, LINEAR, 0.3, 0.1, 0.5, flag, ctypes.byref(ms), ctypes.byref(n)) == 0
            assert ms.value > 0
            assert lib.rtiow_read_guides(h, None, None, None, W * H) == 0                       # rendered by the call
            assert lib.rtiow_read_coverage(h, None, None, None, None, W * H) == (0 if flag else E_STATE)   # ... the layers only when asked for
            G = 4                                            # the C call was never told a lattice
            ids, counts = cpu.layers(prec, scene_id, cam, G)
            want, covered = upscale_wide_np(c, has, N, A, Z, ids, counts, G * G, cpu.hits(prec, scene_id, cam, 2), 2, 0.3, 0.1, 0.5, flag)
            assert same_bits(r.read_upscaled(), want) and n.value == int(covered.sum()) and (n.value > 0) == bool(flag), (prec, flag)
            if flag:
                assert same_bits(r.coverage()[0], ids) and same_bits(r.coverage()[1], counts)


# ---- 3. the two calls share a buffer; refusals, staleness, isolation

@pytest.mark.parametrize("prec", [32, 64])
def test_the_readers_serve_whichever_call_ran_last(rt, cpu, prec):
    W, H, scene_id = ODD + (3,)
    cam = view(rt, prec, scene_id, W, H)
    with rt.Renderer(0, prec) as r:
        start(r, rt, prec, scene_id, cam)
        r.accumulate(2)
        r.render_coverage(2)
        narrow_setting, wide_setting = SETTINGS[1], SETTINGS[0]       # factors 3 and 2: the buffer changes its size between them
        narrow, narrow_covered = model(r, cpu, prec, scene_id, cam, LINEAR, narrow_setting, 2, np_model=upscale_np)
        wide, _ = model(r, cpu, prec, scene_id, cam, LINEAR, wide_setting, 2)
        call = lambda f, s: f(s[0], LINEAR, *s[1:])
        assert call(r.upscale, narrow_setting) == int(narrow_covered.sum())
        assert same_bits(r.read_upscaled(), narrow)
        check(r, cpu, prec, scene_id, cam, LINEAR, wide_setting, 2, ("after upscale",))
        assert r.upscaled_device_ptr()[1] == wide.nbytes
        call(r.upscale, narrow_setting)
        assert same_bits(r.read_upscaled(), narrow) and r.upscaled_device_ptr()[1] == narrow.nbytes
        same_factor = (narrow_setting[0],) + wide_setting[1:]
        assert not same_bits(check(r, cpu, prec, scene_id, cam, LINEAR, same_factor, 2, ("same factor",)), narrow)


def test_refusals_leave_the_handle_as_it_was(rt):
    W, H, prec = ODD + (32,)
    nan = float("nan")
    good = (2, DENOISED, 0.3, 0.1, 0.5, 1)
    with rt.Renderer(0, prec) as r:
        lib, h = r._lib, r._h
        call = lambda *a: lib.rtiow_upscale_wide(h, *a, None, None)
        text = lambda: lib.rtiow_last_error_string(h).decode()
        ptr, size = ctypes.c_void_p(), ctypes.c_size_t(0)
        readers = lambda: (lib.rtiow_read_upscaled(h, None, 0), lib.rtiow_upscaled_device_ptr(h, ctypes.byref(ptr), ctypes.byref(size)))
        for source in (DENOISED, LINEAR, HISTORY):            # before scene and camera
            assert call(2, source, 0.3, 0.1, 0.5, 1) == E_STATE and "rtiow_set_scene" in text(), source
        assert readers() == (E_STATE, E_STATE)
        assert call(7, DENOISED, 0.3, 0.1, 0.5, 1) == E_BADARG                                   # arguments come first
        start(r, rt, prec, 3, rt.camera(prec, W, H, 1, 10))
        assert call(*good) == E_STATE and "before rtiow_denoise" in text()                      # DENOISED before a filter
        assert call(2, LINEAR, 0.3, 0.1, 0.5, 1) == E_STATE and "no chunk" in text()            # LINEAR without a chunk
        assert call(2, HISTORY, 0.3, 0.1, 0.5, 1) == E_STATE and "no temporal image" in text()  # HISTORY without a temporal image
        assert readers() == (E_STATE, E_STATE)                                                  # the refused calls wrote nothing
        r.accumulate(2)
        r.denoise()
        assert call(2, HISTORY, 0.3, 0.1, 0.5, 1) == E_STATE
        assert r.upscale_wide(3, use_coverage=1) > 0
        before = _bits(r)
        ms, n = ctypes.c_float(-1), ctypes.c_uint64(7)
        bad = [(F,) + good[1:] for F in (-1, 0, 1, 5, 8)] + [(2, s) + good[2:] for s in (-1, 3, 9)]
        bad += [good[:k] + (v,) + good[k + 1:] for k in (2, 3, 4) for v in (0.0, -1.0, nan)] + [good[:5] + (f,) for f in (-1, 2, 3)]
        for args in bad:
            assert lib.rtiow_upscale_wide(h, *args, ctypes.byref(ms), ctypes.byref(n)) == E_BADARG and ms.value == 0 and n.value == 0, args
            assert "rtiow_upscale_wide" in text(), args
        r.history_update(); r.history_commit()
        assert call(2, HISTORY, 0.3, 0.1, 0.5, 1) == E_STATE and "no temporal image" in text()  # the commit took it
        r.reset_accumulation()
        assert call(2, LINEAR, 0.3, 0.1, 0.5, 1) == E_STATE                                     # a reset: no chunk
        r.accumulate(2)                                                                         # ... the same two samples again
        after = _bits(r)
        for name in before:
            assert same_bits(before[name], after[name]), name
        assert readers()[1] == 0 and size.value == before["upscaled"].nbytes and ptr.value


def test_the_image_goes_stale_with_a_new_frame_only(rt, cpu):
    W, H, prec, scene_id = ODD + (32, 3)
    cam = view(rt, prec, scene_id, W, H)
    with rt.Renderer(0, prec) as r:
        lib, h = r._lib, r._h
        ptr, size = ctypes.c_void_p(), ctypes.c_size_t(0)
        stale = lambda: (lib.rtiow_read_upscaled(h, None, 0), lib.rtiow_upscaled_device_ptr(h, ctypes.byref(ptr), ctypes.byref(size))) == (E_STATE, E_STATE)
        start(r, rt, prec, scene_id, cam)
        r.accumulate(2)
        r.render_coverage(2)
        image = check(r, cpu, prec, scene_id, cam, LINEAR, SETTINGS[1], 2, ("survives",))
        events = (lambda: r.accumulate(1), lambda: r.denoise(), lambda: r.resolve_edges(), lambda: r.history_update(), lambda: r.history_commit(),
                  lambda: r.reset_accumulation(), lambda: r.init_rng(7), lambda: r.accumulate(1), lambda: r.set_guide_mode(rt.GUIDES_SPECULAR),
                  lambda: r.set_guide_lens(2), lambda: r.render_guides(), lambda: r.render_coverage(4), lambda: r.set_guide_lens(0),
                  lambda: r.set_guide_mode(rt.GUIDES_FIRST_HIT))
        for k, event in enumerate(events):
            event()
            assert not stale() and same_bits(r.read_upscaled(), image), k
        scene = rt.build_scene(scene_id, prec)
        for name, change in (("set_camera", lambda: r.set_camera(cam)), ("set_scene", lambda: r.set_scene(scene)), ("edit_scene", lambda: r.edit_scene(scene)),
                             ("set_shard", lambda: r.set_shard(0, 1, 8))):
            assert not stale(), name
            change()
            assert stale(), name
            r.init_rng(1227)
            r.accumulate(2)
            assert stale(), name                              # nothing but an upscale brings it back
            r.render_coverage(2)
            assert same_bits(check(r, cpu, prec, scene_id, cam, LINEAR, SETTINGS[1], 2, (name,)), image), name


def test_the_guides_are_the_first_hit_buffers_in_every_guide_mode(rt, cpu):
    W, H, prec, scene_id = ODD + (32, 3)
    cam = view(rt, prec, scene_id, W, H)
    with rt.Renderer(0, prec) as r:
        start(r, rt, prec, scene_id, cam)
        r.accumulate(2)
        r.render_coverage(2)
        image = check(r, cpu, prec, scene_id, cam, LINEAR, SETTINGS[0], 2, ("first hit",))
        r.set_guide_mode(rt.GUIDES_SPECULAR); r.set_guide_lens(2)
        assert same_bits(check(r, cpu, prec, scene_id, cam, LINEAR, SETTINGS[0], 2, ("specular, lens",)), image)


@pytest.mark.parametrize("prec", [32, 64])
def test_the_call_touches_nothing_but_its_own_image(rt, prec):
    W, H = BIG
    states = []
    for upscale in (False, True):
        with rt.Renderer(0, prec) as r:
            _budget_frame(r, rt, prec, 3, W, H)
            r.history_update()
            r.history_plan()
            r.denoise_history()
            r.render_coverage(2)
            if upscale:
                counts = [r.upscale_wide(F, source, use_coverage=flag) for F, source, flag in ((2, DENOISED, 1), (4, LINEAR, 1), (3, HISTORY, 1), (2, HISTORY, 0))]
                assert min(counts[:3]) > 0 and counts[3] == 0
                assert r.read_upscaled().shape == (2 * H, 2 * W, 3)
            s = _everything(r)
            r.accumulate_budget(2, INF, 0)                   # the next chunk's bits
            s["next_fb"], s["next_linear"] = r.read_framebuffer(), r.read_linear()
            states.append(s)
    for name in states[0]:
        assert same_bits(states[0][name], states[1][name]), name
