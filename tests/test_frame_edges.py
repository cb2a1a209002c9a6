"""The preview chain and the render at the edges of frame, camera and sample count.

The numpy restatements of tests/preview_model.py are run here on the inputs that tests/test_denoise.py, tests/test_denoise_variance.py
and tests/test_history.py never feed them: frames of one pixel, one column, one row, below and around an 8 x 8 guide tile, a 16 x 16 filter
workgroup and the sorted schedule's 4096-pixel threshold (section A); cameras inside a sphere, straight above, grazing, far outside the
grid, facing the sky, and history (the update, the plan and the clipped update, which share one gather) across moves that put pixels
behind the base camera, off its frame, on its edge and onto other surfaces (B); accumulations in which nobody, or everybody exactly once, was sampled (C); frames whose hand-out order does not fit
row << 16 | column (D).  Everything is compared BIT FOR BIT.  Section E, not marked gpu, shows on the CPU oracle alone that the cases
reach what they are for.

Class counts of section E as obtained (scene 3, fp32, base = the reference view, default parameters; behind / off-frame / edge-gather /
in-frame rejected / carried; edge overlaps the last two):

    48 x 32   orbit25 0/551/32/284/701   tele 0/0/0/6/1530   zoomout 0/1152/32/5/379   near 0/0/5/0/1536   roll 0/68/74/24/1444
              opposite 292/88/5/1009/147   elsewhere 0/1536/0/0/0
    80 x 64   orbit25 0/2160/34/1008/1952   opposite 834/245/8/3753/288   zoomout 0/3840/140/3/1277
    1 x 1     zoomout 0/0/1/0/1   opposite 0/0/1/1/0        1 x 37    tele 0/0/37/0/37   opposite 3/0/33/34/0
    37 x 1    orbit25 12/2/23/23/0   tele 0/0/23/1/36       5 x 3     orbit25 0/3/6/3/9   opposite 3/0/4/10/2
    8 x 8     roll 0/0/16/9/55   opposite 10/3/1/49/2       9 x 9     zoomout 0/56/16/0/25   opposite 13/2/0/66/0
    15 x 17   roll 0/2/30/2/251                             16 x 16   roll 0/0/28/2/254   17 x 16   roll 0/2/30/2/268
    65536 x 2 (vfov 0.004, base the same view, a step of 13 columns along the camera's u axis)   0/16/65649/8/131048
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from tests.conftest import compact
from tests.preview_drive import E_BADARG, E_STATE, INF, begin, check_against_err, check_clipped, check_update, move, orbit, run_mixed, state
from tests.preview_model import as_base, dot, filter_np, gamma, guides_np, plan_np, reproject, same_bits, update_np, variance_filter_np, vec
from tests.test_grid_plan import _plan

SIG = (0.5, 0.1, 0.1, 1.0)                                  # denoise: colour, normal, albedo, depth
VSIG_ON, VSIG_OFF = (4.0, 0.1, 0.2, 0.05), (INF, 0.1, 0.2, 0.05)  # denoise_variance: the colour term on and off
LOOSE = (0.0, -1.0, INF)                                    # history_update at the ends of its ranges
B = 8                                                       # bounce limit of sections A to C
_begin = functools.partial(begin, sched=2)                  # every handle here sets RTIOW_SCHED_SORTED before its RNG

# (W, H): smallest; thin; below a guide tile; a guide tile and one over; around a filter workgroup; the LDS halo ends at the frame;
# either side of the sorted schedule's threshold
FRAMES = [(1, 1), (1, 37), (37, 1), (5, 3), (8, 8), (9, 9), (15, 17), (16, 16), (17, 16), (32, 48), (63, 65), (64, 64)]
THIN_OR_TINY = [f for f in FRAMES if f[0] * f[1] < 4095]
PLACEMENT_FRAMES = [(48, 32), (80, 64)]                     # 80 x 64: a multiple of 16 both ways, and large enough to be ranked

# rt.camera_look arguments; the reference view is camera_look()
PLACEMENTS = {
    "inside_glass": dict(lookfrom=(0, 1, 0.3), lookat=(4, 1, 0)),
    "inside_ground": dict(lookfrom=(3, -2, 3), lookat=(0, -1, 0)),
    "straight_down": dict(lookfrom=(0, 30, 0), vup=(0, 0, -1)),
    "grazing": dict(lookfrom=(13, 0.02, 3), lookat=(0, 0.02, 0)),
    "far_tele": dict(lookfrom=(260, 40, 60), vfov=1, focus_dist=270),
    "wide": dict(lookfrom=(3, 1, 2), lookat=(0, 0.5, 0), vfov=120),
    "all_sky": dict(lookat=(26, 40, 6)),
    "no_lens": dict(defocus_angle=0),
    "large_lens": dict(defocus_angle=5),
}
MOVES = {
    "orbit25": dict(lookfrom=orbit(25)),
    "tele": dict(vfov=11),
    "zoomout": dict(vfov=40),
    "near": dict(lookfrom=(6.5, 1, 1.5)),
    "roll": dict(vup=(0.5, 0.87, 0)),
    "opposite": dict(lookfrom=(-13, 2, -3)),
    "elsewhere": dict(lookat=(0, 0, 14)),
}
# section D: a real picture of the scene on 65536 x 2, and the same view stepped sideways along its own u axis (13 columns)
NARROW = dict(vfov=0.004)
_U = (3 / math.sqrt(178), 0.0, -13 / math.sqrt(178))
NARROW_STEP = dict(vfov=0.004, lookfrom=tuple(a + 0.0045 * u for a, u in zip((13.0, 2.0, 3.0), _U)), lookat=tuple(0.0045 * u for u in _U))


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _id(frame):
    return "%dx%d" % frame


_ORACLE = {}


def _oracle_image(rt, oracle, prec, scene_id, W, H, S, bounces, **look):
    """The oracle's image of a camera_look view: computed once per configuration, shared, never written."""
    key = (prec, scene_id, W, H, S, bounces, tuple(sorted(look.items())))
    if key not in _ORACLE:
        img = oracle.render(prec, compact(oracle.build_scene(scene_id, prec)), rt.camera_look(prec, W, H, S, bounces, **look), 1227)[0]
        img.setflags(write=False)
        _ORACLE[key] = img
    return _ORACLE[key]


def _check_denoise(r, levels_list, where, history=False):
    """denoise() -- or denoise_history() -- against the restatement on what the handle itself reads back."""
    src = r.history()[0] if history else r.read_linear()
    n, a, z = r.guides()
    for levels in levels_list:
        got = (r.denoise_history if history else r.denoise)(levels, *SIG)
        assert same_bits(got, filter_np(src, n, a, z, levels, *SIG)), (where, levels)
        assert np.isfinite(got).all(), (where, levels)


def _check_denoise_variance(r, levels_list, where, sigmas=(VSIG_ON, VSIG_OFF)):
    lin, V = r.read_linear(), r.variance()
    n, a, z = r.guides()
    for sig in sigmas:
        for levels in levels_list:
            got = r.denoise_variance(levels, *sig)
            assert np.isfinite(got).all(), (where, levels, sig)
            assert same_bits(got, variance_filter_np(lin, V, n, a, z, levels, *sig)), (where, levels, sig)
            if sig[0] == INF:                             # the recurrences coincide
                assert same_bits(got, r.denoise(levels, *sig)), (where, levels, "against denoise()")


def _check_guides(r, rt, oracle, prec, scene_id, cam, where):
    n, a, z = r.guides()
    wn, wa, wz, hit = guides_np(rt, oracle, prec, scene_id, cam, r.local_row_map())
    assert same_bits(z, wz), where
    assert same_bits(n, wn), where
    assert same_bits(a, wa), where
    return hit


# ---- A. the whole chain on edge frames

@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES, ids=_id)
@pytest.mark.parametrize("prec", [32, 64])
def test_render_and_filters_on_edge_frames(rt, oracle, prec, frame):
    W, H = frame
    S = 24                                                  # enough for the sorted schedule to rank a frame of 4096 pixels
    sc = compact(oracle.build_scene(3, prec))
    at = lambda n: _oracle_image(rt, oracle, prec, 3, W, H, n, B)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, rt.camera(prec, W, H, S, B))
        for sched, threads in ((rt.SCHED_STATIC, 8), (rt.SCHED_PERSISTENT, 0), (rt.SCHED_SORTED, 0)):
            r.set_schedule(sched)
            r.render(threads)
            assert same_bits(r.read_framebuffer(), at(S)), ("render", sched)
        assert r.stats()["phases"] == (2 if W * H >= 4096 else 1)
        # plain chunks, the linear read, the guides, the fixed filter
        for chunk, total in ((2, 2), (3, 5)):
            r.accumulate(chunk)
            assert same_bits(r.read_framebuffer(), at(total)), ("accumulate", total)
        assert same_bits(gamma(r.read_linear()), r.read_framebuffer())
        _check_guides(r, rt, oracle, prec, 3, rt.camera(prec, W, H, S, B), "guides")
        _check_denoise(r, (1, 3, 8), "plain")               # at 8 the step exceeds the frame: only the centre tap is left
        # uniform chunks that keep the second moment
        r.reset_accumulation()
        r.accumulate_with_variance(2); r.accumulate_with_variance(3)
        assert same_bits(r.read_framebuffer(), at(5))
        counts, _ = check_against_err(r, ("uniform", prec, frame))
        assert (counts == 5).all()
        _check_denoise_variance(r, (1, 3, 5), "uniform")
        # a mix of counts
        r.reset_accumulation()
        run_mixed(r, 3)
        counts, _ = check_against_err(r, ("mixed", prec, frame))
        if W * H >= 1024:
            assert len(np.unique(counts)) >= 2
        img = r.read_framebuffer()
        for n in np.unique(counts):
            sel = counts == n
            assert same_bits(img[sel], at(int(n))[sel]), ("adaptive", n)
        assert same_bits(gamma(r.read_linear()), img)
        _check_denoise(r, (1, 3), "mixed")
        _check_denoise_variance(r, (1, 3, 5), "mixed")


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES, ids=_id)
@pytest.mark.parametrize("prec", [32, 64])
def test_history_on_edge_frames(rt, prec, frame):
    W, H = frame
    default = (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, rt.api.HISTORY_MAX)
    home = rt.camera_look(prec, W, H, 1, B)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, home)
        r.accumulate(3)
        cur = state(r, False)
        c0, m0, count = check_update(r, home, cur, None, default, "no base")
        assert count == 0
        _check_denoise(r, (1, 3), "first frame", history=True)
        r.history_commit()
        base = as_base(home, cur, c0, m0)
        carried = 0
        for name, kw in MOVES.items():
            cam = rt.camera_look(prec, W, H, 1, B, **kw)
            move(r, cam, 1228)
            r.accumulate(2)
            cur = state(r, False)
            check_update(r, cam, cur, base, LOOSE, (prec, frame, name, LOOSE))
            carried += check_update(r, cam, cur, base, default, (prec, frame, name))[2]
            _check_denoise(r, (1, 3), (prec, frame, name), history=True)
        assert carried > 0


# ---- B. camera placements

@pytest.mark.gpu
@pytest.mark.parametrize("name,scene_id,frame", [(n, 3, f) for n in PLACEMENTS for f in PLACEMENT_FRAMES]
                         + [(n, 1, PLACEMENT_FRAMES[0]) for n in list(PLACEMENTS)[:3]], ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("prec", [32, 64])
def test_render_and_guides_of_a_placement(rt, oracle, prec, name, scene_id, frame):
    W, H = frame
    S = 24
    cam = rt.camera_look(prec, W, H, S, B, **PLACEMENTS[name])
    want = _oracle_image(rt, oracle, prec, scene_id, W, H, S, B, **PLACEMENTS[name])
    assert np.isfinite(want).all()
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, scene_id, cam, source=rt.SCENE_GRID, sched=rt.SCHED_SORTED)
        r.render(0)
        assert same_bits(r.read_framebuffer(), want), "sorted, grid"
        assert r.stats()["phases"] == (2 if W * H >= 4096 else 1)
        _check_guides(r, rt, oracle, prec, scene_id, cam, "grid")
        r.set_scene_source(rt.SCENE_LDS_EXACT); r.set_schedule(rt.SCHED_STATIC)
        r.render(8)
        assert same_bits(r.read_framebuffer(), want), "static, exact"
        r.set_scene_source(rt.SCENE_SCALAR)
        r.set_camera(cam); r.init_rng(1227)                 # stale guides: rendered again, from the scalar loop
        _check_guides(r, rt, oracle, prec, scene_id, cam, "scalar")


@pytest.mark.gpu
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("frame", PLACEMENT_FRAMES, ids=_id)
@pytest.mark.parametrize("prec", [32, 64])
def test_history_across_large_moves(rt, prec, frame, adaptive):
    W, H = frame
    default = (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, rt.api.HISTORY_MAX)
    home = rt.camera_look(prec, W, H, 1, B)

    def sample(r):
        if adaptive:
            run_mixed(r, 2)
        else:
            r.accumulate(3)

    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, home)
        sample(r)
        cur = state(r, adaptive)
        c0, m0, _ = check_update(r, home, cur, None, default, "no base")
        r.history_commit()
        base = as_base(home, cur, c0, m0)
        counts = {}
        for name, kw in MOVES.items():
            cam = rt.camera_look(prec, W, H, 1, B, **kw)
            where = (prec, frame, adaptive, name)
            move(r, cam, 1228)
            r.history_plan(*default)                        # before the first sample: the plan needs the guides alone
            plan = r.history_plan_lengths()
            sample(r)
            cur = state(r, adaptive)
            assert same_bits(plan, plan_np(cam, cur["N"], cur["t"], base, default)[0]), where
            check_update(r, cam, cur, base, LOOSE, where + (LOOSE,))
            counts[name] = check_update(r, cam, cur, base, default, where)[2]
            plain_rgb, length = r.history()
            assert same_bits(cur["n"].astype(r.dtype) + plan, length), where
            # the three kernels share one gather: the clipped update on the same classes of pixel, and gamma = inf, which clamps nothing
            check_clipped(r, cam, cur, base, default, 1, rt.api.HISTORY_CLIP_GAMMA, where)
            want = check_clipped(r, cam, cur, base, default, 1, INF, where + (INF,))
            assert want["clipped"] == 0 and same_bits(r.history()[0], plain_rgb), where
        assert counts["elsewhere"] == 0 and 0 < counts["opposite"] < counts["orbit25"] < counts["near"], counts


# ---- C. sample-count edges through the chain

@pytest.mark.gpu
@pytest.mark.parametrize("frame", [(64, 40), (16, 16)], ids=_id)
@pytest.mark.parametrize("prec", [32, 64])
def test_nobody_sampled_goes_through_the_chain(rt, prec, frame):
    W, H = frame
    default = (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, rt.api.HISTORY_MAX)
    home, moved = rt.camera_look(prec, W, H, 1, B), rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(1.5))
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, home)
        _, active = r.accumulate_adaptive(4, 0.0, min_samples=0, max_samples=3)     # 4 more samples would pass max_samples
        counts, _ = r.adaptive_state()
        assert active == 0 and (counts == 0).all() and r.accumulated_samples == 0
        lin = r.read_linear()
        assert (lin == 0).all() and (r.read_framebuffer() == 0).all() and (r.variance() == 0).all()
        _check_denoise(r, (1, 3), "nobody sampled")
        _check_denoise_variance(r, (1, 3), "nobody sampled", sigmas=(VSIG_ON,))
        cur = state(r, True)
        c0, m0, count = check_update(r, home, cur, None, default, "nobody sampled, no base")
        assert count == 0 and (m0 == 0).all() and (c0 == 0).all()
        _check_denoise(r, (1, 3), "nobody sampled", history=True)
        r.history_commit()
        base = as_base(home, cur, c0, m0)
        move(r, moved, 1228)                               # a base whose M is 0 everywhere carries nothing
        r.accumulate(3)
        cur = state(r, False)
        for params in (default, LOOSE):
            c1, m1, count = check_update(r, moved, cur, base, params, ("after an empty base", params))
            assert count == 0 and same_bits(c1, cur["c"]) and (m1 == 3).all()
        r.history_commit()
        base = as_base(moved, cur, c1, m1)
        move(r, home, 1229)                                # ... and the frame after that carries again
        r.accumulate(2)
        _, _, count = check_update(r, home, state(r, False), base, default, "after a sampled base")
        assert count > 0.5 * W * H


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [(64, 40), (16, 16)], ids=_id)
@pytest.mark.parametrize("prec", [32, 64])
def test_one_sample_each_goes_through_the_chain(rt, oracle, prec, frame):
    W, H = frame
    default = (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, rt.api.HISTORY_MAX)
    home, moved = rt.camera_look(prec, W, H, 1, B), rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(1.5))
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, home)
        _, active = r.accumulate_adaptive(1, 0.0, min_samples=1, max_samples=1)
        counts, err = r.adaptive_state()
        assert active == W * H and (counts == 1).all() and np.isinf(err).all() and (r.variance() == 0).all()
        assert same_bits(r.read_framebuffer(), _oracle_image(rt, oracle, prec, 3, W, H, 1, B))
        _check_denoise(r, (1, 3), "one sample")
        _check_denoise_variance(r, (1, 3, 5), "one sample")  # V == 0: i_p = f_k / eps, finite
        cur = state(r, True)
        c0, m0, _ = check_update(r, home, cur, None, default, "one sample, no base")
        assert (m0 == 1).all()
        r.history_commit()
        base = as_base(home, cur, c0, m0)
        move(r, moved, 1228)
        r.accumulate_adaptive(1, 0.0, min_samples=1, max_samples=1)
        cur = state(r, True)
        _, m1, count = check_update(r, moved, cur, base, default, "one sample on one sample")
        assert count > 0.5 * W * H and float(m1.max()) == 2
        _check_denoise(r, (1, 3), "one sample on one sample", history=True)


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [(64, 40), (16, 16)], ids=_id)
@pytest.mark.parametrize("prec", [32, 64])
def test_max_history_at_its_lower_end(rt, prec, frame):
    W, H = frame
    tol, cos = rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS
    home, moved = rt.camera_look(prec, W, H, 1, B), rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(1.5))
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, home)
        r.accumulate(3)
        # include/rtiow.h: max_history <= 0 is RTIOW_E_BADARG, and the refused call writes no temporal image
        assert r._lib.rtiow_history_update(r._h, tol, cos, 0.0, None, None) == E_BADARG
        assert r._lib.rtiow_read_history(r._h, None, None, W * H) == E_STATE
        cur = state(r, False)
        c0, m0, _ = check_update(r, home, cur, None, (tol, cos, 0.5), "no base, cap 0.5")      # the cap is on m, not on n
        assert (m0 == 3).all()
        r.history_commit()
        base = as_base(home, cur, c0, m0)
        move(r, moved, 1228)
        r.accumulate(2)
        cur = state(r, False)
        _, m1, count = check_update(r, moved, cur, base, (tol, cos, 0.5), "cap 0.5 below every count")
        assert count > 0.5 * W * H and float(m1.max()) == 2.5 and set(np.unique(m1)) == {2.0, 2.5}


# ---- D. frames whose hand-out order does not fit (row << 16 | column)

def _no_order(r, rt):
    with pytest.raises(rt.RtiowError) as e:
        r.debug_read_order()
    return e.value.code == E_STATE


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["reference", "narrow"])
@pytest.mark.parametrize("frame", [(65536, 2), (2, 32768)], ids=_id)
@pytest.mark.parametrize("prec", [32, 64])
def test_unfit_frame_renders(rt, oracle, prec, frame, view):
    """The reference view of 65536 x 2 has a viewport 32768 times as wide as high: hit share 0.0004, almost every ray leaves sideways
    (the far bounces); vfov = 0.004 is a real picture of the scene, every primary ray a hit."""
    W, H = frame
    S, bounces = 2, 4
    look = NARROW if view == "narrow" else {}
    want = _oracle_image(rt, oracle, prec, 3, W, H, S, bounces, **look)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, rt.camera_look(prec, W, H, S, bounces, **look))
        for sched, threads in ((rt.SCHED_STATIC, 8), (rt.SCHED_PERSISTENT, 0), (rt.SCHED_SORTED, 0)):
            r.set_schedule(sched)
            r.render(threads)
            assert same_bits(r.read_framebuffer(), want), sched


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["reference", "narrow"])
@pytest.mark.parametrize("frame", [(65536, 2), (2, 32768)], ids=_id)
def test_unfit_frame_is_never_ranked(rt, oracle, frame, view):
    """24 samples: a frame that fits is ranked by a prepass and its order carried to the next render; this one runs in tile order, in
    one phase, every time, and leaves no order behind."""
    W, H = frame
    S, bounces = 24, 4
    look = NARROW if view == "narrow" else {}
    want = _oracle_image(rt, oracle, 32, 3, W, H, S, bounces, **look)
    with rt.Renderer(0, 32, debug=True) as r:
        _begin(r, rt, 32, 3, rt.camera_look(32, W, H, S, bounces, **look))
        for _ in range(2):
            r.render(0)
            st = r.stats()
            assert st["phases"] == 1 and st["order_reused"] == 0 and st["prepass_samples"] == 0 and st["staged_stores"] == 0, st
            assert _no_order(r, rt)
        assert same_bits(r.read_framebuffer(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [(65536, 2), (2, 32768)], ids=_id)
def test_unfit_frame_accumulates_and_refuses_adaptive(rt, oracle, frame):
    W, H = frame
    bounces = 4
    at = lambda n: _oracle_image(rt, oracle, 32, 3, W, H, n, bounces)
    with rt.Renderer(0, 32, debug=True) as r:
        _begin(r, rt, 32, 3, rt.camera(32, W, H, 2, bounces))
        r.accumulate(1)
        assert same_bits(r.read_framebuffer(), at(1))
        active = ctypes.c_int(-1)
        assert r._lib.rtiow_accumulate_adaptive(r._h, 1, 0, 0.0, 8, None, ctypes.byref(active)) == E_BADARG and active.value == 0
        r.accumulate(1)                                     # the refused call changed nothing: the second chunk, unranked
        assert r.accumulated_samples == 2 and same_bits(r.read_framebuffer(), at(2))
        assert _no_order(r, rt)
        r.reset_accumulation()                              # ... refused on an empty accumulation too
        assert r._lib.rtiow_accumulate_adaptive(r._h, 1, 0, 0.0, 8, None, None) == E_BADARG
        assert r._lib.rtiow_read_variance(r._h, None, W * H) == E_STATE
        r.render(0)
        assert same_bits(r.read_framebuffer(), at(2))


@pytest.mark.gpu
def test_unfit_frame_guides_and_filter(rt, oracle):
    W, H, bounces = 65536, 2, 4
    cam = rt.camera_look(32, W, H, 2, bounces, **NARROW)
    with rt.Renderer(0, 32) as r:
        _begin(r, rt, 32, 3, cam)
        r.accumulate(2)
        assert same_bits(r.read_framebuffer(), _oracle_image(rt, oracle, 32, 3, W, H, 2, bounces, **NARROW))
        assert same_bits(gamma(r.read_linear()), r.read_framebuffer())
        assert _check_guides(r, rt, oracle, 32, 3, cam, "guides").all()
        _check_denoise(r, (3,), "65536 x 2")


@pytest.mark.gpu
def test_unfit_frame_history(rt):
    W, H, bounces = 65536, 2, 4
    default = (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, rt.api.HISTORY_MAX)
    home, moved = rt.camera_look(32, W, H, 1, bounces, **NARROW), rt.camera_look(32, W, H, 1, bounces, **NARROW_STEP)
    with rt.Renderer(0, 32) as r:
        _begin(r, rt, 32, 3, home)
        r.accumulate(2)
        cur = state(r, False)
        c0, m0, _ = check_update(r, home, cur, None, default, "no base")
        r.history_commit()
        base = as_base(home, cur, c0, m0)
        move(r, moved, 1228)
        r.accumulate(1)
        cur = state(r, False)
        _, _, count = check_update(r, moved, cur, base, default, "a step sideways")
        assert count > 0.5 * W * H
        _check_denoise(r, (2,), "65536 x 2", history=True)


@pytest.mark.gpu
def test_tall_frame_fits_in_two_shards(rt, oracle):
    """2 x 32768 under set_shard(rank, 2, 8) has 16384 local rows: chunks are ranked, adaptive chunks run, the shards assemble."""
    W, H, bounces = 2, 32768, 4
    want = _oracle_image(rt, oracle, 32, 3, W, H, 2, bounces)
    plain, adaptive = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
    for rank in (0, 1):
        with rt.Renderer(0, 32, debug=True) as r:
            r.set_camera(rt.camera(32, W, H, 2, bounces)); r.set_scene(rt.build_scene(3, 32))
            r.set_shard(rank, 2, 8); r.init_rng(1227)
            assert r.local_rows == 16384
            r.accumulate(1); r.accumulate(1)
            info, order, _, keys = r.debug_read_order()
            assert info["kind"] == rt.api.ORDER_ACCUMULATE and (info["W"], info["local_rows"]) == (W, 16384) and keys is not None
            listed = order[order >= 0]
            assert len(listed) == W * 16384 and int((listed >> 16).max()) == 16383 and len(np.unique(listed)) == len(listed)
            rt.place_rows(plain, r.read_framebuffer(), rank, 2, 8)
            r.reset_accumulation()
            _, active = r.accumulate_adaptive(2, 0.0, min_samples=2)
            assert active == W * 16384 and r.debug_read_order()[0]["kind"] == rt.api.ORDER_ADAPTIVE
            rt.place_rows(adaptive, r.read_framebuffer(), rank, 2, 8)
    assert same_bits(plain, want)
    assert same_bits(adaptive, want)


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [(65535, 2), (2, 32767)], ids=_id)
def test_largest_frames_whose_order_fits(rt, oracle, frame):
    W, H = frame
    S, bounces = 24, 4
    with rt.Renderer(0, 32, debug=True) as r:
        _begin(r, rt, 32, 3, rt.camera(32, W, H, S, bounces))
        r.render(0)
        assert same_bits(r.read_framebuffer(), _oracle_image(rt, oracle, 32, 3, W, H, S, bounces))
        st = r.stats()
        assert st["phases"] == 2 and st["staged_stores"] == 1, st
        info, order, slot_of, _ = r.debug_read_order()
        assert info["kind"] == rt.api.ORDER_RENDER and (info["W"], info["local_rows"]) == (W, H)
        listed = order[order >= 0]
        assert len(listed) == W * H and len(np.unique(listed)) == W * H
        assert int((listed & 0xffff).max()) == W - 1 and int((listed >> 16).max()) == H - 1      # the largest packed column and row
        assert np.array_equal(order[slot_of.ravel()], (np.arange(H)[:, None] << 16 | np.arange(W)[None, :]).ravel())
        r.render(0)
        assert r.stats()["order_reused"] == 1
        # the other two writers of the order: a ranked chunk and an adaptive chunk's active list
        want = _oracle_image(rt, oracle, 32, 3, W, H, 2, bounces)
        r.accumulate(1); r.accumulate(1)
        info, order, _, _ = r.debug_read_order()
        listed = order[order >= 0]
        assert info["kind"] == rt.api.ORDER_ACCUMULATE and len(np.unique(listed)) == W * H
        assert int((listed & 0xffff).max()) == W - 1 and int((listed >> 16).max()) == H - 1
        assert same_bits(r.read_framebuffer(), want)
        r.reset_accumulation()
        _, active = r.accumulate_adaptive(2, 0.0, min_samples=2)
        info, order, _, _ = r.debug_read_order()
        listed = order[order >= 0]
        assert active == W * H and info["kind"] == rt.api.ORDER_ADAPTIVE and len(np.unique(listed)) == W * H
        assert int((listed & 0xffff).max()) == W - 1 and int((listed >> 16).max()) == H - 1
        assert same_bits(r.read_framebuffer(), want)


# ---- E. the cases reach what they are for: the CPU oracle alone (no GPU)


def _oracle_state(rt, oracle, prec, cam, n=2):
    """A current frame for update_np from the oracle's guides alone: constant colour, n samples everywhere."""
    W, H = cam.img_width, cam.img_height
    normal, _, depth, _ = guides_np(rt, oracle, prec, 3, cam, np.arange(H))
    return {"c": np.ones((H, W, 3), depth.dtype), "n": np.full((H, W), n, np.int32), "N": normal, "t": depth}


def _classes(rt, oracle, prec, W, H, base_look, look, params):
    """Pixels of the moved camera by what history_reproject_kernel does with them: behind the base camera (den <= 0), off its frame,
    gathering through its edge, in its frame with every tap rejected, carried.  The edge class overlaps the last two."""
    base_cam, cam = rt.camera_look(prec, W, H, 1, B, **base_look), rt.camera_look(prec, W, H, 1, B, **look)
    b, cur = _oracle_state(rt, oracle, prec, base_cam), _oracle_state(rt, oracle, prec, cam)
    base = as_base(base_cam, b, b["c"], b["n"].astype(b["c"].dtype))
    den, u, v = reproject(cam, cur, base_cam)
    with np.errstate(invalid="ignore"):
        front = den > 0
        window = front & (u > -1) & (u < W) & (v > -1) & (v < H)
        edge = window & ((u < 0) | (u > W - 1) | (v < 0) | (v > H - 1))
    _, m_out, count = update_np(cam, cur, base, *params)
    carried = m_out > cur["n"]
    assert count == carried.sum() and not (carried & ~window).any()
    got = {"behind": int((~front).sum()), "off": int((front & ~window).sum()), "edge": int(edge.sum()),
           "rejected": int((window & ~carried).sum()), "carried": int(carried.sum())}
    assert got["behind"] + got["off"] + got["rejected"] + got["carried"] == W * H
    return got


@pytest.mark.parametrize("prec", [32, 64])
def test_cpu_large_moves_reach_every_class(native, oracle, prec):
    default = (native.api.HISTORY_DEPTH_TOL, native.api.HISTORY_NORMAL_COS, native.api.HISTORY_MAX)
    for W, H in PLACEMENT_FRAMES:
        got = {name: _classes(native, oracle, prec, W, H, {}, kw, default) for name, kw in MOVES.items()}
        for cls in ("behind", "off", "edge", "rejected", "carried"):
            assert any(g[cls] > 0 for g in got.values()), (prec, W, H, cls, got)
        assert min(got["opposite"][c] for c in ("behind", "rejected", "carried")) > 0, got["opposite"]
        assert got["elsewhere"]["off"] == W * H                     # nothing shared
        loose = _classes(native, oracle, prec, W, H, {}, MOVES["roll"], LOOSE)
        assert 0 < loose["carried"] < got["roll"]["carried"]        # depth_tol 0: only taps of exactly the reprojected depth
    if prec == 32:
        assert got["opposite"] == {"behind": 834, "off": 245, "edge": 8, "rejected": 3753, "carried": 288}
        assert _classes(native, oracle, 32, 48, 32, {}, MOVES["opposite"], default) == {"behind": 292, "off": 88, "edge": 5, "rejected": 1009, "carried": 147}


@pytest.mark.parametrize("frame", THIN_OR_TINY, ids=_id)
@pytest.mark.parametrize("prec", [32, 64])
def test_cpu_moves_carry_and_gather_through_the_edge_on_small_frames(native, oracle, prec, frame):
    default = (native.api.HISTORY_DEPTH_TOL, native.api.HISTORY_NORMAL_COS, native.api.HISTORY_MAX)
    got = {name: _classes(native, oracle, prec, *frame, {}, kw, default) for name, kw in MOVES.items()}
    assert any(g["carried"] > 0 for g in got.values()), got
    assert any(g["edge"] > 0 for g in got.values()), got


def test_cpu_the_step_on_the_wide_frame_carries(native, oracle):
    default = (native.api.HISTORY_DEPTH_TOL, native.api.HISTORY_NORMAL_COS, native.api.HISTORY_MAX)
    got = _classes(native, oracle, 32, 65536, 2, NARROW, NARROW_STEP, default)
    assert got["carried"] > 0.5 * 65536 * 2 and got["edge"] > 0 and got["off"] > 0, got


@pytest.mark.parametrize("scene_id", [3, 1])
@pytest.mark.parametrize("prec", [32, 64])
def test_cpu_placements_are_what_they_claim(native, oracle, prec, scene_id):
    dt = np.float32 if prec == 32 else np.float64
    sc = compact(native.build_scene(scene_id, prec))
    cr = np.asarray(sc["center_radius"], dt).reshape(-1, 4)
    for W, H in PLACEMENT_FRAMES:
        hit_share = {}
        for name, kw in PLACEMENTS.items():
            cam = native.camera_look(prec, W, H, 1, B, **kw)
            normal, _, depth, hit = guides_np(native, oracle, prec, scene_id, cam, np.arange(H))
            hit_share[name] = float(hit.mean())
            if name.startswith("inside"):
                # guide_kernel flips the outward normal iff !(D . outward < 0): here every pixel hits, and every hit is from inside
                O = np.array(cam.center[:], dt)
                fi, fj = np.arange(W).astype(dt)[None, :, None], np.arange(H).astype(dt)[:, None, None]
                D = ((vec(cam.pixel00_loc, dt) + fi * vec(cam.pixel_delta_u, dt)) + fj * vec(cam.pixel_delta_v, dt)) - O
                P = O + depth[..., None] * D
                k = np.argmin(np.abs(np.linalg.norm(P[..., None, :].astype(np.float64) - cr[None, None, :, :3], axis=-1) - cr[:, 3]), axis=-1)
                outward = (P - cr[k, :3]) / cr[k, 3:4]
                assert hit.all() and (dot(D, outward) > 0).all() and (dot(D, normal) < 0).all(), (name, W, H)
        assert hit_share["all_sky"] == 0 and hit_share["straight_down"] == 1 and 0 < hit_share["grazing"] < 1 and 0 < hit_share["wide"] < 1, hit_share
    # every primary ray of the far placement starts beyond the grid's Rfar (the far-ray clip), about the library's recentring point
    plan = _plan(native, cr)
    assert plan["usable"]
    O = np.array(PLACEMENTS["far_tele"]["lookfrom"], np.float64)
    assert ((O - plan["centre"]) ** 2).sum() > plan["rfar"] ** 2
    assert ((np.array([13.0, 2.0, 3.0]) - plan["centre"]) ** 2).sum() < plan["rfar"] ** 2       # the reference view starts inside
