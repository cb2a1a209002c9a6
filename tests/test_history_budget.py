"""History-guided sample budgets on the GPU: rtiow_history_plan computes the history length m every pixel of
the current camera will carry before the first sample of the frame is traced, and rtiow_accumulate_budget is an adaptive chunk whose rule
is "sample pixel p while n_p + m_p is below a target".  The plan is section 11's m, so it is checked BIT FOR BIT against
tests/preview_model.py's plan_np; the rule is integer and T arithmetic, so active sets and counts are predicted exactly; and every
pixel still holds the bits rtiow_render leaves at its own count."""
import ctypes

import numpy as np
import pytest

from tests.preview_drive import (CAP_LOW, CAP_MIX, E_BADARG, E_STATE, INF, SLACK, begin, budget_moves, budget_sampler, check_update,
                                 commit_base, compare, history_defaults, move, one_shot, orbit_reference, sample, state, uniform_sampler, walk)
from tests.preview_model import budget_rule, plan_np, same_bits, update_np

pytestmark = pytest.mark.gpu

BIG = 2 ** 31 - 1
BUDGET_MOVES = ("orbit", "dolly", "roll")
SIZES = ((9, 9), (67, 41), (203, 117))             # neither of the larger two a multiple of 8 or 16; one tile and a bit


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _classes(m, cap):
    """Pixels with m = 0, 0 < m < cap, m = cap."""
    return int((m == 0).sum()), int(((m > 0) & (m < cap)).sum()), int((m == m.dtype.type(cap)).sum())


def _mixed_plan(r, rt, prec, scene_id, W, H, first="orbit", then="home", source=3, cap=CAP_MIX, B=10):
    """A base after a mix of counts at view `first`, the camera moved to `then`, the plan at `cap` read back and checked to hold all
    three classes of pixel (CAP_LOW: the two it can hold).  Returns (cams, base, params, plane)."""
    cams = budget_moves(rt, prec, W, H, B)
    params = history_defaults(rt)[:2] + (cap,)
    begin(r, rt, prec, scene_id, cams[first], source)
    sample(r, True)
    base = commit_base(r, cams[first], params)
    move(r, cams[then])
    count = r.history_plan(*params)
    m = r.history_plan_lengths()
    assert count == int((m > 0).sum())
    if W * H >= 1000:
        for k, size in enumerate(_classes(m, cap)):
            if k == 1 and cap < 4:                                    # below both counts of the base: every covered pixel is at the cap
                assert size == 0
                continue
            assert size >= 0.01 * W * H, (prec, scene_id, W, H, "class %d of the plan is nearly empty" % k, _classes(m, cap))
    return cams, base, params, m


def _run_budget(r, m, samples, target, min_samples, max_samples=BIG, limit=40):
    """Budget chunks until none is active, every chunk's active set and counts predicted from the plane and the counts before it."""
    chunks = 0
    while True:
        before = r.adaptive_state()[0]
        mask = budget_rule(before, m, samples, target, min_samples, max_samples)
        _, active = r.accumulate_budget(samples, target, min_samples, max_samples)
        after = r.adaptive_state()[0]
        where = (samples, target, min_samples, max_samples, chunks)
        assert active == int(mask.sum()), where
        assert np.array_equal(after, before + samples * mask.astype(np.int32)), where
        assert r.stats()["primary_rays"] == active * samples, where
        chunks += 1
        if active == 0:
            break
        assert chunks < limit, where
    n = after
    have = n.astype(m.dtype) + m
    done = (n >= min_samples) & (have >= m.dtype.type(target))
    assert (done | (n.astype(np.int64) + samples > max_samples)).all()
    if max_samples == BIG:
        assert (n >= min_samples).all() and (have >= m.dtype.type(target)).all()
    return n, chunks


_SHOTS = {}


def _shot(rt, prec, scene_id, W, H, n, B):
    """rtiow_render at samples_per_pixel = n and the home view, rendered once per configuration."""
    key = (prec, scene_id, W, H, int(n), B)
    if key not in _SHOTS:
        _SHOTS[key] = one_shot(rt, prec, scene_id, W, H, int(n), B)
    return _SHOTS[key]


def _exact_at_own_count(rt, img, counts, prec, scene_id, W, H, B, where):
    for n in np.unique(counts):
        sel = counts == n
        if n == 0:
            assert (img[sel] == 0).all(), where                       # never sampled: reads 0
            continue
        assert same_bits(img[sel], _shot(rt, prec, scene_id, W, H, n, B)[sel]), (where, int(n))


# ---- 1. the plan is section 11's m, bit for bit

@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_the_plan_is_the_updates_length(rt, prec, scene_id, size):
    W, H = size
    default = history_defaults(rt)
    cams = budget_moves(rt, prec, W, H)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, scene_id, cams["home"])
        sample(r, True)
        assert sorted(np.unique(r.adaptive_state()[0])) in ([4, 8], [4], [8])
        base = commit_base(r, cams["home"], default)
        sweeps = {"orbit": [default, default[:2] + (CAP_LOW,), default[:2] + (CAP_MIX,), (0.0, -1.0, INF)],
                  "dolly": [default, (default[0], -1.0, CAP_LOW), (0.0, -1.0, INF)],
                  "roll": [default, (0.0, default[1], CAP_LOW), default[:2] + (INF,)]}
        for name in BUDGET_MOVES:
            move(r, cams[name], 1228)
            for params in sweeps[name]:
                count = r.history_plan(*params)
                m = r.history_plan_lengths()
                normal, _, depth = r.guides()
                want_m, want_count = plan_np(cams[name], normal, depth, base, params)
                where = (prec, scene_id, size, name, params)
                assert m.dtype == r.dtype and same_bits(m, want_m), where
                assert count == want_count == int((m > 0).sum()), where
                if W * H < 1000 or params[0] == 0.0:
                    continue
                none, below, at = _classes(m, params[2])
                floor = 0.01 * W * H
                assert none >= floor, (where, none)
                if params[2] == CAP_LOW:
                    assert at >= floor and below == 0, (where, below, at)
                elif params[2] == CAP_MIX:
                    assert below >= floor and at >= floor, (where, below, at)
                else:
                    assert below >= floor and at == 0, (where, below, at)
                    assert 4 * (1 - 1e-6) <= m[m > 0].min() and m.max() <= 8 * (1 + 1e-6)


@pytest.mark.parametrize("prec", [32, 64])
def test_no_base_means_an_empty_plan(rt, prec):
    W, H = 67, 41
    cams = budget_moves(rt, prec, W, H)

    def empty(r, where):
        assert r.history_plan() == 0, where
        m = r.history_plan_lengths()
        assert m.shape == (r.height, r.width) and m.dtype == r.dtype and not m.any(), where

    with rt.Renderer(0, prec) as r:
        r.set_camera(cams["home"]); r.set_scene(rt.build_scene(3, prec))
        empty(r, "no base, no RNG and no chunk")
        r.init_rng(1227); sample(r, True)
        empty(r, "before any commit")
        r.history_update(); r.history_commit()
        move(r, cams["orbit"])
        assert r.history_plan() > 0
        assert r.history_plan(sync=False) is None and r.history_plan_lengths().any()
        r.history_reset()
        empty(r, "after history_reset")
        sample(r, True); r.history_update(); r.history_commit()
        r.set_scene(rt.build_scene(3, prec))
        empty(r, "after set_scene")
        r.init_rng(1227); sample(r, True); r.history_update(); r.history_commit()
        move(r, rt.camera_look(prec, W + 10, H, 1, 10))
        empty(r, "a base of another frame size")
        sample(r, True); r.history_update(); r.history_commit()
        move(r, rt.camera_look(prec, W + 10, H, 1, 10, lookfrom=(13.0, 2.0, 3.0), lookat=(26.0, 4.0, 6.0)))
        empty(r, "a camera facing away")
        # an empty plan is a plan: the target is everybody's
        n, _ = _run_budget(r, r.history_plan_lengths(), 2, 3.0, 0)
        assert (n == 4).all()


# ---- 2. the plan agrees with the update

@pytest.mark.parametrize("size", SIZES[1:])
@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_the_plan_agrees_with_the_update(rt, prec, scene_id, size):
    W, H = size
    with rt.Renderer(0, prec) as r:
        cams, base, params, m = _mixed_plan(r, rt, prec, scene_id, W, H, first="home", then="orbit")
        n, _ = _run_budget(r, m, 2, 8.0, 1)
        assert len(np.unique(n)) >= 3                                 # 2, 4 and 8 samples at least
        _, want_m, want_count = check_update(r, cams["orbit"], state(r, True), base, params, (prec, scene_id, size))
        assert same_bits(r.history()[1], m + n.astype(r.dtype))      # Mout = m + (T)n, in T
        assert same_bits(want_m, m + n.astype(r.dtype))
        assert want_count == int((m > 0).sum())
        assert same_bits(r.history_plan_lengths(), m)                # the update leaves the plan alone


# ---- 3. the rule

@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_the_rule(rt, prec, scene_id, size):
    W, H = size
    with rt.Renderer(0, prec) as r:
        _, _, _, m = _mixed_plan(r, rt, prec, scene_id, W, H, first="home", then="dolly")
        c0, e0 = r.adaptive_state()
        assert (c0 == 0).all() and np.isinf(e0).all()
        # (samples, target, min_samples, max_samples): min_samples 0 and 1, the target below the cap, at it, above it and between two
        # values T has, +inf with a small max_samples, a max_samples that stops pixels short of min_samples
        for k, case in enumerate(((2, 4.0, 0, BIG), (2, 4.0, 1, BIG), (1, CAP_MIX, 0, BIG), (3, 8.0, 1, BIG), (2, 8.0, 0, 5),
                                  (1, 6.0 + 2.0 ** -30, 0, BIG), (3, INF, 0, 7), (2, INF, 3, 3))):
            r.reset_accumulation()                                    # the plan survives it
            if k % 2:
                r.init_rng(1227 + k)                                  # ... and init_rng
            n, chunks = _run_budget(r, m, *case)
            samples, target, min_samples, max_samples = case
            if target == 4.0 and min_samples == 0 and W * H >= 1000:
                assert (n[m > 0] == 0).all() and (n[m == 0] == 4).all()
            if target == INF:
                assert (n == (max_samples // samples) * samples).all()
            ea = r.adaptive_state()[1]
            assert np.isinf(ea[n < 2]).all() and np.isfinite(ea[n >= 2]).all()
            assert r.accumulated_samples == n.max()


# ---- 4. every pixel is exact at its own count

@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_every_pixel_is_exact_at_its_own_count(rt, prec, scene_id):
    """The camera ends at the home view, where rtiow_render's one-shot images are (tests/preview_drive.py's one_shot); a chunk of 2 and a
    target of 8 over a plan with m in {0} + [4, 6] leave three counts: 8, 4 and 2."""
    W, H, B = 67, 41, 10
    for source, sched in ((0, 0), (1, 1), (2, 2), (3, 2)):
        with rt.Renderer(0, prec) as r:
            _, _, _, m = _mixed_plan(r, rt, prec, scene_id, W, H, first="orbit", then="home", source=source, B=B)
            r.set_schedule(sched, 0)
            n, chunks = _run_budget(r, m, 2, 8.0, 0)
            img = r.read_framebuffer()
            assert sorted(np.unique(n)) == [2, 4, 8], (prec, scene_id, source, np.unique(n))
            assert chunks == 5
            _exact_at_own_count(rt, img, n, prec, scene_id, W, H, B, (prec, scene_id, source, sched))
            # the second moment is kept: the variance calls work afterwards
            var = r.variance()
            assert np.isfinite(var[n >= 2]).all()
            r.denoise_variance(2)


# ---- 5. with min_samples = 0 a fully covered pixel is not sampled

@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_a_fully_covered_pixel_keeps_its_history(rt, prec, scene_id):
    W, H = 203, 117
    with rt.Renderer(0, prec) as r:
        cams, base, params, m = _mixed_plan(r, rt, prec, scene_id, W, H, first="home", then="roll", cap=CAP_LOW)
        assert set(np.unique(m)) == {0.0, CAP_LOW}
        n, chunks = _run_budget(r, m, 2, CAP_LOW, 0)                 # m = target: not below it
        covered = m > 0
        assert (n[covered] == 0).all() and (n[~covered] == 4).all() and chunks == 3
        assert (r.read_framebuffer()[covered] == 0).all()
        cur = state(r, True)
        c, length, _ = check_update(r, cams["roll"], cur, base, params, (prec, scene_id))
        gathered = update_np(cams["roll"], dict(cur, c=np.zeros_like(cur["c"]), n=np.zeros_like(cur["n"])), base, *params)[0]
        rgb = r.history()[0]
        assert same_bits(rgb[covered], gathered[covered])           # Cout = h
        assert gathered[covered].any()
        assert same_bits(rgb[~covered], cur["c"][~covered])         # no history: Cout = c
        assert same_bits(length, m + n.astype(r.dtype))


# ---- 6. alternating with rtiow_accumulate_adaptive; nothing else moved

@pytest.mark.parametrize("prec", [32, 64])
def test_budget_and_adaptive_chunks_alternate(rt, prec):
    W, H, B, scene_id = 67, 41, 10, 3
    with rt.Renderer(0, prec) as r:
        _, _, _, m = _mixed_plan(r, rt, prec, scene_id, W, H, first="roll", then="home", B=B)

        def budget(samples, target, min_samples):
            before = r.adaptive_state()[0]
            mask = budget_rule(before, m, samples, target, min_samples, BIG)
            assert r.accumulate_budget(samples, target, min_samples)[1] == int(mask.sum())
            assert np.array_equal(r.adaptive_state()[0], before + samples * mask.astype(np.int32))

        def adaptive(samples, quantile, min_samples):
            cb, eb = r.adaptive_state()
            thr = float(np.quantile(eb[np.isfinite(eb)], quantile)) if np.isfinite(eb).any() else 0.1
            mask = (cb < min_samples) | (eb.astype(np.float64) > thr)
            assert r.accumulate_adaptive(samples, thr, min_samples=min_samples)[1] == int(mask.sum())
            assert np.array_equal(r.adaptive_state()[0], cb + samples * mask.astype(np.int32))

        budget(2, 8.0, 0)
        adaptive(2, 0.5, 2)
        budget(2, 8.0, 0)
        adaptive(2, 0.5, 0)
        budget(2, 8.0, 3)
        n = r.adaptive_state()[0]
        assert len(np.unique(n)) >= 3
        _exact_at_own_count(rt, r.read_framebuffer(), n, prec, scene_id, W, H, B, prec)
        assert r._lib.rtiow_accumulate(r._h, 1, 0, None) == E_STATE   # still the adaptive mode


@pytest.mark.parametrize("prec", [32, 64])
def test_a_plan_leaves_everything_else_alone(rt, prec):
    W, H = 67, 41
    cams = budget_moves(rt, prec, W, H)

    def run(with_plan):
        out = []
        plan = (lambda *a: r.history_plan(*a)) if with_plan else (lambda *a: None)
        with rt.Renderer(0, prec) as r:
            begin(r, rt, prec, 1, cams["home"])
            plan()
            sample(r, True)
            r.history_update(); r.history_commit()
            move(r, cams["orbit"])
            plan(0.0, -1.0, INF)
            plan()
            sample(r, True)
            plan(0.05, 0.5, 3.0)
            out += [r.read_framebuffer(), r.read_linear()] + list(r.adaptive_state())
            out += [np.array([r.history_update()])] + list(r.history())
            out += [r.denoise(2), r.denoise_variance(2), r.denoise_history(2)]
            plan()
            r.render(0)
            out += [r.read_framebuffer()]
            r.history_commit()
            move(r, cams["roll"])
            plan()
            r.accumulate(3)
            out += [r.read_framebuffer(), np.array([r.history_update()])] + list(r.history())
        return out

    plain, touched = run(False), run(True)
    assert len(plain) == len(touched)
    for k, (a, b) in enumerate(zip(plain, touched)):
        assert same_bits(a, b), (prec, k)


# ---- 7. states and error codes

def test_states_and_error_codes(rt):
    W, H = 96, 64
    npix = W * H
    cams = budget_moves(rt, 32, W, H)
    nul = (None, None)
    with rt.Renderer(0, 32) as r:
        lib = r._lib
        active = ctypes.c_int(-1)
        plan = lambda *a: lib.rtiow_history_plan(r._h, *a, *nul)
        read = lambda n=npix: lib.rtiow_read_history_plan(r._h, None, n)
        budget = lambda s=2, mn=1, t=8.0, mx=100: lib.rtiow_accumulate_budget(r._h, s, mn, t, mx, None, ctypes.byref(active))
        assert plan(0.1, 0.9, 8.0) == E_STATE and read() == E_STATE                      # no camera, no scene
        r.set_camera(cams["home"])
        assert plan(0.1, 0.9, 8.0) == E_STATE and read() == E_STATE                      # no scene
        r.set_scene(rt.build_scene(3, 32))
        assert budget() == E_STATE                                                       # no RNG
        for bad in ((-0.1, 0.9, 8.0), (float("nan"), 0.9, 8.0), (0.1, 1.5, 8.0), (0.1, -1.5, 8.0), (0.1, float("nan"), 8.0),
                    (0.1, 0.9, 0.0), (0.1, 0.9, -1.0), (0.1, 0.9, float("nan"))):
            assert plan(*bad) == E_BADARG, bad
        assert read() == E_STATE                                                         # the bad calls wrote nothing
        assert plan(0.0, -1.0, INF) == 0 and plan(0.1, 1.0, 1e-3) == 0                   # the ends of the ranges; no RNG, no chunk
        assert read() == 0 and read(npix + 1) == E_BADARG
        assert budget() == E_STATE                                                       # a plan, but still no RNG
        r.init_rng(1227)
        assert read() == 0                                                               # the plan survives init_rng
        for bad in ((0, 1, 8.0, 100), (-1, 1, 8.0, 100), (2, -1, 8.0, 100), (2, 5, 8.0, 4), (2, 1, 0.0, 100), (2, 1, -1.0, 100),
                    (2, 1, float("nan"), 100)):
            assert budget(*bad) == E_BADARG and active.value == 0, bad
        assert (r.adaptive_state()[0] == 0).all()                                        # refused calls sampled nothing ...
        assert lib.rtiow_history_update(r._h, 0.1, 0.9, 8.0, *nul) == E_STATE            # ... and began no accumulation
        assert budget(2, 0, INF, 4) == 0 and active.value == npix
        assert budget(2, 0, 1e-30, 100) == 0 and active.value == 0
        before = [r.read_framebuffer()] + list(r.adaptive_state())
        assert budget(0, 1, 8.0, 100) == E_BADARG
        for x, y in zip(before, [r.read_framebuffer()] + list(r.adaptive_state())):
            assert same_bits(x, y)
        # the plan survives every chunk, an accumulation reset, init_rng and a new guide mode ...
        r.accumulate_adaptive(1, 0.0, min_samples=3)
        r.set_guide_mode(rt.api.GUIDES_SPECULAR)
        kept = r.history_plan_lengths()
        r.reset_accumulation(); r.init_rng(3)
        assert same_bits(r.history_plan_lengths(), kept)
        r.set_guide_mode(rt.api.GUIDES_FIRST_HIT)
        # ... plain chunks shut the budget chunk out until the next reset, and change nothing when it is refused
        r.accumulate(2)
        plain = r.read_framebuffer()
        assert budget() == E_STATE and active.value == 0
        assert r.accumulated_samples == 2 and same_bits(r.read_framebuffer(), plain)
        r.reset_accumulation()
        assert budget() == 0 and active.value == npix
        # ... and it goes stale exactly when the temporal image does: commit, set_camera, set_scene, set_shard, history_reset
        for keeps_accumulation, go_stale in ((True, lambda: r.history_commit()), (False, lambda: r.set_camera(cams["orbit"])),
                                             (False, lambda: r.set_scene(rt.build_scene(3, 32))), (True, lambda: r.history_reset()),
                                             (False, lambda: (r.set_shard(0, 1, 8), r.set_shard(0, 1, 8)))):
            r.set_camera(cams["home"]); r.init_rng(1227)
            assert plan(0.1, 0.9, 8.0) == 0
            assert budget() == 0 and active.value == npix and read() == 0
            r.history_update()
            assert read() == 0                                                           # an update leaves the plan alone
            go_stale()
            assert read() == E_STATE
            before = r.adaptive_state()[0] if keeps_accumulation else None
            assert budget() == E_STATE and active.value == 0                             # the plan is stale (or the RNG is gone)
            if keeps_accumulation:
                assert (before == 2).all() and np.array_equal(r.adaptive_state()[0], before)
    with rt.Renderer(0, 32) as r:                        # a sharded handle: no plan, so no budget chunk
        lib = r._lib
        begin(r, rt, 32, 3, cams["home"])
        r.set_shard(1, 3, 8); r.init_rng(1227)
        assert lib.rtiow_history_plan(r._h, 0.1, 0.9, 8.0, *nul) == E_STATE
        assert lib.rtiow_read_history_plan(r._h, None, W * r.local_rows) == E_STATE
        assert lib.rtiow_accumulate_budget(r._h, 2, 1, 8.0, 100, None, None) == E_STATE
        r.accumulate_adaptive(2, 0.0, min_samples=2)                                     # the shard itself still renders


# ---- 8. it pays

# scripts/history_budget_probe.py measured, on tests/preview_drive.py's walk (8 cameras 0.5 degrees apart, 320 x 180, 50 bounces, fp32)
# at the defaults of raytracingincuda_amd/api.py against that walk with 4 uniform samples a frame, per scene
# (profiles/history_budget/history_budget_probe.json): primary rays, whole-frame MSE and MSE over the disoccluded set (m = 0 in the last
# frame's plan) of the temporal image at the last frame, each as budget / uniform.  The budget walk traces fewer rays and brings the
# disoccluded set's MSE to a quarter; it does NOT lower the whole-frame MSE -- no setting of the sweep that stays within the uniform
# walk's rays does (DESIGN.md section 4.12 has the table) -- so for the whole frame the test asserts what was measured, not <= 1.  The
# slack is tests/preview_drive.py's 15 %; the comparison is against the uniform walk of the same run.
R_RAYS = {1: 0.9844, 3: 0.9736}
R_FRAME = {1: 1.2121, 3: 1.1394}
R_DISOCCLUDED = {1: 0.2498, 3: 0.2462}


def test_it_pays(rt, capsys):
    a = rt.api
    got = {}
    for scene_id in (1, 3):
        ref = orbit_reference(rt, scene_id)
        uniform = walk(rt, scene_id, uniform_sampler())
        budget = walk(rt, scene_id, budget_sampler(a.BUDGET_CHUNK, a.BUDGET_TARGET, a.BUDGET_MIN_SAMPLES))
        got[scene_id] = compare(uniform, budget, ref)
    with capsys.disabled():
        print("\nbudget / uniform over an 8-frame orbit: {scene: (rays, frame MSE, disoccluded MSE)} =",
              {k: tuple(round(v[q], 4) for q in ("rays", "frame", "disoccluded")) for k, v in got.items()})
    for scene_id, q in got.items():
        assert q["disoccluded_pixels"] > 0, scene_id
        assert q["rays"] <= 1, (scene_id, q)
        assert q["disoccluded"] <= 1, (scene_id, q)
        assert q["frame"] <= SLACK * R_FRAME[scene_id], (scene_id, q)
        assert q["disoccluded"] <= SLACK * R_DISOCCLUDED[scene_id], (scene_id, q)
