"""Adaptive progressive rendering (rtiow_accumulate_adaptive) on the GPU.  Every pixel stops at its own sample count, and the bar is still
BIT-EXACT: a pixel with count n holds the very bits rtiow_render (and the CPU oracle) give that pixel with samples_per_pixel = n, because
its samples are one sequential RNG chain summed in sample order and every chunk resumes it from its exact state."""
import functools

import numpy as np
import pytest

from tests import preview_drive
from tests.conftest import compact
from tests.preview_drive import one_shot, run_mixed
from tests.preview_model import luminance, positive_part, same_bits

pytestmark = pytest.mark.gpu

SCHEDULES = (0, 1, 2)        # RTIOW_SCHED_STATIC, PERSISTENT, SORTED
SOURCES = (0, 1, 2, 3)       # RTIOW_SCENE_LDS, SCALAR, LDS_EXACT, GRID
_setup = functools.partial(preview_drive.setup, sched=2)


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def test_every_pixel_is_exact_at_its_own_count(rt):
    W, H, B = 320, 192, 25
    for prec in (32, 64):
        for scene_id in (3, 1):
            with rt.Renderer(0, prec) as r:
                _setup(r, rt, prec, scene_id, W, H, B=B)
                run_mixed(r, 4)
                counts, _ = r.adaptive_state()
                img = r.read_framebuffer()
                assert r.accumulated_samples == counts.max()
            distinct = np.unique(counts)
            assert len(distinct) >= 2, (prec, scene_id, distinct)            # the threshold left a mix
            for n in distinct:
                want = one_shot(rt, prec, scene_id, W, H, int(n), B)
                sel = counts == n
                assert same_bits(img[sel], want[sel]), (prec, scene_id, n)


def test_every_pixel_matches_the_oracle_at_its_own_count(rt, oracle):
    W, H, B = 64, 40, 25
    for prec in (32, 64):
        sc = compact(oracle.build_scene(3, prec))
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3, W, H, B=B)
            run_mixed(r, 3)
            counts, _ = r.adaptive_state()
            img = r.read_framebuffer()
        assert len(np.unique(counts)) >= 2
        for n in np.unique(counts):
            want, _ = oracle.render(prec, sc, rt.camera(prec, W, H, int(n), B), 1227)
            sel = counts == n
            assert same_bits(img[sel], want[sel]), (prec, n)


def test_the_decision_rule(rt):
    W, H = 96, 72
    for prec in (32, 64):
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3, W, H)
            c0, e0 = r.adaptive_state()
            assert (c0 == 0).all() and np.isinf(e0).all()
            for samples, min_s, max_s in ((2, 3, 40), (3, 3, 40), (4, 0, 13), (2, 8, 40), (5, 0, 40), (1, 0, 40)):
                cb, eb = r.adaptive_state()
                thr = float(np.quantile(eb[np.isfinite(eb)], 0.4)) if np.isfinite(eb).any() else 0.1
                mask = ((cb < min_s) | (eb.astype(np.float64) > thr)) & (cb.astype(np.int64) + samples <= max_s)
                _, active = r.accumulate_adaptive(samples, thr, min_samples=min_s, max_samples=max_s)
                ca, ea = r.adaptive_state()
                assert active == int(mask.sum()), (prec, samples, min_s, max_s)
                assert np.array_equal(ca, cb + samples * mask.astype(np.int32)), (prec, samples, min_s, max_s)
                assert np.isinf(ea[ca < 2]).all() and np.isfinite(ea[ca >= 2]).all()
                assert r.stats()["primary_rays"] == active * samples


def test_the_error_estimate(rt):
    """err from the library against numpy's, per-sample colours rebuilt from sixteen 1-sample plain previews (acc_n = n * preview^2)."""
    W, H, B, N, prec = 64, 40, 25, 16, 64
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H, B=B)
        prev = np.zeros((H, W, 3))
        ys = []
        for n in range(1, N + 1):
            r.accumulate(1)
            acc = n * r.read_framebuffer().astype(np.float64) ** 2
            ys.append(luminance(acc - prev))
            prev = acc
    ys = np.array(ys)
    s2 = (ys ** 2).sum(axis=0)
    m = luminance(prev) / N
    var = positive_part((s2 - N * m * m) / (N - 1))       # x > 0 ? x : 0, as the library states max(0, x): a NaN gives 0
    want = np.sqrt(var / N) / (m + 1e-3)
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H, B=B)
        r.accumulate_adaptive(N, 0.0, min_samples=N)
        counts, err = r.adaptive_state()
    assert (counts == N).all()
    sel = var > 1e-9 * m * m                                   # above the rounding of the rebuilt colours
    assert sel.mean() > 0.9
    np.testing.assert_allclose(err[sel], want[sel], rtol=1e-3)


def test_limits(rt):
    W, H, B = 64, 40, 25
    for prec in (32, 64):
        # everyone active (min_samples and max_samples at their largest): the preview is the plain accumulation's
        with rt.Renderer(0, prec) as a, rt.Renderer(0, prec) as p:
            _setup(a, rt, prec, 3, W, H, B=B)
            _setup(p, rt, prec, 3, W, H, B=B)
            total = 0
            for k in (2, 3, 5):
                _, active = a.accumulate_adaptive(k, 0.0, min_samples=2 ** 31 - 1, max_samples=2 ** 31 - 1)
                p.accumulate(k)
                total += k
                counts, _ = a.adaptive_state()
                assert active == W * H and (counts == total).all() and a.accumulated_samples == total
                assert same_bits(a.read_framebuffer(), p.read_framebuffer()), (prec, total)
        # rel_error = 0: a pixel stops only when its error is exactly 0 (no spread left that the sums resolve)
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3, W, H, B=B)
            r.accumulate_adaptive(2, 0.0)
            for _ in range(3):
                cb, eb = r.adaptive_state()
                _, active = r.accumulate_adaptive(2, 0.0)
                ca, _ = r.adaptive_state()
                assert active == int((eb != 0).sum()) and np.array_equal(ca - cb, 2 * (eb != 0).astype(np.int32)), prec
        # a huge rel_error: everyone stops at min_samples
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3, W, H, B=B)
            _, active = r.accumulate_adaptive(4, 1e30, min_samples=4)
            assert active == W * H
            for _ in range(2):
                _, active = r.accumulate_adaptive(4, 1e30, min_samples=4)
                assert active == 0
            counts, _ = r.adaptive_state()
            assert (counts == 4).all()
            assert same_bits(r.read_framebuffer(), one_shot(rt, prec, 3, W, H, 4, B))
        # max_samples is never passed, not even for a pixel below min_samples
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3, W, H, B=B)
            for k in range(5):
                _, active = r.accumulate_adaptive(3, 0.0, min_samples=10, max_samples=10)
                counts, _ = r.adaptive_state()
                assert (counts <= 10).all()
                assert active == (W * H if k < 3 else 0)
            assert (counts == 9).all()


def test_schedule_source_and_shards_do_not_change_counts_or_bits(rt):
    W, H, B = 96, 72, 25
    for prec in (32, 64):
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3, W, H, B=B)
            thresholds = run_mixed(r, 3)
            want_counts, _ = r.adaptive_state()
            want_img = r.read_framebuffer()
        assert len(np.unique(want_counts)) >= 2

        def replay(r):
            r.accumulate_adaptive(4, 0.0, min_samples=4)
            for thr in thresholds:
                r.accumulate_adaptive(4, thr, min_samples=4)

        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3, W, H, B=B)
            for sched in SCHEDULES:
                for source in SOURCES:
                    r.set_schedule(sched, 0)
                    r.set_scene_source(source)
                    r.reset_accumulation()
                    replay(r)
                    counts, _ = r.adaptive_state()
                    assert np.array_equal(counts, want_counts), (prec, sched, source)
                    assert same_bits(r.read_framebuffer(), want_img), (prec, sched, source)
        nranks, strip = 2, 8
        full = np.zeros_like(want_img)
        full_counts = np.zeros_like(want_counts)
        for rank in range(nranks):
            with rt.Renderer(0, prec) as r:
                _setup(r, rt, prec, 3, W, H, B=B, shard=(rank, nranks, strip))
                replay(r)
                part = r.read_framebuffer()
                counts, _ = r.adaptive_state()
                rows = r.local_row_map()
            rt.place_rows(full, part, rank, nranks, strip)
            full_counts[rows] = counts
        assert np.array_equal(full_counts, want_counts) and same_bits(full, want_img), prec


def test_render_between_calls_leaves_the_state_alone(rt):
    W, H, B = 96, 72, 25
    for prec in (32, 64):
        with rt.Renderer(0, prec) as a, rt.Renderer(0, prec) as b:
            _setup(a, rt, prec, 3, W, H, S=5, B=B)
            _setup(b, rt, prec, 3, W, H, S=5, B=B)
            a.accumulate_adaptive(4, 0.0, min_samples=4)
            b.accumulate_adaptive(4, 0.0, min_samples=4)
            _, err = a.adaptive_state()
            thr = float(np.median(err))
            b.render(0)
            assert same_bits(b.read_framebuffer(), one_shot(rt, prec, 3, W, H, 5, B))
            b.count_segments(0)
            a.accumulate_adaptive(4, thr, min_samples=4)
            b.accumulate_adaptive(4, thr, min_samples=4)
            assert np.array_equal(a.adaptive_state()[0], b.adaptive_state()[0])
            assert same_bits(a.read_framebuffer(), b.read_framebuffer()), prec


def test_modes_resets_and_errors(rt):
    W, H, B, prec = 64, 40, 25, 32
    cam = rt.camera(prec, W, H, 1, B)
    with rt.Renderer(0, prec) as r:
        with pytest.raises(rt.RtiowError) as e:
            r.accumulate_adaptive(1, 0.1)
        assert e.value.code == -2                                # no camera, no scene
        r.set_camera(cam)
        r.set_scene(rt.build_scene(3, prec))
        with pytest.raises(rt.RtiowError) as e:
            r.accumulate_adaptive(1, 0.1)
        assert e.value.code == -2                                # RNG not initialised
        r.init_rng(1227)
        for args in ((0, 0.1, 0, 10), (-1, 0.1, 0, 10), (1, 0.1, -1, 10), (1, 0.1, 5, 4), (1, -0.5, 0, 10), (1, float("nan"), 0, 10)):
            with pytest.raises(rt.RtiowError) as e:
                r.accumulate_adaptive(args[0], args[1], min_samples=args[2], max_samples=args[3])
            assert e.value.code == -1, args
        assert r._lib.rtiow_read_adaptive_state(r._h, None, None, W * H + 1) == -1

        # the first chunk fixes the mode until a reset
        r.accumulate_adaptive(2, 0.0)
        with pytest.raises(rt.RtiowError) as e:
            r.accumulate(1)
        assert e.value.code == -2
        r.set_scene_source(0)                                    # these keep the state (and the mode)
        r.set_schedule(1, 0)
        with pytest.raises(rt.RtiowError) as e:
            r.accumulate(1)
        assert e.value.code == -2
        r.accumulate_adaptive(3, 0.0, min_samples=5)
        assert (r.adaptive_state()[0] == 5).all()
        r.reset_accumulation()
        r.accumulate(1)
        with pytest.raises(rt.RtiowError) as e:
            r.accumulate_adaptive(1, 0.0)
        assert e.value.code == -2

        resets = {
            "set_camera": lambda r: r.set_camera(cam),
            "set_scene": lambda r: r.set_scene(rt.build_scene(3, prec)),
            "set_shard": lambda r: r.set_shard(0, 1, 8),
            "init_rng": lambda r: r.init_rng(1227),
            "reset_accumulation": lambda r: r.reset_accumulation(),
        }
        want2 = one_shot(rt, prec, 3, W, H, 2, B, source=0, sched=1)
        for name, reset in resets.items():
            r.reset_accumulation()
            r.accumulate_adaptive(2, 0.0)
            reset(r)
            r.init_rng(1227)
            counts, err = r.adaptive_state()
            assert (counts == 0).all() and np.isinf(err).all() and r.accumulated_samples == 0, name
            r.accumulate(1)                                      # plain chunks are allowed again
            r.reset_accumulation()
            _, active = r.accumulate_adaptive(2, 0.0)
            assert active == W * H and same_bits(r.read_framebuffer(), want2), name


def test_a_bound_torch_framebuffer_receives_the_preview(rt, oracle):
    import torch
    W, H, B, prec = 80, 48, 8, 32
    want, _ = oracle.render(prec, compact(oracle.build_scene(3, prec)), rt.camera(prec, W, H, 3, B), 1227)
    fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, W, H, 1, B)); r.set_scene(rt.build_scene(3, prec)); r.init_rng(1227)
        r.bind_framebuffer(fb.data_ptr(), fb.numel() * 4)
        r.accumulate_adaptive(2, 1e30, min_samples=3, max_samples=3, sync=False)   # n = 2
        _, active = r.accumulate_adaptive(1, 1e30, min_samples=3, max_samples=3, sync=False)
        assert active == W * H
        r.synchronize()
        assert r.accumulated_samples == 3
    torch.cuda.synchronize()
    assert same_bits(fb.cpu().numpy(), want)
