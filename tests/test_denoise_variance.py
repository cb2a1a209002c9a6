"""Variance-guided denoising on the GPU: the variance plane of an adaptive accumulation and the a-trous
filter whose colour edge-stop follows it.  The plane is checked against the error the library already publishes and against numpy on
rebuilt samples; the filter, defined operation by operation in T with plain * + - /, BIT FOR BIT against its numpy restatement in
tests/preview_model.py and, with the colour term off, against rtiow_denoise itself."""
import ctypes

import numpy as np
import pytest

from tests.preview_drive import E_BADARG, E_STATE, INF, check_against_err, run_mixed
from tests.preview_drive import setup as _setup    # not a bare `setup`: older pytests take that name for a module hook
from tests.preview_model import luminance, positive_part, same_bits, variance_filter_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _variance_call(r, npix):
    buf = np.empty(max(npix, 1), r.dtype)
    return r._lib.rtiow_read_variance(r._h, buf.ctypes.data, npix)


# ---- 4. the variance plane

@pytest.mark.parametrize("prec", [32, 64])
def test_variance_matches_the_published_error(rt, prec):
    W, H = 203, 117
    with rt.Renderer(0, prec) as r:                      # uniform with variance
        _setup(r, rt, prec, 3, W, H)
        r.accumulate_with_variance(5); r.accumulate_with_variance(3)
        counts, V = check_against_err(r, ("uniform", prec))
        assert (counts == 8).all() and (V > 0).mean() > 0.5
    with rt.Renderer(0, prec) as r:                      # (d) a mix of counts
        _setup(r, rt, prec, 1, W, H)
        run_mixed(r, 3)
        counts, V = check_against_err(r, ("mixed", prec))
        assert len(np.unique(counts)) >= 2
    with rt.Renderer(0, prec) as r:                      # (d) a shard
        _setup(r, rt, prec, 3, W, H, shard=(1, 3, 8))
        run_mixed(r, 2)
        counts, V = check_against_err(r, ("shard", prec))
        assert V.shape == (r.local_rows, W) and 0 < r.local_rows < H
    # (c) counts below two: everyone at 1 sample, and nobody sampled at all (4 more samples would pass max_samples = 3)
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H)
        r.accumulate_adaptive(1, 0.0, min_samples=1, max_samples=1)
        counts, V = check_against_err(r, ("one sample", prec))
        assert (counts == 1).all() and (V == 0).all()
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H)
        _, active = r.accumulate_adaptive(4, 0.0, min_samples=0, max_samples=3)
        counts, V = check_against_err(r, ("no sample", prec))
        assert active == 0 and (counts == 0).all() and (V == 0).all()


def test_variance_against_rebuilt_samples(rt):
    """(b) as tests/test_adaptive.py::test_the_error_estimate: per-sample colours rebuilt from sixteen 1-sample plain previews."""
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
    want = var / N
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H, B=B)
        r.accumulate_with_variance(N)
        counts, _ = r.adaptive_state()
        V = r.variance()
    assert (counts == N).all()
    sel = var > 1e-9 * m * m                                   # above the rounding of the rebuilt colours
    assert sel.mean() > 0.9
    np.testing.assert_allclose(V[sel], want[sel], rtol=1e-3)


# ---- 5. the filter, bit for bit

def _check_filter(r, levels, sig):
    lin = r.read_linear()
    V = r.variance()
    n, a, z = r.guides()
    got = r.denoise_variance(levels, *sig)
    want = variance_filter_np(lin, V, n, a, z, levels, *sig)
    assert np.isfinite(got).all()
    if sig[0] == INF:                                    # the recurrences coincide: the committed kernel gives the same colour
        assert same_bits(got, r.denoise(levels, *sig)), ("against denoise()", levels, sig)
    return same_bits(got, want)


@pytest.mark.parametrize("prec", [32, 64])
def test_filter_is_exact(rt, prec):
    W, H = 203, 117                     # not a multiple of 8 or 16 in either direction
    cases = ((1, (4.0, 0.1, 0.2, 0.05)), (5, (4.0, 0.1, 0.2, 0.05)), (8, (2.5, 0.3, 0.1, 1.0)), (5, (1.0, INF, 0.1, INF)),
             (1, (INF, 0.1, 0.2, 0.05)), (5, (INF, 0.2, INF, 0.5)), (8, (INF, 0.1, 0.2, 0.05)), (5, (INF, INF, INF, INF)), (8, (INF, INF, INF, INF)))
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H)
        r.accumulate_with_variance(4); r.accumulate_with_variance(4)
        for levels, sig in cases:
            assert _check_filter(r, levels, sig), ("uniform", prec, 3, levels, sig)
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 1, W, H)
        run_mixed(r, 3)
        assert len(np.unique(r.adaptive_state()[0])) >= 2
        for levels, sig in cases:
            assert _check_filter(r, levels, sig), ("mixed", prec, 1, levels, sig)
    with rt.Renderer(0, prec) as r:                      # the other pairing, fewer cases
        _setup(r, rt, prec, 1, W, H)
        r.accumulate_with_variance(8)
        for levels, sig in cases[1:3] + cases[5:6]:
            assert _check_filter(r, levels, sig), ("uniform", prec, 1, levels, sig)
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H)
        run_mixed(r, 3)
        for levels, sig in cases[1:3] + cases[5:6]:
            assert _check_filter(r, levels, sig), ("mixed", prec, 3, levels, sig)


def test_uniform_with_variance_is_the_plain_accumulation(rt):
    W, H = 128, 72
    for prec in (32, 64):
        with rt.Renderer(0, prec) as a, rt.Renderer(0, prec) as p:
            _setup(a, rt, prec, 3, W, H)
            _setup(p, rt, prec, 3, W, H)
            for k in (3, 5):
                assert a.accumulate_with_variance(k) >= 0
                p.accumulate(k)
                assert same_bits(a.read_framebuffer(), p.read_framebuffer()) and same_bits(a.read_linear(), p.read_linear()), (prec, k)
            assert a.accumulate_with_variance(2, sync=False) is None
            a.synchronize()
            assert a.accumulated_samples == 10


# ---- 6. nothing else moved

def test_the_new_calls_leave_everything_else_alone(rt):
    W, H = 128, 72
    for prec in (32, 64):
        with rt.Renderer(0, prec) as ref:
            _setup(ref, rt, prec, 1, W, H)
            run_mixed(ref, 4)
            want_fb = ref.read_framebuffer()
            want_counts, want_err = ref.adaptive_state()
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 1, W, H)
            run_mixed(r, 3)
            fb = r.read_framebuffer()
            c0, e0 = r.adaptive_state()
            lin = r.read_linear()
            d0 = r.denoise()
            v0 = r.variance()
            dv = r.denoise_variance()
            assert same_bits(r.read_denoised(), dv), prec               # the last call's image
            assert not same_bits(dv, d0), prec
            assert r.denoise_variance(3, 2.0, 0.2, 0.3, 0.4, sync=False) is None
            r.synchronize()
            assert same_bits(r.read_denoised(), r.denoise_variance(3, 2.0, 0.2, 0.3, 0.4)), prec
            ptr, nbytes = r.denoised_device_ptr()
            assert ptr and nbytes == W * H * 3 * (prec // 8)
            assert same_bits(r.denoise(), d0), prec                       # denoise() before and after
            assert same_bits(r.read_denoised(), d0), prec
            assert same_bits(r.variance(), v0) and same_bits(r.read_linear(), lin), prec
            c1, e1 = r.adaptive_state()
            assert same_bits(c1, c0) and same_bits(e1, e0) and same_bits(r.read_framebuffer(), fb), prec
            # the next chunk's bits: the fourth call of run_mixed, with its threshold (the median error after the first call)
            with rt.Renderer(0, prec) as t:
                _setup(t, rt, prec, 1, W, H)
                t.accumulate_adaptive(4, 0.0, min_samples=4)
                thr = float(np.median(t.adaptive_state()[1]))
            r.accumulate_adaptive(4, thr, min_samples=4)
            c2, e2 = r.adaptive_state()
            assert same_bits(r.read_framebuffer(), want_fb) and same_bits(c2, want_counts) and same_bits(e2, want_err), prec


# ---- 7. states and errors

def test_states_and_error_codes(rt):
    W, H = 96, 64
    npix = W * H
    ok = (5, 4.0, 1.0, 1.0, 1.0)
    with rt.Renderer(0, 32) as r:
        lib = r._lib
        _setup(r, rt, 32, 3, W, H)
        # before any chunk
        assert lib.rtiow_denoise_variance(r._h, *ok, None) == E_STATE
        assert _variance_call(r, npix) == E_STATE
        # after plain chunks
        r.accumulate(2)
        assert lib.rtiow_denoise_variance(r._h, *ok, None) == E_STATE
        assert _variance_call(r, npix) == E_STATE
        assert lib.rtiow_read_denoised(r._h, None, 0) == E_STATE                       # nothing was filtered
        r.reset_accumulation()
        r.accumulate_with_variance(2)
        assert _variance_call(r, npix) == 0
        for bad in (npix + 1, npix - 1, 0):
            assert _variance_call(r, bad) == E_BADARG, bad
        assert lib.rtiow_read_variance(r._h, None, npix) == E_BADARG
        for levels in (0, 9, -1):
            assert lib.rtiow_denoise_variance(r._h, levels, 4.0, 1.0, 1.0, 1.0, None) == E_BADARG, levels
        for bad in (0.0, -1.0, float("nan")):
            for pos in range(4):
                sig = [1.0] * 4
                sig[pos] = bad
                assert lib.rtiow_denoise_variance(r._h, 5, *sig, None) == E_BADARG, (bad, pos)
        assert lib.rtiow_read_denoised(r._h, None, 0) == E_STATE                       # the bad calls filtered nothing
        ms = ctypes.c_float(-1)
        assert lib.rtiow_denoise_variance(r._h, *ok, ctypes.byref(ms)) == 0 and ms.value > 0
        assert r.read_denoised().shape == (H, W, 3)
        # after a reset
        r.reset_accumulation()
        assert lib.rtiow_denoise_variance(r._h, *ok, None) == E_STATE
        assert _variance_call(r, npix) == E_STATE
        # stale guides are rendered first, and a new camera drops the image
        r.accumulate_with_variance(2)
        r.set_camera(rt.camera(32, W, H, 1, 25))
        r.set_scene(rt.build_scene(3, 32)); r.init_rng(1227)
        assert lib.rtiow_read_denoised(r._h, None, 0) == E_STATE
        assert lib.rtiow_read_guides(r._h, None, None, None, npix) == E_STATE
        r.accumulate_with_variance(2)
        assert r.denoise_variance(2).shape == (H, W, 3)
        assert lib.rtiow_read_guides(r._h, None, None, None, npix) == 0
    with rt.Renderer(0, 32) as r:                        # a sharded handle: the plane yes, the filter no
        _setup(r, rt, 32, 3, W, H, shard=(1, 3, 8))
        r.accumulate_with_variance(2)
        assert r.variance().shape == (r.local_rows, W)
        assert _variance_call(r, npix) == E_BADARG
        assert r._lib.rtiow_denoise_variance(r._h, *ok, None) == E_STATE


# ---- 8. it denoises, at every sample count

def test_it_denoises_at_every_sample_count(rt, capsys):
    """q = MSE(denoised) / MSE(noisy) on the linear image against a 1024-sample accumulation, 320 x 180, 50 bounces, fp32: q_fixed from
    denoise() at its defaults (the committed filter), q_var from denoise_variance() at its defaults, at 4, 16 and 64 uniform samples."""
    W, H, B, prec = 320, 180, 50, 32
    q = {}
    for scene_id in (1, 3):
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, scene_id, W, H, B=B)
            r.accumulate(1024)
            ref = r.read_linear().astype(np.float64)
        with rt.Renderer(0, prec) as r, rt.Renderer(0, prec) as p:
            _setup(r, rt, prec, scene_id, W, H, B=B)
            _setup(p, rt, prec, scene_id, W, H, B=B)
            n = 0
            for total in (4, 16, 64):
                r.accumulate_with_variance(total - n)
                p.accumulate(total - n)
                n = total
                lin = r.read_linear()
                assert same_bits(lin, p.read_linear()), (scene_id, n)
                mse_noisy = float(np.mean((lin.astype(np.float64) - ref) ** 2))
                fixed = r.denoise().astype(np.float64) ** 2
                assert same_bits(r.read_denoised(), p.denoise()), (scene_id, n)       # the committed filter sees the same accumulation
                var = r.denoise_variance().astype(np.float64) ** 2
                q[scene_id, n] = (float(np.mean((fixed - ref) ** 2)) / mse_noisy, float(np.mean((var - ref) ** 2)) / mse_noisy)
    with capsys.disabled():
        print("\nMSE ratio denoised / noisy against 1024 spp: (scene, samples): (q_fixed, q_var)")
        for key in sorted(q):
            print("  %s: q_fixed %.4f  q_var %.4f  q_var / q_fixed %.4f" % (key, q[key][0], q[key][1], q[key][1] / q[key][0]))
    for scene_id in (1, 3):
        qf, qv = q[scene_id, 16]
        assert qv <= 1.05 * qf and qv <= 0.5, (scene_id, 16, qf, qv)
        qf, qv = q[scene_id, 4]
        assert qv <= 0.8 * qf, (scene_id, 4, qf, qv)
        qf, qv = q[scene_id, 64]
        assert qv <= 0.85 * qf, (scene_id, 64, qf, qv)
