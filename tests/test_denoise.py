"""Denoised previews of progressive rendering on the GPU: the linear read of the accumulation, the first-hit
guide buffers and the edge-avoiding a-trous filter.  Every output is defined operation by operation in T with plain * + - / and sqrt,
so each is checked BIT FOR BIT against its numpy restatement in tests/preview_model.py (the guides' hit distances against the CPU oracle's
hit_world)."""
import ctypes

import numpy as np
import pytest

from tests.preview_drive import E_BADARG, E_STATE, run_mixed
from tests.preview_drive import setup as _setup    # not a bare `setup`: older pytests take that name for a module hook
from tests.preview_model import filter_np, gamma, guides_np, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


# ---- 1. the linear read

def test_linear_read_is_exact(rt):
    W, H = 203, 117
    for prec in (32, 64):
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3, W, H)
            assert r._lib.rtiow_read_linear(r._h, None, 0) == E_STATE          # no chunk yet
            for k in (3, 5):
                r.accumulate(k)
                lin = r.read_linear()
                assert lin.dtype == r.dtype and lin.shape == (H, W, 3)
                assert same_bits(gamma(lin), r.read_framebuffer()), (prec, k)
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 1, W, H)
            run_mixed(r, 3)
            counts, _ = r.adaptive_state()
            assert len(np.unique(counts)) >= 2
            assert same_bits(gamma(r.read_linear()), r.read_framebuffer()), prec


# ---- 2. the guides

@pytest.mark.parametrize("prec", [32, 64])
def test_guides_are_exact(rt, oracle, prec):
    W, H = 160, 96
    cases = [(3, 3, None), (3, 1, None), (1, 3, None), (1, 1, None), (1, 3, (1, 3, 8))]   # (scene, source GRID/SCALAR, shard)
    for scene_id, source, shard in cases:
        cam = rt.camera(prec, W, H, 1, 10)
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, scene_id, W, H, B=10, source=source, shard=shard)
            rows = r.local_row_map()
            n, a, z = r.guides()
        wn, wa, wz, hit = guides_np(rt, oracle, prec, scene_id, cam, rows)
        assert 0.2 < hit.mean() < 0.99, (scene_id, hit.mean())
        where = (prec, scene_id, source, shard)
        assert same_bits(z, wz), where
        assert same_bits(n, wn), where
        assert same_bits(a, wa), where


# ---- 3. the filter

def _check_filter(r, levels, sig):
    lin = r.read_linear()
    n, a, z = r.guides()
    got = r.denoise(levels, *sig)
    want = filter_np(lin, n, a, z, levels, *sig)
    return same_bits(got, want)


@pytest.mark.parametrize("prec", [32, 64])
def test_filter_is_exact(rt, prec):
    W, H = 203, 117                     # not a multiple of 8 or 16 in either direction
    inf = float("inf")
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H)
        r.accumulate(8)
        for levels, sig in ((1, (0.5, 0.1, 0.1, 1.0)), (5, (0.5, 0.1, 0.1, 1.0)), (5, (inf, 0.2, inf, 0.5)), (5, (inf, inf, inf, inf)),
                            (8, (0.3, inf, 0.1, inf))):
            assert _check_filter(r, levels, sig), ("plain", prec, levels, sig)
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 1, W, H)
        run_mixed(r, 3)
        for levels, sig in ((1, (1.0, 0.2, 0.3, 2.0)), (5, (0.5, 0.1, 0.1, 1.0)), (3, (inf, 0.1, inf, inf))):
            assert _check_filter(r, levels, sig), ("adaptive", prec, levels, sig)


# ---- 4. nothing else moved

def test_denoise_leaves_the_accumulation_alone(rt):
    W, H = 128, 72
    for prec in (32, 64):
        with rt.Renderer(0, prec) as ref:
            _setup(ref, rt, prec, 3, W, H)
            ref.accumulate(4); ref.accumulate(4)
            want = ref.read_framebuffer()
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3, W, H)
            r.accumulate(4)
            fb = r.read_framebuffer()
            r.denoise()
            r.denoise(3, 0.2, 0.3, 0.4, 0.5, sync=False)
            r.synchronize()
            assert same_bits(r.read_framebuffer(), fb), prec
            assert r.accumulated_samples == 4
            r.accumulate(4)
            assert same_bits(r.read_framebuffer(), want), prec
            assert r.accumulated_samples == 8
            ptr, nbytes = r.denoised_device_ptr()
            assert ptr and nbytes == W * H * 3 * (prec // 8)
        with rt.Renderer(0, prec) as r:                  # adaptive: counts, errors and preview stay
            _setup(r, rt, prec, 1, W, H)
            run_mixed(r, 3)
            c0, e0 = r.adaptive_state()
            fb = r.read_framebuffer()
            r.denoise()
            c1, e1 = r.adaptive_state()
            assert same_bits(c1, c0) and same_bits(e1, e0) and same_bits(r.read_framebuffer(), fb), prec


def test_guides_go_stale_and_error_codes(rt):
    W, H = 96, 64
    lib = None
    with rt.Renderer(0, 32) as r:
        lib = r._lib
        _setup(r, rt, 32, 3, W, H)
        npix = W * H
        assert lib.rtiow_read_guides(r._h, None, None, None, npix) == E_STATE          # never rendered
        assert r.render_guides() >= 0
        assert lib.rtiow_read_guides(r._h, None, None, None, npix) == 0
        assert lib.rtiow_read_guides(r._h, None, None, None, npix + 1) == E_BADARG
        n0, _, z0 = r.guides()
        r.set_camera(rt.camera(32, W, H, 1, 25))
        assert lib.rtiow_read_guides(r._h, None, None, None, npix) == E_STATE          # stale after set_camera
        r.set_scene(rt.build_scene(3, 32)); r.init_rng(1227)
        # no chunk since the reset
        assert lib.rtiow_denoise(r._h, 5, 1.0, 1.0, 1.0, 1.0, None) == E_STATE
        assert lib.rtiow_read_linear(r._h, None, 0) == E_STATE
        assert lib.rtiow_read_denoised(r._h, None, 0) == E_STATE
        r.accumulate(2)
        for levels in (0, 9, -1):
            assert lib.rtiow_denoise(r._h, levels, 1.0, 1.0, 1.0, 1.0, None) == E_BADARG, levels
        for bad in (0.0, -1.0, float("nan")):
            for pos in range(4):
                sig = [1.0] * 4
                sig[pos] = bad
                assert lib.rtiow_denoise(r._h, 5, *sig, None) == E_BADARG, (bad, pos)
        assert lib.rtiow_read_denoised(r._h, None, 0) == E_STATE                       # the bad calls filtered nothing
        # rtiow_denoise renders stale guides first, and they are those of rtiow_render_guides
        r.denoise(2)
        n1, _, z1 = r.guides()
        assert same_bits(n1, n0) and same_bits(z1, z0)
        r.reset_accumulation()
        assert lib.rtiow_denoise(r._h, 5, 1.0, 1.0, 1.0, 1.0, None) == E_STATE
    with rt.Renderer(0, 32) as r:                        # a sharded handle: guides yes, denoise no
        _setup(r, rt, 32, 3, W, H, shard=(1, 3, 8))
        r.accumulate(2)
        assert r.read_linear().shape == (r.local_rows, W, 3)
        n, a, z = r.guides()
        assert z.shape == (r.local_rows, W)
        assert lib.rtiow_denoise(r._h, 5, 1.0, 1.0, 1.0, 1.0, None) == E_STATE
        p, nb = ctypes.c_void_p(), ctypes.c_size_t(0)
        assert lib.rtiow_denoised_device_ptr(r._h, ctypes.byref(p), ctypes.byref(nb)) == E_STATE


# ---- 5. it denoises

def test_it_denoises(rt, capsys):
    W, H, B, prec = 320, 180, 50, 32
    ratios = {}
    for scene_id in (1, 3):
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, scene_id, W, H, B=B)
            r.accumulate(1024)
            ref = r.read_linear().astype(np.float64)
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, scene_id, W, H, B=B)
            r.accumulate(16)
            noisy = r.read_linear().astype(np.float64)
            den = r.denoise().astype(np.float64) ** 2
        mse_noisy = float(np.mean((noisy - ref) ** 2))
        mse_den = float(np.mean((den - ref) ** 2))
        ratios[scene_id] = mse_den / mse_noisy
    with capsys.disabled():
        print("\ndenoise MSE ratio (16 spp denoised / 16 spp, against 1024 spp):", {k: round(v, 4) for k, v in ratios.items()})
    for scene_id, q in ratios.items():
        assert q <= 0.5, (scene_id, q)
