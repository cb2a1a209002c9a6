"""History clipped to the current frame's neighbourhood colours on the GPU: rtiow_history_update_clipped is
rtiow_history_update with the gathered history colour clamped, per channel, to mean +- gamma sigma of the current accumulation's
(2r + 1)^2 window.  The clamp is defined operation by operation in T with plain * + - / and sqrt, so every output is checked BIT FOR BIT
against the numpy restatement below (_clip_np, next to tests/test_history.py's _update_np); history lengths and the pixel count are the
plain update's."""
import ctypes

import numpy as np
import pytest

from tests.test_denoise import _filter_np, _same_bits
from tests.test_history import (E_BADARG, E_STATE, INF, SLACK, _as_base, _begin, _move, _moves, _orbit, _sample, _state, _update_np,
                                orbit_reference)

pytestmark = pytest.mark.gpu

CASES = ((1, 0.75), (2, 1.5), (3, 0.25), (1, 0.0))          # (clip_radius, clip_gamma)


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _default(rt):
    return (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, rt.api.HISTORY_MAX)


# ---- the numpy restatement of section 14

def _clip_np(cur, h, m, radius, gamma):
    """(h clamped, the pixels in which a channel of h changed).  h, m: the gathered history and its capped length of section 11."""
    c, n = cur["c"], cur["n"]
    dt = c.dtype.type
    Hh, W = n.shape
    A = np.zeros_like(c); Q = np.zeros_like(c)
    k = np.zeros((Hh, W), np.int64)
    cp = np.pad(c, ((radius, radius), (radius, radius), (0, 0)))
    vp = np.pad(n > 0, radius)                                   # outside the frame: does not count
    with np.errstate(all="ignore"):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                cq = cp[radius + dy:radius + dy + Hh, radius + dx:radius + dx + W]
                ok = vp[radius + dy:radius + dy + Hh, radius + dx:radius + dx + W]
                A = np.where(ok[..., None], A + cq, A)
                Q = np.where(ok[..., None], Q + cq * cq, Q)
                k = k + ok
        kT = k.astype(c.dtype)[..., None]
        mu = A / kT
        s = Q / kT - mu * mu
        s = np.where(s > 0, s, dt(0))
        e = dt(gamma) * np.sqrt(s)
        lo, hi = mu - e, mu + e
        act = ((m > 0) & (k >= 2))[..., None]
        below = act & (h < lo)
        above = act & ~(h < lo) & (h > hi)
    out = np.where(below, lo, np.where(above, hi, h)).astype(c.dtype)
    assert out.dtype == A.dtype == Q.dtype == c.dtype
    return out, (below | above).any(axis=-1)


def _blend_np(cur, h, m):
    c, n = cur["c"], cur["n"]
    nT = n.astype(c.dtype)
    Mout = m + nT
    with np.errstate(all="ignore"):
        alpha = nT / Mout
        Cout = np.where((Mout > 0)[..., None], h + alpha[..., None] * (c - h), c.dtype.type(0)).astype(c.dtype)
    return Cout, Mout


def _clipped_np(cam, cur, base, params, radius, gamma):
    """Section 11 with the clamp of section 14 between the cap and the blend.  _update_np with c = 0 and n = 0 returns h and m themselves
    (alpha = 0: Cout = h + 0 (0 - h), the bits of h); blending them again with the real c and n must reproduce _update_np's own image."""
    zero = {"c": np.zeros_like(cur["c"]), "n": np.zeros_like(cur["n"]), "N": cur["N"], "t": cur["t"]}
    h, m, carried = _update_np(cam, zero, base, *params)
    plain_c, plain_m, plain_count = _update_np(cam, cur, base, *params)
    again_c, again_m = _blend_np(cur, h, m)
    assert _same_bits(again_c, plain_c) and _same_bits(again_m, plain_m) and carried == plain_count
    hc, mask = _clip_np(cur, h, m, radius, gamma)
    C, M = _blend_np(cur, hc, m)
    return {"C": C, "M": M, "h": h, "m": m, "reprojected": carried, "clipped": int(mask.sum()), "mask": mask, "plain_C": plain_c}


def _check_clipped(r, cam, cur, base, params, radius, gamma, where):
    """A plain update, then the clipped one with the same three arguments, against each other and against the restatement; the clipped
    image is what the handle holds afterwards.  Returns the restatement."""
    plain_count = r.history_update(*params)
    plain_rgb, plain_len = r.history()
    count, clipped = r.history_update_clipped(radius, gamma, *params)
    rgb, length = r.history()
    want = _clipped_np(cam, cur, base, params, radius, gamma)
    assert _same_bits(length, want["M"]), where
    assert _same_bits(rgb, want["C"]), where
    assert (count, clipped) == (want["reprojected"], want["clipped"]), (where, count, clipped, want["reprojected"], want["clipped"])
    assert _same_bits(length, plain_len) and count == plain_count, where
    assert _same_bits(plain_rgb, want["plain_C"]), where
    keep = ~want["mask"]
    assert _same_bits(np.ascontiguousarray(rgb[keep]), np.ascontiguousarray(plain_rgb[keep])), where
    return want


# ---- 1. exactness

@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_clipped_update_is_exact(rt, prec, scene_id, adaptive):
    W, H = 203, 117                                     # not a multiple of 16 in either direction
    params = _default(rt)
    cams = _moves(rt, prec, W, H)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, scene_id, cams["home"])
        _sample(r, adaptive)
        cur = _state(r, adaptive)
        first = _check_clipped(r, cams["home"], cur, None, params, 1, 0.75, "first frame")
        assert first["reprojected"] == 0 and first["clipped"] == 0 and _same_bits(first["C"], cur["c"])
        r.history_commit()
        base = _as_base(cams["home"], cur, first["C"], first["M"])
        for name in ("orbit", "dolly", "roll"):
            _move(r, cams[name], 1228)
            _sample(r, adaptive)
            cur = _state(r, adaptive)
            r.history_plan(*params)
            planned = r.history_plan_lengths() + cur["n"].astype(r.dtype)
            for radius, gamma in CASES:
                where = (prec, scene_id, adaptive, name, radius, gamma)
                want = _check_clipped(r, cams[name], cur, base, params, radius, gamma, where)
                assert _same_bits(planned, r.history()[1]), where
                assert want["clipped"] > 0, where
                if (radius, gamma) == (1, 0.75) and name == "orbit":
                    kept = int(((want["m"] > 0) & ~want["mask"]).sum())
                    print("clipped %d, carried and not clipped %d of %d" % (want["clipped"], kept, W * H))
                    assert want["clipped"] >= 0.01 * W * H and kept >= 0.01 * W * H, (where, want["clipped"], kept)


# ---- 2. gamma = +inf is the plain update

@pytest.mark.parametrize("prec", [32, 64])
def test_infinite_gamma_is_the_plain_update(rt, prec):
    W, H = 150, 90
    params = _default(rt)
    cams = _moves(rt, prec, W, H)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 1, cams["home"])
        r.accumulate(4)
        r.history_update(*params); r.history_commit()
        _move(r, cams["orbit"], 1228)
        r.accumulate(4)
        count = r.history_update(*params)
        rgb, length = r.history()
        assert count > 0.5 * W * H
        for radius in (1, 3):
            assert r.history_update_clipped(radius, 0.0, *params)[1] > 0          # the image between is another one
            assert not _same_bits(r.history()[0], rgb)
            assert r.history_update_clipped(radius, INF, *params) == (count, 0), radius
            got = r.history()
            assert _same_bits(got[0], rgb) and _same_bits(got[1], length), radius


# ---- 3. tile and frame edges

@pytest.mark.parametrize("frame", [(1, 1), (1, 37), (37, 1), (5, 3), (15, 17), (16, 16), (17, 16), (33, 31), (63, 65)], ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("prec", [32, 64])
def test_windows_at_tile_and_frame_edges(rt, prec, frame):
    """The same camera twice with independent noise: every pixel is carried, and the windows cross the frame's edge, cross workgroup
    borders and, in the small frames, exceed the frame."""
    W, H = frame
    params = _default(rt)
    cam = rt.camera_look(prec, W, H, 1, 10)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, cam)
        r.accumulate(3)
        cur = _state(r, False)
        c0, m0, _ = _update_np(cam, cur, None, *params)
        r.history_update(*params); r.history_commit()
        base = _as_base(cam, cur, c0, m0)
        _move(r, cam, 1228)
        r.accumulate(3)
        cur = _state(r, False)
        for radius in (1, 2, 3):
            want = _check_clipped(r, cam, cur, base, params, radius, 0.5, (prec, frame, radius))
            assert want["reprojected"] == W * H, (prec, frame, radius)
            if W * H == 1:
                assert want["clipped"] == 0                  # k = 1: no bounds
            elif W * H >= 15 * 17:
                assert want["clipped"] > 0, (prec, frame, radius)


# ---- 4. unsampled pixels

@pytest.mark.parametrize("prec", [32, 64])
def test_windows_skip_unsampled_pixels(rt, prec):
    W, H = 203, 117
    cams = _moves(rt, prec, W, H)
    params = _default(rt)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, cams["home"])
        _sample(r, True)                                 # every pixel 4 or 8 samples
        cur = _state(r, True)
        c0, m0, _ = _update_np(cams["home"], cur, None, *params)
        r.history_update(*params); r.history_commit()
        base = _as_base(cams["home"], cur, c0, m0)
        _move(r, cams["orbit"], 1228)
        r.history_plan(*params)
        r.accumulate_budget(2, 6.0, 0)                   # min_samples = 0: a pixel whose history reaches the target is not sampled
        cur = _state(r, True)
        sampled = int((cur["n"] > 0).sum())
        assert 0.01 * W * H <= sampled <= 0.99 * W * H, sampled
        for radius, gamma in ((1, 0.75), (3, 0.25)):
            want = _check_clipped(r, cams["orbit"], cur, base, params, radius, gamma, (prec, radius, gamma))
            assert want["clipped"] > 0
            assert (want["mask"] & (cur["n"] == 0)).any()            # a never-sampled pixel is clipped by its sampled neighbours


@pytest.mark.parametrize("prec", [32, 64])
def test_nobody_sampled_clips_nothing(rt, prec):
    W, H = 64, 40
    cams = _moves(rt, prec, W, H)
    params = _default(rt)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, cams["home"])
        r.accumulate(3)
        cur = _state(r, False)
        c0, m0, _ = _update_np(cams["home"], cur, None, *params)
        r.history_update(*params); r.history_commit()
        base = _as_base(cams["home"], cur, c0, m0)
        _move(r, cams["orbit"], 1228)
        _, active = r.accumulate_adaptive(4, 0.0, min_samples=0, max_samples=3)     # 4 more samples would pass max_samples
        assert active == 0 and (r.adaptive_state()[0] == 0).all()
        cur = _state(r, True)
        for radius in (1, 3):
            want = _check_clipped(r, cams["orbit"], cur, base, params, radius, 0.0, (prec, radius))
            rgb, _ = r.history()
            assert want["clipped"] == 0 and want["reprojected"] > 0.5 * W * H
            assert np.isfinite(rgb).all() and _same_bits(rgb, want["h"])             # Cout is the gathered history


# ---- 5. a chain

@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("prec", [32, 64])
def test_a_chain_of_clipped_commits_is_exact(rt, prec, adaptive):
    W, H = 203, 117
    cams = _moves(rt, prec, W, H)
    params = (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, 12.0)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, cams["home"])
        base = None
        for k, name in enumerate(("home", "orbit", "dolly")):
            if k:
                _move(r, cams[name], 1227 + k)
            _sample(r, adaptive)
            cur = _state(r, adaptive)
            want = _check_clipped(r, cams[name], cur, base, params, 1, 0.75, (prec, adaptive, name))
            assert (want["clipped"] > 0) == (k > 0)
            r.history_commit()                            # the base is the clipped image: the next frame is exact only then
            base = _as_base(cams[name], cur, want["C"], want["M"])
        assert float(base["M"].max()) > float(cur["n"].max())


# ---- 6. denoise_history

@pytest.mark.parametrize("prec", [32, 64])
def test_denoise_history_filters_the_clipped_image(rt, prec):
    W, H = 150, 90
    cams = _moves(rt, prec, W, H)
    sig = (0.5, 0.1, 0.1, 1.0)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, cams["home"])
        r.accumulate(4)
        r.history_update(); r.history_commit()
        _move(r, cams["orbit"], 7)
        r.accumulate(4)
        r.history_update()
        plain, _ = r.history()
        assert r.history_update_clipped()[1] > 0
        rgb, _ = r.history()
        n, a, z = r.guides()
        assert not _same_bits(rgb, plain)
        for levels in (1, 3):
            got = r.denoise_history(levels, *sig)
            assert _same_bits(got, _filter_np(rgb, n, a, z, levels, *sig)), (prec, levels)
            assert _same_bits(r.read_denoised(), got)
        ptr, nbytes = r.history_device_ptr()
        assert ptr and nbytes == W * H * 4 * (prec // 8)


# ---- 7. nothing else moved

@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("prec", [32, 64])
def test_clipped_update_leaves_everything_else_alone(rt, prec, adaptive):
    W, H = 128, 72
    cams = _moves(rt, prec, W, H)

    def run(with_clip):
        out = []
        with rt.Renderer(0, prec) as r:
            _begin(r, rt, prec, 1, cams["home"])
            _sample(r, adaptive)
            r.history_update(); r.history_commit()
            _move(r, cams["orbit"])
            _sample(r, adaptive, calls=1)
            r.history_plan()
            if with_clip:
                assert r.history_update_clipped()[1] > 0
                r.history_update_clipped(3, 0.0, 0.0, -1.0, INF, sync=False)
                r.synchronize()
            out += [r.read_framebuffer(), r.read_linear(), r.history_plan_lengths(), *r.guides()]
            if adaptive:
                out += [*r.adaptive_state(), r.variance()]
            out += [np.array([r.history_update()]), *r.history()]             # the base and the guides it is gathered by
            if adaptive:
                r.accumulate_adaptive(4, 0.0, min_samples=8)
            else:
                r.accumulate(3)
            out += [r.read_framebuffer(), r.read_linear(), np.array([r.accumulated_samples])]
            if adaptive:
                out += list(r.adaptive_state())
        return out

    plain, touched = run(False), run(True)
    assert len(plain) == len(touched)
    for k, (a, b) in enumerate(zip(plain, touched)):
        assert _same_bits(a, b), (prec, adaptive, k)


# ---- 8. states and error codes

def test_states_and_error_codes(rt):
    W, H = 96, 64
    npix = W * H
    cams = _moves(rt, 32, W, H)
    nul = (None, None, None)
    nan = float("nan")
    with rt.Renderer(0, 32) as r:
        lib = r._lib
        clip = lambda *a: lib.rtiow_history_update_clipped(r._h, *a, *nul)
        _begin(r, rt, 32, 3, cams["home"])
        assert clip(0.1, 0.9, 8.0, 1, 0.75) == E_STATE                                   # no chunk since the reset
        assert lib.rtiow_read_history(r._h, None, None, npix) == E_STATE
        r.accumulate(2)
        r.history_update(); r.history_commit()
        _move(r, cams["orbit"], 1228)
        assert clip(0.1, 0.9, 8.0, 1, 0.75) == E_STATE                                   # a new camera: no chunk yet
        r.accumulate(2)
        for bad in ((-0.1, 0.9, 8.0), (nan, 0.9, 8.0), (0.1, 1.5, 8.0), (0.1, -1.5, 8.0), (0.1, nan, 8.0), (0.1, 0.9, 0.0), (0.1, 0.9, -1.0),
                    (0.1, 0.9, nan)):
            assert clip(*bad, 1, 0.75) == E_BADARG, bad
        for radius, gamma in ((0, 0.75), (4, 0.75), (-1, 0.75), (1, -0.5), (1, nan), (1, -INF)):
            assert clip(0.1, 0.9, 8.0, radius, gamma) == E_BADARG, (radius, gamma)
        assert lib.rtiow_read_history(r._h, None, None, npix) == E_STATE                 # the refused calls wrote nothing
        count = r.history_update(0.1, 0.9, 8.0)                                          # ... and history() answers as before them
        before = r.history()
        assert clip(0.1, 0.9, 8.0, 0, 0.75) == E_BADARG
        after = r.history()
        assert _same_bits(before[0], after[0]) and _same_bits(before[1], after[1])
        ms, n, k = ctypes.c_float(-1), ctypes.c_uint64(7), ctypes.c_uint64(7)
        assert lib.rtiow_history_update_clipped(r._h, 0.1, 0.9, 8.0, 1, nan, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(k)) == E_BADARG
        assert (ms.value, n.value, k.value) == (0.0, 0, 0)
        assert clip(0.0, -1.0, INF, 1, 0.0) == 0 and clip(0.1, 1.0, 1e-3, 3, INF) == 0    # the ends of the ranges; asynchronous
        assert lib.rtiow_history_update_clipped(r._h, 0.1, 0.9, 8.0, 2, 0.5, None, ctypes.byref(n), None) == 0 and n.value == count
        assert lib.rtiow_history_update_clipped(r._h, 0.1, 0.9, 8.0, 2, 0.5, ctypes.byref(ms), None, ctypes.byref(k)) == 0
        assert ms.value > 0 and 0 < k.value <= count
        assert lib.rtiow_history_commit(r._h) == 0                                       # the commit takes the clipped image
        assert lib.rtiow_read_history(r._h, None, None, npix) == E_STATE
        r.reset_accumulation()
        assert clip(0.1, 0.9, 8.0, 1, 0.75) == E_STATE
    with rt.Renderer(0, 32) as r:                        # a sharded handle: not this either
        _begin(r, rt, 32, 3, cams["home"])
        r.set_shard(1, 3, 8); r.init_rng(1227)
        r.accumulate(2)
        assert r._lib.rtiow_history_update_clipped(r._h, 0.1, 0.9, 8.0, 1, 0.75, *nul) == E_STATE


# ---- 9. it helps

def clip_walk(rt, scene_id, step_deg, clip, max_history=None, frames=8, spp=4, W=320, H=180, B=50, prec=32, denoise=True):
    """tests/test_history.py's orbit_walk with history_update_clipped(*clip) in place of history_update (clip = None: the plain update).
    Returns the linear images of the last frame: temporal image and denoise_history() of it (squared back to linear)."""
    a = rt.api
    params = (a.HISTORY_DEPTH_TOL, a.HISTORY_NORMAL_COS, a.HISTORY_MAX if max_history is None else max_history)
    cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=_orbit(step_deg * k)) for k in range(frames)]
    out = {}
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, scene_id, cams[0])
        for k, cam in enumerate(cams):
            _move(r, cam, 1227 + k)
            r.accumulate(spp)
            if clip is None:
                out["reprojected"], out["clipped"] = r.history_update(*params), 0
            else:
                out["reprojected"], out["clipped"] = r.history_update_clipped(*clip, *params)
            if k == frames - 1:
                out["temporal"] = r.history()[0].astype(np.float64)
                if denoise:
                    out["denoise_history"] = r.denoise_history().astype(np.float64) ** 2
            else:
                r.history_commit()
    return out


def mse(img, ref, sel=None):
    d = (img - ref) ** 2
    return float(np.mean(d if sel is None else d[sel]))


# scripts/history_clip_probe.py measured, on the walks above at the defaults of raytracingincuda_amd/api.py
# (profiles/history_clip/history_clip_probe.json, "defaults"):
#   R_T = MSE(temporal image of the clipped walk) / MSE(temporal image of the plain walk), per (degrees a frame, scene)
# The test allows tests/test_history.py's 15 % over the measured values.
R_T = {(0.5, 1): 0.7969, (0.5, 3): 0.8458, (2.0, 1): 0.7514, (2.0, 3): 0.8415}


@pytest.mark.parametrize("step_deg", [2.0, 0.5])
def test_it_helps(rt, capsys, step_deg):
    clip = (rt.api.HISTORY_CLIP_RADIUS, rt.api.HISTORY_CLIP_GAMMA)
    got = {}
    for scene_id in (1, 3):
        ref = orbit_reference(rt, scene_id, step_deg=step_deg)
        plain = clip_walk(rt, scene_id, step_deg, None, denoise=False)
        clipped = clip_walk(rt, scene_id, step_deg, clip, denoise=False)
        assert clipped["reprojected"] > 0 and clipped["clipped"] > 0
        got[scene_id] = mse(clipped["temporal"], ref) / mse(plain["temporal"], ref)
    with capsys.disabled():
        print("\nclipped / plain temporal MSE after an 8-frame orbit at %g degrees a frame, r = %d, gamma = %g: {scene: ratio} =" % ((step_deg,) + clip),
              {k: round(v, 4) for k, v in got.items()})
    for scene_id, ratio in got.items():
        if step_deg == 2.0:
            assert ratio <= 1, (scene_id, ratio)
        assert ratio <= SLACK * R_T[step_deg, scene_id], (step_deg, scene_id, ratio)
