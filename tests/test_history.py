"""Temporal history for progressive previews on the GPU: rtiow_history_update reprojects every pixel of the
current camera into the frame committed from an earlier one, gathers the matching history and blends it with the accumulation by sample
count.  Every output is defined operation by operation in T with plain * + - /, so it is checked BIT FOR BIT against the numpy
restatement below; the cameras come from camera_look."""
import ctypes
import math

import numpy as np
import pytest

from tests.test_denoise import _filter_np, _same_bits

pytestmark = pytest.mark.gpu

E_BADARG, E_STATE = -1, -2
INF = float("inf")
LOOKFROM = (13.0, 2.0, 3.0)


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _orbit(deg, lookfrom=LOOKFROM):
    """lookfrom turned by `deg` degrees about the y axis."""
    a = math.radians(deg)
    x, y, z = lookfrom
    return (x * math.cos(a) + z * math.sin(a), y, -x * math.sin(a) + z * math.cos(a))


def _moves(rt, prec, W, H, B=10):
    """The reference's view and three small moves of it: an orbit, a dolly towards the scene and a roll."""
    look = lambda **kw: rt.camera_look(prec, W, H, 1, B, **kw)
    return {"home": look(), "orbit": look(lookfrom=_orbit(1.5)), "dolly": look(lookfrom=tuple(0.96 * v for v in LOOKFROM)),
            "roll": look(vup=(0.05, 1.0, 0.02))}


def _begin(r, rt, prec, scene_id, cam, source=3):
    r.set_camera(cam)
    r.set_scene(rt.build_scene(scene_id, prec))
    r.set_scene_source(source)
    r.init_rng(1227)


def _move(r, cam, seed=1227):
    r.set_camera(cam)
    r.init_rng(seed)


def _sample(r, adaptive, calls=2):
    """Plain chunks, or tests/test_adaptive.py's pattern: everyone 4 samples, then the median error as the threshold (a mix of counts)."""
    if not adaptive:
        for _ in range(calls):
            r.accumulate(3)
        return
    r.accumulate_adaptive(4, 0.0, min_samples=4)
    thr = float(np.median(r.adaptive_state()[1]))
    for _ in range(calls - 1):
        r.accumulate_adaptive(4, thr, min_samples=4)


def _state(r, adaptive):
    """What section 11 reads of the current frame: colour and count of rtiow_read_linear, normal and depth of the guides."""
    c = r.read_linear()
    n = r.adaptive_state()[0] if adaptive else np.full(c.shape[:2], r.accumulated_samples, np.int32)
    normal, _, depth = r.guides()
    return {"c": c, "n": n, "N": normal, "t": depth}


# ---- the numpy restatement of section 11

def _v(field, dt):
    return np.array(field[:], dt)


def _base_constants(cam, dt):
    """In double from the stored fields, each rounded once to T."""
    O, p00, du, dv = (_v(f, np.float64) for f in (cam.center, cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
    a = p00 - O
    w = np.array([du[1] * dv[2] - du[2] * dv[1], du[2] * dv[0] - du[0] * dv[2], du[0] * dv[1] - du[1] * dv[0]])
    f = (a[0] * w[0] + a[1] * w[1]) + a[2] * w[2]
    if f < 0:
        w, f = -w, -f
    with np.errstate(all="ignore"):
        iu = np.float64(1.0) / ((du[0] * du[0] + du[1] * du[1]) + du[2] * du[2])
        iv = np.float64(1.0) / ((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2])
    return {"O": O.astype(dt), "a": a.astype(dt), "w": w.astype(dt), "du": du.astype(dt), "dv": dv.astype(dt), "f": dt(f), "iu": dt(iu), "iv": dt(iv)}


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _update_np(cam, cur, base, depth_tol, normal_cos, max_history):
    """(Cout, Mout, reprojected pixels).  base: None, or {"cam", "H", "M", "N", "z"} as rtiow_history_commit keeps them."""
    c, n, N, t = cur["c"], cur["n"], cur["N"], cur["t"]
    dt = c.dtype.type
    Hh, W = n.shape
    h = np.zeros_like(c)
    m = np.zeros((Hh, W), c.dtype)
    k = _base_constants(base["cam"], dt) if base is not None else None
    if k is not None and base["M"].shape == (Hh, W) and np.isfinite(k["f"]) and k["f"] != 0:
        O, p00, du, dv = (_v(f, dt) for f in (cam.center, cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
        fi = np.arange(W).astype(dt)[None, :, None]
        fj = np.arange(Hh).astype(dt)[:, None, None]
        with np.errstate(all="ignore"):
            D = ((p00 + fi * du) + fj * dv) - O
            hit = t > 0
            d = np.where(hit[..., None], (O + t[..., None] * D) - k["O"], D)
            den = _dot(d, k["w"])
            s = k["f"] / den
            e = s[..., None] * d - k["a"]
            u = _dot(e, k["du"]) * k["iu"]
            v = _dot(e, k["dv"]) * k["iv"]
            te = den / k["f"]
            ok = (den > 0) & (u > dt(-1)) & (u < dt(W)) & (v > dt(-1)) & (v < dt(Hh))
            xf = np.floor(np.where(ok, u, dt(0)))
            yf = np.floor(np.where(ok, v, dt(0)))
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            fx, fy = u - xf, v - yf
            gx, gy = dt(1) - fx, dt(1) - fy
            b = (gx * gy, fx * gy, gx * fy, fx * fy)
            tol = dt(depth_tol) * te
            S = np.zeros_like(c); L = np.zeros((Hh, W), c.dtype); Bs = np.zeros((Hh, W), c.dtype)
            for tap in range(4):
                qx, qy = x0 + (tap & 1), y0 + (tap >> 1)
                inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < Hh)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, Hh - 1)
                Hq, Mq, Nq, zq = base["H"][qyc, qxc], base["M"][qyc, qxc], base["N"][qyc, qxc], base["z"][qyc, qxc]
                same = np.where(hit, (zq > 0) & (np.abs(zq - te) <= tol) & (_dot(N, Nq) >= dt(normal_cos)), zq == 0)
                valid = inside & (Mq > 0) & same
                S = np.where(valid[..., None], S + b[tap][..., None] * Hq, S)
                L = np.where(valid, L + b[tap] * Mq, L)
                Bs = np.where(valid, Bs + b[tap], Bs)
            got = Bs > 0
            h = np.where(got[..., None], S / Bs[..., None], dt(0)).astype(c.dtype)
            m = np.where(got, L / Bs, dt(0)).astype(c.dtype)
            m = np.where(m < dt(max_history), m, dt(max_history)).astype(c.dtype)
    nT = n.astype(c.dtype)
    Mout = m + nT
    with np.errstate(all="ignore"):
        alpha = nT / Mout
        Cout = np.where((Mout > 0)[..., None], h + alpha[..., None] * (c - h), dt(0)).astype(c.dtype)
    return Cout, Mout, int((m > 0).sum())


def _as_base(cam, cur, Cout, Mout):
    return {"cam": cam, "H": Cout, "M": Mout, "N": cur["N"], "z": cur["t"]}


def _check_update(r, cam, cur, base, params, where):
    """history() and the pixel count after an update with `params` against the restatement; returns the restatement."""
    count = r.history_update(*params)
    rgb, length = r.history()
    want_c, want_m, want_count = _update_np(cam, cur, base, *params)
    assert _same_bits(length, want_m), where
    assert _same_bits(rgb, want_c), where
    assert count == want_count, (where, count, want_count)
    return want_c, want_m, want_count


# ---- 1. exactness

@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_update_is_exact(rt, prec, scene_id, adaptive):
    W, H = 203, 117                                     # not a multiple of 16 in either direction
    rt_default = (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, rt.api.HISTORY_MAX)
    cams = _moves(rt, prec, W, H)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, scene_id, cams["home"])
        _sample(r, adaptive)
        cur = _state(r, adaptive)
        c0, m0, _ = _check_update(r, cams["home"], cur, None, rt_default, "first frame")
        r.history_commit()
        base = _as_base(cams["home"], cur, c0, m0)
        sweeps = {"orbit": [rt_default, (0.0, rt_default[1], rt_default[2]), (rt_default[0], -1.0, INF)],
                  "dolly": [rt_default, (rt_default[0], rt_default[1], 2.5), (0.0, -1.0, INF)],
                  "roll": [rt_default, (rt_default[0], -1.0, 2.5), (rt_default[0], rt_default[1], INF)]}
        for name, params_list in sweeps.items():
            _move(r, cams[name], 1228)
            _sample(r, adaptive)
            cur = _state(r, adaptive)
            for params in params_list:
                _, m, count = _check_update(r, cams[name], cur, base, params, (prec, scene_id, adaptive, name, params))
                if params == rt_default:
                    assert count > 0.5 * W * H, (name, count)        # a small move keeps most of the frame
                    assert m.max() > cur["n"].max()
                if params[2] == 2.5:
                    assert (m - cur["n"].astype(m.dtype)).max() <= 2.5


# ---- 2. no history means no change

@pytest.mark.parametrize("prec", [32, 64])
def test_no_history_means_no_change(rt, prec):
    W, H = 150, 90
    cams = _moves(rt, prec, W, H)

    def unchanged(r, adaptive, where):
        lin = r.read_linear()
        n = r.adaptive_state()[0] if adaptive else np.full((r.height, r.width), r.accumulated_samples, np.int32)
        count = r.history_update()
        rgb, length = r.history()
        assert count == 0, where
        assert _same_bits(rgb, lin), where
        assert _same_bits(length, n.astype(r.dtype)), where

    for adaptive in (False, True):
        with rt.Renderer(0, prec) as r:
            _begin(r, rt, prec, 3, cams["home"])
            _sample(r, adaptive)
            unchanged(r, adaptive, "before any commit")
            r.history_commit()
            _move(r, cams["orbit"]); _sample(r, adaptive)
            assert r.history_update() > 0
            r.history_reset()
            unchanged(r, adaptive, "after history_reset")
            r.history_commit()
            r.set_scene(rt.build_scene(3, prec)); r.init_rng(1227); _sample(r, adaptive)
            unchanged(r, adaptive, "after set_scene")
            r.history_commit()
            _move(r, rt.camera_look(prec, W + 10, H, 1, 10)); _sample(r, adaptive)
            unchanged(r, adaptive, "a base of another frame size")
            r.history_commit()
            # facing away from the scene: what the new camera sees lies behind the base camera or outside its frame
            away = rt.camera_look(prec, W + 10, H, 1, 10, lookfrom=(13.0, 2.0, 3.0), lookat=(26.0, 4.0, 6.0))
            _move(r, away); _sample(r, adaptive)
            unchanged(r, adaptive, "a camera facing away")


# ---- 3. oracle-free sanity

def test_same_camera_is_the_count_weighted_mean(rt):
    """fp64: commit, set the same camera again, accumulate: every pixel reprojects onto itself (u, v within rounding of x, y), so M is
    M_base + n and the colour the count-weighted mean of the two accumulations."""
    prec, W, H = 64, 160, 96
    cam = rt.camera_look(prec, W, H, 1, 10)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, cam)
        r.accumulate(6)
        c1 = r.read_linear()
        r.history_update(max_history=INF)
        r.history_commit()
        _move(r, cam, 99)
        r.accumulate(2)
        c2 = r.read_linear()
        count = r.history_update(depth_tol=1e-6, normal_cos=0.999999, max_history=INF)
        rgb, length = r.history()
    assert count == W * H
    assert np.allclose(length, 8.0, rtol=1e-9, atol=0)
    # the bilinear gather lands within rounding of the pixel itself: the neighbours' share of the weight is ~1e-13
    assert np.allclose(rgb, (6.0 * c1 + 2.0 * c2) / 8.0, rtol=1e-9, atol=1e-9 * float(max(c1.max(), c2.max())))


# ---- 4. idempotence and commit

@pytest.mark.parametrize("prec", [32, 64])
def test_update_is_idempotent_and_counts_nothing_twice(rt, prec):
    W, H = 150, 90
    cams = _moves(rt, prec, W, H)
    params = (0.05, 0.8, INF)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 1, cams["home"])
        r.accumulate(4)
        cur = _state(r, False)
        c0, m0, _ = _check_update(r, cams["home"], cur, None, params, "home")
        r.history_commit()
        base = _as_base(cams["home"], cur, c0, m0)
        _move(r, cams["orbit"], 5)
        r.accumulate(2)
        r.history_update(*params)
        first = r.history()
        r.history_update(*params)
        again = r.history()
        assert _same_bits(first[0], again[0]) and _same_bits(first[1], again[1])
        r.accumulate(3)                                   # a further chunk: the update is over the whole accumulation, n = 5
        cur = _state(r, False)
        assert int(cur["n"].max()) == 5
        _, m, _ = _check_update(r, cams["orbit"], cur, base, params, "after a further chunk")
        assert float(m.max()) <= 4 + 5


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("prec", [32, 64])
def test_a_chain_of_commits_is_exact(rt, prec, adaptive):
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
            c, m, count = _check_update(r, cams[name], cur, base, params, (prec, adaptive, name))
            assert (count > 0) == (k > 0)
            r.history_commit()
            base = _as_base(cams[name], cur, c, m)
        assert float(base["M"].max()) > float(cur["n"].max())


# ---- 5. denoise_history

@pytest.mark.parametrize("prec", [32, 64])
def test_denoise_history_is_the_filter_of_the_temporal_image(rt, prec):
    W, H = 150, 90
    cams = _moves(rt, prec, W, H)
    sig = (0.5, 0.1, 0.1, 1.0)
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, 3, cams["home"])
        r.accumulate(4)
        r.history_update(); r.history_commit()
        _move(r, cams["orbit"], 7)
        r.accumulate(4)
        own = r.denoise(3, *sig)
        assert r.history_update() > 0
        rgb, _ = r.history()
        n, a, z = r.guides()
        assert not _same_bits(rgb, r.read_linear())
        for levels in (1, 3):
            got = r.denoise_history(levels, *sig)
            assert _same_bits(got, _filter_np(rgb, n, a, z, levels, *sig)), (prec, levels)
            assert _same_bits(r.read_denoised(), got)
        assert _same_bits(r.denoise(3, *sig), own)       # rtiow_denoise still reads the accumulation
        ptr, nbytes = r.history_device_ptr()
        assert ptr and nbytes == W * H * 4 * (prec // 8)


# ---- 6. nothing else moved

@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("prec", [32, 64])
def test_history_leaves_everything_else_alone(rt, prec, adaptive):
    W, H = 128, 72
    cams = _moves(rt, prec, W, H)

    def run(with_history):
        out = []
        with rt.Renderer(0, prec) as r:
            _begin(r, rt, prec, 1, cams["home"])
            _sample(r, adaptive)
            if with_history:
                r.history_update(); r.history_commit()
            _move(r, cams["orbit"])
            _sample(r, adaptive, calls=1)
            if with_history:
                r.history_update()
                r.denoise_history(2)
                r.history_update(0.0, -1.0, INF, sync=False)
                r.synchronize()
            out += [r.read_framebuffer(), r.read_linear()]
            if adaptive:
                out += list(r.adaptive_state())
            if with_history:
                r.history_commit()
                r.history_reset()
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


# ---- 7. states and error codes

def test_states_and_error_codes(rt):
    W, H = 96, 64
    npix = W * H
    cams = _moves(rt, 32, W, H)
    nul = (None, None)
    with rt.Renderer(0, 32) as r:
        lib = r._lib
        p, nb = ctypes.c_void_p(), ctypes.c_size_t(0)
        stale = lambda: (lib.rtiow_history_commit(r._h), lib.rtiow_read_history(r._h, None, None, npix),
                         lib.rtiow_history_device_ptr(r._h, ctypes.byref(p), ctypes.byref(nb)),
                         lib.rtiow_denoise_history(r._h, 2, 1.0, 1.0, 1.0, 1.0, None))
        _begin(r, rt, 32, 3, cams["home"])
        assert lib.rtiow_history_update(r._h, 0.1, 0.9, 8.0, *nul) == E_STATE           # no chunk since the reset
        assert stale() == (E_STATE,) * 4
        assert lib.rtiow_history_reset(r._h) == 0
        r.accumulate(2)
        for bad in ((-0.1, 0.9, 8.0), (float("nan"), 0.9, 8.0), (0.1, 1.5, 8.0), (0.1, -1.5, 8.0), (0.1, float("nan"), 8.0),
                    (0.1, 0.9, 0.0), (0.1, 0.9, -1.0), (0.1, 0.9, float("nan"))):
            assert lib.rtiow_history_update(r._h, *bad, *nul) == E_BADARG, bad
        assert stale() == (E_STATE,) * 4                                                 # the bad calls wrote nothing
        assert lib.rtiow_history_update(r._h, 0.0, -1.0, INF, *nul) == 0                 # the ends of the ranges; asynchronous
        assert lib.rtiow_history_update(r._h, 0.1, 1.0, 1e-3, *nul) == 0
        assert lib.rtiow_read_history(r._h, None, None, npix) == 0
        assert lib.rtiow_read_history(r._h, None, None, npix + 1) == E_BADARG
        assert lib.rtiow_history_device_ptr(r._h, None, ctypes.byref(nb)) == E_BADARG
        assert lib.rtiow_history_device_ptr(r._h, ctypes.byref(p), ctypes.byref(nb)) == 0 and nb.value == npix * 16
        for levels in (0, 9):
            assert lib.rtiow_denoise_history(r._h, levels, 1.0, 1.0, 1.0, 1.0, None) == E_BADARG
        assert lib.rtiow_denoise_history(r._h, 2, 0.0, 1.0, 1.0, 1.0, None) == E_BADARG
        assert lib.rtiow_denoise_history(r._h, 2, 1.0, 1.0, 1.0, 1.0, None) == 0
        # the temporal image survives a further chunk, an accumulation reset and init_rng (it is what the last update wrote) ...
        r.accumulate(2); r.reset_accumulation(); r.init_rng(3)
        assert lib.rtiow_read_history(r._h, None, None, npix) == 0
        assert lib.rtiow_history_update(r._h, 0.1, 0.9, 8.0, *nul) == E_STATE            # ... but an update needs a chunk
        # ... and goes stale on commit, set_camera, set_scene, set_shard and history_reset
        assert lib.rtiow_history_commit(r._h) == 0
        assert stale() == (E_STATE,) * 4
        for go_stale in (lambda: r.set_camera(cams["orbit"]), lambda: r.set_scene(rt.build_scene(3, 32)), lambda: r.history_reset(),
                         lambda: (r.set_shard(0, 1, 8), r.set_shard(0, 1, 8))):
            r.set_camera(cams["home"]); r.init_rng(1227); r.accumulate(1)
            r.history_update()
            assert lib.rtiow_read_history(r._h, None, None, npix) == 0
            go_stale()
            assert stale() == (E_STATE,) * 4
        # the base survives set_camera, reset_accumulation and init_rng; set_scene, set_shard and history_reset empty it
        for empties, change in ((False, lambda: r.set_camera(cams["orbit"])), (False, lambda: r.reset_accumulation()),
                                (True, lambda: r.set_scene(rt.build_scene(3, 32))), (True, lambda: r.set_shard(0, 1, 4)),
                                (True, lambda: r.history_reset())):
            r.set_camera(cams["home"]); r.init_rng(1227); r.accumulate(1)
            r.history_update(); r.history_commit()
            change()
            r.set_camera(cams["dolly"]); r.init_rng(1227); r.accumulate(1)
            assert (r.history_update() == 0) == empties, empties
    with rt.Renderer(0, 32) as r:                        # a sharded handle: none of it
        lib = r._lib
        _begin(r, rt, 32, 3, cams["home"])
        r.set_shard(1, 3, 8); r.init_rng(1227)
        r.accumulate(2)
        p, nb = ctypes.c_void_p(), ctypes.c_size_t(0)
        assert lib.rtiow_history_reset(r._h) == E_STATE
        assert lib.rtiow_history_update(r._h, 0.1, 0.9, 8.0, *nul) == E_STATE
        assert lib.rtiow_history_commit(r._h) == E_STATE
        assert lib.rtiow_read_history(r._h, None, None, W * r.local_rows) == E_STATE
        assert lib.rtiow_history_device_ptr(r._h, ctypes.byref(p), ctypes.byref(nb)) == E_STATE
        assert lib.rtiow_denoise_history(r._h, 2, 1.0, 1.0, 1.0, 1.0, None) == E_STATE


# ---- 8. it helps

# scripts/history_probe.py measured, on this walk at the default parameters (profiles/history/history_probe.json, "orbit"):
#   q_t  = MSE(temporal) / MSE(noisy), q_dt = MSE(denoise_history) / MSE(denoise), per scene
# The test allows 15 % over the measured values: that covers run-to-run differences in which pixels lose their history at silhouettes.
Q_T = {1: 0.1995, 3: 0.1648}
Q_DT = {1: 0.3909, 3: 0.3713}
SLACK = 1.15


def orbit_reference(rt, scene_id, frames=8, step_deg=0.5, W=320, H=180, B=50, prec=32, ref_samples=1024):
    """The linear image of ref_samples samples at the last camera of orbit_walk."""
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, scene_id, rt.camera_look(prec, W, H, 1, B, lookfrom=_orbit(step_deg * (frames - 1))))
        r.accumulate(ref_samples)
        return r.read_linear().astype(np.float64)


def orbit_walk(rt, scene_id, frames=8, step_deg=0.5, spp=4, W=320, H=180, B=50, prec=32, params=None, ref=None):
    """`frames` cameras, lookfrom turned step_deg about the y axis per frame, spp samples each with independent noise
    (init_rng(1227 + frame)), update and commit every frame.  Returns the linear images of the last frame: reference (orbit_reference),
    noisy accumulation, temporal image, denoise() and denoise_history() (both squared back to linear)."""
    params = params or (rt.api.HISTORY_DEPTH_TOL, rt.api.HISTORY_NORMAL_COS, rt.api.HISTORY_MAX)
    cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=_orbit(step_deg * k)) for k in range(frames)]
    out = {"ref": ref if ref is not None else orbit_reference(rt, scene_id, frames, step_deg, W, H, B, prec)}
    with rt.Renderer(0, prec) as r:
        _begin(r, rt, prec, scene_id, cams[0])
        for k, cam in enumerate(cams):
            _move(r, cam, 1227 + k)
            r.accumulate(spp)
            out["reprojected"] = r.history_update(*params)
            if k == frames - 1:
                out["noisy"] = r.read_linear().astype(np.float64)
                out["temporal"] = r.history()[0].astype(np.float64)
                out["denoise"] = r.denoise().astype(np.float64) ** 2
                out["denoise_history"] = r.denoise_history().astype(np.float64) ** 2
            else:
                r.history_commit()
    return out


def quality(out):
    mse = lambda k: float(np.mean((out[k] - out["ref"]) ** 2))
    return mse("temporal") / mse("noisy"), mse("denoise_history") / mse("denoise")


def test_it_helps(rt, capsys):
    got = {}
    for scene_id in (1, 3):
        got[scene_id] = quality(orbit_walk(rt, scene_id))
    with capsys.disabled():
        print("\nhistory over an 8-frame orbit, 4 spp per frame: {scene: (q_t, q_dt)} =", {k: (round(a, 4), round(b, 4)) for k, (a, b) in got.items()})
    for scene_id, (q_t, q_dt) in got.items():
        assert q_t < 1 and q_dt < 1, (scene_id, q_t, q_dt)
        assert q_t <= SLACK * Q_T[scene_id], (scene_id, q_t)
        assert q_dt <= SLACK * Q_DT[scene_id], (scene_id, q_dt)
