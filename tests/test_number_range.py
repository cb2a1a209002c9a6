"""The render and the preview chain on overflowed, NaN and subnormal pixels.

Every other image the suite renders holds normal, finite numbers.  tests/range_scene.py edits scene 3's ALBEDOS alone -- rays, hits, RNG
draws and segment counts stay scene 3's, no loop's exit depends on an edited value -- so that colour sums overflow to +inf, become NaN
(inf - inf, 0 inf, a NaN albedo) or stay subnormal.  Each stage is then compared with its numpy definition (tests/preview_model.py and
its companions) fed the device's own inputs: BIT FOR BIT, through same_bits where no NaN can occur (everything gamma-encoded: a NaN sum
is stored as 0) and through same_bits_nan where one can (x86 and gfx950 give a NaN different bits).  Sections A to H are marked gpu;
section Z, not marked, pins on the CPU oracle that the scenes hold what the GPU tests are about, and that each model, perturbed the way
a kernel could be wrong on exactly these inputs, changes pixels of those frames.

What the comparisons settled by text (INTEGRATION.md sections 2, 8, 9, 10):
  * rtiow_render stores 0 for a NaN sum; rtiow_read_linear and everything behind it keep the NaN.
  * max(0, x) in err_p and V_p is x > 0 ? x : 0: a pixel whose sum and s2 both overflowed has err = 0 and V = 0, one with a NaN sum
    err = NaN (never active by its error again) and V = 0.
  * one non-finite pixel reaches, through L levels of a filter, the pixels within Chebyshev distance 2 (2^L - 1), and no others.

Perturbed models that section Z shows to change the pinned frames (each is what a kernel could plausibly compute instead):
  gamma as sqrt(max(c, 0)); the clamp of the variance as var < 0 ? 0 : var; the select's err > rel_error as !(err <= rel_error); the
  clip's h < lo as !(h >= lo); a filter that skips non-finite taps; quantise with the NaN count dropped.

Channels of rtiow_read_linear by class as obtained on an MI355X, range_scene(), NaN / +inf / -inf / subnormal / zero / normal
(test_accumulation_keeps_the_nan_the_framebuffer_drops prints them):

    64 x 40, 2 spp 50 bounces   fp32  99 / 42 / 0 / 180 / 0 / 7359     fp64  111 / 51 / 0 / 153 / 9 / 7356
    64 x 40, 4 spp 12 bounces   fp32 123 / 66 / 0 / 141 / 0 / 7350     fp64  138 / 63 / 0 / 123 / 0 / 7356
    33 x 17, 2 spp 50 bounces   fp32  24 / 21 / 0 /  36 / 0 / 1602     fp64   21 /  9 / 0 /  30 / 0 / 1623
    33 x 17, 4 spp 12 bounces   fp32  36 / 21 / 0 /  21 / 0 / 1605     fp64   36 / 27 / 0 /  15 / 0 / 1605

Pixels of the adaptive state by class, summed over the three chunks of test_adaptive_rule_error_and_variance (NaN sum: err NaN, V 0 /
infinite sum: err 0, V 0 / s2 alone infinite: err +inf, V +inf), 64 x 40: fp32 119 / 55 / 7 and 153 / 71 / 8, fp64 123 / 64 / 0 and
161 / 77 / 0 (in fp64 n m m overflows with s2, so that class is empty).  The clipped update moved 4 to 12 infinite histories to a finite
bound on 64 x 40, none on 33 x 17 in fp32.
"""
import functools

import numpy as np
import pytest

from tests import preview_model as pm
from tests import range_scene as rs
from tests.edge_resolve_model import NO_LAYER, coverage_np, resolve_np
from tests.lens_guides_model import lens_guides_np
from tests.preview_drive import INF, begin, check_clipped, check_update, filter_state, guide_sigmas, history_defaults, move, orbit, state
from tests.preview_model import (as_base, budget_rule, chain_np, feedback_np, filter_np, gamma, gather_np, guides_np, luminance, noise_np, plan_np,
                                 positive_part, same_bits, same_bits_nan, temporal_noise_np, update_np, variance_filter_np)
from tests.upscale_drive import Cpu
from tests.upscale_drive import check as upscale_check
from tests.upscale_model import DENOISED, HISTORY, LINEAR, upscale_np
from tests.upscale_wide_model import upscale_wide_np

FRAMES, SETTINGS = rs.FRAMES, rs.SETTINGS
SIGS = ((0.5, 0.1, 0.1, 1.0), (INF, 0.2, INF, 0.5), (INF, INF, INF, INF))       # denoise: finite and infinite sigmas of tests/test_denoise.py
VSIGS = ((4.0, 0.1, 0.2, 0.05), (INF, 0.1, 0.2, 0.05))                          # denoise_variance: the colour term on and off
LEVELS = (1, 5)
_id = lambda v: "%dx%d" % v if v in FRAMES else "%dspp_%db" % v if v in SETTINGS else str(v)
cases = lambda f: pytest.mark.parametrize("prec", [32, 64])(pytest.mark.parametrize("frame", FRAMES, ids=_id)(
    pytest.mark.parametrize("setting", SETTINGS, ids=_id)(f)))
quiet = functools.partial(np.errstate, all="ignore")


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


# ---- what the tests share: the scenes, and the oracle's frames (computed once, never written)

_CACHE = {}


def _scene(native, prec, name):
    key = ("scene", prec, name)
    if key not in _CACHE:
        _CACHE[key] = {"plain": rs.plain_scene, "range": rs.range_scene, "valid": rs.valid_range_scene}[name](native, prec)
    return _CACHE[key]


def _ref(native, oracle, prec, name, W, H, S, B):
    """(framebuffer, stats) of the CPU oracle."""
    key = ("ref", prec, name, W, H, S, B)
    if key not in _CACHE:
        fb, stats = oracle.render(prec, _scene(native, prec, name), native.camera(prec, W, H, S, B), 1227)
        fb.setflags(write=False)
        _CACHE[key] = (fb, stats)
    return _CACHE[key]


def _pixel_classes(lin):
    """(NaN, infinite, subnormal) pixel masks of a linear image; a pixel is in the first class one of its channels falls in."""
    tiny = np.finfo(lin.dtype).tiny
    with quiet():
        nan = np.isnan(lin).any(-1)
        inf = ~nan & np.isinf(lin).any(-1)
        sub = ~nan & ~inf & ((lin > 0) & (lin < tiny)).any(-1)
    return nan, inf, sub


def _holds_every_class(lin, where):
    nan, inf, sub = _pixel_classes(lin)
    assert nan.any() and inf.any() and sub.any(), (where, int(nan.sum()), int(inf.sum()), int(sub.sum()))
    return nan, inf, sub


def _dilate(mask, radius):
    H, W = mask.shape
    p = np.pad(mask, radius)
    out = np.zeros_like(mask)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            out |= p[dy:dy + H, dx:dx + W]
    return out


# ---- A. the render

@pytest.mark.gpu
@cases
def test_render_is_the_oracles(rt, oracle, prec, frame, setting):
    (W, H), (S, B) = frame, setting
    sc = _scene(rt, prec, "range")
    want, stats = _ref(rt, oracle, prec, "range", W, H, S, B)
    cls = rs.classes(want)
    assert min(cls["inf"], cls["zero"], cls["subnormal"]) >= 1 and not np.isnan(want).any(), cls
    cam = rt.camera(prec, W, H, S, B)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, sc, cam, sched=rt.SCHED_SORTED)
        for sched, threads in ((rt.SCHED_STATIC, 8), (rt.SCHED_PERSISTENT, 0), (rt.SCHED_SORTED, 0)):
            for source in (rt.SCENE_LDS, rt.SCENE_SCALAR, rt.SCENE_LDS_EXACT, rt.SCENE_GRID):
                r.set_schedule(sched); r.set_scene_source(source)
                r.render(threads)
                assert same_bits(r.read_framebuffer(), want), (sched, source)      # strict: a NaN sum reads 0
        assert r.count_segments(0) == stats[1] == _ref(rt, oracle, prec, "plain", W, H, S, B)[1][1]
        fb = r.read_framebuffer()
        lev, nans = r.read_levels()
        host_lev, host_nans = rt.levels(fb)
        assert nans == 0 and host_nans == 0 and np.array_equal(lev, host_lev)
        assert np.isinf(fb).any() and (lev[np.isinf(fb)] == 255).all() and (lev[fb == 0] == 0).all()
        if r.large_grid()["usable"]:                         # the grid reads geometry alone: usable or not as for scene 3
            r.render_large()
            assert same_bits(r.read_framebuffer(), want), "render_large"
    full = np.zeros_like(want)
    for rank in range(2):                                    # a shard: rows are global
        with rt.Renderer(0, prec) as r:
            begin(r, rt, prec, sc, cam, sched=rt.SCHED_SORTED, shard=(rank, 2, 8))
            r.render(0)
            rt.place_rows(full, r.read_framebuffer(), rank, 2, 8)
    assert same_bits(full, want), "shards"


# ---- B. the accumulation

@pytest.mark.gpu
@cases
def test_accumulation_keeps_the_nan_the_framebuffer_drops(rt, oracle, prec, frame, setting):
    (W, H), (S, B) = frame, setting
    sc = _scene(rt, prec, "range")
    want = _ref(rt, oracle, prec, "range", W, H, S, B)[0]
    plain = _ref(rt, oracle, prec, "plain", W, H, S, B)[0]
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, sc, rt.camera(prec, W, H, 1, B), sched=rt.SCHED_SORTED)
        for chunks in ((S,), (1,) * S, (1, S - 1), (S - 1, 1)):
            r.reset_accumulation()
            total = 0
            for k in chunks:
                r.accumulate(k)
                total += k
                assert same_bits(r.read_framebuffer(), _ref(rt, oracle, prec, "range", W, H, total, B)[0]), (chunks, total)
            lin, fb = r.read_linear(), r.read_framebuffer()
            assert same_bits(fb, want) and same_bits(gamma(lin), fb), chunks
        nan, inf, sub = _holds_every_class(lin, "read_linear")
        # the NaN is where the framebuffer reads 0 and scene 3's does not; a colour that underflowed to exactly 0 (dark on dark) reads 0
        # without being one
        zero = lin == 0
        assert np.array_equal(np.isnan(lin), (fb == 0) & (plain != 0) & ~zero) and zero.sum() < np.isnan(lin).sum()
        assert not (lin == -np.inf).any() and np.array_equal(lin == np.inf, fb == np.inf)
        print("\nread_linear classes", prec, frame, setting, rs.linear_classes(lin))
        r.reset_accumulation()                               # the adaptive route to the same sums
        r.accumulate_with_variance(1); r.accumulate_with_variance(S - 1)
        assert same_bits(r.read_framebuffer(), want) and same_bits_nan(r.read_linear(), lin)


# ---- C. the adaptive state

def _check_noise(r, where):
    """err and V of sections 8 and 10 by class of the pixel's sum: s2 cannot be read back, but what it must hold in each class can be
    said -- a NaN sum: the estimate is NaN, positive_part gives var = 0, so V = 0 and err = 0 / NaN; an infinite sum: a sample's
    luminance overflowed, so did its square, s2 = +inf, var = inf - inf, again 0, err = 0 / inf = 0; a finite sum with V = +inf:
    s2 = +inf alone, err = +inf; everything else: err = sqrt(V) / (m + 1e-3) as tests/preview_drive.py's check_against_err has it."""
    counts, err = r.adaptive_state()
    V, lin = r.variance(), r.read_linear()
    dt = lin.dtype.type
    have = counts >= 2
    assert (V[~have] == 0).all() and (err[~have] == np.inf).all(), where
    nan, inf, _ = _pixel_classes(lin)
    e, v = noise_np(np.nan, np.nan, 2, dt)
    assert np.isnan(e) and v == 0
    assert np.isnan(err[have & nan]).all() and same_bits(V[have & nan], np.zeros(int((have & nan).sum()), dt)), where
    e, v = noise_np(np.inf, np.inf, 2, dt)
    assert e == 0 and v == 0
    assert (err[have & inf] == 0).all() and same_bits(V[have & inf], np.zeros(int((have & inf).sum()), dt)), where
    finite = have & ~nan & ~inf
    assert not np.isnan(V).any() and not np.isnan(err[finite]).any() and (V >= 0).all(), where
    over = finite & np.isinf(V)
    assert (err[over] == np.inf).all(), where
    rest = finite & ~over
    with quiet():
        m = luminance(lin.astype(np.float64))
        np.testing.assert_allclose(np.sqrt(V.astype(np.float64))[rest] / (m[rest] + 1e-3), err[rest].astype(np.float64), rtol=1e-5, atol=1e-12,
                                   err_msg=str(where))
    return counts, err, V, (nan, inf, over)


@pytest.mark.gpu
@cases
def test_adaptive_rule_error_and_variance(rt, oracle, prec, frame, setting):
    (W, H), (S, B) = frame, setting
    sc = _scene(rt, prec, "range")
    met = np.zeros(3, np.int64)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, sc, rt.camera(prec, W, H, 1, B), sched=rt.SCHED_SORTED)
        for chunk, (samples, min_s, quantile) in enumerate(((S, S, None), (2, 0, 0.5), (1, 0, 0.3))):
            cb, eb = r.adaptive_state()
            with quiet():
                known = eb[np.isfinite(eb) & (eb > 0)]
                thr = 0.0 if quantile is None else float(np.quantile(known, quantile))
                mask = (cb < min_s) | (eb.astype(np.float64) > thr)               # NaN compares false: section 8's rule as written
            _, active = r.accumulate_adaptive(samples, thr, min_samples=min_s)
            ca, ea, V, (nan, inf, over) = _check_noise(r, (prec, frame, setting, chunk))
            assert active == int(mask.sum()) and np.array_equal(ca, cb + samples * mask.astype(np.int32)), chunk
            met += (int(nan.sum()), int(inf.sum()), int(over.sum()))
            if chunk:                                        # a NaN error and a 0 error stop a pixel; +inf keeps it running
                assert not mask[np.isnan(eb)].any() and not mask[eb == 0].any() and mask[eb == np.inf].all(), chunk
                assert np.isnan(eb).any() and (eb == 0).any() and 0 < active < W * H, chunk
            img = r.read_framebuffer()
            for n in np.unique(ca):
                sel = ca == n
                assert same_bits(img[sel], _ref(rt, oracle, prec, "range", W, H, int(n), B)[0][sel]), (chunk, n)
            assert same_bits(gamma(r.read_linear()), img), chunk
        assert len(np.unique(ca)) >= 2 and (met[:2] > 0).all(), met
        print("\nadaptive classes (NaN sum, infinite sum, s2 alone infinite), summed over three chunks", prec, frame, setting, met)


# ---- D. the guides and the filters

def _spoiled(img):
    """Pixels of a gamma-encoded image that a non-finite value reached: a NaN is stored as 0, an infinity stays."""
    return (~np.isfinite(img) | (img == 0)).any(-1)


def _large(a):
    """Pixels with a finite channel so large that the square of a difference with it can overflow: (dx dx + dy dy) + dz dz stays finite
    while every |d| is below sqrt(max / 3), so while every channel is below half of that."""
    with quiet():
        return (np.abs(a) >= np.sqrt(np.finfo(a.dtype).max / 12)).any(-1)


def _check_reach(out, levels, bad_in, colour, albedo, where):
    """The property that needs no model: the spoiled pixels of the output contain every non-finite input pixel and lie within Chebyshev
    distance 2 (2^L - 1) of one -- or of a pixel whose colour or albedo is finite and _large: its squared distance overflows, and a
    term that sigma = +inf turns off is a product with 0, so inf 0 = NaN (a finite sigma gives w = 0 there, which is harmless).
    A 0 is not a stored NaN where the pixel's own input channel is subnormal or 0: the centre tap's w c, at most 9/64 of it, then rounds
    to 0 with every other tap's, and the sum is an honest 0 (a normal c keeps its pixel positive through every level: each level's
    output is at least 9/64 of its input)."""
    tiny = np.finfo(out.dtype).tiny
    with quiet():
        underflow = (out == 0) & (np.abs(colour) < tiny)
    assert not (bad_in & ~_spoiled(out)).any(), (where, levels, "a non-finite input pixel came out finite")
    reached = ((~np.isfinite(out) | (out == 0)) & ~underflow).any(-1)
    sources = bad_in | _large(colour) | _large(albedo)
    assert not (reached & ~_dilate(sources, 2 * ((1 << levels) - 1))).any(), (where, levels, "beyond the reach")


@pytest.mark.gpu
@pytest.mark.parametrize("guides", ["first_hit", "specular", "lens"])
@cases
def test_filters_are_their_definitions(rt, oracle, prec, frame, setting, guides):
    (W, H), (S, B) = frame, setting
    sc = _scene(rt, prec, "range")
    params = history_defaults(rt)
    home = rt.camera_look(prec, W, H, 1, B)
    moved = rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(1.5))
    where = (prec, frame, setting, guides)
    with rt.Renderer(0, prec) as r:
        if guides != "first_hit":
            r.set_guide_mode(rt.GUIDES_SPECULAR, 8, INF)
        if guides == "lens":
            r.set_guide_lens(2)
        begin(r, rt, prec, sc, home, sched=rt.SCHED_SORTED)
        r.accumulate_with_variance(S)
        r.history_update(*params); r.history_commit()
        move(r, moved, 1228)
        r.accumulate_with_variance(S)
        r.history_update(*params)
        # the guides against the CPU: the albedo is NaN / inf on the edited spheres
        rows = np.arange(H)
        n1, a1, z1 = r.guides()
        wn, wa, wz, _ = guides_np(rt, oracle, prec, sc, moved, rows)
        assert same_bits(n1, wn) and same_bits(z1, wz) and same_bits_nan(a1, wa), where
        assert np.isnan(a1).any() and np.isinf(a1).any(), where
        N, A, Z = filter_state(r)
        with quiet():
            if guides == "specular":
                cn, ca, cz = chain_np(rt, oracle, prec, sc, moved, rows, 8, INF)[:3]
            elif guides == "lens":
                cn, ca, cz = lens_guides_np(rt, oracle, prec, sc, moved, rows, 2, 8, INF)[:3]
            else:
                cn, ca, cz = wn, wa, wz
        assert same_bits(N, cn) and same_bits(Z, cz) and same_bits_nan(A, ca), where
        lin, V = r.read_linear(), r.variance()
        C, M = r.history()
        counts = r.adaptive_state()[0]
        _holds_every_class(lin, where)
        assert not np.isfinite(C).all() and np.isfinite(M).all(), where
        bad_guides = ~(np.isfinite(N).all(-1) & np.isfinite(A).all(-1) & np.isfinite(Z))
        bad_lin = bad_guides | ~np.isfinite(lin).all(-1)
        bad_C = bad_guides | ~np.isfinite(C).all(-1)
        for levels in LEVELS:
            with quiet():
                for sig in SIGS:
                    got = r.denoise(levels, *sig)
                    assert same_bits(got, filter_np(lin, N, A, Z, levels, *sig)), (where, "denoise", levels, sig)
                    _check_reach(got, levels, bad_lin, lin, A, where + ("denoise", sig))
                    got = r.denoise_history(levels, *sig)
                    assert same_bits(got, filter_np(C, N, A, Z, levels, *sig)), (where, "denoise_history", levels, sig)
                    _check_reach(got, levels, bad_C, C, A, where + ("denoise_history", sig))
                for sig in VSIGS:
                    got = r.denoise_variance(levels, *sig)
                    assert same_bits(got, variance_filter_np(lin, V, N, A, Z, levels, *sig)), (where, "denoise_variance", levels, sig)
                    _check_reach(got, levels, bad_lin, lin, A, where + ("denoise_variance", sig))
                    if sig[0] == INF:
                        assert same_bits(got, r.denoise(levels, *sig)), (where, "against denoise()", levels)
                    for radius in (1, 3):
                        got = r.denoise_history_variance(levels, *sig, radius)
                        v0 = r.history_variance()
                        want_v0 = temporal_noise_np(C, M, counts, V, radius)
                        assert same_bits_nan(v0, want_v0), (where, "history_variance", radius)
                        assert same_bits(got, variance_filter_np(C, want_v0, N, A, Z, levels, *sig)), (where, "denoise_history_variance", levels, sig, radius)
                        _check_reach(got, levels, bad_C, C, A, where + ("denoise_history_variance", sig, radius))


# ---- E. the history

@pytest.mark.gpu
@cases
def test_history_carries_clips_and_feeds_back_non_finite_colours(rt, prec, frame, setting):
    """A two-frame orbit and a three-commit chain, on the range scene and on scene 3 side by side: the lengths, the plans and the counts do
    not read colour, so the two handles agree on them bit for bit."""
    (W, H), (S, B) = frame, setting
    params = history_defaults(rt)
    sig = (rt.api.HISTORY_FEEDBACK_SIGMA_COLOR,) + guide_sigmas(rt)
    cams = [rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(deg)) for deg in (0.0, 1.5, 3.0, 0.0)]
    where = (prec, frame, setting)
    with rt.Renderer(0, prec) as r, rt.Renderer(0, prec) as p:
        begin(r, rt, prec, _scene(rt, prec, "range"), cams[0], sched=rt.SCHED_SORTED)
        begin(p, rt, prec, _scene(rt, prec, "plain"), cams[0], sched=rt.SCHED_SORTED)
        both = lambda call: (call(r), call(p))

        def lengths_agree(tag):
            assert same_bits(r.history()[1], p.history()[1]) and np.array_equal(r.adaptive_state()[0], p.adaptive_state()[0]), (where, tag)

        # commit 1: the home view, every pixel S samples
        both(lambda h: h.accumulate_with_variance(S))
        cur = state(r, True)
        _holds_every_class(cur["c"], where)
        c0, m0, _ = check_update(r, cams[0], cur, None, params, where + ("no base",), same_bits_nan)
        p.history_update(*params)
        lengths_agree("home")
        both(lambda h: h.history_commit())
        base = as_base(cams[0], cur, c0, m0)

        # frame 2: the orbit, sampled by the plan; plain and clipped updates; commit 2 through the filter
        both(lambda h: move(h, cams[1], 1228))
        both(lambda h: h.history_plan(*params))
        plan = r.history_plan_lengths()
        assert same_bits(plan, p.history_plan_lengths()), where
        for samples, target, min_s in ((2, 6.0, 0), (1, 3.0, 1)):
            cb = r.adaptive_state()[0]
            mask = budget_rule(cb, plan, samples, target, min_s, 2 ** 31 - 1)
            got = both(lambda h: h.accumulate_budget(samples, target, min_s)[1])
            assert got[0] == got[1] == int(mask.sum()) and np.array_equal(r.adaptive_state()[0], cb + samples * mask.astype(np.int32)), where
        cur = state(r, True)
        assert len(np.unique(cur["n"])) >= 2, where
        assert same_bits(plan, plan_np(cams[1], cur["N"], cur["t"], base, params)[0]), where
        with quiet():
            h, m = gather_np(cams[1], cur, base, *params)
        assert np.isnan(h).any() and np.isinf(h).any() and np.isfinite(m).all(), (where, "nothing non-finite was reprojected")
        with quiet():
            check_update(r, cams[1], cur, base, params, where + ("orbit",), same_bits_nan)
            p.history_update(*params)
            lengths_agree("orbit")
            for radius in (1, 3):
                want = check_clipped(r, cams[1], cur, base, params, radius, rt.api.HISTORY_CLIP_GAMMA, where + ("clipped", radius), same_bits_nan)
                assert want["clipped"] > 0, (where, radius)
                print("\nclipped", where, radius, want["clipped"], "of them infinite history moved to a finite bound:",
                      int((np.isinf(want["h"]) & np.isfinite(want["C"])).any(-1).sum()))
                p.history_update_clipped(radius, rt.api.HISTORY_CLIP_GAMMA, *params)
                lengths_agree(("clipped", radius))
            C, M = r.history()
            N, A, Z = filter_state(r)
            r.history_commit_filtered(*sig, feedback=0.5); p.history_commit_filtered(*sig, feedback=0.5)
            rgb, length = r.history_base()
            want_rgb, want_m = feedback_np(C, M, N, A, Z, sig, 0.5)
        assert same_bits(length, want_m) and same_bits(length, p.history_base()[1]) and same_bits_nan(rgb, want_rgb), where
        assert np.isnan(rgb).any() and int(np.isnan(rgb).any(-1).sum()) > int(np.isnan(C).any(-1).sum()), (where, "the filtered commit spread no NaN")
        bad = ~(np.isfinite(C).all(-1) & np.isfinite(N).all(-1) & np.isfinite(A).all(-1) & np.isfinite(Z))
        assert not (~np.isfinite(rgb).all(-1) & ~_dilate(bad, 2)).any(), (where, "the filtered commit reached beyond its one level")
        base = as_base(cams[1], cur, rgb, M)

        # frame 3: from the filtered base; commit 3; frame 4: back home
        for k, seed in ((2, 1229), (3, 1230)):
            both(lambda h: move(h, cams[k], seed))
            both(lambda h: h.history_plan(*params))
            both(lambda h: h.accumulate_with_variance(S))
            cur = state(r, True)
            assert same_bits(r.history_plan_lengths(), p.history_plan_lengths()), (where, k)
            with quiet():
                assert same_bits(r.history_plan_lengths(), plan_np(cams[k], cur["N"], cur["t"], base, params)[0]), (where, k)
                c, m, count = check_update(r, cams[k], cur, base, params, where + ("frame", k), same_bits_nan)
            p.history_update(*params)
            lengths_agree(k)
            assert count > 0.5 * W * H and not np.isfinite(c).all(), (where, k)
            both(lambda h: h.history_commit())
            base = as_base(cams[k], cur, c, m)


# ---- F. edge resolve and the upscalers

@pytest.mark.gpu
@cases
def test_edge_resolve_and_upscalers(rt, oracle, prec, frame, setting):
    (W, H), (S, B) = frame, setting
    sc = _scene(rt, prec, "range")
    cam = rt.camera_look(prec, W, H, 1, B)
    cpu = Cpu(rt, oracle)
    G = 2
    where = (prec, frame, setting)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, sc, cam, sched=rt.SCHED_SORTED)
        r.accumulate(S)
        _holds_every_class(r.read_linear(), where)
        r.history_update()
        r.render_coverage(G)
        layers = coverage_np(oracle, prec, sc, cam, np.arange(H), G)
        for name, a, b in zip(("ids", "counts", "normal", "depth"), r.coverage(), layers):
            assert same_bits(a, b), (where, name)
        g = r.denoise(1)
        assert _spoiled(g).any() and np.isfinite(g).all(), where     # an infinite pixel leaves the filter as a NaN (inf - inf), stored as 0
        Nf, _, Zf = r.guides()
        for radius, sn, sz, prior in ((1, 0.3, 0.5, 8.0), (3, INF, 2.0, INF)):
            g = r.denoise(1)                                 # a denoised image is resolved once
            count = r.resolve_edges(radius, sn, sz, prior)
            out = r.read_denoised()
            with quiet():
                want, wrote = resolve_np(g, *layers[:4], Nf, Zf, np.full((H, W), S, np.int32), G * G, radius, sn, sz, prior)
            assert same_bits(out, want) and count == int(wrote.sum()), (where, radius, int((out != want).any(-1).sum()))
            mixed = layers[0][..., 1] != NO_LAYER
            assert same_bits(np.ascontiguousarray(out[~mixed]), np.ascontiguousarray(g[~mixed])), where
        with quiet():
            for F in (2, 3):
                for source in (DENOISED, LINEAR, HISTORY):
                    for share in (0, 1):
                        setting_u = (F, 0.3, 0.1, 0.5, share)
                        out = upscale_check(r.upscale, upscale_np, r, cpu, prec, sc, cam, source, setting_u, G, where + ("upscale",))
                        assert _spoiled(out).any(), (where, F, source, share)
                        out = upscale_check(r.upscale_wide, upscale_wide_np, r, cpu, prec, sc, cam, source, setting_u, G, where + ("upscale_wide",))
                        assert _spoiled(out).any(), (where, F, source, share)


# ---- G. valid input alone: finite albedos >= 0, the ground at 1e7

@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES, ids=_id)
@pytest.mark.parametrize("prec", [32, 64])
def test_valid_input_that_overflows_fp32(rt, oracle, prec, frame):
    W, H = frame
    S, B = 2, 50
    sc = _scene(rt, prec, "valid")
    params = history_defaults(rt)
    want = _ref(rt, oracle, prec, "valid", W, H, S, B)[0]
    same = same_bits_nan if prec == 32 else same_bits         # fp64 stays finite: strict all the way
    assert np.isinf(want).any() if prec == 32 else np.isfinite(want).all()
    home = rt.camera(prec, W, H, S, B)
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, sc, home, sched=rt.SCHED_SORTED)
        r.render(0)
        assert same_bits(r.read_framebuffer(), want)
        for chunk, (samples, min_s) in enumerate(((1, 1), (1, 2), (2, 0))):
            cb, eb = r.adaptive_state()
            with quiet():
                thr = 0.0 if chunk < 2 else float(np.median(eb[np.isfinite(eb)]))
                mask = (cb < min_s) | (eb.astype(np.float64) > thr)
            _, active = r.accumulate_adaptive(samples, thr, min_samples=min_s)
            ca, ea, V, (nan, inf, over) = _check_noise(r, (prec, frame, chunk))
            assert active == int(mask.sum()) and np.array_equal(ca, cb + samples * mask.astype(np.int32)), chunk
            if chunk == 1:
                assert same_bits(r.read_framebuffer(), want)
        lin = r.read_linear()
        if prec == 32:
            assert np.isinf(lin).any() and (nan | inf | over).any()
        else:
            assert np.isfinite(lin).all() and np.isfinite(V).all() and np.isfinite(ea[ca >= 2]).all()
        N, A, Z = filter_state(r)
        assert np.isfinite(A).all()
        with quiet():
            for levels in LEVELS:
                for sig in VSIGS:
                    got = r.denoise_variance(levels, *sig)
                    assert same_bits(got, variance_filter_np(lin, V, N, A, Z, levels, *sig)), (prec, frame, levels, sig)
                    assert prec == 32 or np.isfinite(got).all()
            cur = state(r, True)
            c0, m0, _ = check_update(r, home, cur, None, params, "no base", same)
            r.history_commit()
            moved = rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(1.5))
            move(r, moved, 1228)
            r.accumulate_with_variance(S)
            c1, _, count = check_update(r, moved, state(r, True), as_base(home, cur, c0, m0), params, "orbit", same)
        assert count > 0.5 * W * H and (prec == 32) != bool(np.isfinite(c1).all())


# ---- H. rtiow_read_levels with real NaNs: only a framebuffer the caller wrote into holds one

@pytest.mark.gpu
@pytest.mark.parametrize("frame", [(33, 17), (1, 1)], ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("prec", [32, 64])
def test_levels_count_the_nans_a_caller_wrote(rt, prec, frame):
    import torch
    W, H = frame
    n = W * H * 3
    assert n % 4 == 3                                        # the last lane's word is a tail of three channels
    fb = torch.zeros((H, W, 3), dtype=torch.float32 if prec == 32 else torch.float64, device="cuda:0")
    with rt.Renderer(0, prec) as r:
        begin(r, rt, prec, _scene(rt, prec, "range"), rt.camera(prec, W, H, 2, 12))
        r.bind_framebuffer(fb.data_ptr(), fb.numel() * fb.element_size())
        r.render(0)
        torch.cuda.synchronize()
        lev, nans = r.read_levels()
        host = fb.cpu().numpy()
        assert nans == 0 and np.array_equal(lev, rt.levels(host)[0]) and not np.isnan(host).any()
        flat = fb.view(-1)
        written = {0, n - 1}                                 # the first channel and the last (in the tail)
        flat[0] = float("nan"); flat[n - 1] = float("nan")
        if H > 1:
            fb[H // 2, :, :] = float("nan")                  # a whole row
            fb[3, 5, 1] = float("nan")                       # an isolated channel
            written |= set(range((H // 2) * W * 3, (H // 2 + 1) * W * 3)) | {(3 * W + 5) * 3 + 1}
        torch.cuda.synchronize()
        lev, nans = r.read_levels()
        host = fb.cpu().numpy()
        host_lev, host_nans = rt.levels(host)
        assert nans == host_nans == len(written) == int(np.isnan(host).sum()), (nans, host_nans, len(written))
        assert np.array_equal(lev, host_lev)
        assert np.array_equal(lev[~np.isnan(host)], rt.levels(np.nan_to_num(host, nan=0.5))[0][~np.isnan(host)])


# ---- Z. on the CPU oracle alone (no GPU): the scenes hold what the tests are about, and perturbed models change those frames

@pytest.mark.parametrize("setting", SETTINGS, ids=_id)
@pytest.mark.parametrize("prec", [32, 64])
def test_cpu_range_scene_holds_every_class(native, oracle, prec, setting):
    W, H = FRAMES[0]
    S, B = setting
    plain, edited = _scene(native, prec, "plain"), _scene(native, prec, "range")
    for key in ("center_radius", "refraction_index", "type", "valid"):        # albedo edits alone
        assert same_bits(plain[key], edited[key]), key
    assert same_bits(plain["albedo_fuzz"][:, 3].copy(), edited["albedo_fuzz"][:, 3].copy())
    fb, stats = _ref(native, oracle, prec, "range", W, H, S, B)
    fb0, stats0 = _ref(native, oracle, prec, "plain", W, H, S, B)
    cls, cls0 = rs.classes(fb), rs.classes(fb0)
    assert min(cls["inf"], cls["zero"], cls["subnormal"]) >= 8 and cls["normal"] >= 2000, cls
    assert cls0["inf"] == 0 and cls0["subnormal"] == 0 and cls0["zero"] <= 1, cls0
    assert stats == stats0                                   # rays, hits, draws and segments are scene 3's
    assert not np.isnan(fb).any()
    small, _ = _ref(native, oracle, prec, "range", *FRAMES[1], S, B)
    cls = rs.classes(small)
    assert min(cls["inf"], cls["zero"], cls["subnormal"]) >= 1, cls


def test_cpu_valid_variant_overflows_fp32_alone(native, oracle):
    W, H = FRAMES[0]
    for prec in (32, 64):
        a = _scene(native, prec, "valid")["albedo_fuzz"][:, :3]
        assert np.isfinite(a).all() and (a >= 0).all() and a.max() == 1e7
    fb32, stats32 = _ref(native, oracle, 32, "valid", W, H, 2, 50)
    fb64, _ = _ref(native, oracle, 64, "valid", W, H, 2, 50)
    assert int(np.isinf(fb32).any(-1).sum()) == 16 and not np.isnan(fb32).any() and np.isfinite(fb64).all()
    assert stats32 == _ref(native, oracle, 32, "plain", W, H, 2, 50)[1]
    assert np.isinf(_ref(native, oracle, 32, "valid", *FRAMES[1], 2, 50)[0]).any()


def _stand_in(native, oracle, prec, setting):
    """A linear frame with the classes of the device's read_linear, from the oracle's gamma-encoded one: its square, NaN where it reads
    0 and scene 3's does not; with the oracle's guides (NaN / inf albedos) and a variance plane of the classes section C meets."""
    W, H = FRAMES[0]
    S, B = setting
    fb = _ref(native, oracle, prec, "range", W, H, S, B)[0]
    plain = _ref(native, oracle, prec, "plain", W, H, S, B)[0]
    with quiet():
        lin = np.where((fb == 0) & (plain != 0), fb.dtype.type(np.nan), fb * fb).astype(fb.dtype)
        N, A, Z, _ = guides_np(native, oracle, prec, _scene(native, prec, "range"), native.camera_look(prec, W, H, 1, B), np.arange(H))
        Y = luminance(lin)
        V = np.where(np.isfinite(Y), (Y * Y) * fb.dtype.type(0.25), fb.dtype.type(0)).astype(fb.dtype)      # overflows where Y does not
    return lin, V, N, A, Z


@pytest.mark.parametrize("setting", SETTINGS, ids=_id)
@pytest.mark.parametrize("prec", [32, 64])
def test_cpu_perturbed_models_change_the_pinned_frames(native, oracle, prec, setting, monkeypatch):
    """Each perturbation is one way a kernel could be wrong on these inputs and right on every finite frame: the GPU tests compare with the
    unperturbed model, so each must change at least one pixel here."""
    dt = np.float32 if prec == 32 else np.float64
    lin, V, N, A, Z = _stand_in(native, oracle, prec, setting)
    H, W = V.shape
    nan, inf, sub = _holds_every_class(lin, "stand-in")
    changed = {}
    with quiet():
        # 1. gamma: c > 0 ? sqrt(c) : 0 as sqrt(max(c, 0)) keeps the NaN -- store_pixel, and the last level of every filter
        bad_gamma = lambda x: np.sqrt(np.maximum(x, x.dtype.type(0)))
        finite = np.nan_to_num(lin, nan=0.25, posinf=4.0)
        assert same_bits(bad_gamma(finite), gamma(finite))                          # right on a finite frame
        changed["store_pixel"] = int((~_eq(bad_gamma(lin), gamma(lin))).sum())
        want = filter_np(lin, N, A, Z, 1, *SIGS[0])
        wantv = variance_filter_np(lin, V, N, A, Z, 1, *VSIGS[0])
        monkeypatch.setattr(pm, "gamma", bad_gamma)
        changed["filter gamma"] = int((~_eq(filter_np(lin, N, A, Z, 1, *SIGS[0]), want)).sum())
        changed["variance filter gamma"] = int((~_eq(variance_filter_np(lin, V, N, A, Z, 1, *VSIGS[0]), wantv)).sum())
        monkeypatch.undo()
        # 2. the clamp of the variance: !(var > 0) as var < 0 keeps the NaN of inf - inf
        Y = luminance(lin)
        s2 = np.where(np.isnan(Y), dt(np.nan), (Y * Y) * dt(3)).astype(dt)       # inf where Y is, and where Y Y overflows alone
        counts = np.full((H, W), 2, np.int32)
        err, Vp = noise_np(Y * dt(2), s2, counts, dt)
        bad_err, bad_V = noise_np(Y * dt(2), s2, counts, dt, clamp=lambda x: np.where(x < 0, 0.0, x))
        ok = np.isfinite(s2)
        assert same_bits(err[ok], bad_err[ok]) and same_bits(Vp[ok], bad_V[ok])
        changed["err clamp"], changed["V clamp"] = int((~_eq(err, bad_err)).sum()), int((~_eq(Vp, bad_V)).sum())
        assert (err[inf] == 0).all() and (Vp[inf] == 0).all() and np.isnan(err[nan]).all() and (Vp[nan] == 0).all()
        # s2 alone overflowed: in fp32, where the estimate passes through double; in fp64 n m m overflows with it and var is 0
        assert (err[np.isinf(Vp)] == np.inf).all() and np.isinf(Vp).any() == (prec == 32)
        # 3. a NaN-false comparison as its negation: the select and the clip
        thr = float(np.median(err[np.isfinite(err)]))
        changed["select"] = int(((err > thr) != ~(err <= thr)).sum())
        cur = {"c": lin, "n": counts, "N": N, "t": Z}
        base = as_base(native.camera_look(prec, W, H, 1, setting[1]), cur, lin, counts.astype(dt))
        moved = native.camera_look(prec, W, H, 1, setting[1], lookfrom=orbit(1.5))
        params = history_defaults(native)
        Nm, _, Zm, _ = guides_np(native, oracle, prec, _scene(native, prec, "range"), moved, np.arange(H))
        cur = {"c": lin, "n": counts, "N": Nm, "t": Zm}      # the same colours seen from the moved camera: what matters is what is gathered
        h, m = gather_np(moved, cur, base, *params)
        assert np.isnan(h).any() and np.isinf(h).any()
        clipped, mask = pm.clip_np(cur, h, m, 1, 0.75)
        lo_hi = _clip_negated(cur, h, m, 1, 0.75)
        changed["clip"] = int((~_eq(clipped, lo_hi)).sum())
        # 4. a filter that skips non-finite taps (a 'NaN-safe' kernel) is not the definition
        safe = filter_np(np.nan_to_num(lin, nan=0.0, posinf=0.0), N, np.nan_to_num(A, nan=0.0, posinf=0.0), Z, 1, *SIGS[0])
        changed["filter skips"] = int((~_eq(safe, want)).sum())
        # 5. quantise with the count dropped: the host writer reports what the caller wrote
        fb = gamma(lin); fb[0, 0, 0] = np.nan
        changed["levels count"] = native.levels(fb)[1]
    assert all(v > 0 for v in changed.values()), changed


def _eq(a, b):
    """Elementwise: equal bits, or NaN on both sides."""
    with quiet():
        return (a == b) & (np.signbit(a) == np.signbit(b)) | (np.isnan(a) & np.isnan(b))


def _clip_negated(cur, h, m, radius, g):
    """clip_np with h < lo written !(h >= lo) and h > hi written !(h <= hi): a NaN h, or a NaN bound, is then moved."""
    c, n = cur["c"], cur["n"]
    dt = c.dtype.type
    Hh, W = n.shape
    A = np.zeros_like(c); Q = np.zeros_like(c)
    k = np.zeros((Hh, W), np.int64)
    cp = np.pad(c, ((radius, radius), (radius, radius), (0, 0)))
    vp = np.pad(n > 0, radius)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            cq = cp[radius + dy:radius + dy + Hh, radius + dx:radius + dx + W]
            ok = vp[radius + dy:radius + dy + Hh, radius + dx:radius + dx + W]
            A = np.where(ok[..., None], A + cq, A)
            Q = np.where(ok[..., None], Q + cq * cq, Q)
            k = k + ok
    kT = k.astype(c.dtype)[..., None]
    mu = A / kT
    e = dt(g) * np.sqrt(positive_part(Q / kT - mu * mu))
    lo, hi = mu - e, mu + e
    act = ((m > 0) & (k >= 2))[..., None]
    below = act & ~(h >= lo)
    above = act & ~below & ~(h <= hi)
    return np.where(below, lo, np.where(above, hi, h)).astype(c.dtype)
