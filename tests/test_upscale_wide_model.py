"""tests/upscale_wide_model.py pinned on the CPU: the CRC-32 of its images on the small synthetic frame of tests/test_upscale_model.py (hand-built
guides, layers and a random image); the model against a scalar restatement written pixel by pixel; and the properties INTEGRATION.md
section 23 states -- at g = 0 exactly the 3 x 3 taps with c = {1/6, 4/6, 1/6} count, a constant colour comes back as that constant, every
sigma = +inf without the share is the renormalised cubic B-spline interpolation, taps outside the frame and taps without colour are
skipped, no counting tap gives 0, and Wp = 0 falls back to S1 / W1.  tests/test_upscale_wide.py compares the library with the model bit
for bit; this keeps the model itself from moving where there is no GPU."""
import numpy as np
import pytest

from tests.preview_model import gamma, same_bits
from tests.test_upscale_model import H, S, W, _crc, synthetic
from tests.upscale_wide_model import INF, bspline, upscale_wide_np

# (F, sigma_normal, sigma_albedo, sigma_depth, use_coverage)
SETTINGS = {"f2": (2, 0.3, 0.1, 0.5, 1), "f3": (3, INF, 0.2, INF, 1), "f4": (4, 0.1, INF, 2.0, 0), "f2inf": (2, INF, INF, INF, 1)}
PINS = {
    32: {"f2": "8149c6a3", "f3": "8989f6be", "f4": "44037439", "f2inf": "7a91a401"},
    64: {"f2": "885c546a", "f3": "1657e3e5", "f4": "8ffe9ac4", "f2inf": "bf070870"},
}


def _T(prec):
    return np.float32 if prec == 32 else np.float64


def scalar_weights(T, g):
    """The four weights of an axis on scalars of T, as INTEGRATION.md section 23 writes them."""
    h = T(1) - g
    return (((h * h) * h) / T(6), (((T(3) * g - T(6)) * g) * g + T(4)) / T(6), (((T(3) * h - T(6)) * h) * h + T(4)) / T(6), ((g * g) * g) / T(6))


def scalar_upscale_wide(T, c, has, N, A, Z, ids, counts, hits, F, sn, sa, sz, use_coverage):
    """INTEGRATION.md section 23 pixel by pixel on scalars of T: the second statement the vectorised model is held to.  Also returns the
    number of taps that counted per output pixel."""
    ko, No, Ao, Zo = hits
    with np.errstate(all="ignore"):
        i_n, i_a, i_z = T(1.0 / (sn * sn)), T(1.0 / (sa * sa)), T(1.0 / (sz * sz))
    out = np.zeros((F * H, F * W, 3), T)
    covered = np.zeros((F * H, F * W), bool)
    taps = np.zeros((F * H, F * W), int)
    sq = lambda d: (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    for J in range(F * H):
        for I in range(F * W):
            i, j = I // F, J // F
            oa = (T(I - F * i) + T(0.5)) / T(F) - T(0.5)
            ob = (T(J - F * j) + T(0.5)) / T(F) - T(0.5)
            x0, gx = (i - 1, T(1) + oa) if oa < 0 else (i, oa)
            y0, gy = (j - 1, T(1) + ob) if ob < 0 else (j, ob)
            cx, cy = scalar_weights(T, gx), scalar_weights(T, gy)
            S1, W1, Sp, Wp = [T(0)] * 3, T(0), [T(0)] * 3, T(0)
            for v in range(4):
                for u in range(4):
                    qx, qy, b = x0 - 1 + u, y0 - 1 + v, cy[v] * cx[u]
                    if not (0 <= qx < W and 0 <= qy < H) or not b > 0 or not has[qy, qx]:
                        continue
                    taps[J, I] += 1
                    dz = Z[qy, qx] - Zo[J, I]
                    e = (sq(N[qy, qx] - No[J, I]) * i_n + sq(A[qy, qx] - Ao[J, I]) * i_a) + (dz * dz) * i_z
                    w = b / (T(1) + e)
                    S1 = [S1[ch] + w * c[qy, qx, ch] for ch in range(3)]
                    W1 = W1 + w
                    if use_coverage:
                        k = ko[J, I]
                        m = counts[qy, qx, 0] if ids[qy, qx, 0] == k else (counts[qy, qx, 1] if ids[qy, qx, 1] == k else 0)
                        if m > 0:
                            wp = w * (T(m) / T(S))
                            Sp = [Sp[ch] + wp * c[qy, qx, ch] for ch in range(3)]
                            Wp = Wp + wp
            covered[J, I] = Wp > 0
            for ch in range(3):
                val = Sp[ch] / Wp if Wp > 0 else (S1[ch] / W1 if W1 > 0 else T(0))
                out[J, I, ch] = np.sqrt(val) if val > 0 else T(0)
    return out, covered, taps


@pytest.mark.parametrize("prec", [32, 64])
def test_the_model_keeps_its_bits(prec):
    T = _T(prec)
    got = {}
    for name, (F, sn, sa, sz, flag) in SETTINGS.items():
        c, has, N, A, Z, ids, counts, hits = synthetic(T, F)
        out, covered = upscale_wide_np(c, has, N, A, Z, ids, counts, S, hits, F, sn, sa, sz, flag)
        assert out.dtype == T and out.shape == (F * H, F * W, 3) and np.isfinite(out).all()
        # the vectorised model is the scalar statement, bit for bit, on every pixel
        want, want_covered, _ = scalar_upscale_wide(T, c, has, N, A, Z, ids, counts, hits, F, sn, sa, sz, flag)
        assert same_bits(out, want) and (covered == want_covered).all(), name
        assert covered.any() == bool(flag) and not covered.all(), name
        got[name] = out
    assert {name: _crc(a) for name, a in got.items()} == PINS[prec]


@pytest.mark.parametrize("prec", [32, 64])
def test_at_g_zero_exactly_the_three_by_three_taps_count(prec):
    """The centre sub-pixel of F = 3 has o = 0, so g = 0 and h = 1: c = {1/6, 4/6, 1/6, 0} in T, the fourth row and column of taps have
    b = 0 and do not count, and the nine others weigh {1, 4, 1} x {1, 4, 1} / 36."""
    T = _T(prec)
    F = 3
    assert bspline(np.zeros(1, T))[:, 0].tolist() == [T(1) / T(6), T(4) / T(6), T(1) / T(6), T(0)]
    c, has, N, A, Z, ids, counts, hits = synthetic(T, F)
    has = np.ones_like(has)
    out, _ = upscale_wide_np(c, has, N, A, Z, ids, counts, S, hits, F, INF, INF, INF, 0)
    _, _, taps = scalar_upscale_wide(T, c, has, N, A, Z, ids, counts, hits, F, INF, INF, INF, 0)
    centre = taps[1::3, 1::3]
    assert (centre[1:-1, 1:-1] == 9).all() and centre[0, 0] == 4 and centre[0, 1] == 6      # interior, corner, edge of the frame
    assert (taps[0::3, 0::3][2:-1, 2:-1] == 16).all()                                      # off the centre all sixteen count (taps i - 2 .. i + 1)
    # the nine taps, weighed in T in tap order
    k = (T(1) / T(6), T(4) / T(6), T(1) / T(6))
    for j in range(1, H - 1):
        for i in range(1, W - 1):
            s, wsum = [T(0)] * 3, T(0)
            for v in range(3):
                for u in range(3):
                    b = k[v] * k[u]
                    s = [s[ch] + b * c[j - 1 + v, i - 1 + u, ch] for ch in range(3)]
                    wsum = wsum + b
            want = np.array([np.sqrt(s[ch] / wsum) for ch in range(3)], T)
            assert same_bits(np.ascontiguousarray(out[3 * j + 1, 3 * i + 1]), want), (i, j)
    # ... and a tap of the fourth row or column is not read into the sums: poison them
    poisoned = c.copy()
    poisoned[3, :] = np.nan; poisoned[:, 3] = np.nan
    again, _ = upscale_wide_np(poisoned, has, N, A, Z, ids, counts, S, hits, F, INF, INF, INF, 0)
    assert same_bits(np.ascontiguousarray(again[3 * 1 + 1, 3 * 1 + 1]), np.ascontiguousarray(out[3 * 1 + 1, 3 * 1 + 1]))   # taps 0..2 of pixel (1, 1)


@pytest.mark.parametrize("F", [2, 3, 4])
@pytest.mark.parametrize("prec", [32, 64])
def test_a_constant_colour_comes_back(prec, F):
    """Every sigma = +inf, no share, colour everywhere: out = (sum of b c) / (sum of b) with c constant.  Each sum has at most 16 positive
    terms (error at most 15 eps relative, plus one for each product b c), and the division adds one: about 34 eps in all; the tolerance is
    64 eps relative on the linear value, whatever the guides say."""
    T = _T(prec)
    c, has, N, A, Z, ids, counts, hits = synthetic(T, F)
    const = np.array([0.7, 0.013, 3.5], T)
    c = np.broadcast_to(const, c.shape).copy()
    out, covered = upscale_wide_np(c, np.ones_like(has), N, A, Z, ids, counts, S, hits, F, INF, INF, INF, 0)
    assert not covered.any()
    linear = out.astype(np.float64) ** 2                     # the store's sqrt and this square add 2 eps
    np.testing.assert_allclose(linear, np.broadcast_to(const.astype(np.float64), linear.shape), rtol=(64 + 2) * np.finfo(T).eps, atol=0)


def _bspline64(t):
    """The cubic B-spline as a function of the distance t (float64): 2/3 - t^2 + |t|^3 / 2 inside 1, (2 - |t|)^3 / 6 inside 2, else 0."""
    t = abs(t)
    return 2.0 / 3.0 - t * t + t * t * t / 2.0 if t < 1 else ((2.0 - t) ** 3 / 6.0 if t < 2 else 0.0)


@pytest.mark.parametrize("F", [2, 3, 4])
@pytest.mark.parametrize("prec", [32, 64])
def test_every_sigma_off_without_the_share_is_bspline_interpolation(prec, F):
    """Against the B-spline evaluated by distance in float64, the taps outside the frame dropped and the rest renormalised.  The tolerance
    is the constant-colour case's 64 eps of T on the linear value plus 2 for the stored sqrt and its square; for fp64 the reference has
    the same error of its own, so twice that."""
    T = _T(prec)
    c, has, N, A, Z, ids, counts, hits = synthetic(T, F)
    has = np.ones_like(has)
    out, covered = upscale_wide_np(c, has, N, A, Z, ids, counts, S, hits, F, INF, INF, INF, 0)
    assert not covered.any()
    c64 = c.astype(np.float64)
    want = np.zeros((F * H, F * W, 3))
    for J in range(F * H):
        for I in range(F * W):
            fx, fy = (I + 0.5) / F - 0.5, (J + 0.5) / F - 0.5
            acc, wsum = np.zeros(3), 0.0
            for qy in range(int(np.floor(fy)) - 2, int(np.floor(fy)) + 4):
                for qx in range(int(np.floor(fx)) - 2, int(np.floor(fx)) + 4):
                    b = _bspline64(fx - qx) * _bspline64(fy - qy)
                    if 0 <= qx < W and 0 <= qy < H and b > 0:
                        acc += b * c64[qy, qx]; wsum += b
            want[J, I] = acc / wsum
    np.testing.assert_allclose(out.astype(np.float64) ** 2, want, rtol=66 * np.finfo(T).eps * (2 if prec == 64 else 1), atol=0)


@pytest.mark.parametrize("prec", [32, 64])
def test_taps_outside_and_without_colour_are_skipped_and_no_tap_gives_zero(prec):
    T = _T(prec)
    F = 2
    c, has, N, A, Z, ids, counts, hits = synthetic(T, F)
    has = has.copy()
    has[1:5, 2:6] = False                                     # a block of 4 x 4: the output pixels at its middle have no tap
    poisoned = c.copy()
    poisoned[~has] = np.nan                                   # a skipped tap's colour is never read into a sum
    for flag in (0, 1):
        out, covered = upscale_wide_np(c, has, N, A, Z, ids, counts, S, hits, F, 0.3, 0.1, 0.5, flag)
        again, _ = upscale_wide_np(poisoned, has, N, A, Z, ids, counts, S, hits, F, 0.3, 0.1, 0.5, flag)
        assert same_bits(out, again) and np.isfinite(out).all()
        # output pixels (7, 5) .. (8, 6): x0 = 3, y0 = 2, taps 2..5 x 1..4
        assert (out[5:7, 7:9] == 0).all() and not covered[5:7, 7:9].any()
        assert (out[4, 7] > 0).all() and (out[8:, 12:] > 0).all()
        _, _, taps = scalar_upscale_wide(T, c, has, N, A, Z, ids, counts, hits, F, 0.3, 0.1, 0.5, flag)
        assert (taps[5:7, 7:9] == 0).all()
        everywhere = scalar_upscale_wide(T, c, np.ones_like(has), N, A, Z, ids, counts, hits, F, 0.3, 0.1, 0.5, flag)[2]
        assert everywhere[0, 0] == 4 and everywhere[0, 4] == 8 and everywhere[4, 4] == 16 and everywhere[-1, -1] == 4      # the frame's corner and edge
    none = np.zeros_like(has)
    out, covered = upscale_wide_np(c, none, N, A, Z, ids, counts, S, hits, F, 0.3, 0.1, 0.5, 1)
    assert (out == 0).all() and not covered.any()


@pytest.mark.parametrize("prec", [32, 64])
def test_without_a_shared_tap_the_result_is_the_unshared_one(prec):
    T = _T(prec)
    F = 4
    c, has, N, A, Z, ids, counts, hits = synthetic(T, F)
    plain, _ = upscale_wide_np(c, has, N, A, Z, ids, counts, S, hits, F, 0.3, 0.1, 0.5, 0)
    shared, covered = upscale_wide_np(c, has, N, A, Z, ids, counts, S, hits, F, 0.3, 0.1, 0.5, 1)
    assert covered.any() and (~covered).any()
    assert (hits[0] == 33)[~covered].any() and not (hits[0] == 33)[covered].any()     # a surface no layer holds never has a share
    assert same_bits(np.ascontiguousarray(shared[~covered]), np.ascontiguousarray(plain[~covered]))
    assert not same_bits(np.ascontiguousarray(shared[covered]), np.ascontiguousarray(plain[covered]))


def test_the_gamma_store_is_the_previews():
    c, has, N, A, Z, ids, counts, hits = synthetic(np.float32, 3)
    has = np.zeros_like(has); has[2, 3] = True                # one pixel with colour: every output pixel it reaches returns it
    out, _ = upscale_wide_np(c, has, N, A, Z, ids, counts, S, hits, 3, INF, INF, INF, 0)
    reached = (out > 0).any(axis=-1)
    assert reached[7, 10] and reached.sum() > 9
    np.testing.assert_allclose(out[reached], np.broadcast_to(gamma(c)[2, 3], out[reached].shape), rtol=4 * np.finfo(np.float32).eps)
