"""tests/upscale_model.py pinned on the CPU: the CRC-32 of its images on a small synthetic frame with hand-built guides, layers and a
random image; the model against a scalar restatement written pixel by pixel; and the properties INTEGRATION.md section 22 states -- every
sigma = +inf without the share is plain bilinear interpolation, the centre sub-pixel at F = 3 returns its traced pixel's colour exactly, a
tap without colour is skipped, no counting tap gives 0, and Wp = 0 falls back to S1 / W1.  tests/test_upscale.py compares the library with
the model bit for bit; this keeps the model itself from moving where there is no GPU."""
import zlib

import numpy as np
import pytest

from tests.edge_resolve_model import NO_LAYER, SKY, scene_of
from tests.preview_model import gamma, same_bits
from tests.upscale_model import DENOISED, HISTORY, INF, LINEAR, colour_of, output_hits, upscale_np

W, H, S = 7, 5, 16
# (F, sigma_normal, sigma_albedo, sigma_depth, use_coverage)
SETTINGS = {"f2": (2, 0.3, 0.1, 0.5, 1), "f3": (3, INF, 0.2, INF, 1), "f4": (4, 0.1, INF, 2.0, 0), "f2inf": (2, INF, INF, INF, 1)}
PINS = {
    32: {"f2": "2692df2d", "f3": "493ef259", "f4": "22d5686e", "f2inf": "5c4383ea", "hits": "dd46318d"},
    64: {"f2": "7c1043ec", "f3": "cd97e11c", "f4": "fd40ba9e", "f2inf": "241734b0", "hits": "0662f5c7"},
}


def _crc(a):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff)


def synthetic(T, F, seed=23):
    """A 7 x 5 traced frame -- sky above, sphere 5 left, sphere 7 right, mixed pixels between them -- with a random linear image, pixels
    without colour, and for the F x larger output the surface each pixel's own ray hit: mostly its traced pixel's first layer, with a
    share of others (the second layer, a surface no tap has, the sky)."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((H, W, 2), np.int32); counts = np.zeros((H, W, 2), np.int32)
    ids[..., 0] = 5; ids[:, 4:, 0] = 7; ids[:1, :, 0] = SKY
    ids[..., 1] = NO_LAYER; counts[..., 0] = S
    for y in range(1, H):
        ids[y, 3] = (5, 7) if y % 2 else (7, 5); counts[y, 3] = (10, 6) if y % 2 else (9, 5)
    for x in range(W):
        ids[1, x] = (SKY, ids[2, x, 0]); counts[1, x] = (8, 8) if x % 2 else (11, 5)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    N = unit(rng.normal(size=(H, W, 3))).astype(T); A = rng.uniform(0, 1, (H, W, 3)).astype(T); Z = rng.uniform(1, 12, (H, W)).astype(T)
    sky = ids[..., 0] == SKY
    N[sky] = 0; A[sky] = 0; Z[sky] = 0
    c = rng.uniform(0, 1, (H, W, 3)).astype(T)
    has = rng.uniform(size=(H, W)) > 0.2
    has[0, 0] = False; has[2, 2] = has[2, 3] = has[3, 2] = has[3, 3] = False      # a block of four: output pixels between them have no tap
    up = lambda v: np.repeat(np.repeat(v, F, 0), F, 1)
    ko = up(ids[..., 0]).copy()
    pick = rng.uniform(size=ko.shape)
    second = up(ids[..., 1])
    ko = np.where((pick < 0.2) & (second != NO_LAYER), second, ko)
    ko = np.where((pick > 0.9), 33, ko)                       # a sphere no traced pixel's layers hold: Wp = 0
    ko = np.where((pick > 0.8) & (pick <= 0.9), SKY, ko).astype(np.int32)
    No = unit(up(N) + 0.1 * rng.normal(size=ko.shape + (3,)) + 1e-3).astype(T)
    Ao = np.clip(up(A) + 0.05 * rng.normal(size=ko.shape + (3,)), 0, 1).astype(T)
    Zo = (up(Z) + 0.1 * rng.normal(size=ko.shape)).astype(T)
    miss = ko == SKY
    No[miss] = 0; Ao[miss] = 0; Zo[miss] = 0
    return c, has, N, A, Z, ids, counts, (ko, No, Ao, Zo)


def scalar_upscale(T, c, has, N, A, Z, ids, counts, hits, F, sn, sa, sz, use_coverage):
    """INTEGRATION.md section 22 pixel by pixel on scalars of T: the second statement the vectorised model is held to."""
    ko, No, Ao, Zo = hits
    with np.errstate(all="ignore"):
        i_n, i_a, i_z = T(1.0 / (sn * sn)), T(1.0 / (sa * sa)), T(1.0 / (sz * sz))
    out = np.zeros((F * H, F * W, 3), T)
    covered = np.zeros((F * H, F * W), bool)
    sq = lambda d: (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    for J in range(F * H):
        for I in range(F * W):
            i, j = I // F, J // F
            oa = (T(I - F * i) + T(0.5)) / T(F) - T(0.5)
            ob = (T(J - F * j) + T(0.5)) / T(F) - T(0.5)
            x0, gx = (i - 1, T(1) + oa) if oa < 0 else (i, oa)
            y0, gy = (j - 1, T(1) + ob) if ob < 0 else (j, ob)
            taps = ((x0, y0, (T(1) - gx) * (T(1) - gy)), (x0 + 1, y0, gx * (T(1) - gy)), (x0, y0 + 1, (T(1) - gx) * gy), (x0 + 1, y0 + 1, gx * gy))
            S1, W1, Sp, Wp = [T(0)] * 3, T(0), [T(0)] * 3, T(0)
            for qx, qy, b in taps:
                if not (0 <= qx < W and 0 <= qy < H) or not b > 0 or not has[qy, qx]:
                    continue
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
                v = Sp[ch] / Wp if Wp > 0 else (S1[ch] / W1 if W1 > 0 else T(0))
                out[J, I, ch] = np.sqrt(v) if v > 0 else T(0)
    return out, covered


@pytest.mark.parametrize("prec", [32, 64])
def test_the_model_keeps_its_bits(native, oracle, prec):
    T = np.float32 if prec == 32 else np.float64
    got = {}
    for name, (F, sn, sa, sz, flag) in SETTINGS.items():
        c, has, N, A, Z, ids, counts, hits = synthetic(T, F)
        out, covered = upscale_np(c, has, N, A, Z, ids, counts, S, hits, F, sn, sa, sz, flag)
        assert out.dtype == T and out.shape == (F * H, F * W, 3) and np.isfinite(out).all()
        # the vectorised model is the scalar statement, bit for bit, on every pixel
        want, want_covered = scalar_upscale(T, c, has, N, A, Z, ids, counts, hits, F, sn, sa, sz, flag)
        assert same_bits(out, want) and (covered == want_covered).all(), name
        assert covered.any() == bool(flag) and not covered.all(), name
        got[name] = out
    # the output pixels' hits of a small real frame, a frame that is no multiple of the tile, at the factor that is no power of two
    cam = native.camera(prec, 13, 9, 1, 5)
    k, No, Ao, Zo = output_hits(oracle, prec, scene_of(native, 3, prec), cam, np.arange(9), 3)
    assert k.shape == (27, 39) and (k == SKY).any() and (k >= 0).any() and (Ao[k == SKY] == 0).all() and (Zo[k >= 0] > 0).all()
    got["hits"] = np.concatenate([k.ravel().view(np.uint8), No.ravel().view(np.uint8), Ao.ravel().view(np.uint8), Zo.ravel().view(np.uint8)])
    assert {name: _crc(a) for name, a in got.items()} == PINS[prec]


@pytest.mark.parametrize("F", [2, 3, 4])
@pytest.mark.parametrize("prec", [32, 64])
def test_every_sigma_off_without_the_share_is_bilinear_interpolation(prec, F):
    T = np.float32 if prec == 32 else np.float64
    c, has, N, A, Z, ids, counts, hits = synthetic(T, F)
    has = np.ones_like(has)
    out, covered = upscale_np(c, has, N, A, Z, ids, counts, S, hits, F, INF, INF, INF, 0)
    assert not covered.any()
    # pixel centres of the output in the traced frame's coordinates; taps outside the frame drop out and the rest are renormalised
    c64 = c.astype(np.float64)
    want = np.zeros((F * H, F * W, 3))
    for J in range(F * H):
        for I in range(F * W):
            fx, fy = (I + 0.5) / F - 0.5, (J + 0.5) / F - 0.5
            x0, y0 = int(np.floor(fx)), int(np.floor(fy))
            acc, wsum = np.zeros(3), 0.0
            for qx, qy, b in ((x0, y0, (1 - (fx - x0)) * (1 - (fy - y0))), (x0 + 1, y0, (fx - x0) * (1 - (fy - y0))),
                              (x0, y0 + 1, (1 - (fx - x0)) * (fy - y0)), (x0 + 1, y0 + 1, (fx - x0) * (fy - y0))):
                if 0 <= qx < W and 0 <= qy < H and b > 0:
                    acc += b * c64[qy, qx]; wsum += b
            want[J, I] = acc / wsum
    np.testing.assert_allclose(out.astype(np.float64) ** 2, want, rtol=4e-6 if prec == 32 else 1e-14, atol=0)


@pytest.mark.parametrize("prec", [32, 64])
def test_the_centre_sub_pixel_at_three_returns_its_traced_pixel(prec):
    """At F = 3 the centre sub-pixel's ray is the guide ray: o = 0, so b = 1 for the pixel itself and 0 for the other taps, and with the
    output pixel's guides equal to the traced pixel's e = 0: out = c exactly, stored as the preview stores it."""
    T = np.float32 if prec == 32 else np.float64
    F = 3
    c, has, N, A, Z, ids, counts, (ko, No, Ao, Zo) = synthetic(T, F)
    No[1::3, 1::3], Ao[1::3, 1::3], Zo[1::3, 1::3] = N, A, Z
    for sigmas in ((0.3, 0.1, 0.5), (INF, INF, INF)):
        out, _ = upscale_np(c, has, N, A, Z, ids, counts, S, (ko, No, Ao, Zo), F, *sigmas, 0)
        centre = np.ascontiguousarray(out[1::3, 1::3])
        assert same_bits(np.ascontiguousarray(centre[has]), np.ascontiguousarray(gamma(c)[has]))
        assert (centre[~has] == 0).all()                      # its only tap holds no colour


@pytest.mark.parametrize("prec", [32, 64])
def test_taps_without_colour_are_skipped_and_no_tap_gives_zero(prec):
    T = np.float32 if prec == 32 else np.float64
    F = 2
    c, has, N, A, Z, ids, counts, hits = synthetic(T, F)
    poisoned = c.copy()
    poisoned[~has] = np.nan                                   # a skipped tap's colour is never read into a sum
    for flag in (0, 1):
        out, covered = upscale_np(c, has, N, A, Z, ids, counts, S, hits, F, 0.3, 0.1, 0.5, flag)
        again, _ = upscale_np(poisoned, has, N, A, Z, ids, counts, S, hits, F, 0.3, 0.1, 0.5, flag)
        assert same_bits(out, again) and np.isfinite(out).all()
        # the four output pixels between traced pixels (2,2), (3,2), (2,3), (3,3) have all their taps there; (0, 0)'s corner has one tap
        assert (out[5:7, 5:7] == 0).all() and (out[0, 0] == 0).all() and not covered[5:7, 5:7].any()
        assert (out[8:, 10:] > 0).any()
    none = np.zeros_like(has)
    out, covered = upscale_np(c, none, N, A, Z, ids, counts, S, hits, F, 0.3, 0.1, 0.5, 1)
    assert (out == 0).all() and not covered.any()


@pytest.mark.parametrize("prec", [32, 64])
def test_without_a_shared_tap_the_result_is_the_unshared_one(prec):
    T = np.float32 if prec == 32 else np.float64
    F = 4
    c, has, N, A, Z, ids, counts, hits = synthetic(T, F)
    plain, _ = upscale_np(c, has, N, A, Z, ids, counts, S, hits, F, 0.3, 0.1, 0.5, 0)
    shared, covered = upscale_np(c, has, N, A, Z, ids, counts, S, hits, F, 0.3, 0.1, 0.5, 1)
    assert covered.any() and (~covered).any()
    assert (hits[0] == 33)[~covered].any() and not (hits[0] == 33)[covered].any()     # a surface no layer holds never has a share
    assert same_bits(np.ascontiguousarray(shared[~covered]), np.ascontiguousarray(plain[~covered]))
    assert not same_bits(np.ascontiguousarray(shared[covered]), np.ascontiguousarray(plain[covered]))


def test_colour_of_each_source():
    g = np.array([[[0.5, 0.25, 2.0]]], np.float32)
    c, has = colour_of(DENOISED, g=g)
    assert c.tolist() == [[[0.25, 0.0625, 4.0]]] and has.all()
    lin = np.ones((1, 2, 3), np.float32)
    assert colour_of(LINEAR, linear=lin, n=np.array([[0, 3]]))[1].tolist() == [[False, True]]
    assert colour_of(HISTORY, C=lin, M=np.array([[2.5, 0.0]], np.float32))[1].tolist() == [[True, False]]
