"""Wide-support guided upscaling's executable specification: a numpy restatement of INTEGRATION.md section 23, defined operation by operation
in T with plain * + - / and sqrt, so that tests/test_upscale_wide.py compares rtiow_upscale_wide's image with it BIT FOR BIT.  It is
tests/upscale_model.py with sixteen taps under the cubic B-spline where that has four under the bilinear hat: the output pixels' hits
(output_hits) and the colour of a source (colour_of) are that module's.  tests/test_upscale_wide_model.py pins the outputs on the CPU."""
import numpy as np

from tests.preview_model import dot, gamma
from tests.upscale_model import DENOISED, HISTORY, INF, LINEAR, colour_of, output_hits  # noqa: F401  (the tests take them from here)


def bspline(g):
    """[4, n] weights of the four taps of an axis from g [n] in T: c[0] = ((h h) h) / 6, c[1] = (((3 g - 6) g) g + 4) / 6,
    c[2] = (((3 h - 6) h) h + 4) / 6, c[3] = ((g g) g) / 6 with h = 1 - g."""
    dt = g.dtype.type
    h = (dt(1) - g).astype(dt)
    inner = lambda t: ((((dt(3) * t - dt(6)) * t) * t + dt(4)) / dt(6)).astype(dt)
    return np.stack([(((h * h) * h) / dt(6)).astype(dt), inner(g), inner(h), (((g * g) * g) / dt(6)).astype(dt)])


def axis(n, F, dt):
    """Per output coordinate of an axis of n traced pixels: x0 (the second tap's traced coordinate) and g."""
    I = np.arange(F * n)
    i = I // F
    o = (((I - F * i).astype(dt) + dt(0.5)) / dt(F) - dt(0.5)).astype(dt)
    return np.where(o < 0, i - 1, i), np.where(o < 0, dt(1) + o, o).astype(dt)


def upscale_wide_np(c, has, N, A, Z, ids, counts, S, hits, F, sigma_normal, sigma_albedo, sigma_depth, use_coverage):
    """(image [F H, F W, 3] gamma-encoded, covered [F H, F W] bool: Wp > 0) of rtiow_upscale_wide; the arguments are upscale_np's."""
    dt = c.dtype.type
    H, W = c.shape[:2]
    ko, No, Ao, Zo = hits
    with np.errstate(all="ignore"):
        i_n, i_a, i_z = (dt(1.0 / (s * s)) for s in (sigma_normal, sigma_albedo, sigma_depth))
    (x0, gx), (y0, gy) = axis(W, F, dt), axis(H, F, dt)
    cx, cy = bspline(gx), bspline(gy)
    one = dt(1)
    S1 = np.zeros((F * H, F * W, 3), dt); W1 = np.zeros((F * H, F * W), dt)
    Sp = np.zeros_like(S1); Wp = np.zeros_like(W1)
    for v in range(4):
        for u in range(4):
            qx, qy = x0 - 1 + u, y0 - 1 + v
            b = (cy[v][:, None] * cx[u][None, :]).astype(dt)
            inside = ((qy >= 0) & (qy < H))[:, None] & ((qx >= 0) & (qx < W))[None, :]
            ys, xs = np.clip(qy, 0, H - 1)[:, None], np.clip(qx, 0, W - 1)[None, :]
            cq = c[ys, xs]
            counting = inside & (b > 0) & has[ys, xs]
            d = N[ys, xs] - No
            en = dot(d, d)
            da = A[ys, xs] - Ao
            ea = dot(da, da)
            dz = Z[ys, xs] - Zo
            with np.errstate(all="ignore"):
                e = (en * i_n + ea * i_a) + (dz * dz) * i_z
                w = (b / (one + e)).astype(dt)
                S1 = np.where(counting[..., None], S1 + w[..., None] * cq, S1)
                W1 = np.where(counting, W1 + w, W1)
                if use_coverage:
                    iq, nq = ids[ys, xs], counts[ys, xs]
                    m = np.where(iq[..., 0] == ko, nq[..., 0], np.where(iq[..., 1] == ko, nq[..., 1], 0))
                    shared = counting & (m > 0)
                    wp = (w * (m.astype(dt) / dt(S))).astype(dt)
                    Sp = np.where(shared[..., None], Sp + wp[..., None] * cq, Sp)
                    Wp = np.where(shared, Wp + wp, Wp)
    covered = Wp > 0
    with np.errstate(all="ignore"):
        out = np.where(covered[..., None], Sp / Wp[..., None], np.where((W1 > 0)[..., None], S1 / W1[..., None], dt(0)))
    return gamma(out.astype(dt)).astype(dt), covered
