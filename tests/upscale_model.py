"""Guided upscaling's executable specification: a numpy restatement of INTEGRATION.md section 22, defined operation by operation in T with
plain * + - / and sqrt, so that tests/test_upscale.py compares rtiow_upscale's image with it BIT FOR BIT.  Pure numpy, in the manner of
tests/edge_resolve_model.py, whose pieces it reuses: the output pixels' hits are that module's sub-sample hits on the F x F lattice (the
CPU oracle's hit_world), the traced pixels' guides and layers its first_hit_np / coverage_np.  tests/test_upscale_model.py pins the
outputs on the CPU."""
import numpy as np

from tests.edge_resolve_model import subsample_hits
from tests.preview_model import dot, gamma

DENOISED, LINEAR, HISTORY = 0, 1, 2
INF = float("inf")


def output_hits(oracle, prec, scene, cam, rows, F):
    """(k [F R, F W] int32, N [F R, F W, 3], A [F R, F W, 3], Z [F R, F W]) of the output pixels of a COMPACT scene: output pixel
    (I, J) = (F i + a, F j + b) is sub-sample s = a + F b of traced pixel (i, j); the albedo of hit k comes from the scene tables ({1,1,1}
    for a dielectric); a miss has k = -1 and zeros."""
    dt = np.float32 if prec == 32 else np.float64
    k, N, t = subsample_hits(oracle, prec, scene, cam, rows, F)
    R, W = k.shape[1:]
    grid = lambda v: v.reshape((F, F, R, W) + v.shape[3:]).transpose((2, 0, 3, 1) + tuple(range(4, v.ndim + 1))).reshape((F * R, F * W) + v.shape[3:])
    k, N, t = grid(k), grid(N), grid(t)
    hit = k >= 0
    kk = np.where(hit, k, 0)
    af = np.asarray(scene["albedo_fuzz"], dt).reshape(-1, 4)
    glass = (np.asarray(scene["type"]) == 2)[kk]
    A = np.where(hit[..., None], np.where(glass[..., None], dt(1), af[kk, :3]), dt(0)).astype(dt)
    return k.astype(np.int32), N.astype(dt), A, t.astype(dt)


def colour_of(source, g=None, linear=None, n=None, C=None, M=None):
    """(c [H, W, 3], has [H, W] bool) of a source: DENOISED g g of the stored image, every pixel; LINEAR rtiow_read_linear's value where its
    count n > 0; HISTORY Cout where Mout > 0."""
    if source == DENOISED:
        return g * g, np.ones(g.shape[:2], bool)
    if source == LINEAR:
        return linear, np.asarray(n) > 0
    return C, M > 0


def upscale_np(c, has, N, A, Z, ids, counts, S, hits, F, sigma_normal, sigma_albedo, sigma_depth, use_coverage):
    """(image [F H, F W, 3] gamma-encoded, covered [F H, F W] bool: Wp > 0) of rtiow_upscale.  c, has: colour_of's; N, A, Z the FIRST-HIT
    guides of the traced pixels; ids, counts [H, W, 2] their coverage layers with S = G G (not read without use_coverage); hits =
    output_hits' (k, N, A, Z)."""
    dt = c.dtype.type
    H, W = c.shape[:2]
    ko, No, Ao, Zo = hits
    with np.errstate(all="ignore"):
        i_n, i_a, i_z = (dt(1.0 / (s * s)) for s in (sigma_normal, sigma_albedo, sigma_depth))

    def axis(n):
        """Per output coordinate: the first tap's traced coordinate and the weight of the second."""
        I = np.arange(F * n)
        i = I // F
        o = (((I - F * i).astype(dt) + dt(0.5)) / dt(F) - dt(0.5)).astype(dt)
        return np.where(o < 0, i - 1, i), np.where(o < 0, dt(1) + o, o).astype(dt)

    (x0, gx), (y0, gy) = axis(W), axis(H)
    one = dt(1)
    bx, by = ((one - gx).astype(dt), gx), ((one - gy).astype(dt), gy)
    S1 = np.zeros((F * H, F * W, 3), dt); W1 = np.zeros((F * H, F * W), dt)
    Sp = np.zeros_like(S1); Wp = np.zeros_like(W1)
    for tap in range(4):
        qx, qy = x0 + (tap & 1), y0 + (tap >> 1)
        b = (by[tap >> 1][:, None] * bx[tap & 1][None, :]).astype(dt)
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
