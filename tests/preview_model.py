"""The preview chain's executable specification: numpy restatements of INTEGRATION.md sections 9 to 16, each defined operation by
operation in T with plain * + - / and sqrt, so that the GPU tests compare the library's outputs with them BIT FOR BIT.  Pure numpy: no
GPU code is imported here, and a function that needs the host library (`rt`) or the CPU oracle takes it as an argument.
tests/test_preview_model.py pins every function's output bits on the CPU; tests/preview_drive.py holds what drives a Renderer."""
import numpy as np

from tests.conftest import compact
from tests.lattice import lattice_scene

K = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
B3 = (1 / 4, 1 / 2, 1 / 4)
LATTICE = "lattice"       # tests/lattice.py instead of a built-in scene: refraction indices other than 1.5 (below 1 and exactly 1 among them), hollow spheres


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_bits_nan(a, b):
    """same_bits where a NaN can occur: x86 and gfx950 give a NaN different bits (inf - inf has the sign set on the one and clear on the
    other, and propagation picks payloads), so the NaN masks must be equal and every other value identical bit for bit -- +0 and -0,
    +inf and -inf and the subnormals are told apart as same_bits tells them."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    bits = np.dtype("u%d" % a.dtype.itemsize)
    return np.array_equal(np.ascontiguousarray(a).view(bits)[~na], np.ascontiguousarray(b).view(bits)[~nb])


def positive_part(x):
    """max(0, x) as the library states it (sections 8, 10, 14 and 15): x > 0 ? x : 0.  A NaN compares false and gives 0, where
    np.maximum would keep it; on every other value the two agree."""
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x, np.zeros_like(x))


def scene_tables(rt, scene, prec):
    """The compact scene tables: of a built-in scene id, of tests/lattice.py (LATTICE), or the tables themselves (tests/range_scene.py)."""
    if isinstance(scene, dict):
        return scene
    return lattice_scene(prec) if scene == LATTICE else compact(rt.build_scene(scene, prec))


def gamma(x):
    z = np.zeros_like(x)
    pos = x > 0
    z[pos] = np.sqrt(x[pos])
    return z


def luminance(c):
    return (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def vec(field, dt):
    return np.array(field[:], dt)


def mse(img, ref, sel=None):
    d = (img - ref) ** 2
    return float(np.mean(d if sel is None else d[sel]))


def quality(out):
    """(q_t, q_dt) of a walk's images: MSE(temporal) / MSE(noisy) and MSE(denoise_history) / MSE(denoise), against out["ref"]."""
    q = lambda k: mse(out[k], out["ref"])
    return q("temporal") / q("noisy"), q("denoise_history") / q("denoise")


# ---- section 9: the first-hit guides and the edge-avoiding a-trous filter

def guides_np(rt, oracle, prec, scene_id, cam, rows):
    """(normal, albedo, depth) as defined: centre ray per pixel, hit_world on the CPU oracle, the rest in T with plain ops."""
    dt = np.float32 if prec == 32 else np.float64
    sc = scene_tables(rt, scene_id, prec)
    cr = np.asarray(sc["center_radius"], dt).reshape(-1, 4)
    W = cam.img_width
    O = np.array(cam.center[:], dt)
    p00, du, dv = (np.array(v[:], dt) for v in (cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
    fi = np.arange(W).astype(dt)[None, :, None]
    fj = np.asarray(rows).astype(dt)[:, None, None]
    ps = (p00 + fi * du) + fj * dv
    D = ps - O
    rays = np.concatenate([np.broadcast_to(O, D.shape), D], axis=-1).reshape(-1, 6)
    t, k = oracle.hit_world(prec, cr, rays)
    t = t.reshape(len(rows), W); k = k.reshape(len(rows), W)
    hit = k >= 0
    kk = np.where(hit, k, 0)
    with np.errstate(all="ignore"):
        P = O + t[..., None] * D
        inv_r = dt(1) / cr[kk, 3]
        out = (P - cr[kk, :3]) * inv_r[..., None]
        dn = (D[..., 0] * out[..., 0] + D[..., 1] * out[..., 1]) + D[..., 2] * out[..., 2]
    normal = np.where((dn < 0)[..., None], out, -out)
    af = np.asarray(sc["albedo_fuzz"], dt).reshape(-1, 4)
    glass = (np.asarray(sc["type"]) == 2)[kk]
    albedo = np.where(glass[..., None], dt(1), af[kk, :3])
    normal = np.where(hit[..., None], normal, dt(0)).astype(dt)
    albedo = np.where(hit[..., None], albedo, dt(0)).astype(dt)
    depth = np.where(hit, t, dt(0)).astype(dt)
    return normal, albedo, depth, hit


def filter_np(c0, normal, albedo, depth, levels, sc, sn, sa, sz):
    dt = c0.dtype.type
    H, W, _ = c0.shape
    inv = [1.0 / (s * s) for s in (sc, sn, sa, sz)]
    c = c0
    for k in range(levels):
        s = 1 << k
        ic, i_n, i_a, i_z = dt(inv[0] * 4.0 ** k), dt(inv[1]), dt(inv[2]), dt(inv[3])
        S = np.zeros_like(c); Wt = np.zeros((H, W), c.dtype)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ys = np.arange(H) + dy * s; xs = np.arange(W) + dx * s
                vy = (ys >= 0) & (ys < H); vx = (xs >= 0) & (xs < W)
                valid = vy[:, None] & vx[None, :]
                yq = np.clip(ys, 0, H - 1); xq = np.clip(xs, 0, W - 1)
                cq = c[yq][:, xq]; nq = normal[yq][:, xq]; aq = albedo[yq][:, xq]; zq = depth[yq][:, xq]
                kern = dt(K[dx + 2]) * dt(K[dy + 2])
                d = cq - c; dn = nq - normal; da = aq - albedo; dz = zq - depth
                ec = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                en = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                ea = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]
                ez = dz * dz
                e = ((ec * ic + en * i_n) + ea * i_a) + ez * i_z
                w = kern / (dt(1) + e)
                S = np.where(valid[..., None], S + w[..., None] * cq, S)
                Wt = np.where(valid, Wt + w, Wt)
        c = S / Wt[..., None]
    return gamma(c)


# ---- sections 8 and 10: the error estimate and the variance plane, in double from Y = Y(acc) in T, s2 in T and the count

def noise_np(Y, s2, n, dt, clamp=positive_part):
    """(err float32, V in dt) of a pixel's record: m = Y / n, var = max(0, (s2 - n m m) / (n - 1)) with max as positive_part states it,
    err = sqrt(var / n) / (m + 1e-3), V = (T)(var / n); err = +inf and V = 0 below two samples."""
    Y, s2 = np.asarray(Y, np.float64), np.asarray(s2, np.float64)
    dn = np.asarray(n).astype(np.float64)
    with np.errstate(all="ignore"):
        mean = Y / dn
        var = clamp((s2 - dn * mean * mean) / (dn - 1.0))
        err = (np.sqrt(var / dn) / (mean + 1e-3)).astype(np.float32)
        V = (var / dn).astype(dt)
    few = np.asarray(n) < 2
    return np.where(few, np.float32(np.inf), err).astype(np.float32), np.where(few, dt(0), V).astype(dt)


# ---- section 10: the filter whose colour edge-stop follows the variance plane

def shifted(a, dy, dx):
    """(a at p + (dx, dy), clamped; whether that tap lies in the frame)."""
    H, W = a.shape[:2]
    ys = np.arange(H) + dy; xs = np.arange(W) + dx
    valid = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    return a[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)], valid


def variance_filter_np(c0, v0, normal, albedo, depth, levels, sv, sn, sa, sz):
    dt = c0.dtype.type
    H, W, _ = c0.shape
    with np.errstate(over="ignore"):
        sv2 = dt(sv * sv)
    colour_on = bool(np.isfinite(sv2))
    i_n, i_a, i_z = (dt(1.0 / (s * s)) for s in (sn, sa, sz))
    eps = dt(1e-8)
    c, v = c0, v0
    for k in range(levels):
        s = 1 << k
        if colour_on:
            gv = np.zeros((H, W), c.dtype); gw = np.zeros((H, W), c.dtype)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    vq, valid = shifted(v, dy, dx)
                    b = dt(B3[dx + 1]) * dt(B3[dy + 1])
                    gv = np.where(valid, gv + b * vq, gv)
                    gw = np.where(valid, gw + b, gw)
            g = gv / gw
            ip = dt(4.0 ** k) / (sv2 * g + eps)
        else:
            ip = np.zeros((H, W), c.dtype)
        S = np.zeros_like(c); Wt = np.zeros((H, W), c.dtype); U = np.zeros((H, W), c.dtype)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, valid = shifted(c, dy * s, dx * s)
                vq, _ = shifted(v, dy * s, dx * s)
                nq, _ = shifted(normal, dy * s, dx * s); aq, _ = shifted(albedo, dy * s, dx * s); zq, _ = shifted(depth, dy * s, dx * s)
                kern = dt(K[dx + 2]) * dt(K[dy + 2])
                d = cq - c; dn = nq - normal; da = aq - albedo; dz = zq - depth
                ec = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                en = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                ea = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]
                ez = dz * dz
                e = ((ec * ip + en * i_n) + ea * i_a) + ez * i_z
                w = kern / (dt(1) + e)
                S = np.where(valid[..., None], S + w[..., None] * cq, S)
                Wt = np.where(valid, Wt + w, Wt)
                U = np.where(valid, U + (w * w) * vq, U)
        c = S / Wt[..., None]
        v = U / (Wt * Wt)
    assert c.dtype == c0.dtype and v.dtype == c0.dtype
    return gamma(c)


# ---- section 11: the history update

def base_constants(cam, dt):
    """In double from the stored fields, each rounded once to T."""
    O, p00, du, dv = (vec(f, np.float64) for f in (cam.center, cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
    a = p00 - O
    w = np.array([du[1] * dv[2] - du[2] * dv[1], du[2] * dv[0] - du[0] * dv[2], du[0] * dv[1] - du[1] * dv[0]])
    f = (a[0] * w[0] + a[1] * w[1]) + a[2] * w[2]
    if f < 0:
        w, f = -w, -f
    with np.errstate(all="ignore"):
        iu = np.float64(1.0) / ((du[0] * du[0] + du[1] * du[1]) + du[2] * du[2])
        iv = np.float64(1.0) / ((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2])
    return {"O": O.astype(dt), "a": a.astype(dt), "w": w.astype(dt), "du": du.astype(dt), "dv": dv.astype(dt), "f": dt(f), "iu": dt(iu), "iv": dt(iv)}


def reproject(cam, cur, base_cam):
    """(den, u, v) of section 11 for every pixel of `cam` in the frame of `base_cam`."""
    dt = cur["t"].dtype.type
    Hh, W = cur["t"].shape
    k = base_constants(base_cam, dt)
    O, p00, du, dv = (vec(f, dt) for f in (cam.center, cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
    fi = np.arange(W).astype(dt)[None, :, None]
    fj = np.arange(Hh).astype(dt)[:, None, None]
    with np.errstate(all="ignore"):
        D = ((p00 + fi * du) + fj * dv) - O
        d = np.where((cur["t"] > 0)[..., None], (O + cur["t"][..., None] * D) - k["O"], D)
        den = dot(d, k["w"])
        e = (k["f"] / den)[..., None] * d - k["a"]
        return den, dot(e, k["du"]) * k["iu"], dot(e, k["dv"]) * k["iv"]


def blend_np(cur, h, m):
    c, n = cur["c"], cur["n"]
    nT = n.astype(c.dtype)
    Mout = m + nT
    with np.errstate(all="ignore"):
        alpha = nT / Mout
        Cout = np.where((Mout > 0)[..., None], h + alpha[..., None] * (c - h), c.dtype.type(0)).astype(c.dtype)
    return Cout, Mout


def gather_np(cam, cur, base, depth_tol, normal_cos, max_history):
    """(h, m): the gathered history and its capped length, before the blend.  base: None, or {"cam", "H", "M", "N", "z"} as
    rtiow_history_commit keeps them."""
    c, n, N, t = cur["c"], cur["n"], cur["N"], cur["t"]
    dt = c.dtype.type
    Hh, W = n.shape
    h = np.zeros_like(c)
    m = np.zeros((Hh, W), c.dtype)
    k = base_constants(base["cam"], dt) if base is not None else None
    if k is not None and base["M"].shape == (Hh, W) and np.isfinite(k["f"]) and k["f"] != 0:
        den, u, v = reproject(cam, cur, base["cam"])
        with np.errstate(all="ignore"):
            hit = t > 0
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
                same = np.where(hit, (zq > 0) & (np.abs(zq - te) <= tol) & (dot(N, Nq) >= dt(normal_cos)), zq == 0)
                valid = inside & (Mq > 0) & same
                S = np.where(valid[..., None], S + b[tap][..., None] * Hq, S)
                L = np.where(valid, L + b[tap] * Mq, L)
                Bs = np.where(valid, Bs + b[tap], Bs)
            got = Bs > 0
            h = np.where(got[..., None], S / Bs[..., None], dt(0)).astype(c.dtype)
            m = np.where(got, L / Bs, dt(0)).astype(c.dtype)
            m = np.where(m < dt(max_history), m, dt(max_history)).astype(c.dtype)
    return h, m


def update_np(cam, cur, base, depth_tol, normal_cos, max_history):
    """(Cout, Mout, reprojected pixels): the gather, then the blend."""
    h, m = gather_np(cam, cur, base, depth_tol, normal_cos, max_history)
    Cout, Mout = blend_np(cur, h, m)
    return Cout, Mout, int((m > 0).sum())


def as_base(cam, cur, Cout, Mout):
    return {"cam": cam, "H": Cout, "M": Mout, "N": cur["N"], "z": cur["t"]}


# ---- section 13: the plan and the budget rule

def plan_np(cam, normal, depth, base, params):
    """(m, pixels with m > 0) of the restatement: section 11 with c = 0 and n = 0, where Mout is m itself.  normal, depth: the current
    camera's first-hit guides."""
    cur = {"c": np.zeros(normal.shape, normal.dtype), "n": np.zeros(depth.shape, np.int32), "N": normal, "t": depth}
    _, m, count = update_np(cam, cur, base, *params)
    return m, count


def budget_rule(counts, m, samples, target, min_samples, max_samples):
    """The rule: the sum and the comparison in T."""
    dt = m.dtype.type
    have = counts.astype(m.dtype) + m
    return ((counts < min_samples) | (have < dt(target))) & (counts.astype(np.int64) + samples <= max_samples)


# ---- section 14: the clamp to the neighbourhood's colours

def clip_np(cur, h, m, radius, gamma):
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


def clipped_np(cam, cur, base, params, radius, gamma, same=same_bits):
    """Section 11 with the clamp of section 14 between the cap and the blend.  h and m come from gather_np itself: update_np with c = 0
    and n = 0 returns them too where h is finite (alpha = 0: Cout = h + 0 (0 - h), the bits of h), but turns an infinite h into a NaN,
    which the clamp would then leave alone where it moves the infinity to its bound.  same: how colours are compared (same_bits_nan
    where one can be NaN)."""
    zero = {"c": np.zeros_like(cur["c"]), "n": np.zeros_like(cur["n"]), "N": cur["N"], "t": cur["t"]}
    h, m = gather_np(cam, cur, base, *params)
    carried = int((m > 0).sum())
    plain_c, plain_m, plain_count = update_np(cam, cur, base, *params)
    through_c, through_m, _ = update_np(cam, zero, base, *params)
    finite = np.isfinite(h).all(axis=-1)
    assert same(np.ascontiguousarray(through_c[finite]), np.ascontiguousarray(h[finite])) and same_bits(through_m, m) and carried == plain_count
    hc, mask = clip_np(cur, h, m, radius, gamma)
    C, M = blend_np(cur, hc, m)
    return {"C": C, "M": M, "h": h, "m": m, "reprojected": carried, "clipped": int(mask.sum()), "mask": mask, "plain_C": plain_c}


# ---- section 15: the temporal image's noise plane

def window_np(C, M, radius):
    """(the spatial V^0 of every pixel, its k): the spread of Cout's luminance over the window's pixels with Mout > 0."""
    dt = C.dtype.type
    Hh, W = M.shape
    Y = (dt(0.2126) * C[..., 0] + dt(0.7152) * C[..., 1]) + dt(0.0722) * C[..., 2]
    A = np.zeros((Hh, W), C.dtype); Q = np.zeros((Hh, W), C.dtype)
    k = np.zeros((Hh, W), np.int64)
    Yp = np.pad(Y, radius)
    vp = np.pad(M > 0, radius)                                   # outside the frame: does not count
    with np.errstate(all="ignore"):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                Yq = Yp[radius + dy:radius + dy + Hh, radius + dx:radius + dx + W]
                ok = vp[radius + dy:radius + dy + Hh, radius + dx:radius + dx + W]
                A = np.where(ok, A + Yq, A)
                Q = np.where(ok, Q + Yq * Yq, Q)
                k = k + ok
        kT = k.astype(C.dtype)
        mu = A / kT
        s = Q / kT - mu * mu
        s = np.where(s > 0, s, dt(0))
    V = np.where(k >= 2, s, dt(0)).astype(C.dtype)
    assert Y.dtype == A.dtype == Q.dtype == s.dtype == C.dtype
    return V, k


def temporal_noise_np(C, M, n, V, radius):
    """V^0.  C, M: the temporal image; n: the accumulation's counts; V: rtiow_read_variance's plane, or None after plain chunks."""
    spatial, _ = window_np(C, M, radius)
    if V is None:
        return spatial
    with np.errstate(all="ignore"):
        alpha = n.astype(C.dtype) / M
        measured = alpha * V
    out = np.where(n >= 2, measured, spatial).astype(C.dtype)
    assert alpha.dtype == measured.dtype == C.dtype
    return out


def noise_classes(n, k):
    """Pixels by where their V^0 comes from: n the accumulation's counts, k window_np's."""
    return {"measured": int((n >= 2).sum()), "one sample": int((n == 1).sum()), "never sampled": int((n == 0).sum()),
            "spatial with k >= 2": int(((n < 2) & (k >= 2)).sum())}


# ---- section 16: the filtered commit

def feedback_np(C, M, N, A, Z, sigmas, feedback):
    """(H', M').  C [H, W, 3], M [H, W]: the temporal image; N, A, Z: the filter guides; sigmas = (colour, normal, albedo, depth)."""
    dt = C.dtype.type
    Hh, W = M.shape
    ic, i_n, i_a, i_z = (dt(1.0 / (s * s)) for s in sigmas)
    S = np.zeros_like(C); Wt = np.zeros((Hh, W), C.dtype)
    pad = lambda a: np.pad(a, ((2, 2), (2, 2)) + ((0, 0),) * (a.ndim - 2))
    Cp, Np, Ap, Zp = pad(C), pad(N), pad(A), pad(Z)
    ok_p = np.pad(M > 0, 2)                                  # outside the frame: does not count; NaN > 0 is false
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                win = lambda a: a[2 + dy:2 + dy + Hh, 2 + dx:2 + dx + W]
                cq, nq, aq, zq, ok = win(Cp), win(Np), win(Ap), win(Zp), win(ok_p)
                kern = dt(K[dx + 2]) * dt(K[dy + 2])
                d = cq - C; dn = nq - N; da = aq - A; dz = zq - Z
                ec = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                en = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                ea = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]
                ez = dz * dz
                e = ((ec * ic + en * i_n) + ea * i_a) + ez * i_z
                w = kern / (dt(1) + e)
                S = np.where(ok[..., None], S + w[..., None] * cq, S)
                Wt = np.where(ok, Wt + w, Wt)
        F = S / Wt[..., None]
        out = F if feedback == 1 else C + dt(feedback) * (F - C)
    out = np.where((M > 0)[..., None], out, C).astype(C.dtype)
    assert out.dtype == S.dtype == Wt.dtype == C.dtype
    return out, M.copy()


# ---- section 12: guides that follow mirrors and glass to the first diffuse surface

def chain_np(rt, oracle, prec, scene_id, cam, rows, max_bounces, max_fuzz):
    """(normal', albedo', depth', bounces, facts) as section 12 defines them: hit_world on the CPU oracle once per bounce level for the
    chains still alive, the rest in T with plain operations.  facts counts what the tests want to have met."""
    dt = np.float32 if prec == 32 else np.float64
    sc = scene_tables(rt, scene_id, prec)
    cr = np.asarray(sc["center_radius"], dt).reshape(-1, 4)
    af = np.asarray(sc["albedo_fuzz"], dt).reshape(-1, 4)
    eta = np.asarray(sc["refraction_index"], dt).reshape(-1)
    with np.errstate(all="ignore"):
        inv_eta = dt(1) / eta                               # the shade table's (T)1 / eta
    ty = np.asarray(sc["type"]).reshape(-1)
    W, R = cam.img_width, len(rows)
    C = np.array(cam.center[:], dt)
    p00, du, dv = (np.array(v[:], dt) for v in (cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
    fi = np.arange(W).astype(dt)[None, :, None]
    fj = np.asarray(rows).astype(dt)[:, None, None]
    ps = (p00 + fi * du) + fj * dv
    D = (ps - C).reshape(-1, 3).copy()
    n = len(D)
    O = np.broadcast_to(C, D.shape).copy()
    A = np.ones((n, 3), dt); Z = np.zeros(n, dt); b = np.zeros(n, np.int32)
    normal = np.zeros((n, 3), dt); albedo = np.zeros((n, 3), dt); depth = np.zeros(n, dt)
    alive = np.ones(n, bool)
    facts = {"tir": 0, "specular_at_cap": 0, "rough_metal_first_hit": 0, "levels": 0}
    with np.errstate(all="ignore"):
        while alive.any():
            facts["levels"] += 1
            assert facts["levels"] <= max_bounces + 1
            idx = np.flatnonzero(alive)
            t, k = oracle.hit_world(prec, cr, np.concatenate([O[idx], D[idx]], axis=1))
            miss = k < 0
            mi = idx[miss]
            later = mi[b[mi] > 0]
            albedo[later] = A[later]; depth[later] = Z[later]
            alive[mi] = False
            hi, t, k = idx[~miss], t[~miss], k[~miss]
            Dh = D[hi]
            P = O[hi] + t[:, None] * Dh
            inv_r = dt(1) / cr[k, 3]
            out = (P - cr[k, :3]) * inv_r[:, None]
            front = dot(Dh, out) < 0
            N = np.where(front[:, None], out, -out)
            glass, metal = ty[k] == 2, ty[k] == 1
            specular = glass | (metal & (af[k, 3].astype(np.float64) <= max_fuzz))
            An = np.where(glass[:, None], A[hi], A[hi] * af[k, :3])
            Zn = Z[hi] + t
            end = ~specular | (b[hi] == max_bounces)
            facts["specular_at_cap"] += int((specular & end).sum())
            facts["rough_metal_first_hit"] += int((metal & ~specular & (b[hi] == 0)).sum())
            e = hi[end]
            normal[e] = N[end]; albedo[e] = An[end]; depth[e] = Zn[end]
            alive[e] = False
            go = ~end
            ci, Dc, Nc, g = hi[go], Dh[go], N[go], glass[go]
            A[ci] = An[go]; Z[ci] = Zn[go]; O[ci] = P[go]; b[ci] += 1
            # metal
            c2 = dt(2) * dot(Dc, Nc)
            Dm = Dc - c2[:, None] * Nc
            # dielectric
            ln = np.sqrt(dot(Dc, Dc))
            il = dt(1) / ln
            u = Dc * il[:, None]
            m = -dot(u, Nc)
            ct = np.where(m < 1, m, dt(1))
            st = np.sqrt(dt(1) - ct * ct)
            ri = np.where(front[go], inv_eta[k[go]], eta[k[go]])
            tir = ri * st > 1
            facts["tir"] += int((tir & g).sum())
            c2 = dt(2) * -ct
            refl = u - c2[:, None] * Nc
            perp = ri[:, None] * (u + ct[:, None] * Nc)
            kk = -np.sqrt(np.abs(dt(1) - dot(perp, perp)))
            refr = perp + kk[:, None] * Nc
            r = np.where(tir[:, None], refl, refr)
            Dg = r * ln[:, None]
            D[ci] = np.where(g[:, None], Dg, Dm)
    for a in (normal, albedo, depth, A, Z, O, D):
        assert a.dtype == dt
    return normal.reshape(R, W, 3), albedo.reshape(R, W, 3), depth.reshape(R, W), b.reshape(R, W), facts
