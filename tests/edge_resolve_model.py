"""The edge resolve's executable specification: numpy restatements of INTEGRATION.md section 17 -- the coverage layers and the resolve of
the mixed pixels -- each defined operation by operation in T with plain * + - / and sqrt, so that tests/test_edge_resolve.py compares
the library's outputs with them BIT FOR BIT.  Pure numpy, in the manner of tests/preview_model.py, whose pieces it reuses; the
sub-sample hits come from the CPU oracle's hit_world.  tests/test_edge_resolve_model.py pins the outputs on the CPU."""
import numpy as np

from tests.conftest import compact
from tests.lattice import lattice_scene
from tests.preview_model import LATTICE, dot, gamma, guides_np, shifted

SKY, NO_LAYER = -1, -2
INF = float("inf")


def scene_of(rt, scene_id, prec):
    """The compact scene tables of a built-in scene or of tests/lattice.py, or the tables themselves (tests/range_scene.py)."""
    if isinstance(scene_id, dict):
        return scene_id
    return lattice_scene(prec) if scene_id == LATTICE else compact(rt.build_scene(scene_id, prec))


def subsample_hits(oracle, prec, scene, cam, rows, G):
    """(k [S, R, W] int, N [S, R, W, 3], t [S, R, W]) of the G x G lattice of every pixel of global rows `rows`: sub-sample s = a + G b at
    offsets o = ((T)a + 0.5) / G - 0.5, the ray D = ((pixel00 + fx du) + fy dv) - O, hit_world on the oracle, the normal facing the
    ray as guides_np builds it; a miss has k = -1, N = 0, t = 0."""
    dt = np.float32 if prec == 32 else np.float64
    cr = np.asarray(scene["center_radius"], dt).reshape(-1, 4)
    W = cam.img_width
    O = np.array(cam.center[:], dt)
    p00, du, dv = (np.array(v[:], dt) for v in (cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
    fG = dt(G)
    ks, Ns, ts = [], [], []
    for s in range(G * G):
        a, b = s % G, s // G
        oa = (dt(a) + dt(0.5)) / fG - dt(0.5)
        ob = (dt(b) + dt(0.5)) / fG - dt(0.5)
        fx = (np.arange(W).astype(dt) + oa)[None, :, None]
        fy = (np.asarray(rows).astype(dt) + ob)[:, None, None]
        ps = (p00 + fx * du) + fy * dv
        D = (ps - O).astype(dt)
        rays = np.concatenate([np.broadcast_to(O, D.shape), D], axis=-1).reshape(-1, 6)
        t, k = oracle.hit_world(prec, cr, rays)
        t = t.reshape(len(rows), W); k = k.reshape(len(rows), W)
        hit = k >= 0
        kk = np.where(hit, k, 0)
        with np.errstate(all="ignore"):
            P = O + t[..., None] * D
            inv_r = dt(1) / cr[kk, 3]
            out = (P - cr[kk, :3]) * inv_r[..., None]
            dn = dot(D, out)
        N = np.where((dn < 0)[..., None], out, -out)
        ks.append(np.where(hit, k, SKY).astype(np.int32))
        Ns.append(np.where(hit[..., None], N, dt(0)).astype(dt))
        ts.append(np.where(hit, t, dt(0)).astype(dt))
    return np.stack(ks), np.stack(Ns), np.stack(ts)


def layers_np(k, N, t):
    """The two layers of every pixel from its sub-samples (k [S, ...], N [S, ..., 3], t [S, ...]): ids and counts [..., 2] int32, normal
    [..., 2, 3], depth [..., 2].  The distinct k by count descending, the smaller k first on a tie; the sums run over the sub-samples
    in index order from 0 and are scaled by (T)1 / (T)c; a pure pixel's second layer is {-2, 0, 0, 0}; a third surface is dropped."""
    dt = N.dtype.type
    S = k.shape[0]
    c = np.stack([(k == k[s]).sum(axis=0) for s in range(S)]).astype(np.int64)
    key = c * (1 << 32) - (k.astype(np.int64) + 2)            # the larger count, then the smaller k
    ids, counts = [], []
    taken = np.zeros(k.shape, bool)
    for _ in range(2):
        masked = np.where(taken, -1, key)
        best = masked.argmax(axis=0)
        have = np.take_along_axis(masked, best[None], 0)[0] >= 0
        kid = np.where(have, np.take_along_axis(k, best[None], 0)[0], NO_LAYER)
        ids.append(kid.astype(np.int32))
        counts.append(np.where(have, np.take_along_axis(c, best[None], 0)[0], 0).astype(np.int32))
        taken |= k == kid
    normal, depth = [], []
    for kid, cnt in zip(ids, counts):
        sn = np.zeros(k.shape[1:] + (3,), dt); sz = np.zeros(k.shape[1:], dt)
        for s in range(S):
            m = k[s] == kid
            sn = np.where(m[..., None], sn + N[s], sn)
            sz = np.where(m, sz + t[s], sz)
        have = cnt > 0
        scale = dt(1) / np.where(have, cnt, 1).astype(dt)
        normal.append(np.where(have[..., None], sn * scale[..., None], dt(0)).astype(dt))
        depth.append(np.where(have, sz * scale, dt(0)).astype(dt))
    return np.stack(ids, -1), np.stack(counts, -1), np.stack(normal, -2), np.stack(depth, -1)


def coverage_np(oracle, prec, scene, cam, rows, G):
    """(ids, counts, normal, depth) of rtiow_read_coverage for a COMPACT scene, and the number of distinct surfaces of each pixel."""
    k, N, t = subsample_hits(oracle, prec, scene, cam, rows, G)
    surfaces = np.zeros(k.shape[1:], np.int32)
    for s in range(k.shape[0]):
        surfaces += ~np.stack([k[r] == k[s] for r in range(s)] + [np.zeros(k.shape[1:], bool)]).any(axis=0)
    return layers_np(k, N, t) + (surfaces,)


def first_hit_np(rt, oracle, prec, scene_id, cam, rows):
    """(normal, depth) of the first-hit guides of a built-in scene or the lattice: what the resolve weighs its taps by."""
    if scene_id == LATTICE:
        k, N, t = subsample_hits(oracle, prec, lattice_scene(prec), cam, rows, 1)     # G = 1: the offset is ((T)0 + 0.5) / 1 - 0.5 = 0, the centre ray
        return N[0], t[0]
    normal, _, depth, _ = guides_np(rt, oracle, prec, scene_id, cam, rows)
    return normal, depth


def resolve_np(g, ids, counts, normal, depth, N, Z, n_eff, S, radius, sigma_normal, sigma_depth, prior):
    """(image, rewritten [H, W] bool) of rtiow_resolve_edges: g the gamma-encoded denoised image [H, W, 3]; ids, counts, normal, depth
    the layers; N, Z the first-hit guides; n_eff [H, W] the count behind each pixel (int32 counts or T history lengths); S = G G."""
    dt = g.dtype.type
    with np.errstate(all="ignore"):
        i_n, i_z = dt(1.0 / (sigma_normal * sigma_normal)), dt(1.0 / (sigma_depth * sigma_depth))
    mixed = ids[..., 1] != NO_LAYER
    pid = ids[..., 0]
    L = g * g
    R = np.zeros_like(g)
    rest = np.ones(g.shape[:2], dt)
    rewritten = np.zeros(g.shape[:2], bool)
    for l in range(2):
        Sx = np.zeros_like(g); Wt = np.zeros(g.shape[:2], dt)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                gq, valid = shifted(g, dy, dx)
                pq, mq = shifted(pid, dy, dx)[0], shifted(mixed, dy, dx)[0]
                Nq, Zq = shifted(N, dy, dx)[0], shifted(Z, dy, dx)[0]
                tap = valid & ~mq & (pq == ids[..., l]) & mixed
                d = Nq - normal[..., l, :]
                en = dot(d, d)
                dz = Zq - depth[..., l]
                with np.errstate(all="ignore"):
                    e = en * i_n + (dz * dz) * i_z
                    w = dt(1) / (dt(1) + e)
                    Sx = np.where(tap[..., None], Sx + w[..., None] * (gq * gq), Sx)
                    Wt = np.where(tap, Wt + w, Wt)
        found = mixed & (Wt > 0)
        with np.errstate(all="ignore"):
            F = Sx / Wt[..., None]
        a = counts[..., l].astype(dt) / dt(S)
        R = np.where(found[..., None], R + a[..., None] * F, R)
        rest = np.where(found, rest - a, rest)
        rewritten |= found
    R = R + rest[..., None] * L
    if prior == INF:
        out = R
    else:
        beta = dt(prior) / (dt(prior) + np.asarray(n_eff).astype(dt))
        out = L + beta[..., None] * (R - L)
    return np.where(rewritten[..., None], gamma(out), g).astype(dt), rewritten
