"""The lens-sampled filter guides' executable specification: a numpy restatement of INTEGRATION.md section 18 -- the lattice of lens
points, the ray of each, the chain of section 12 started from it, and the mean -- defined operation by operation in T with plain
* + - / and sqrt, so that tests/test_lens_guides.py compares the library's outputs with it BIT FOR BIT.  Pure numpy, in the manner of
tests/preview_model.py, whose pieces it reuses; hit_world goes through the CPU oracle.  tests/test_lens_guides_model.py pins the outputs
on the CPU."""
import numpy as np

from tests.conftest import compact
from tests.lattice import lattice_scene
from tests.preview_model import LATTICE, dot

KAPPA = {2: 1.0, 4: 0.8944271909999159}      # sqrt(0.8) for the 4 x 4 lattice: the second moment per axis of the uniform unit disk


def scene_of(rt, scene, prec):
    """The compact scene tables: of a built-in scene id, of tests/lattice.py (LATTICE), or the tables themselves."""
    if isinstance(scene, dict):
        return scene
    return lattice_scene(prec) if scene == LATTICE else compact(rt.build_scene(scene, prec))


def lens_points(dt, G):
    """[(lx, ly)] of lens sample s = a + G b (b outer): o = (T)(2 a + 1) / (T)G - 1 scaled by kappa."""
    fG, kappa = dt(G), dt(KAPPA[G])
    o = [dt(2 * a + 1) / fG - dt(1) for a in range(G)]
    return [(kappa * o[s % G], kappa * o[s // G]) for s in range(G * G)]


def targets(cam, dt, rows):
    """ps [R, W, 3]: the ray target of the guides, (pixel00 + (T)i du) + (T)j dv with j the global row."""
    p00, du, dv = (np.array(v[:], dt) for v in (cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
    fi = np.arange(cam.img_width).astype(dt)[None, :, None]
    fj = np.asarray(rows).astype(dt)[:, None, None]
    return ((p00 + fi * du) + fj * dv).astype(dt)


def chain_from(oracle, prec, sc, O, D, max_bounces, max_fuzz):
    """(normal' [n, 3], albedo' [n, 3], depth' [n], b [n]) of section 12's chain started from the rays (O [n, 3], D [n, 3]): hit_world
    on the CPU oracle once per bounce level for the chains still alive, the rest in T with plain operations.  max_bounces = 0 ends every
    chain at its first hit."""
    dt = np.float32 if prec == 32 else np.float64
    cr = np.asarray(sc["center_radius"], dt).reshape(-1, 4)
    af = np.asarray(sc["albedo_fuzz"], dt).reshape(-1, 4)
    eta = np.asarray(sc["refraction_index"], dt).reshape(-1)
    with np.errstate(all="ignore"):
        inv_eta = dt(1) / eta                               # the shade table's (T)1 / eta
    ty = np.asarray(sc["type"]).reshape(-1)
    O, D = O.astype(dt).copy(), D.astype(dt).copy()
    n = len(D)
    A = np.ones((n, 3), dt); Z = np.zeros(n, dt); b = np.zeros(n, np.int32)
    normal = np.zeros((n, 3), dt); albedo = np.zeros((n, 3), dt); depth = np.zeros(n, dt)
    alive = np.ones(n, bool)
    levels = 0
    with np.errstate(all="ignore"):
        while alive.any():
            levels += 1
            assert levels <= max_bounces + 1
            idx = np.flatnonzero(alive)
            t, k = oracle.hit_world(prec, cr, np.concatenate([O[idx], D[idx]], axis=1))
            miss = k < 0
            mi = idx[miss]
            later = mi[b[mi] > 0]
            albedo[later] = A[later]; depth[later] = Z[later]
            alive[mi] = False
            hi, t, k = idx[~miss], t[~miss].astype(dt), k[~miss]
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
    return normal, albedo, depth, b


def lens_ray_np(oracle, prec, sc, cam, rows, lx, ly, max_bounces_eff, max_fuzz):
    """(normal'_s, albedo'_s, depth'_s, b_s) [R, W, ...] of the rays from the lens point (lx, ly): O_s = (O + lx U) + ly V per component,
    D_s = ps - O_s, then the chain."""
    dt = np.float32 if prec == 32 else np.float64
    W, R = cam.img_width, len(rows)
    C, U, V = (np.array(v[:], dt) for v in (cam.center, cam.defocus_disk_u, cam.defocus_disk_v))
    Os = ((C + dt(lx) * U) + dt(ly) * V).astype(dt)
    ps = targets(cam, dt, rows)
    D = (ps - Os).reshape(-1, 3)
    O = np.broadcast_to(Os, D.shape)
    n, a, z, b = chain_from(oracle, prec, sc, O, D, max_bounces_eff, max_fuzz)
    return n.reshape(R, W, 3), a.reshape(R, W, 3), z.reshape(R, W), b.reshape(R, W)


def lens_guides_np(rt, oracle, prec, scene, cam, rows, G, max_bounces_eff, max_fuzz):
    """(normal, albedo, depth, bounces) of rtiow_read_filter_guides with the G x G lens lattice in effect, for the global rows `rows`:
    the sums over the lens samples in s order from 0, times q = (T)1 / (T)S; bounces the largest b_s.  max_bounces_eff: the handle's
    max_bounces in RTIOW_GUIDES_SPECULAR, 0 in RTIOW_GUIDES_FIRST_HIT."""
    dt = np.float32 if prec == 32 else np.float64
    sc = scene_of(rt, scene, prec)
    W, R = cam.img_width, len(rows)
    Ns = np.zeros((R, W, 3), dt); As = np.zeros((R, W, 3), dt); Zs = np.zeros((R, W), dt)
    bounces = np.zeros((R, W), np.int32)
    for lx, ly in lens_points(dt, G):
        n, a, z, b = lens_ray_np(oracle, prec, sc, cam, rows, lx, ly, max_bounces_eff, max_fuzz)
        Ns = Ns + n; As = As + a; Zs = Zs + z
        bounces = np.maximum(bounces, b)
    q = dt(1) / dt(G * G)
    normal, albedo, depth = Ns * q, As * q, Zs * q
    for a in (normal, albedo, depth):
        assert a.dtype == dt
    return normal, albedo, depth, bounces
