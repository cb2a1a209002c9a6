"""Scene edits that keep the history: the numpy restatement of INTEGRATION.md section 19, on top of tests/preview_model.py (sections 11,
13 and 14), which it imports and does not edit.  Every value in T with plain * + - /, so that the GPU tests compare BIT FOR BIT.  Pure
numpy; the CPU oracle is handed in for (t, k) = hit_world(O, D).  tests/test_scene_motion_model.py pins these functions on the CPU."""
import numpy as np

from tests.conftest import compact
from tests.preview_model import base_constants, blend_np, clip_np, dot, vec

MOVED, CHANGED = 1, 2


def tables(scene, prec):
    """The kept spheres' tables in T, numbered as the library numbers them (invalid slots dropped)."""
    dt = np.float32 if prec == 32 else np.float64
    sc = compact(scene) if scene.get("valid") is not None else scene
    return {"cr": np.ascontiguousarray(sc["center_radius"], dt).reshape(-1, 4), "af": np.ascontiguousarray(sc["albedo_fuzz"], dt).reshape(-1, 4),
            "ri": np.ascontiguousarray(sc["refraction_index"], dt).reshape(-1), "ty": np.ascontiguousarray(sc["type"], np.int32).reshape(-1)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)


def flags(cur, snap):
    """MOVED | CHANGED per kept sphere: the current tables against the snapshot's, bits against bits."""
    moved = (_bits(cur["cr"]) != _bits(snap["cr"])).any(axis=1)
    changed = (_bits(cur["af"]) != _bits(snap["af"])).any(axis=1) | (_bits(cur["ri"]) != _bits(snap["ri"])).any(axis=1) | (cur["ty"] != snap["ty"])
    return moved * MOVED + changed * CHANGED


def first_hit(oracle, prec, cur, cam, rows):
    """The ray of rtiow_render_guides for every local pixel and its first hit in the scene `cur`: D, t (+inf: none), k (-1: none)."""
    dt = cur["cr"].dtype.type
    W = cam.img_width
    O, p00, du, dv = (vec(f, dt) for f in (cam.center, cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
    fi = np.arange(W).astype(dt)[None, :, None]
    fj = np.asarray(rows).astype(dt)[:, None, None]
    D = ((p00 + fi * du) + fj * dv) - O
    rays = np.concatenate([np.broadcast_to(O, D.shape), D], axis=-1).reshape(-1, 6)
    t, k = oracle.hit_world(prec, cur["cr"], rays)
    return O, D, t.reshape(len(rows), W), k.reshape(len(rows), W)


def guides_of(O, D, t, k, cur):
    """(normal, depth) of rtiow_render_guides from (t, k)."""
    dt = D.dtype.type
    hit = k >= 0
    kk = np.where(hit, k, 0)
    with np.errstate(all="ignore"):
        P = O + t[..., None] * D
        out = (P - cur["cr"][kk, :3]) * (dt(1) / cur["cr"][kk, 3])[..., None]
        dn = dot(D, out)
    normal = np.where(hit[..., None], np.where((dn < 0)[..., None], out, -out), dt(0)).astype(dt)
    return normal, np.where(hit, t, dt(0)).astype(dt)


def plane_np(O, D, t, k, cur, snap):
    """(Q [rows, W, 3], carry int32, ids int32): the motion plane of section 19."""
    dt = D.dtype.type
    f = flags(cur, snap)
    hit = k >= 0
    kk = np.where(hit, k, 0)
    fk = f[kk]
    with np.errstate(all="ignore"):
        P = O + t[..., None] * D
        o = (P - cur["cr"][kk, :3]) * (dt(1) / cur["cr"][kk, 3])[..., None]
        Qm = snap["cr"][kk, :3] + snap["cr"][kk, 3][..., None] * o
    changed = hit & ((fk & CHANGED) != 0)
    moved = hit & ~changed & ((fk & MOVED) != 0)
    still = hit & ~changed & ~moved
    Q = np.where(moved[..., None], Qm, np.where(still[..., None], P, dt(0))).astype(dt)
    return Q, np.where(changed, 0, 1).astype(np.int32), k.astype(np.int32)


def gather_np(cam, cur, base, depth_tol, normal_cos, max_history, Q=None, carry=None):
    """(h, m) of section 11 for every pixel, gathered through the motion plane when Q and carry are given: at a hit pixel d = Q - O'
    instead of (O + t D) - O', and carry == 0 takes no taps.  cur: {"N", "t"} at least."""
    N, t = cur["N"], cur["t"]
    dt = t.dtype.type
    Hh, W = t.shape
    h = np.zeros((Hh, W, 3), t.dtype)
    m = np.zeros((Hh, W), t.dtype)
    k = base_constants(base["cam"], dt) if base is not None else None
    if k is None or base["M"].shape != (Hh, W) or not (np.isfinite(k["f"]) and k["f"] != 0):
        return h, m
    O, p00, du, dv = (vec(f, dt) for f in (cam.center, cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
    fi = np.arange(W).astype(dt)[None, :, None]
    fj = np.arange(Hh).astype(dt)[:, None, None]
    with np.errstate(all="ignore"):
        D = ((p00 + fi * du) + fj * dv) - O
        hit = t > 0
        at_hit = (O + t[..., None] * D) - k["O"] if Q is None else Q - k["O"]
        d = np.where(hit[..., None], at_hit, D)
        den = dot(d, k["w"])
        e = (k["f"] / den)[..., None] * d - k["a"]
        u, v = dot(e, k["du"]) * k["iu"], dot(e, k["dv"]) * k["iv"]
        te = den / k["f"]
        ok = (den > 0) & (u > dt(-1)) & (u < dt(W)) & (v > dt(-1)) & (v < dt(Hh))
        if carry is not None:
            ok = ok & ~(hit & (carry == 0))
        xf = np.floor(np.where(ok, u, dt(0)))
        yf = np.floor(np.where(ok, v, dt(0)))
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
        fx, fy = u - xf, v - yf
        gx, gy = dt(1) - fx, dt(1) - fy
        b = (gx * gy, fx * gy, gx * fy, fx * fy)
        tol = dt(depth_tol) * te
        S = np.zeros_like(h); L = np.zeros_like(m); Bs = np.zeros_like(m)
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
        h = np.where(got[..., None], S / Bs[..., None], dt(0)).astype(t.dtype)
        m = np.where(got, L / Bs, dt(0)).astype(t.dtype)
        m = np.where(m < dt(max_history), m, dt(max_history)).astype(t.dtype)
    return h, m


def update_np(cam, cur, base, params, Q, carry):
    """(Cout, Mout, reprojected pixels) of rtiow_history_update while motion is in effect."""
    h, m = gather_np(cam, cur, base, *params, Q=Q, carry=carry)
    Cout, Mout = blend_np(cur, h, m)
    return Cout, Mout, int((m > 0).sum())


def clipped_np(cam, cur, base, params, radius, gamma, Q, carry):
    """rtiow_history_update_clipped while motion is in effect: the clamp of section 14 between the cap and the blend."""
    h, m = gather_np(cam, cur, base, *params, Q=Q, carry=carry)
    hc, mask = clip_np(cur, h, m, radius, gamma)
    C, M = blend_np(cur, hc, m)
    return {"C": C, "M": M, "h": h, "m": m, "reprojected": int((m > 0).sum()), "clipped": int(mask.sum()), "mask": mask}


def plan_np(cam, normal, depth, base, params, Q, carry):
    """(m, pixels with m > 0) of rtiow_history_plan while motion is in effect."""
    _, m = gather_np(cam, {"N": normal, "t": depth}, base, *params, Q=Q, carry=carry)
    return m, int((m > 0).sum())


def view(rt, prec, scene_id, W, H, B=10):
    """The camera of the tests: the reference's, but for the material lattice, whose glass sphere of radius 2 around that camera is the
    first hit of every pixel: there the eye stands outside it, at (9, 2, 2)."""
    if scene_id == "lattice":
        return rt.camera_look(prec, W, H, 1, B, lookfrom=(9.0, 2.0, 2.0))
    return rt.camera(prec, W, H, 1, B)


# ---- the edits the tests share: functions of a scene dict (slot order, 'valid' kept) returning an edited copy

def edited(scene, **changes):
    out = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in scene.items()}
    for key, fn in changes.items():
        fn(out[key])
    return out


def kept_slots(scene):
    return np.flatnonzero(np.asarray(scene["valid"]) != 0) if scene.get("valid") is not None else np.arange(len(scene["type"]))


def small_spheres(scene):
    """Slots of the kept spheres with 0 < radius < 0.6, in slot order."""
    r = np.asarray(scene["center_radius"], np.float64).reshape(-1, 4)[:, 3]
    return [int(s) for s in kept_slots(scene) if 0 < r[s] < 0.6]


def big_spheres(scene):
    """Slots of the kept spheres with 0.6 <= radius < 100 (not the ground), in slot order."""
    r = np.asarray(scene["center_radius"], np.float64).reshape(-1, 4)[:, 3]
    return [int(s) for s in kept_slots(scene) if 0.6 <= r[s] < 100]


def translate(scene, slots, delta):
    def fn(cr):
        cr.reshape(-1, 4)[np.asarray(slots), :3] += np.asarray(delta, cr.dtype)
    return edited(scene, center_radius=fn)


def scale_radius(scene, slots, factor):
    def fn(cr):
        cr.reshape(-1, 4)[np.asarray(slots), 3] *= cr.dtype.type(factor)
    return edited(scene, center_radius=fn)


def recolour(scene, slots):
    def fn(af):
        af.reshape(-1, 4)[np.asarray(slots), :3] = af.dtype.type(0.25)
    return edited(scene, albedo_fuzz=fn)
