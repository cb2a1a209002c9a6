"""Edit influence: the numpy restatement of INTEGRATION.md section 20, on top of tests/scene_motion_model.py (section 19), which it imports
and does not edit.  Every value in T with plain * + - / and sqrt, left to right as the section writes it, so that the GPU tests compare
BIT FOR BIT.  Pure numpy.

The edit list.  Through the kept spheres in ascending k, against the snapshot: MOVED (with or without CHANGED): two entries, {C'_k, r'_k}
of the snapshot, then {C_k, r_k} of the current scene; CHANGED only: one entry, {C_k, r_k}; neither: none.  Each entry has the owner k.

The plane, per pixel p with the guides' depth t_p, the motion plane's carry_p and id k_p:
    a miss (depth == 0) or carry_p == 0:   lambda_p = 0
    otherwise   P = O + t_p D per component, s = 0, and for every entry e in list order with owner_e != k_p:
                    v = C_e - P, d2 = (v.x v.x + v.y v.y) + v.z v.z, q = (r_e r_e) / d2,
                    omega = q >= 1 ? 1 : 1 - sqrt(1 - q)      (NaN compares false), s = s + omega
                lambda_p = s > 0 ? min(1, kappa s) : 0        (kappa rounded once to T)
    fade_p = carry_p == 0 ? 0 : 1 - lambda_p
The gathers are section 19's with fade in the place of carry (fade == 0 takes no taps) and one more operation after the cap: m = m * fade.

The kernel stages the list in LDS CHUNK = 32 entries at a time (EDIT_LIST_CHUNK of csrc/library/edit_list.h, which
tests/test_edit_influence.py reads and compares with this constant), so a list longer than CHUNK entries crosses a chunk edge.  Nothing
here depends on CHUNK: the sum runs in list order whatever the staging.
tests/test_edit_influence_model.py pins these functions on the CPU."""
import numpy as np

from tests import scene_motion_model as M
from tests.preview_model import blend_np, clip_np, vec

CHUNK = 32


def edit_list(cur, snap):
    """(entries [E, 4] in T as {C.xyz, r}, owners [E] int32) of the current tables against the snapshot's (M.tables)."""
    entries, owners = [], []
    for k, f in enumerate(M.flags(cur, snap)):
        if f & M.MOVED:
            entries += [snap["cr"][k], cur["cr"][k]]
            owners += [k, k]
        elif f & M.CHANGED:
            entries.append(cur["cr"][k])
            owners.append(k)
    dt = cur["cr"].dtype
    return (np.array(entries, dt).reshape(-1, 4), np.array(owners, np.int32))


def points(cam, depth, rows=None):
    """P = O + t D per component for every local pixel (rows: their global rows; default every row of the frame)."""
    dt = depth.dtype.type
    Hh, W = depth.shape
    O, p00, du, dv = (vec(f, dt) for f in (cam.center, cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
    fi = np.arange(W).astype(dt)[None, :, None]
    fj = np.asarray(range(Hh) if rows is None else rows).astype(dt)[:, None, None]
    with np.errstate(all="ignore"):
        D = ((p00 + fi * du) + fj * dv) - O
        return (O + depth[..., None] * D).astype(dt)


def solid_sum(P, ids, entries, owners):
    """s: the sum of omega over the entries whose owner is not the pixel's own sphere, in list order."""
    dt = P.dtype.type
    s = np.zeros(P.shape[:-1], P.dtype)
    with np.errstate(all="ignore"):
        for e, owner in zip(entries, owners):
            v = e[:3] - P
            d2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
            q = (e[3] * e[3]) / d2
            omega = np.where(q >= dt(1), dt(1), dt(1) - np.sqrt(dt(1) - q)).astype(P.dtype)
            s = np.where(ids != owner, s + omega, s).astype(P.dtype)
    return s


def influence_np(cam, depth, carry, ids, entries, owners, kappa, rows=None):
    """(lambda, fade, s) of section 20 in T.  kappa == 0 (off: the library makes no plane then) gives lambda = 0 and fade = carry."""
    dt = depth.dtype.type
    lit = (depth != 0) & (carry != 0)
    s = np.where(lit, solid_sum(points(cam, depth, rows), ids, entries, owners), dt(0)).astype(depth.dtype)
    with np.errstate(all="ignore"):
        ks = np.where(s > 0, dt(kappa) * s, dt(0))               # not formed where s == 0: inf * 0 is never asked for
        lam = np.where(s > 0, np.where(ks < dt(1), ks, dt(1)), dt(0)).astype(depth.dtype)
    fade = np.where(carry == 0, dt(0), dt(1) - lam).astype(depth.dtype)
    return lam, fade, s


def gather_np(cam, cur, base, depth_tol, normal_cos, max_history, Q, fade):
    """(h, m) of section 19 through the faded plane: fade == 0 takes no taps, and m = m * fade after the cap."""
    h, m = M.gather_np(cam, cur, base, depth_tol, normal_cos, max_history, Q=Q, carry=fade)
    return h, (m * fade.astype(m.dtype)).astype(m.dtype)


def update_np(cam, cur, base, params, Q, fade):
    """(Cout, Mout, reprojected pixels) of rtiow_history_update through the faded plane."""
    h, m = gather_np(cam, cur, base, *params, Q, fade)
    Cout, Mout = blend_np(cur, h, m)
    return Cout, Mout, int((m > 0).sum())


def clipped_np(cam, cur, base, params, radius, gamma, Q, fade):
    """rtiow_history_update_clipped through the faded plane: the clamp of section 14 between the fade and the blend."""
    h, m = gather_np(cam, cur, base, *params, Q, fade)
    hc, mask = clip_np(cur, h, m, radius, gamma)
    C, Mo = blend_np(cur, hc, m)
    return {"C": C, "M": Mo, "h": h, "m": m, "reprojected": int((m > 0).sum()), "clipped": int(mask.sum()), "mask": mask}


def plan_np(cam, normal, depth, base, params, Q, fade):
    """(m, pixels with m > 0) of rtiow_history_plan through the faded plane."""
    _, m = gather_np(cam, {"N": normal, "t": depth}, base, *params, Q, fade)
    return m, int((m > 0).sum())
