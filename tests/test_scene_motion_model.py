"""tests/scene_motion_model.py on the CPU: its bits pinned by CRCs, the vectorised gather held to a scalar per-pixel statement of
INTEGRATION.md section 19, an edit that changes nothing held to tests/preview_model.py bit for bit, and -- on the oracle alone -- the six
classes of pixel the GPU tests rely on counted in every scene they use.  The base here is synthetic: the first-hit guides of the
unedited scene with a colour and a length drawn from a fixed generator."""
import zlib

import numpy as np
import pytest

from tests import scene_motion_model as M
from tests.lattice import lattice_scene
from tests.preview_model import LATTICE, base_constants, same_bits, vec
from tests.preview_model import clipped_np as plain_clipped_np, plan_np as plain_plan_np, update_np as plain_update_np

W, H = 64, 40
PARAMS = (0.1, 0.9, 32.0)
SCENES = [3, LATTICE, 1]


def scene_of(rt, prec, scene_id):
    return lattice_scene(prec) if scene_id == LATTICE else rt.build_scene(scene_id, prec)


def setting(rt, oracle, prec, scene_id, combined=True):
    """A base under the unedited scene, the combined edit of the class test (or no edit), and the current frame's planes."""
    dt = np.float32 if prec == 32 else np.float64
    scene = scene_of(rt, prec, scene_id)
    cam = M.view(rt, prec, scene_id, W, H)
    snap = M.tables(scene, prec)
    O, D, t, k = M.first_hit(oracle, prec, snap, cam, range(H))
    N0, z0 = M.guides_of(O, D, t, k, snap)
    rng = np.random.default_rng(7)
    base = {"cam": cam, "H": rng.random((H, W, 3)).astype(dt), "M": np.full((H, W), 3, dt), "N": N0, "z": z0}
    small = M.small_spheres(scene)
    kept = list(M.kept_slots(scene))
    seen = sorted(small, key=lambda s: -int((k == kept.index(s)).sum()))
    edit = scene
    if combined:
        edit = M.translate(scene, small, (0.03125, 0.0, 0.015625))           # every small sphere a fraction of its radius ...
        edit = M.translate(edit, seen[:2], (0.5, 0.0, 0.375))                # ... two of them several pixels ...
        edit = M.recolour(edit, seen[2:5])                                   # ... three get another colour ...
        big = sorted(M.big_spheres(scene), key=lambda b: -int((k == kept.index(b)).sum()))
        edit = M.translate(edit, big[:1], (0.0, 0.0, 0.75))                  # ... and the big sphere the frame shows most of uncovers what it hid
    cur_t = M.tables(edit, prec)
    O, D, t, k = M.first_hit(oracle, prec, cur_t, cam, range(H))
    N, z = M.guides_of(O, D, t, k, cur_t)
    Q, carry, ids = M.plane_np(O, D, t, k, cur_t, snap)
    cur = {"c": rng.random((H, W, 3)).astype(dt), "n": np.full((H, W), 3, np.int32), "N": N, "t": z}
    return {"cam": cam, "base": base, "cur": cur, "Q": Q, "carry": carry, "ids": ids, "flags": M.flags(cur_t, snap), "plain_cur": dict(cur, N=N0, t=z0)}


def scalar_m(cam, cur, base, params, Q, carry, x, y):
    """Section 19's m of one pixel, operation by operation on numpy scalars."""
    dt = cur["t"].dtype.type
    k = base_constants(base["cam"], dt)
    O, p00, du, dv = (vec(f, dt) for f in (cam.center, cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
    t, N = cur["t"][y, x], cur["N"][y, x]
    hit = t > 0
    with np.errstate(all="ignore"):
        D = [((p00[c] + dt(x) * du[c]) + dt(y) * dv[c]) - O[c] for c in range(3)]
        d = [Q[y, x, c] - k["O"][c] for c in range(3)] if hit else D
        den = (d[0] * k["w"][0] + d[1] * k["w"][1]) + d[2] * k["w"][2]
        if not den > 0 or (hit and carry[y, x] == 0):
            return dt(0)
        s = k["f"] / den
        e = [s * d[c] - k["a"][c] for c in range(3)]
        u = ((e[0] * k["du"][0] + e[1] * k["du"][1]) + e[2] * k["du"][2]) * k["iu"]
        v = ((e[0] * k["dv"][0] + e[1] * k["dv"][1]) + e[2] * k["dv"][2]) * k["iv"]
        te = den / k["f"]
        if not (u > dt(-1) and u < dt(W) and v > dt(-1) and v < dt(H)):
            return dt(0)
        xf, yf = np.floor(u), np.floor(v)
        fx, fy = u - xf, v - yf
        gx, gy = dt(1) - fx, dt(1) - fy
        b = (gx * gy, fx * gy, gx * fy, fx * fy)
        tol = dt(params[0]) * te
        sl, sb = dt(0), dt(0)
        for tap in range(4):
            qx, qy = int(xf) + (tap & 1), int(yf) + (tap >> 1)
            if qx < 0 or qx >= W or qy < 0 or qy >= H:
                continue
            Mq, Nq, zq = base["M"][qy, qx], base["N"][qy, qx], base["z"][qy, qx]
            ok = Mq > 0
            if hit:
                nn = (N[0] * Nq[0] + N[1] * Nq[1]) + N[2] * Nq[2]
                ok = ok and zq > 0 and abs(zq - te) <= tol and nn >= dt(params[1])
            else:
                ok = ok and zq == 0
            if ok:
                sl, sb = sl + b[tap] * Mq, sb + b[tap]
        m = sl / sb if sb > 0 else dt(0)
        return m if m < dt(params[2]) else dt(params[2])


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id", SCENES)
def test_six_classes_of_pixel_and_the_scalar_statement(native, oracle, prec, scene_id):
    s = setting(native, oracle, prec, scene_id)
    cam, base, cur, Q, carry, ids = (s[k] for k in ("cam", "base", "cur", "Q", "carry", "ids"))
    _, m = M.gather_np(cam, cur, base, *PARAMS, Q=Q, carry=carry)
    _, plain_m = M.gather_np(cam, s["plain_cur"], base, *PARAMS)              # the walk without the edit
    f = np.where(ids >= 0, s["flags"][np.maximum(ids, 0)], 0)
    hit = ids >= 0
    moved = hit & ((f & M.MOVED) != 0) & ((f & M.CHANGED) == 0)
    unmoved = hit & (f == 0)
    classes = {"unmoved": unmoved & (m > 0), "moved and carried": moved & (m > 0), "moved, every tap rejected": moved & (m == 0),
               "disoccluded": unmoved & (m == 0) & (plain_m > 0), "changed": hit & (carry == 0), "sky": ~hit}
    counts = {name: int(sel.sum()) for name, sel in classes.items()}
    print(prec, scene_id, counts)
    assert all(counts.values()), counts
    assert (m[classes["changed"]] == 0).all() and (carry[~classes["changed"]] == 1).all()
    # the scalar statement, on every pixel of the rarer classes and a lattice of the rest
    pick = np.zeros((H, W), bool)
    pick[::3, ::5] = True
    for name in ("moved and carried", "moved, every tap rejected", "disoccluded", "changed"):
        pick |= classes[name]
    for y, x in zip(*np.nonzero(pick)):
        got = scalar_m(cam, cur, base, PARAMS, Q, carry, x, y)
        assert got.dtype == m.dtype and got.tobytes() == m[y, x].tobytes(), (x, y, got, m[y, x])


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id", SCENES)
def test_an_edit_that_changes_nothing_is_the_plain_model(native, oracle, prec, scene_id):
    s = setting(native, oracle, prec, scene_id, combined=False)
    cam, base, cur, Q, carry = (s[k] for k in ("cam", "base", "cur", "Q", "carry"))
    assert (carry == 1).all() and not s["flags"].any()
    for a, b in zip(M.update_np(cam, cur, base, PARAMS, Q, carry), plain_update_np(cam, cur, base, *PARAMS)):
        assert a == b if isinstance(a, int) else same_bits(a, b)
    got, want = M.clipped_np(cam, cur, base, PARAMS, 1, 0.75, Q, carry), plain_clipped_np(cam, cur, base, PARAMS, 1, 0.75)
    for key in ("C", "M", "h", "m", "mask"):
        assert same_bits(got[key], want[key]), key
    assert (got["reprojected"], got["clipped"]) == (want["reprojected"], want["clipped"])
    m, count = M.plan_np(cam, cur["N"], cur["t"], base, PARAMS, Q, carry)
    want_m, want_count = plain_plan_np(cam, cur["N"], cur["t"], base, PARAMS)
    assert same_bits(m, want_m) and count == want_count


# zlib.crc32 of the model's outputs for setting(prec, scene_id): Q, carry, ids, the update's C and M, the clipped C, the plan's m
PINS = {
    (32, 3): (4140633802, 3399487021, 4021504972, 3030104934, 2255156112, 389860583, 1242165254),
    (64, 3): (2857814240, 3399487021, 4021504972, 2710175747, 2237480468, 2810113694, 2418237149),
    (32, LATTICE): (2902927013, 3948131755, 3039477681, 1235688850, 306250624, 2126676548, 2459470029),
    (64, LATTICE): (1216604849, 3948131755, 3039477681, 3258528010, 3736294252, 3935594817, 3897605368),
    (32, 1): (2701318264, 3048314421, 2710335689, 4088871583, 2802681929, 1301155791, 1213075885),
    (64, 1): (2788432509, 3048314421, 2710335689, 1891592734, 3706375883, 1578394780, 2641239396),
}


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id", SCENES)
def test_the_models_bits_are_pinned(native, oracle, prec, scene_id):
    s = setting(native, oracle, prec, scene_id)
    cam, base, cur, Q, carry, ids = (s[k] for k in ("cam", "base", "cur", "Q", "carry", "ids"))
    C, Mo, _ = M.update_np(cam, cur, base, PARAMS, Q, carry)
    clipped = M.clipped_np(cam, cur, base, PARAMS, 1, 0.75, Q, carry)["C"]
    m, _ = M.plan_np(cam, cur["N"], cur["t"], base, PARAMS, Q, carry)
    got = tuple(zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in (Q, carry, ids, C, Mo, clipped, m))
    assert got == PINS[(prec, scene_id)]
