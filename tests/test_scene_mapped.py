"""Scene edits that add and remove spheres (rtiow_edit_scene_mapped, rtiow_read_scene_origin) on the GPU: the
motion plane, the ids, the influence plane, the plan, the temporal colour and length and the counters, every pixel BIT FOR BIT against
tests/scene_mapped_model.py, on 40x24 (edge tiles in both tilings), 65x9 and 1x1, scenes 1 and 3, in both precisions: 4 bounces, one
sample per chunk, a base committed from one earlier frame.  That base has M = 1 at every pixel, so a pixel that carries gathers m = 1
exactly.  The edited slots are chosen from the oracle's first-hit ids on the CPU, so that every case has pixels in the class it is about."""
import ctypes

import numpy as np
import pytest

from tests import edit_influence_model as E
from tests import scene_mapped_model as S
from tests import scene_motion_model as M
from tests.conftest import compact
from tests.preview_drive import E_BADARG, E_STATE, INF, as_base, check_update, history_defaults, state
from tests.preview_model import budget_rule, same_bits

pytestmark = pytest.mark.gpu

FRAMES = [(40, 24), (65, 9), (1, 1)]
CASES = [(s, W, H) for s in (1, 3) for W, H in FRAMES]
IDS = ["%s-%dx%d" % c for c in CASES]
KAPPAS = (0.5, INF)
CLIP = (1, 0.75)
B = 4
CALL = "rtiow_edit_scene_mapped"
I32P = ctypes.POINTER(ctypes.c_int32)


# ---- what the frame shows, from the oracle on the CPU

def first_ids(oracle, prec, scene, cam):
    """(t, k) of every pixel's first hit in `scene`, k in the numbering of its kept spheres."""
    _, _, t, k = M.first_hit(oracle, prec, M.tables(scene, prec), cam, range(cam.img_height))
    return t, k


def number_of(scene, slot):
    return [int(s) for s in M.kept_slots(scene)].index(int(slot))


def radii(scene):
    return np.asarray(scene["center_radius"], np.float64).reshape(-1, 4)[:, 3]


def seen(oracle, prec, scene, cam):
    """The slots the frame shows first, most wanted first: small spheres by pixels, then the other spheres by pixels, then the ground.
    (A 1x1 frame shows one of them; the cases take what it shows.)"""
    _, k = first_ids(oracle, prec, scene, cam)
    kept, r = [int(s) for s in M.kept_slots(scene)], radii(scene)
    pixels = {kept[j]: int(c) for j, c in enumerate(np.bincount(k[k >= 0], minlength=len(kept))) if c}
    rank = lambda s: (0 if r[s] < 0.6 else 1 if r[s] < 100 else 2, -pixels[s], s)
    return sorted(pixels, key=rank)


def removable(oracle, prec, scene, cam, params):
    """The slot test_remove_a_visible_sphere takes away: the first of seen() whose every uncovered pixel the MODEL gives m = 0, worked
    out on the CPU from the oracle alone (a base of one sample holds M = 1 and the guides of the committed scene, whatever its colours).
    The taps that land on the removed sphere always fail.  But an uncovered pixel on the sphere's silhouette reprojects an ulp beside its
    own centre, so one of its four taps can be the base pixel next to it, which showed the ground it shows now: that tap passes and the
    pixel keeps that history, rightly.  And a neighbour of the sphere's own size right behind it shows the same part of itself within the
    depth tolerance.  Both are the gather's own rules (sections 11 and 19) and happen behind a sphere that rtiow_edit_scene moves away
    too.  Measured on the CPU for the most-shown small sphere: scene 1 at 40x24 keeps 1 (fp32) / 3 (fp64) of its 16 uncovered pixels,
    at 65x9 1 / 1 of 3; scene 3 at 40x24 0 / 1 of 3.  Those spheres are passed over for the next one shown."""
    tb = M.tables(scene, prec)
    O, D, t, old_k = M.first_hit(oracle, prec, tb, cam, range(cam.img_height))
    normal, depth = M.guides_of(O, D, t, old_k, tb)
    base = {"cam": cam, "H": np.zeros_like(normal), "M": np.ones_like(depth), "N": normal, "z": depth}
    order = seen(oracle, prec, scene, cam)
    for slot in order:
        without, origin = S.take(scene, [s for s in range(len(scene["type"])) if s != slot])
        fs = S.compose(S.identity(len(tb["ty"])), S.kept_pattern(scene), S.kept_pattern(without), origin)
        want = S.planes(oracle, prec, without, cam, tb, fs, 0.0)
        m, _ = E.plan_np(cam, want["N"], want["t"], base, params, want["Q"], want["fade"])
        if (m[old_k == number_of(scene, slot)] == 0).all():
            return slot
    raise AssertionError("no sphere of this frame uncovers pixels without history: choose another frame")


def unseen_small(oracle, prec, scene, cam, count):
    """Small spheres the frame does not show first, in slot order."""
    shown = set(seen(oracle, prec, scene, cam))
    return [s for s in M.small_spheres(scene) if s not in shown][:count]


def spot(oracle, prec, scene, cam, avoid=()):
    """(centre, radius) of a new sphere that some pixel shows first: on the ray of a pixel, in front of what that pixel shows -- a ground
    pixel in the middle of the ground's if there is one.  avoid: numbers of kept spheres whose pixels are not taken."""
    dt = np.float32 if prec == 32 else np.float64
    O, D, t, k = M.first_hit(oracle, prec, M.tables(scene, prec), cam, range(cam.img_height))
    r = radii(scene)[M.kept_slots(scene)]
    ground = np.argwhere((k >= 0) & (r[np.maximum(k, 0)] >= 100))
    free = np.argwhere(~np.isin(k, list(avoid)))
    y, x = ground[len(ground) // 2] if len(ground) else free[len(free) // 2] if len(free) else (0, 0)
    far = float(t[y, x]) if k[y, x] >= 0 else 12.0
    centre = np.asarray(O, np.float64) + 0.75 * far * np.asarray(D[y, x], np.float64)
    return centre.astype(dt), dt(0.02 * far)


def new_spheres(scene, places):
    """append() of diffuse grey spheres at places = [(centre, radius), ...]."""
    cr = [list(c) + [r] for c, r in places]
    return S.append(scene, cr, [[0.5, 0.25, 0.125, 0.0]] * len(cr), [1.5] * len(cr), [0] * len(cr))


class Frame:
    """A handle with a base committed under `scene` at `cam` from one frame of one sample, the model's base beside it, and the scene the
    handle holds with its map as the model composes it."""

    def __init__(self, rt, prec, scene, cam, source=3, shard=None):
        self.rt, self.prec, self.params = rt, prec, history_defaults(rt)
        self.r = r = rt.Renderer(0, prec)
        r.set_camera(cam)
        r.set_scene(scene)
        r.set_scene_source(source)
        if shard:
            r.set_shard(*shard)
        r.init_rng(1227)
        r.accumulate(1)
        cur = state(r, False)
        c0, m0, _ = check_update(r, cam, cur, None, self.params, "the base frame")
        r.history_commit()
        self.base = as_base(cam, cur, c0, m0)
        self.committed(scene)

    def committed(self, scene):
        self.scene, self.snap = scene, M.tables(scene, self.prec)
        self.fs = S.identity(len(self.snap["ty"]))

    def close(self):
        self.r.close()

    def mapped(self, scene, origin, cam, seed=1300):
        self.r.edit_scene_mapped(scene, origin)
        self.fs = S.compose(self.fs, S.kept_pattern(self.scene), S.kept_pattern(scene), origin)
        self.scene = scene
        self.r.set_camera(cam)
        self.r.init_rng(seed)

    def plain(self, scene, cam, seed=1300):
        self.r.edit_scene(scene)
        self.scene = scene
        self.r.set_camera(cam)
        self.r.init_rng(seed)

    def model(self, oracle, cam, kappa=0.0):
        return S.planes(oracle, self.prec, self.scene, cam, self.snap, self.fs, kappa)

    def check_planes(self, want, where, kappa=0.0):
        """The map, the motion plane as the public read shows it, the guides and (knob on) the influence plane of the handle as it stands."""
        r = self.r
        if kappa:
            assert same_bits(r.edit_influence(), want["lam"]), where
        gq, gc, gi = r.scene_motion()
        assert np.array_equal(gi, want["ids"]), where
        assert same_bits(gq, want["Q"]), where
        assert np.array_equal(gc, (want["fade"] != 0).astype(np.int32)), where
        normal, _, depth = r.guides()
        assert same_bits(depth, want["t"]) and same_bits(normal, want["N"]), where
        assert np.array_equal(r.scene_origin(), self.fs) and r.stats()["num_spheres"] == len(self.fs), where

    def check_chain(self, want, cam, where):
        """Plan, one sample, update and clipped update through the plane against the model; returns the model's and the library's."""
        r, params = self.r, self.params
        Q, fade = want["Q"], want["fade"]
        planned = r.history_plan(*params)
        want_m, want_count = E.plan_np(cam, want["N"], want["t"], self.base, params, Q, fade)
        got_m = r.history_plan_lengths()
        assert same_bits(got_m, want_m) and planned == want_count, (where, planned, want_count)
        r.accumulate(1)
        cur = state(r, False)
        count = r.history_update(*params)
        rgb, length = r.history()
        wc, wm, wcount = E.update_np(cam, cur, self.base, params, Q, fade)
        assert same_bits(length, wm) and same_bits(rgb, wc) and count == wcount, (where, count, wcount)
        assert same_bits(length, want_m + cur["n"].astype(want_m.dtype)), where          # the plan predicted Mout - n
        counts = r.history_update_clipped(*CLIP, *params)
        crgb, clength = r.history()
        wcl = E.clipped_np(cam, cur, self.base, params, *CLIP, Q, fade)
        assert same_bits(clength, wcl["M"]) and same_bits(crgb, wcl["C"]), where
        assert counts == (wcl["reprojected"], wcl["clipped"]), (where, counts)
        assert (wcl["m"][fade == 0] == 0).all(), where
        return {"cur": cur, "plan": want_m, "planned": planned, "C": wc, "M": wm, "count": count, "clipped_C": wcl["C"], "clipped_M": wcl["M"], "counts": counts}

    def commit(self, cam, got):
        """history_commit() after check_chain: the clipped temporal image becomes the base, the scene the snapshot, the map the identity."""
        self.r.history_commit()
        self.base = as_base(cam, got["cur"], got["clipped_C"], got["clipped_M"])
        self.committed(self.scene)


def setting(rt, oracle, prec, scene_id, W, H):
    scene = rt.build_scene(scene_id, prec)
    return scene, rt.camera(prec, W, H, 1, B)


def same_chain(a, b, where, ids=None):
    """Two check_chain results and planes, bit for bit (ids: how the second numbers the first's spheres, None: the same)."""
    for key in ("plan", "C", "M", "clipped_C", "clipped_M"):
        assert same_bits(a[key], b[key]), (where, key)
    assert (a["planned"], a["count"], a["counts"]) == (b["planned"], b["count"], b["counts"]), where
    assert same_bits(a["cur"]["c"], b["cur"]["c"]), where


# ---- the cases

@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id,W,H", CASES, ids=IDS)
def test_identity_map_is_the_plain_edit(native, oracle, prec, scene_id, W, H):
    rt = native
    scene, cam = setting(rt, oracle, prec, scene_id, W, H)
    top = seen(oracle, prec, scene, cam)
    small = M.small_spheres(scene)
    edit = M.recolour(M.translate(scene, [top[0]] + small[:3], (0.0625, 0.0, 0.03125)), small[3:5])
    got = []
    for mapped in (False, True):
        f = Frame(rt, prec, scene, cam)
        try:
            if mapped:
                f.mapped(edit, S.same_slots(edit), cam)
            else:
                f.plain(edit, cam)
            want = f.model(oracle, cam)
            assert (want["ids"] == number_of(scene, top[0])).any() and len(want["owners"]) >= 8
            f.check_planes(want, (scene_id, W, H, mapped))
            got.append((want, f.check_chain(want, cam, (scene_id, W, H, mapped)), f.r.scene_motion()))
        finally:
            f.close()
    same_chain(got[0][1], got[1][1], (scene_id, W, H))
    for a, b in zip(got[0][2], got[1][2]):
        assert same_bits(a, b)


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id,W,H", CASES, ids=IDS)
def test_remove_a_visible_sphere(native, oracle, prec, scene_id, W, H):
    rt = native
    scene, cam = setting(rt, oracle, prec, scene_id, W, H)
    victim = removable(oracle, prec, scene, cam, history_defaults(rt))
    _, old_k = first_ids(oracle, prec, scene, cam)
    gone = old_k == number_of(scene, victim)
    assert gone.any()
    slots = [s for s in range(len(scene["type"])) if s != victim]
    edit, origin = S.take(scene, slots)                          # one slot fewer: every later sphere is renumbered
    for source in (3, 0, 1, 2):
        f = Frame(rt, prec, scene, cam, source=source)
        try:
            where = (scene_id, W, H, source)
            f.mapped(edit, origin, cam)
            assert len(f.fs) == len(f.snap["ty"]) - 1 and number_of(scene, victim) not in f.fs.tolist() and S.NO_ORIGIN not in f.fs.tolist()
            want = f.model(oracle, cam)
            assert want["owners"].tolist() == [S.OWNER_REMOVED], where
            f.check_planes(want, where)
            if source != 3:
                continue
            got = f.check_chain(want, cam, where)
            # what the removed sphere hid fails the gather's tests
            assert (got["plan"][gone] == 0).all(), where
            # the ids are in the new numbering: a sphere behind the victim in slot order is one lower
            _, new_k = first_ids(oracle, prec, edit, cam)
            assert np.array_equal(want["ids"], new_k), where
            later = (old_k > number_of(scene, victim)) & (new_k == old_k - 1)
            assert later.any() or W * H == 1, where
            # a pixel whose first hit, old and new, is the same untouched sphere or the sky keeps the plain call's bits
            untouched = ~gone & (new_k == np.where(old_k > number_of(scene, victim), old_k - 1, old_k))
            assert untouched.any() or W * H == 1, where
            twin = Frame(rt, prec, scene, cam)
            try:
                twin.plain(scene, cam)
                plain = twin.check_chain(twin.model(oracle, cam), cam, where)
            finally:
                twin.close()
            for key in ("plan", "M", "clipped_M"):
                assert same_bits(np.ascontiguousarray(plain[key][untouched]), np.ascontiguousarray(got[key][untouched])), (where, key)
            # ... and accumulate_budget samples the uncovered pixels: one chunk towards the length the base holds
            f.mapped(edit, S.same_slots(edit), cam)
            f.r.history_plan(*f.params)
            m = f.r.history_plan_lengths()
            mask = budget_rule(np.zeros((H, W), np.int32), m, 1, 1.0, 0, 1 << 30)
            assert f.r.accumulate_budget(1, 1.0, 0)[1] == int(mask.sum()) and np.array_equal(f.r.adaptive_state()[0], mask.astype(np.int32)), where
            assert mask[gone].all() and not mask[m == 1].any(), where
        finally:
            f.close()


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id,W,H", CASES, ids=IDS)
def test_add_a_sphere_in_front_of_the_ground(native, oracle, prec, scene_id, W, H):
    rt = native
    scene, cam = setting(rt, oracle, prec, scene_id, W, H)
    edit, origin = new_spheres(scene, [spot(oracle, prec, scene, cam)])
    added = len(M.kept_slots(edit)) - 1
    _, old_k = first_ids(oracle, prec, scene, cam)
    for source in (3, 0, 1, 2):
        f = Frame(rt, prec, scene, cam, source=source)
        try:
            where = (scene_id, W, H, source)
            f.mapped(edit, origin, cam)
            assert f.fs.tolist() == list(range(added)) + [S.NO_ORIGIN]
            want = f.model(oracle, cam)
            own = want["ids"] == added
            assert own.any() and (want["carry"][own] == 0).all() and (want["Q"][own] == 0).all() and (want["carry"][~own] == 1).all(), where
            assert want["owners"].tolist() == [added], where
            f.check_planes(want, where)
            if source != 3:
                continue
            got = f.check_chain(want, cam, where)
            assert (got["plan"][own] == 0).all(), where
            rest = ~own & (want["ids"] == old_k)                 # the rest keep their bits
            twin = Frame(rt, prec, scene, cam)
            try:
                twin.plain(scene, cam)
                plain = twin.check_chain(twin.model(oracle, cam), cam, where)
            finally:
                twin.close()
            assert rest.any() or W * H == 1, where
            for key in ("plan", "M", "clipped_M"):
                assert same_bits(np.ascontiguousarray(plain[key][rest]), np.ascontiguousarray(got[key][rest])), (where, key)
        finally:
            f.close()


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("W,H", FRAMES)
def test_add_four_spheres_across_a_padded_count(native, oracle, prec, W, H):
    """Scene 3 holds 125 spheres, padded to 128; with four more it holds 129, padded to 132: every table is laid out anew."""
    rt = native
    scene, cam = setting(rt, oracle, prec, 3, W, H)
    kept = len(M.kept_slots(scene))
    assert kept == 125 and (kept + 4) // 4 * 4 != (kept + 4 + 4) // 4 * 4
    centre, r = spot(oracle, prec, scene, cam)
    edit, origin = new_spheres(scene, [(centre + np.array(d, centre.dtype) * r * 3, r) for d in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))])
    want_img, _ = oracle.render(prec, compact(edit), cam, 1227)
    for source in (3, 0, 1, 2):
        f = Frame(rt, prec, scene, cam, source=source)
        try:
            where = (W, H, source)
            f.mapped(edit, origin, cam)
            assert f.r.stats()["num_spheres"] == 129 and f.fs.tolist() == list(range(125)) + [S.NO_ORIGIN] * 4
            want = f.model(oracle, cam)
            assert (want["ids"] >= 125).any() and want["owners"].tolist() == [125, 126, 127, 128], where
            f.check_planes(want, where)
            if source == 3:
                f.check_chain(want, cam, where)
            f.r.init_rng(1227)
            f.r.render(0)
            assert same_bits(f.r.read_framebuffer(), want_img), where
        finally:
            f.close()


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id,W,H", CASES, ids=IDS)
def test_permuted_slots_change_the_ids_alone(native, oracle, prec, scene_id, W, H):
    rt = native
    scene, cam = setting(rt, oracle, prec, scene_id, W, H)
    hidden = unseen_small(oracle, prec, scene, cam, 3)
    start, _ = S.drop(scene, hidden)                             # dropped slots in the middle of the committed scene ...
    n = len(start["type"])
    # ... and, carried along, in the middle of the permuted one: the slots backwards, turned until both ends are kept
    turn = next(k for k in range(7, n) if S.kept_pattern(start)[np.roll(np.arange(n)[::-1], k)[[0, -1]]].all())
    perm = np.roll(np.arange(n)[::-1], turn)
    edit, origin = S.take(start, perm)
    assert 0 < np.flatnonzero(S.kept_pattern(start) == 0).min() and np.flatnonzero(S.kept_pattern(start) == 0).max() < n - 1
    assert 0 < np.flatnonzero(S.kept_pattern(edit) == 0).min() and np.flatnonzero(S.kept_pattern(edit) == 0).max() < n - 1
    assert len(M.kept_slots(edit)) == len(M.kept_slots(start)) < n
    # no first-hit ties: both orders give every pixel the same sphere at the same distance
    t0, k0 = first_ids(oracle, prec, start, cam)
    t1, k1 = first_ids(oracle, prec, edit, cam)
    renumber = np.array([number_of(edit, int(np.flatnonzero(perm == s)[0])) for s in M.kept_slots(start)])
    assert same_bits(t0, t1) and np.array_equal(k1, np.where(k0 >= 0, renumber[np.maximum(k0, 0)], -1)), "a first-hit tie: choose another frame"
    assert (k0 >= 0).any() and (k1 != k0).any()
    got = []
    for mapped in (False, True):
        f = Frame(rt, prec, start, cam)
        try:
            if mapped:
                f.mapped(edit, origin, cam)
                assert np.array_equal(f.fs[renumber], np.arange(len(renumber)))
            else:
                f.plain(start, cam)
            want = f.model(oracle, cam)
            assert len(want["owners"]) == 0 and (want["carry"] == 1).all()
            f.check_planes(want, (scene_id, W, H, mapped))
            got.append((want, f.check_chain(want, cam, (scene_id, W, H, mapped)), f.r.scene_motion()))
        finally:
            f.close()
    same_chain(got[0][1], got[1][1], (scene_id, W, H))
    (q0, c0, i0), (q1, c1, i1) = got[0][2], got[1][2]
    assert same_bits(q0, q1) and np.array_equal(c0, c1) and np.array_equal(i1, np.where(i0 >= 0, renumber[np.maximum(i0, 0)], -1))


def all_at_once(oracle, prec, scene, cam):
    """Move, recolour, remove and add in one call; returns (scene', origin, the four slots / numbers the case is about)."""
    top = seen(oracle, prec, scene, cam)
    small = [s for s in M.small_spheres(scene) if s not in top[:1]]
    moved, recoloured, removed = (top[0], small[0], small[1])
    step = M.recolour(M.translate(scene, [moved], (0.0625, 0.0, -0.03125)), [recoloured])
    step, o1 = S.take(step, [s for s in range(len(scene["type"])) if s != removed])
    edit, o2 = new_spheres(step, [spot(oracle, prec, step, cam, avoid=[number_of(step, int(np.flatnonzero(o1 == moved)[0]))])])
    return edit, S.then(o1, o2), (moved, recoloured, removed)


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("kappa", (0.0,) + KAPPAS)
@pytest.mark.parametrize("scene_id,W,H", CASES, ids=IDS)
def test_move_recolour_remove_and_add_in_one_call(native, oracle, prec, scene_id, W, H, kappa):
    rt = native
    scene, cam = setting(rt, oracle, prec, scene_id, W, H)
    edit, origin, (moved, recoloured, removed) = all_at_once(oracle, prec, scene, cam)
    f = Frame(rt, prec, scene, cam)
    try:
        where = (scene_id, W, H, kappa)
        f.r.set_edit_influence(kappa)
        f.mapped(edit, origin, cam)
        want = f.model(oracle, cam, kappa)
        new_moved = f.fs.tolist().index(number_of(scene, moved))
        assert S.flags(M.tables(edit, prec), f.snap, f.fs)[new_moved] == M.MOVED and f.fs[-1] == S.NO_ORIGIN and number_of(scene, removed) not in f.fs.tolist()
        assert want["owners"].tolist() == sorted(want["owners"][:-1].tolist()) + [S.OWNER_REMOVED] and len(want["owners"]) == 5, where
        assert (want["ids"] == new_moved).any() or W * H == 1, where
        assert (want["ids"] == len(f.fs) - 1).any() or W * H == 1, where
        f.check_planes(want, where, kappa)
        f.check_chain(want, cam, where)
        if kappa == INF:
            assert np.array_equal(want["lam"], ((want["s"] > 0) * 1).astype(want["lam"].dtype)), where
    finally:
        f.close()


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id,W,H", CASES, ids=IDS)
def test_two_mapped_edits_compose_before_one_commit_and_a_commit_takes_the_new_shape(native, oracle, prec, scene_id, W, H):
    rt = native
    scene, cam = setting(rt, oracle, prec, scene_id, W, H)
    lib = rt.api.load_hip_library()
    f = Frame(rt, prec, scene, cam)
    try:
        # (a) add a sphere, then move it, no commit between: it still has no origin and carries nothing
        first, o1 = new_spheres(scene, [spot(oracle, prec, scene, cam)])
        f.mapped(first, o1, cam)
        added_slot = len(first["type"]) - 1
        nudge = float(first["center_radius"][added_slot, 3]) * 0.125
        second = M.translate(first, [added_slot], (nudge, 0.0, nudge))
        f.mapped(second, S.same_slots(second), cam, seed=1301)
        assert f.fs[-1] == S.NO_ORIGIN and f.r.scene_origin()[-1] == -1
        want = f.model(oracle, cam)
        own = want["ids"] == len(f.fs) - 1
        assert own.any() and (want["carry"][own] == 0).all(), "added then moved"
        f.check_planes(want, "added then moved")
        f.check_chain(want, cam, "added then moved")
        # ... and a plain edit of that shape leaves the map alone
        f.plain(M.recolour(second, M.small_spheres(second)[:1]), cam, seed=1302)
        assert f.r.scene_origin()[-1] == -1
        want = f.model(oracle, cam)
        f.check_planes(want, "a plain edit after a mapped one")
        got = f.check_chain(want, cam, "a plain edit after a mapped one")
        # commit: the snapshot takes the new shape and the map is the identity
        f.commit(cam, got)
        assert lib.rtiow_read_scene_origin(f.r._h, None, len(f.fs)) == E_STATE
        assert len(f.fs) == len(M.kept_slots(scene)) + 1
        # (b) from the new snapshot: move a kept sphere in one call, remove another in the next
        top = seen(oracle, prec, f.scene, cam)
        mover = top[0]
        other = [s for s in M.small_spheres(f.scene) if s < mover][:1] or [s for s in M.small_spheres(f.scene) if s != mover][:1]
        step = float(radii(f.scene)[mover]) * 0.25               # by a share of its radius: the pixels at its middle still show it
        middle = M.translate(f.scene, [mover], (step, 0.0, 0.5 * step))
        f.mapped(middle, S.same_slots(middle), cam, seed=1303)
        last, o2 = S.take(middle, [s for s in range(len(middle["type"])) if s != other[0]])
        f.mapped(last, o2, cam, seed=1304)
        want = f.model(oracle, cam)
        k_mover = number_of(last, int(np.flatnonzero(o2 == mover)[0]))
        on_it = want["ids"] == k_mover
        assert S.flags(M.tables(last, prec), f.snap, f.fs)[k_mover] == M.MOVED and on_it.any()
        # Q is taken from the snapshot: against the intermediate scene the sphere did not move and Q would be the hit point itself
        O, D, t, _ = M.first_hit(oracle, prec, M.tables(last, prec), cam, range(H))
        assert not same_bits(np.ascontiguousarray(want["Q"][on_it]), np.ascontiguousarray((O + t[..., None] * D)[on_it].astype(want["Q"].dtype)))
        f.check_planes(want, "moved, then another removed")
        got = f.check_chain(want, cam, "moved, then another removed")
        # commit after a mapped edit, then a plain edit_scene() of that shape: accepted and bit-exact
        f.commit(cam, got)
        assert len(f.fs) == len(M.kept_slots(scene)) and lib.rtiow_read_scene_origin(f.r._h, None, len(f.fs)) == E_STATE
        f.plain(M.translate(f.scene, [mover if mover < other[0] else mover - 1], (0.0, 0.0, 0.0625)), cam, seed=1305)
        assert np.array_equal(f.r.scene_origin(), np.arange(len(f.fs)))
        want = f.model(oracle, cam)
        assert len(want["owners"]) == 2
        f.check_planes(want, "a plain edit after the commit")
        f.check_chain(want, cam, "a plain edit after the commit")
    finally:
        f.close()


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id,W,H", CASES, ids=IDS)
def test_edit_influence_with_added_and_removed_entries(native, oracle, prec, scene_id, W, H):
    """Lists of 0 entries (a permutation), 1 (one removed; one added) and more than the kernel's chunk of 32 (20 removed and 20 added)."""
    rt = native
    scene, cam = setting(rt, oracle, prec, scene_id, W, H)
    n = len(scene["type"])
    top = seen(oracle, prec, scene, cam)
    small = M.small_spheres(scene)
    out = [top[0]] + [s for s in small if s != top[0]][:19]
    cr = np.asarray(scene["center_radius"]).reshape(-1, 4)
    many, o_take = S.take(scene, [s for s in range(n) if s not in out])
    many, o_app = new_spheres(many, [(cr[s, :3] + np.array([0.3, 0.0, 0.3], cr.dtype), cr[s, 3]) for s in out])
    edits = {"none": S.take(scene, np.roll(np.arange(n), 5)), "removed": S.take(scene, [s for s in range(n) if s != top[0]]),
             "added": new_spheres(scene, [spot(oracle, prec, scene, cam)]), "many": (many, S.then(o_take, o_app))}
    sizes = {"none": 0, "removed": 1, "added": 1, "many": 40}
    for name, (edit, origin) in edits.items():
        f = Frame(rt, prec, scene, cam)
        try:
            for kappa in KAPPAS:
                where = (scene_id, W, H, name, kappa)
                f.r.set_edit_influence(kappa)
                f.mapped(edit, origin if kappa == KAPPAS[0] else S.same_slots(edit), cam)
                want = f.model(oracle, cam, kappa)
                assert len(want["owners"]) == sizes[name], where
                hit = want["t"] != 0
                if name == "none":
                    assert (want["lam"] == 0).all(), where
                if name == "removed":
                    assert want["owners"].tolist() == [S.OWNER_REMOVED] and ((want["lam"] > 0) == (hit & (want["s"] > 0))).all(), where
                    assert (want["lam"][hit] > 0).any() or W * H == 1, where
                if name == "added":
                    own = want["ids"] == want["owners"][0]
                    assert own.any() and (want["lam"][own] == 0).all() and (want["fade"][own] == 0).all(), where
                if name == "many":
                    assert len(want["owners"]) > E.CHUNK and (want["owners"] == S.OWNER_REMOVED).sum() == 20 and (want["owners"] >= 0).sum() == 20, where
                    assert (want["lam"][hit] > 0).any() or W * H == 1, where
                if kappa == INF:
                    assert np.array_equal(want["lam"], ((want["s"] > 0) * 1).astype(want["lam"].dtype)), where
                f.check_planes(want, where, kappa)
                got = f.check_chain(want, cam, where)
                # the budget counts by the faded plan: one chunk towards the length the base holds
                f.mapped(edit, S.same_slots(edit), cam)
                f.r.history_plan(*f.params)
                mask = budget_rule(np.zeros((H, W), np.int32), got["plan"], 1, 1.0, 0, 1 << 30)
                assert f.r.accumulate_budget(1, 1.0, 0)[1] == int(mask.sum()) and np.array_equal(f.r.adaptive_state()[0], mask.astype(np.int32)), where
        finally:
            f.close()


def raw_call(lib, r, scene, origin, dt, n=None, valid="scene", tables=True):
    """rtiow_edit_scene_mapped itself, with arguments a wrapper would not pass; returns (code, the handle's error text)."""
    cr = np.ascontiguousarray(scene["center_radius"], dt); af = np.ascontiguousarray(scene["albedo_fuzz"], dt)
    ri = np.ascontiguousarray(scene["refraction_index"], dt); ty = np.ascontiguousarray(scene["type"], np.int32)
    va = np.ascontiguousarray(scene["valid"] if isinstance(valid, str) else valid, np.int32) if valid is not None else None
    og = np.ascontiguousarray(origin, np.int32) if origin is not None else None
    rc = lib.rtiow_edit_scene_mapped(r._h, len(ty) if n is None else n, cr.ctypes.data if tables else None, af.ctypes.data, ri.ctypes.data, ty.ctypes.data_as(I32P),
                                     va.ctypes.data_as(I32P) if va is not None else None, og.ctypes.data_as(I32P) if og is not None else None)
    return rc, lib.rtiow_last_error_string(r._h).decode()


@pytest.mark.parametrize("prec", [32, 64])
def test_refusals_leave_the_handle_as_it_was(native, oracle, prec):
    rt = native
    W, H = 40, 24
    scene, cam = setting(rt, oracle, prec, 3, W, H)
    dt = np.float32 if prec == 32 else np.float64
    lib = rt.api.load_hip_library()
    n = len(scene["type"])
    kept = S.kept_pattern(scene)
    same = S.same_slots(scene)
    dropped = int(np.flatnonzero(kept == 0)[0]) if (kept == 0).any() else None
    with rt.Renderer(0, prec) as r:                              # no scene yet: asked after the tables, before the origin
        r.set_camera(cam)
        assert raw_call(lib, r, scene, None, dt, tables=False) == (E_BADARG, S.refusal(CALL, False, n, None, None, None, False, kept)[1])
        assert raw_call(lib, r, scene, None, dt) == (E_STATE, CALL + " before rtiow_set_scene")
        with pytest.raises(rt.RtiowError) as err:
            r.edit_scene_mapped(scene, same)
        assert err.value.code == E_STATE
        with pytest.raises(ValueError):
            r.edit_scene_mapped(scene, same[:-1])
    start = scene if dropped is not None else S.drop(scene, unseen_small(oracle, prec, scene, cam, 1))[0]
    kept = S.kept_pattern(start)
    dropped = int(np.flatnonzero(kept == 0)[0])
    first_kept = int(np.flatnonzero(kept)[0])
    f = Frame(rt, prec, start, cam)
    try:
        r = f.r
        r.init_rng(1227)
        r.render(0)
        before = r.read_framebuffer()
        bad_type = dict(start, type=np.where(np.arange(n) == first_kept, 3, start["type"]).astype(np.int32))
        two = same.copy(); two[np.flatnonzero(kept)[1]] = first_kept
        cases = [
            dict(origin=None, tables=False), dict(origin=None, n=0), dict(origin=None, n=-1),
            dict(origin=None), dict(origin=None, scene=bad_type),
            dict(origin=np.where(same == first_kept, -2, same)), dict(origin=np.where(same == first_kept, n, same)),
            dict(origin=np.where(same == first_kept, dropped, same)), dict(origin=np.where(same == first_kept, n, two)),
            dict(origin=two), dict(origin=two, scene=bad_type),
            dict(origin=same, scene=bad_type), dict(origin=same, valid=np.zeros(n, np.int32)),
        ]
        for case in cases:
            sc = case.get("scene", start)
            nn = case.get("n", n)
            valid = case.get("valid", sc["valid"])
            want = S.refusal(CALL, case.get("tables", True), nn, valid, sc["type"], case["origin"], True, kept)
            assert want[0] != 0, case
            got = raw_call(lib, r, sc, case["origin"], dt, n=case.get("n"), valid=valid, tables=case.get("tables", True))
            assert got == want, (case, got, want)
            assert lib.rtiow_read_scene_origin(r._h, None, len(f.fs)) == E_STATE         # a refused edit puts no motion in effect
        # the orders the model pins, through the library: range before duplicates before types
        assert raw_call(lib, r, bad_type, np.where(same == first_kept, n, two), dt)[1].endswith("a slot the current scene keeps")
        assert raw_call(lib, r, bad_type, two, dt)[1].endswith("(a sphere is continued at most once)")
        # after the refused calls the render's bits are what they were
        r.init_rng(1227)
        r.render(0)
        assert same_bits(r.read_framebuffer(), before)
        # the origin of a dropped slot is not read
        assert raw_call(lib, r, start, np.where(kept == 0, -77, same), dt)[0] == 0
        assert np.array_equal(r.scene_origin(), f.fs)
    finally:
        f.close()
    # a handle the refused calls were made on: the next update is the plain path against the plain model, the base intact
    f = Frame(rt, prec, start, cam)
    try:
        r = f.r
        assert raw_call(lib, r, start, None, dt)[0] == E_BADARG and raw_call(lib, r, start, two, dt)[0] == E_BADARG
        assert same_bits(r.history_base()[1], f.base["M"])
        r.set_camera(cam)
        r.init_rng(1300)
        r.accumulate(1)
        check_update(r, cam, state(r, False), f.base, f.params, "after refused mapped edits")
        # the read's own refusals
        f.mapped(start, same, cam)
        assert lib.rtiow_read_scene_origin(r._h, None, len(f.fs)) == 0                  # no plane needed
        assert lib.rtiow_read_scene_origin(r._h, None, len(f.fs) + 1) == E_BADARG and lib.rtiow_read_scene_origin(r._h, None, len(f.fs) - 1) == E_BADARG
        assert "count must be the number of kept spheres" in lib.rtiow_last_error_string(r._h).decode()
        r.history_reset()
        assert lib.rtiow_read_scene_origin(r._h, None, len(f.fs)) == E_STATE
        assert lib.rtiow_last_error_string(r._h).decode() == "rtiow_read_scene_origin: motion is not in effect (rtiow_edit_scene on a handle with a history base)"
    finally:
        f.close()


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id,W,H", CASES, ids=IDS)
def test_without_a_base_the_call_is_set_scene(native, oracle, prec, scene_id, W, H):
    rt = native
    scene = rt.build_scene(scene_id, prec)
    cam = rt.camera(prec, W, H, 2, B)
    edit, origin, _ = all_at_once(oracle, prec, scene, cam)
    want, _ = oracle.render(prec, compact(edit), cam, 1227)
    lib = rt.api.load_hip_library()
    for shard in (None, (0, 1, 4)):
        with rt.Renderer(0, prec) as r:
            r.set_camera(cam)
            r.set_scene(scene)
            if shard:
                r.set_shard(*shard)
            r.edit_scene_mapped(edit, origin)
            assert r.stats()["num_spheres"] == len(M.kept_slots(edit))
            assert lib.rtiow_read_scene_origin(r._h, None, len(M.kept_slots(edit))) == E_STATE
            with pytest.raises(rt.RtiowError) as err:
                r.scene_origin()
            assert err.value.code == E_STATE
            r.init_rng(1227)
            r.render(0)
            assert same_bits(r.read_framebuffer(), want), (scene_id, W, H, shard)
    with rt.Renderer(0, prec) as r:                              # several ranks: never a base, so never a map
        r.set_camera(cam)
        r.set_scene(scene)
        r.set_shard(1, 2, 4)
        r.edit_scene_mapped(edit, origin)
        r.render_guides()
        assert lib.rtiow_read_scene_origin(r._h, None, len(M.kept_slots(edit))) == E_STATE
        assert lib.rtiow_read_scene_motion(r._h, None, None, None, r.local_rows * W) == E_STATE
