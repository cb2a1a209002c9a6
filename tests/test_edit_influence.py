"""Edit influence (rtiow_set_edit_influence, rtiow_read_edit_influence) on the GPU: the influence plane, the
faded motion plane, the plan, the temporal colour and length and the counters, every pixel BIT FOR BIT against tests/edit_influence_model.py,
on 40x24 (edge tiles in both tilings), 65x9 and 1x1, scenes 1 and 3, in both precisions: 4 bounces, one sample per chunk, a base committed
from one earlier frame.  That base has M = 1 at every pixel, so a pixel that carries gathers m = 1 exactly and the plan's m = 1 * fade
shows the bits of the motion plane's fourth component."""
import os
import re

import numpy as np
import pytest

from tests import edit_influence_model as E
from tests import scene_motion_model as M
from tests.conftest import ROOT
from tests.preview_drive import E_BADARG, E_STATE, INF, as_base, check_update, history_defaults, orbit, state
from tests.preview_model import budget_rule, same_bits
from tests.preview_model import clipped_np as plain_clipped_np, plan_np as plain_plan_np, update_np as plain_update_np

pytestmark = pytest.mark.gpu

FRAMES = [(40, 24), (65, 9), (1, 1)]
CASES = [(s, W, H) for s in (1, 3) for W, H in FRAMES]
KAPPAS = (0.5, INF)
CLIP = (1, 0.75)
B = 4


def chunk_of_the_header():
    text = open(os.path.join(ROOT, "raytracingincuda_amd", "csrc", "library", "edit_list.h")).read()
    return int(re.search(r"constexpr int EDIT_LIST_CHUNK = (\d+);", text).group(1))


def ground(scene):
    r = np.asarray(scene["center_radius"], np.float64).reshape(-1, 4)[:, 3]
    return [int(s) for s in M.kept_slots(scene) if r[s] >= 100]


def seen_most(oracle, prec, scene, cam, slots):
    tb = M.tables(scene, prec)
    _, _, _, k = M.first_hit(oracle, prec, tb, cam, range(cam.img_height))
    kept = list(M.kept_slots(scene))
    return sorted(slots, key=lambda s: -int((k == kept.index(s)).sum()))


def edits(oracle, prec, scene_id, scene, cam):
    """name -> edited scene: (a) nothing, (b) one small sphere moved, (c) the ground recoloured, (d) on scene 1, 44 spheres moved: 88
    entries, more than two chunks of the kernel's staging."""
    small = M.small_spheres(scene)
    out = {"nothing": M.edited(scene), "one": M.translate(scene, seen_most(oracle, prec, scene, cam, small)[:1], (0.25, 0.0, 0.125)),
           "ground": M.recolour(scene, ground(scene)[:1])}
    if scene_id == 1:
        out["many"] = M.translate(scene, small[:44], (0.0625, 0.0, -0.03125))
    return out


class Frame:
    """A handle with a base committed under `scene` at `cam` from one frame of one sample, and the model's base beside it."""

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
        self.snap = M.tables(scene, prec)

    def close(self):
        self.r.close()

    def model(self, oracle, scene, cam, kappa):
        """The model's planes of `scene` at `cam` against the snapshot."""
        cur_t = M.tables(scene, self.prec)
        O, D, t, k = M.first_hit(oracle, self.prec, cur_t, cam, range(cam.img_height))
        Q, carry, ids = M.plane_np(O, D, t, k, cur_t, self.snap)
        normal, depth = M.guides_of(O, D, t, k, cur_t)
        entries, owners = E.edit_list(cur_t, self.snap)
        lam, fade, s = E.influence_np(cam, depth, carry, ids, entries, owners, kappa)
        return {"Q": Q, "carry": carry, "ids": ids, "N": normal, "t": depth, "entries": entries, "owners": owners, "lam": lam, "fade": fade, "s": s}

    def check_planes(self, want, where):
        """The influence plane, and the motion plane as the public read shows it, of the handle as it stands."""
        r = self.r
        lam = r.edit_influence()
        assert same_bits(lam, want["lam"]), where
        gq, gc, gi = r.scene_motion()
        assert np.array_equal(gi, want["ids"]) and same_bits(gq, want["Q"]), where
        assert np.array_equal(gc, (want["fade"] != 0).astype(np.int32)), where
        normal, _, depth = r.guides()
        assert same_bits(depth, want["t"]) and same_bits(normal, want["N"]), where

    def check_chain(self, want, cam, where):
        """Plan, one sample, update and clipped update through the faded plane against the model; returns the model's."""
        r, params = self.r, self.params
        Q, fade = want["Q"], want["fade"]
        planned = r.history_plan(*params)
        want_m, want_count = E.plan_np(cam, want["N"], want["t"], self.base, params, Q, fade)
        got_m = r.history_plan_lengths()
        assert same_bits(got_m, want_m) and planned == want_count, (where, planned, want_count)
        # the base holds M = 1: where the unfaded gather carries m = 1, the plan is the plane's fourth component itself
        plain_m, _ = M.plan_np(cam, want["N"], want["t"], self.base, params, Q, want["carry"])
        one = plain_m == 1
        assert same_bits(np.ascontiguousarray(got_m[one]), np.ascontiguousarray(fade[one])), where
        r.accumulate(1)
        cur = state(r, False)
        count = r.history_update(*params)
        rgb, length = r.history()
        wc, wm, wcount = E.update_np(cam, cur, self.base, params, Q, fade)
        assert same_bits(length, wm) and same_bits(rgb, wc) and count == wcount, (where, count, wcount)
        assert same_bits(length, want_m + cur["n"].astype(want_m.dtype)), where          # the plan predicted Mout - n
        count, clipped = r.history_update_clipped(*CLIP, *params)
        rgb, length = r.history()
        wcl = E.clipped_np(cam, cur, self.base, params, *CLIP, Q, fade)
        assert same_bits(length, wcl["M"]) and same_bits(rgb, wcl["C"]), where
        assert (count, clipped) == (wcl["reprojected"], wcl["clipped"]), (where, count, clipped)
        assert (wcl["m"][fade == 0] == 0).all(), where                                   # a fully faded pixel carries nothing
        return {"cur": cur, "plan": want_m, "C": wc, "M": wm, "clipped_C": wcl["C"], "clipped_M": wcl["M"], "counts": (wcount, wcl["reprojected"], wcl["clipped"])}

    def edit(self, scene, cam, seed=1300):
        self.r.edit_scene(scene)
        self.r.set_camera(cam)
        self.r.init_rng(seed)


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id,W,H", CASES, ids=["%s-%dx%d" % c for c in CASES])
def test_planes_and_chain_against_the_model(native, oracle, prec, scene_id, W, H):
    rt = native
    scene = rt.build_scene(scene_id, prec)
    cam = rt.camera(prec, W, H, 1, B)
    for name, edit in edits(oracle, prec, scene_id, scene, cam).items():
        for source in (3, 0, 1, 2):
            f = Frame(rt, prec, scene, cam, source=source)
            try:
                f.edit(edit, cam)
                for kappa in KAPPAS:
                    where = (scene_id, W, H, name, source, kappa)
                    f.r.set_edit_influence(kappa)
                    want = f.model(oracle, edit, cam, kappa)
                    f.check_planes(want, where)
                    hit = want["t"] != 0
                    if name == "nothing":
                        assert len(want["owners"]) == 0 and (want["lam"] == 0).all(), where
                    if name == "one":
                        assert len(want["owners"]) == 2, where
                    if name == "ground":                         # every hit pixel but the ground's own sees the ground
                        own = want["ids"] == want["owners"][0]
                        assert len(want["owners"]) == 1 and (want["lam"][hit & ~own] > 0).all() and (want["lam"][own | ~hit] == 0).all(), where
                        assert (want["carry"][own] == 0).all() and (want["fade"][own] == 0).all(), where
                    if name == "many":                           # the list crosses the kernel's chunk, twice
                        assert len(want["owners"]) >= 80 and len(want["owners"]) > 2 * chunk_of_the_header(), where
                        assert (want["lam"][hit] > 0).any() or W * H == 1, where
                    if kappa == INF:
                        assert np.array_equal(want["lam"], ((want["s"] > 0) * 1).astype(want["lam"].dtype)), where
                    if source != 3:
                        continue
                    got = f.check_chain(want, cam, where)
                    if name == "nothing":                        # an empty list: the kappa == 0 call and the plain call, bit for bit
                        plain = plain_clipped_np(cam, got["cur"], f.base, f.params, *CLIP)
                        assert same_bits(plain["C"], got["clipped_C"]) and same_bits(plain["M"], got["clipped_M"]), where
                        pc, pm, pcount = plain_update_np(cam, got["cur"], f.base, *f.params)
                        assert same_bits(pc, got["C"]) and same_bits(pm, got["M"]) and pcount == got["counts"][0], where
                        assert same_bits(plain_plan_np(cam, want["N"], want["t"], f.base, f.params)[0], got["plan"]), where
                        f.r.set_edit_influence(0.0)
                        assert f.r.history_update_clipped(*CLIP, *f.params) == got["counts"][1:], where
                        rgb, length = f.r.history()
                        assert same_bits(rgb, got["clipped_C"]) and same_bits(length, got["clipped_M"]), where
                        assert f.r.history_update(*f.params) == got["counts"][0], where
                        rgb, length = f.r.history()
                        assert same_bits(rgb, got["C"]) and same_bits(length, got["M"]), where
                        f.r.history_plan(*f.params)
                        assert same_bits(f.r.history_plan_lengths(), got["plan"]), where
                    f.edit(edit, cam)                            # the next kappa starts from an empty accumulation
            finally:
                f.close()


@pytest.mark.parametrize("prec", [32, 64])
def test_kappa_back_to_zero_gives_the_kappa_zero_bits_and_a_change_renders_the_guides_again(native, oracle, prec):
    rt = native
    W, H = 40, 24
    scene = rt.build_scene(3, prec)
    cam = rt.camera(prec, W, H, 1, B)
    edit = edits(oracle, prec, 3, scene, cam)["one"]
    lib = rt.api.load_hip_library()
    n = W * H
    outs = []
    for toggle in (False, True):
        f = Frame(rt, prec, scene, cam)
        try:
            r = f.r
            f.edit(edit, cam)
            if toggle:
                r.set_edit_influence(0.5)
                r.history_plan(*f.params)
                assert (r.edit_influence() > 0).any()
                r.set_edit_influence(0.0)
                assert lib.rtiow_read_scene_motion(r._h, None, None, None, n) == E_STATE      # the faded plane went stale with the knob
            planned = r.history_plan(*f.params)
            plan = r.history_plan_lengths()
            _, carry, _ = r.scene_motion()
            r.accumulate(1)
            count = r.history_update(*f.params)
            rgb, length = r.history()
            counts = r.history_update_clipped(*CLIP, *f.params)
            crgb, clength = r.history()
            outs.append((planned, plan, carry, count, rgb, length, counts, crgb, clength))
            with pytest.raises(rt.RtiowError) as err:             # kappa == 0: no plane is made
                r.edit_influence()
            assert err.value.code == E_STATE
            # the model of section 19 alone
            want = f.model(oracle, edit, cam, 0.0)
            assert same_bits(plan, M.plan_np(cam, want["N"], want["t"], f.base, f.params, want["Q"], want["carry"])[0])
            if toggle:
                # a new kappa after the guides were rendered: guides, motion plane, plan and temporal image are stale; the same kappa: nothing is
                assert lib.rtiow_read_guides(r._h, None, None, None, n) == 0 and lib.rtiow_read_history(r._h, None, None, n) == 0
                r.set_edit_influence(0.0)
                assert lib.rtiow_read_guides(r._h, None, None, None, n) == 0 and lib.rtiow_read_history(r._h, None, None, n) == 0
                r.set_edit_influence(2.0)
                assert lib.rtiow_read_guides(r._h, None, None, None, n) == E_STATE and lib.rtiow_read_history(r._h, None, None, n) == E_STATE
                assert lib.rtiow_read_history_plan(r._h, None, n) == E_STATE and lib.rtiow_read_edit_influence(r._h, None, n) == E_STATE
                assert r.accumulated_samples == 1                                              # the accumulation is not
                r.history_update(*f.params)                                                    # renders them again, with the plane
                assert lib.rtiow_read_guides(r._h, None, None, None, n) == 0 and lib.rtiow_read_edit_influence(r._h, None, n) == 0
                want = f.model(oracle, edit, cam, 2.0)
                f.check_planes(want, "kappa 2 after the guides")
                cur = state(r, False)
                wc, wm, _ = E.update_np(cam, cur, f.base, f.params, want["Q"], want["fade"])
                rgb, length = r.history()
                assert same_bits(rgb, wc) and same_bits(length, wm)
        finally:
            f.close()
    for a, b in zip(*outs):
        assert a == b if not isinstance(a, np.ndarray) else same_bits(a, b)


@pytest.mark.parametrize("prec", [32, 64])
def test_camera_move_with_an_edit_and_two_edits_before_one_commit(native, oracle, prec):
    rt = native
    W, H = 40, 24
    scene = rt.build_scene(3, prec)
    cam = rt.camera_look(prec, W, H, 1, B)
    cam2 = rt.camera_look(prec, W, H, 1, B, lookfrom=orbit(1.5))
    small = M.small_spheres(scene)
    once = M.translate(scene, small[:6], (0.125, 0.0, -0.0625))
    twice = M.recolour(M.translate(once, small[:3], (0.125, 0.0, 0.0)), small[8:10])
    f = Frame(rt, prec, scene, cam)
    try:
        f.r.set_edit_influence(0.5)
        f.edit(once, cam2)
        want = f.model(oracle, once, cam2, 0.5)
        assert len(want["owners"]) == 12
        f.check_planes(want, "edit + camera move")
        f.check_chain(want, cam2, "edit + camera move")
        # a second edit before any commit: the list is relative to the snapshot, as the motion is
        f.edit(twice, cam2, seed=1301)
        want = f.model(oracle, twice, cam2, 0.5)
        assert len(want["owners"]) == 14
        f.check_planes(want, "two edits before one commit")
        got = f.check_chain(want, cam2, "two edits before one commit")
        # commit: a new snapshot, motion off, no plane; the next edit's list is relative to it
        f.r.history_commit()
        f.base = as_base(cam2, got["cur"], got["clipped_C"], got["clipped_M"])
        f.snap = M.tables(twice, prec)
        assert f.r._lib.rtiow_read_edit_influence(f.r._h, None, W * H) == E_STATE
        f.edit(M.translate(twice, small[:1], (0.0, 0.0, 0.25)), cam2, seed=1302)
        want = f.model(oracle, M.translate(twice, small[:1], (0.0, 0.0, 0.25)), cam2, 0.5)
        assert len(want["owners"]) == 2
        f.check_planes(want, "an edit after the second commit")
    finally:
        f.close()


@pytest.mark.parametrize("prec", [32, 64])
def test_budget_after_the_faded_plan_leaves_render_bits(native, oracle, prec):
    """rtiow_accumulate_budget by the faded plan: the counts the model's select gives, every pixel rtiow_render's bits for its own count."""
    rt = native
    W, H = 40, 24
    scene = rt.build_scene(3, prec)
    cam = rt.camera(prec, W, H, 1, B)
    edit = edits(oracle, prec, 3, scene, cam)["ground"]
    f = Frame(rt, prec, scene, cam)
    try:
        r = f.r
        r.set_edit_influence(0.5)
        r.edit_scene(edit)
        r.init_rng(1227)
        want = f.model(oracle, edit, cam, 0.5)
        r.history_plan(*f.params)
        m = r.history_plan_lengths()
        assert same_bits(m, E.plan_np(cam, want["N"], want["t"], f.base, f.params, want["Q"], want["fade"])[0])
        target, chunk = 3.0, 1
        counts = np.zeros((H, W), np.int32)
        while True:
            mask = budget_rule(counts, m, chunk, target, 0, 1 << 30)
            active = r.accumulate_budget(chunk, target, 0)[1]
            counts = counts + chunk * mask.astype(np.int32)
            assert active == int(mask.sum()) and np.array_equal(r.adaptive_state()[0], counts)
            if not active:
                break
        # m in [0, 1]: a pixel that kept its whole sample needs 2 more, a faded one 3
        assert (counts[m == 1] == 2).all() and (counts[m < 1] == 3).all() and (m == 1).any() and ((m < 1) & (m > 0)).any() and (m == 0).any()
        fb = r.read_framebuffer()
        for c in np.unique(counts[counts > 0]):
            with rt.Renderer(0, prec) as one:
                one.set_camera(rt.camera(prec, W, H, int(c), B))
                one.set_scene(edit)
                one.set_scene_source(3)
                one.init_rng(1227)
                one.render(0)
                ref = one.read_framebuffer()
            sel = counts == c
            assert same_bits(np.ascontiguousarray(fb[sel]), np.ascontiguousarray(ref[sel])), (prec, int(c))
    finally:
        f.close()


def test_refusals_and_the_plane_on_a_shard(native, oracle):
    rt, prec = native, 32
    W, H = 40, 24
    scene = rt.build_scene(3, prec)
    cam = rt.camera(prec, W, H, 1, B)
    lib = rt.api.load_hip_library()
    n = W * H
    with rt.Renderer(0, prec) as r:                              # allowed in every state: before a camera or a scene
        assert lib.rtiow_set_edit_influence(r._h, 0.5) == 0 and lib.rtiow_set_edit_influence(r._h, INF) == 0
        for bad in (float("nan"), -1.0, -INF, -1e-300):
            assert lib.rtiow_set_edit_influence(r._h, bad) == E_BADARG, bad
        with pytest.raises(rt.RtiowError) as err:
            r.set_edit_influence(-2.0)
        assert err.value.code == E_BADARG
        assert lib.rtiow_read_edit_influence(r._h, None, 0) == E_STATE
    f = Frame(rt, prec, scene, cam)
    try:
        r = f.r
        r.set_edit_influence(0.5)
        assert lib.rtiow_read_edit_influence(r._h, None, n) == E_STATE              # motion is not in effect
        r.render_guides()
        assert lib.rtiow_read_edit_influence(r._h, None, n) == E_STATE
        edit = edits(oracle, prec, 3, scene, cam)["one"]
        r.edit_scene(edit)
        assert lib.rtiow_read_edit_influence(r._h, None, n) == E_STATE              # in effect, no plane yet
        r.render_guides()
        assert lib.rtiow_read_edit_influence(r._h, None, n) == 0
        assert lib.rtiow_read_edit_influence(r._h, None, n + 1) == E_BADARG and lib.rtiow_read_edit_influence(r._h, None, n - 1) == E_BADARG
        r.set_edit_influence(0.0)
        r.render_guides()
        assert lib.rtiow_read_edit_influence(r._h, None, n) == E_STATE              # kappa == 0: no plane is made
        assert lib.rtiow_read_scene_motion(r._h, None, None, None, n) == 0
        r.set_edit_influence(0.5)
        r.set_camera(cam)
        assert lib.rtiow_read_edit_influence(r._h, None, n) == E_STATE              # stale with the guides
        r.history_reset()
        r.render_guides()
        assert lib.rtiow_read_edit_influence(r._h, None, n) == E_STATE              # no base, no motion
    finally:
        f.close()
    # a handle with a shard of one rank: the plane is made and read with global rows
    for source in (0, 3):
        f = Frame(rt, prec, scene, cam, source=source, shard=(0, 1, 4))
        try:
            f.r.set_edit_influence(0.5)
            f.edit(edits(oracle, prec, 3, scene, cam)["one"], cam)
            want = f.model(oracle, edits(oracle, prec, 3, scene, cam)["one"], cam, 0.5)
            f.check_planes(want, ("shard", source))
            f.check_chain(want, cam, ("shard", source))
        finally:
            f.close()
    with rt.Renderer(0, prec) as r:                              # several ranks: the knob is recorded, there is never a base, the updates stay refused
        r.set_camera(cam)
        r.set_scene(scene)
        r.set_shard(1, 2, 4)
        r.set_edit_influence(0.5)
        r.edit_scene(scene)
        r.render_guides()
        assert lib.rtiow_read_edit_influence(r._h, None, r.local_rows * W) == E_STATE
        r.init_rng(1227)
        r.accumulate(1)
        with pytest.raises(rt.RtiowError) as err:
            r.history_update()
        assert err.value.code == E_STATE
