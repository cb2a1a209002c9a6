"""Scene edits that keep the history (rtiow_edit_scene, rtiow_read_scene_motion) on the GPU: the motion plane,
the temporal colour and length, the plan and the two counters, every pixel BIT FOR BIT against tests/scene_motion_model.py, over frames
below one guide tile (1x1, 7x5), across a 16x16 workgroup edge (33x17) and of several workgroups (64x40), in both precisions."""
import ctypes

import numpy as np
import pytest

from tests import scene_motion_model as M
from tests.lattice import lattice_scene
from tests.preview_drive import E_BADARG, E_STATE, as_base, check_update, history_defaults, orbit, state
from tests.preview_model import LATTICE, same_bits
from tests.preview_model import clipped_np as plain_clipped_np, plan_np as plain_plan_np, update_np as plain_update_np

pytestmark = pytest.mark.gpu

FRAMES = [(1, 1), (7, 5), (33, 17), (64, 40)]
CASES = [(s, W, H) for s in (3, LATTICE) for W, H in FRAMES] + [(1, 64, 40)]
CLIP = (1, 0.75)


def scene_of(rt, prec, scene_id):
    return lattice_scene(prec) if scene_id == LATTICE else rt.build_scene(scene_id, prec)


def busiest(oracle, prec, scene, cam, slots):
    """Of `slots`, the kept-sphere slots ordered by how many pixels of `cam` show them first (most first); unseen ones last."""
    tb = M.tables(scene, prec)
    _, _, _, k = M.first_hit(oracle, prec, tb, cam, range(cam.img_height))
    kept = list(M.kept_slots(scene))
    seen = {s: int((k == kept.index(s)).sum()) for s in slots}
    return sorted(slots, key=lambda s: -seen[s])


def edits(oracle, prec, scene, cam):
    """name -> edited scene.  The single-sphere edits take the small sphere the frame shows most of."""
    small = M.small_spheres(scene)
    top = busiest(oracle, prec, scene, cam, small)
    cr = np.asarray(scene["center_radius"], np.float64).reshape(-1, 4)
    eye = np.array(cam.center[:], np.float64)
    a, b = top[0], top[1]
    toward = eye - cr[b, :3]
    in_front = cr[b, :3] + toward / np.linalg.norm(toward) * 0.75 - cr[a, :3]
    return {
        "nothing": M.edited(scene),
        "nudge": M.translate(scene, [a], (0.03125, 0.0, 0.015625)),
        "shift": M.translate(scene, [a], (0.5, 0.0, 0.375)),
        "out": M.translate(scene, [a], (300.0, 0.0, 300.0)),
        "front": M.translate(scene, [a], in_front),
        "radius": M.scale_radius(scene, top[:4], 1.5),
        "all_small": M.translate(scene, small, (0.125, 0.0, -0.0625)),
        "material": M.recolour(scene, top[:3]),
        "big": M.translate(scene, busiest(oracle, prec, scene, cam, M.big_spheres(scene))[:1], (0.0, 0.0, 0.75)),
    }


class Frame:
    """A handle with a base committed under `scene` at `cam`, and the model's base beside it."""

    def __init__(self, rt, prec, scene, cam, source=3, shard=None):
        self.rt, self.prec, self.params = rt, prec, history_defaults(rt)
        self.r = rt.Renderer(0, prec)
        r = self.r
        r.set_camera(cam)
        r.set_scene(scene)
        r.set_scene_source(source)
        if shard:
            r.set_shard(*shard)
        r.init_rng(1227)
        r.accumulate(3)
        cur = state(r, False)
        c0, m0, _ = check_update(r, cam, cur, None, self.params, "the base frame")
        r.history_commit()
        self.base = as_base(cam, cur, c0, m0)
        self.snap = M.tables(scene, prec)

    def close(self):
        self.r.close()

    def check_edit(self, oracle, scene, cam, where, seed=1300):
        """edit_scene(scene) at `cam`: plane, plan, update and clipped update against the model.  Returns the model's planes."""
        r, prec, params = self.r, self.prec, self.params
        r.edit_scene(scene)
        r.set_camera(cam)
        r.init_rng(seed)
        cur_t = M.tables(scene, prec)
        O, D, t, k = M.first_hit(oracle, prec, cur_t, cam, range(cam.img_height))
        Q, carry, ids = M.plane_np(O, D, t, k, cur_t, self.snap)
        planned = r.history_plan(*params)
        gq, gc, gi = r.scene_motion()
        assert np.array_equal(gi, ids) and np.array_equal(gc, carry), where
        assert same_bits(gq, Q), where
        normal, _, depth = r.guides()
        wn, wd = M.guides_of(O, D, t, k, cur_t)
        assert same_bits(depth, wd) and same_bits(normal, wn), where
        want_m, want_count = M.plan_np(cam, normal, depth, self.base, params, Q, carry)
        assert same_bits(r.history_plan_lengths(), want_m) and planned == want_count, (where, planned, want_count)
        r.accumulate(3)
        cur = state(r, False)
        count = r.history_update(*params)
        rgb, length = r.history()
        wc, wm, wcount = M.update_np(cam, cur, self.base, params, Q, carry)
        assert same_bits(length, wm) and same_bits(rgb, wc) and count == wcount, (where, count, wcount)
        assert same_bits(length, want_m + cur["n"].astype(want_m.dtype)), where          # the plan predicted Mout
        count, clipped = r.history_update_clipped(*CLIP, *params)
        rgb, length = r.history()
        want = M.clipped_np(cam, cur, self.base, params, *CLIP, Q, carry)
        assert same_bits(length, want["M"]) and same_bits(rgb, want["C"]), where
        assert (count, clipped) == (want["reprojected"], want["clipped"]), (where, count, clipped)
        assert (want["m"][carry == 0] == 0).all(), where                                   # a changed surface carries nothing
        return {"Q": Q, "carry": carry, "ids": ids, "cur": cur, "m": want["m"], "C": want["C"], "M": want["M"]}


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id,W,H", CASES, ids=["%s-%dx%d" % c for c in CASES])
def test_edits_against_the_model(native, oracle, prec, scene_id, W, H):
    rt = native
    scene = scene_of(rt, prec, scene_id)
    cam = M.view(rt, prec, scene_id, W, H)
    for name, edit in edits(oracle, prec, scene, cam).items():
        f = Frame(rt, prec, scene, cam)
        try:
            got = f.check_edit(oracle, edit, cam, (scene_id, W, H, name))
            if name == "nothing":                                # the plain kernels on a twin that never edited: the same bits
                twin = Frame(rt, prec, scene, cam)
                try:
                    twin.r.set_camera(cam)
                    twin.r.init_rng(1300)
                    twin.r.accumulate(3)
                    cur = state(twin.r, False)
                    assert twin.r.history_update_clipped(*CLIP, *f.params) is not None
                    rgb, length = twin.r.history()
                    assert same_bits(rgb, got["C"]) and same_bits(length, got["M"])
                    want = plain_clipped_np(cam, cur, twin.base, f.params, *CLIP)
                    assert same_bits(want["C"], got["C"]) and same_bits(want["M"], got["M"])
                    assert twin.r._lib.rtiow_read_scene_motion(twin.r._h, None, None, None, W * H) == E_STATE
                finally:
                    twin.close()
            if name == "material":
                assert (got["carry"] == 0).any() or W * H < 64
        finally:
            f.close()


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("scene_id", [3, LATTICE])
def test_edit_with_camera_move_two_edits_and_commit(native, oracle, prec, scene_id):
    rt = native
    W, H = 64, 40
    scene = scene_of(rt, prec, scene_id)
    cam = rt.camera_look(prec, W, H, 1, 10)
    cam2 = rt.camera_look(prec, W, H, 1, 10, lookfrom=orbit(1.5))
    cam3 = rt.camera_look(prec, W, H, 1, 10, lookfrom=orbit(3.0))
    e = edits(oracle, prec, scene, cam)
    f = Frame(rt, prec, scene, cam)
    try:
        # an edit together with a camera move
        f.check_edit(oracle, e["all_small"], cam2, "edit + camera move")
        # a second edit before any commit: motion is relative to the snapshot, not to the previous edit
        twice = M.translate(e["all_small"], M.small_spheres(scene), (0.125, 0.0, 0.0))
        got = f.check_edit(oracle, twice, cam2, "two edits before one commit", seed=1301)
        assert f.r.history_base()[1].shape == (H, W) and same_bits(f.r.history_base()[1], f.base["M"])   # the base survived both edits
        # commit: a new snapshot, motion off; a camera move then runs the plain kernels again
        f.r.history_commit()
        f.base = as_base(cam2, got["cur"], got["C"], got["M"])
        f.snap = M.tables(twice, prec)
        assert f.r._lib.rtiow_read_scene_motion(f.r._h, None, None, None, W * H) == E_STATE
        f.r.set_camera(cam3)
        f.r.init_rng(1302)
        f.r.accumulate(3)
        cur = state(f.r, False)
        check_update(f.r, cam3, cur, f.base, f.params, "edit, commit, camera move: the plain path")
        planned = f.r.history_plan(*f.params)
        want_m, want_count = plain_plan_np(cam3, cur["N"], cur["t"], f.base, f.params)
        assert same_bits(f.r.history_plan_lengths(), want_m) and planned == want_count
        # ... and an edit after that commit is relative to the new snapshot
        f.check_edit(oracle, e["all_small"], cam3, "an edit after the second commit", seed=1303)
    finally:
        f.close()


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("source", [0, 1, 2, 3])
def test_plane_on_every_scene_source_and_on_a_shard(native, oracle, prec, source):
    rt = native
    W, H = 33, 17
    scene = scene_of(rt, prec, 3)
    cam = rt.camera(prec, W, H, 1, 10)
    edit = edits(oracle, prec, scene, cam)["all_small"]
    for shard in (None, (0, 1, 4)):
        f = Frame(rt, prec, scene, cam, source=source, shard=shard)
        try:
            f.check_edit(oracle, edit, cam, (source, shard))
        finally:
            f.close()


def test_refusals_and_a_refused_edit_leaves_the_handle_alone(native, oracle):
    rt, prec = native, 32
    W, H = 33, 17
    scene = scene_of(rt, prec, 3)
    cam = rt.camera(prec, W, H, 1, 10)
    lib = rt.api.load_hip_library()
    with rt.Renderer(0, prec) as r:
        r.set_camera(cam)
        with pytest.raises(rt.RtiowError) as err:               # no scene yet
            r.edit_scene(scene)
        assert err.value.code == E_STATE
    f = Frame(rt, prec, scene, cam)
    try:
        r = f.r
        n = W * H
        assert lib.rtiow_read_scene_motion(r._h, None, None, None, n) == E_STATE         # motion not in effect
        fewer = {k: v[:-1] for k, v in scene.items() if hasattr(v, "shape")}
        other = dict(scene, valid=np.where(np.arange(len(scene["valid"])) == int(M.kept_slots(scene)[3]), 0, scene["valid"]).astype(np.int32))
        for bad in (fewer, other):
            with pytest.raises(rt.RtiowError) as err:
                r.edit_scene(bad)
            assert err.value.code == E_BADARG
        assert lib.rtiow_edit_scene(r._h, len(scene["type"]), None, None, None, None, None) == E_BADARG
        assert lib.rtiow_read_scene_motion(r._h, None, None, None, n) == E_STATE         # ... and the refused edits put none in effect
        # the next update is as if the calls had not been made: the plain path against the plain model, the base intact
        r.set_camera(cam)
        r.init_rng(1300)
        r.accumulate(3)
        check_update(r, cam, state(r, False), f.base, f.params, "after refused edits")
        # an accepted edit: the read's own refusals
        r.edit_scene(edits(oracle, prec, scene, cam)["nudge"])
        assert same_bits(r.history_base()[1], f.base["M"])                                 # the base survives rtiow_edit_scene
        assert lib.rtiow_read_scene_motion(r._h, None, None, None, n) == E_STATE         # the plane is stale until guides are rendered
        r.render_guides()
        assert lib.rtiow_read_scene_motion(r._h, None, None, None, n) == 0
        assert lib.rtiow_read_scene_motion(r._h, None, None, None, n + 1) == E_BADARG
        ids = np.empty((H, W), np.int32)
        assert lib.rtiow_read_scene_motion(r._h, None, None, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n) == 0 and ids.min() >= -1
        r.set_camera(cam)
        assert lib.rtiow_read_scene_motion(r._h, None, None, None, n) == E_STATE         # stale with the guides
        r.history_reset()
        r.render_guides()
        assert lib.rtiow_read_scene_motion(r._h, None, None, None, n) == E_STATE         # no base, no motion
    finally:
        f.close()
    with rt.Renderer(0, prec) as r:                              # a handle of several ranks has no base, so never motion
        r.set_camera(cam)
        r.set_scene(scene)
        r.set_shard(1, 2, 4)
        r.edit_scene(scene)
        r.render_guides()
        assert lib.rtiow_read_scene_motion(r._h, None, None, None, r.local_rows * W) == E_STATE


@pytest.mark.parametrize("prec", [32, 64])
def test_budget_after_the_motion_plan_leaves_render_bits(native, oracle, prec):
    """rtiow_accumulate_budget by the motion plan: every pixel holds rtiow_render's bits for its own count."""
    rt = native
    W, H = 33, 17
    scene = scene_of(rt, prec, 3)
    cam = rt.camera(prec, W, H, 1, 10)
    edit = edits(oracle, prec, scene, cam)["all_small"]
    f = Frame(rt, prec, scene, cam)
    try:
        r = f.r
        r.edit_scene(edit)
        r.init_rng(1227)
        r.history_plan(*f.params)
        m = r.history_plan_lengths()
        while r.accumulate_budget(2, 5.0, 0)[1]:
            pass
        counts = r.adaptive_state()[0]
        # the base holds 3 samples a pixel: a pixel that carries them all needs 2 more, one that carries nothing 6 (chunks of 2)
        assert (counts[m == 0] == 6).all() and (counts[m == 3] == 2).all() and (m == 0).any() and (m == 3).any()
        fb = r.read_framebuffer()
        for c in np.unique(counts[counts > 0]):
            with rt.Renderer(0, prec) as one:
                one.set_camera(rt.camera(prec, W, H, int(c), 10))
                one.set_scene(edit)
                one.set_scene_source(3)
                one.init_rng(1227)
                one.render(0)
                ref = one.read_framebuffer()
            sel = counts == c
            assert same_bits(np.ascontiguousarray(fb[sel]), np.ascontiguousarray(ref[sel])), (prec, int(c))
    finally:
        f.close()
