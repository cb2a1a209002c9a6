"""The preview chain on volume scenes on the GPU (-m gpu): rtiow_accumulate_volume, rtiow_accumulate_adaptive_volume,
rtiow_accumulate_budget_volume, rtiow_render_guides_volume and rtiow_render_coverage_volume against their twins, bit for bit, on scenes
that fill a volume (tests/volume_scene.py: beyond a compute unit's LDS the twin reads them through the exact loop over every sphere, the
_volume call through the three-axis grid of rtiow_render_volume), against the CPU oracle, with the camera inside and below the cloud and
looking up a column, on the frame's edges and a shard, with their refusals, and with every existing path left alone.  In the manner of
tests/test_large_preview.py.  What the scenes are is checked without a GPU in tests/test_volume_grid_plan.py."""
import contextlib

import numpy as np
import pytest

from tests import preview_drive, volume_scene
from tests.test_gpu_parity import _same_bits

pytestmark = pytest.mark.gpu
BADARG, STATE = -1, -2
W, H, B, SEED = 48, 32, 8, 1227
CALLS = {                                                    # method -> (C call, twin method, twin's C call)
    "accumulate_volume": ("rtiow_accumulate_volume", "accumulate", "rtiow_accumulate"),
    "accumulate_adaptive_volume": ("rtiow_accumulate_adaptive_volume", "accumulate_adaptive", "rtiow_accumulate_adaptive"),
    "accumulate_budget_volume": ("rtiow_accumulate_budget_volume", "accumulate_budget", "rtiow_accumulate_budget"),
    "render_guides_volume": ("rtiow_render_guides_volume", "render_guides", "rtiow_render_guides"),
    "render_coverage_volume": ("rtiow_render_coverage_volume", "render_coverage", "rtiow_render_coverage"),
}
ARGS = {"accumulate_volume": (2,), "accumulate_adaptive_volume": (2, 0.0), "accumulate_budget_volume": (2,), "render_guides_volume": (),
        "render_coverage_volume": (2,)}


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _open(stack, rt, prec, scene, w=W, h=H, shard=None, debug=False, cam=None, S=1):
    r = stack.enter_context(rt.Renderer(0, prec, debug=debug))
    r.set_camera(cam if cam is not None else rt.camera(prec, w, h, S, B)); r.set_scene(scene)
    if shard:
        r.set_shard(*shard)
    r.init_rng(SEED)
    return r


def _pair(stack, rt, prec, scene, **kw):
    """(the handle of the _volume calls, the handle of the twins), set up alike."""
    return _open(stack, rt, prec, scene, **kw), _open(stack, rt, prec, scene, **kw)


def _sources(rt, volume, twin=None):
    """The twin read the scene through the exact loop -- it really is beyond the LDS -- and the _volume call through the volume grid."""
    if twin is not None:
        assert twin.stats()["scene_source"] == rt.SCENE_SCALAR
    st, grid = volume.stats(), volume.volume_grid()
    assert st["scene_source"] == rt.SCENE_VOLUME_GRID
    assert (st["grid_nx"], st["grid_nz"], st["grid_registered"], st["grid_direct"]) == (grid["nx"], grid["nz"], grid["registered"], grid["direct"])
    assert st["grid_cell"] == grid["cell"] and grid["usable"] and grid["ny"] > 1


def _same_tuple(a, b):
    return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))


def _refusal(r, method, *args):
    with pytest.raises(Exception) as e:
        getattr(r, method)(*args)
    return e.value.code, str(e.value)


# ---- 1. chunks are the one-shot render

@pytest.mark.parametrize("side,prec", [(18, 32), (18, 64), (27, 32)])
def test_chunks_are_the_one_shot_render(rt, oracle, side, prec):
    sc = volume_scene.cube(side, prec)
    with contextlib.ExitStack() as stack:
        volume, twin = _pair(stack, rt, prec, sc)
        shot = _open(stack, rt, prec, sc)
        total = 0
        for chunk in (1, 2, 3):
            assert volume.accumulate_volume(chunk) > 0
            twin.accumulate(chunk)
            total += chunk
            _sources(rt, volume, twin)
            assert volume.accumulated_samples == total
            cam = rt.camera(prec, W, H, total, B)
            want, _ = oracle.render(prec, sc, cam, SEED)
            got = volume.read_framebuffer()
            assert _same_bits(got, want), (side, prec, total)
            shot.set_camera(cam); shot.init_rng(SEED)
            shot.render_volume()
            assert _same_bits(got, shot.read_framebuffer()), (side, prec, total)
            assert _same_bits(volume.read_linear(), twin.read_linear()), (side, prec, total)
        assert float(np.asarray(got, np.float64).std()) > 0.01            # a picture, not a constant


# ---- 2. interchangeable

@pytest.mark.parametrize("prec", [32, 64])
def test_volume_plain_and_large_chunks_interchange(rt, prec):
    """The chunk costs are the segments of the LAST chunk, so they are compared with a handle that ran the same chunks through
    rtiow_accumulate alone; image, linear image and total also with a handle that ran one chunk of six."""
    sc = volume_scene.cube(18, prec)
    with contextlib.ExitStack() as stack:
        mixed, plain = _pair(stack, rt, prec, sc, debug=True)
        once = _open(stack, rt, prec, sc)
        mixed.accumulate_volume(2)
        assert mixed.stats()["scene_source"] == rt.SCENE_VOLUME_GRID
        mixed.accumulate(1)
        assert mixed.stats()["scene_source"] == rt.SCENE_SCALAR
        mixed.accumulate_large(3)
        assert mixed.stats()["scene_source"] == rt.SCENE_DEVICE_GRID
        for chunk in (2, 1, 3):
            plain.accumulate(chunk)
        once.accumulate(6)
        for other in (plain, once):
            assert _same_bits(mixed.read_framebuffer(), other.read_framebuffer()), prec
            assert _same_bits(mixed.read_linear(), other.read_linear()), prec
            assert mixed.accumulated_samples == other.accumulated_samples == 6
        costs = mixed.debug_read_chunk_costs()
        assert np.array_equal(costs, plain.debug_read_chunk_costs()) and costs.min() >= 3
        # ... and the other way round: the device grid first, a plain chunk, the volume grid behind them
        mixed.reset_accumulation(); mixed.init_rng(SEED)
        mixed.accumulate_large(3); mixed.accumulate(1); mixed.accumulate_volume(2)
        _sources(rt, mixed)
        assert _same_bits(mixed.read_framebuffer(), once.read_framebuffer()), prec
        assert _same_bits(mixed.read_linear(), once.read_linear()) and mixed.accumulated_samples == 6
        plain.reset_accumulation(); plain.init_rng(SEED)
        for chunk in (3, 1, 2):
            plain.accumulate(chunk)
        assert np.array_equal(mixed.debug_read_chunk_costs(), plain.debug_read_chunk_costs())


# ---- 3. adaptive

@pytest.mark.parametrize("prec", [32, 64])
def test_adaptive_chunks(rt, prec):
    """Three chunks of 2 samples with min_samples = 2; rel_error by the rule of tests/test_adaptive.py (preview_drive.run_mixed): the
    frame's median error after the first chunk, so that some pixels are carried and some sampled."""
    sc = volume_scene.cube(18, prec)
    npix = W * H
    with contextlib.ExitStack() as stack:
        volume, twin = _pair(stack, rt, prec, sc)
        thr, mixed = 0.0, 0
        for chunk in range(3):
            _, active_v = volume.accumulate_adaptive_volume(2, thr, min_samples=2)
            _, active_t = twin.accumulate_adaptive(2, thr, min_samples=2)
            _sources(rt, volume, twin)
            assert active_v == active_t, (prec, chunk, active_v, active_t)
            assert _same_tuple(volume.adaptive_state(), twin.adaptive_state()), (prec, chunk)
            assert _same_bits(volume.read_framebuffer(), twin.read_framebuffer()), (prec, chunk)
            assert _same_bits(volume.variance(), twin.variance()), (prec, chunk)
            if chunk == 0:
                assert active_t == npix
                thr = float(np.median(twin.adaptive_state()[1]))
            else:
                mixed += 0 < active_t < npix
        assert mixed >= 1                                             # at the second or third chunk some are carried, some sampled
        assert len(np.unique(twin.adaptive_state()[0])) >= 2


# ---- 4. budget

@pytest.mark.parametrize("prec", [32, 64])
def test_budget_chunks_from_the_same_plan(rt, prec):
    sc = volume_scene.cube(18, prec)
    cams = preview_drive.budget_moves(rt, prec, W, H, B)              # the dolly brings a border without history into view
    params = preview_drive.history_defaults(rt)
    with contextlib.ExitStack() as stack:
        volume, twin = _pair(stack, rt, prec, sc, cam=cams["home"])
        code_t, text_t = _refusal(twin, "accumulate_budget", 2)       # no plan yet
        code_v, text_v = _refusal(volume, "accumulate_budget_volume", 2)
        assert code_v == code_t == STATE and "rtiow_accumulate_budget_volume" in text_v
        assert text_v.replace("rtiow_accumulate_budget_volume", "rtiow_accumulate_budget") == text_t
        volume.accumulate_adaptive_volume(4, 0.0, min_samples=4); volume.render_guides_volume()
        twin.accumulate_adaptive(4, 0.0, min_samples=4); twin.render_guides()
        assert volume.history_update(*params) == twin.history_update(*params)
        volume.history_commit(); twin.history_commit()
        preview_drive.move(volume, cams["dolly"]); preview_drive.move(twin, cams["dolly"])
        volume.render_guides_volume()
        assert volume.history_plan(*params) == twin.history_plan(*params)
        plan = twin.history_plan_lengths()
        assert _same_bits(volume.history_plan_lengths(), plan) and 0 < (plan > 0).mean() < 1
        seen = []
        for chunk in range(3):
            _, active_v = volume.accumulate_budget_volume(2, 6.0, 1)
            _, active_t = twin.accumulate_budget(2, 6.0, 1)
            _sources(rt, volume, twin)
            seen.append(active_t)
            assert active_v == active_t, (prec, chunk)
            assert _same_bits(volume.adaptive_state()[0], twin.adaptive_state()[0]), (prec, chunk)
            assert _same_bits(volume.read_framebuffer(), twin.read_framebuffer()), (prec, chunk)
        assert seen[0] == W * H and 0 < seen[-1] < W * H, seen        # the plan does decide: some pixels are done, some are not


# ---- 5. guides

def _moved(scene, dx=0.3):
    """The nine gridded spheres nearest a point in front of the camera, moved along x (sphere 0 is the ground)."""
    out = {k: np.array(v) for k, v in scene.items()}
    near = 1 + np.argsort(np.linalg.norm(scene["center_radius"][1:, :3] - np.array([6.5, 1.0, 1.5]), axis=1))[:9]
    out["center_radius"][near, 0] += dx
    return out


def _compare_guides(rt, volume, twin, where):
    seen = {}
    for mode in (rt.GUIDES_FIRST_HIT, rt.GUIDES_SPECULAR):
        for lens in (0, 2):
            for r in (volume, twin):
                r.set_guide_mode(mode); r.set_guide_lens(lens)
            volume.render_guides_volume(); twin.render_guides()
            _sources(rt, volume)
            assert _same_tuple(volume.guides(), twin.guides()), (where, mode, lens)
            assert _same_tuple(volume.filter_guides(), twin.filter_guides()), (where, mode, lens)
            seen[mode, lens] = twin.filter_guides()[0]
    for r in (volume, twin):
        r.set_guide_mode(rt.GUIDES_FIRST_HIT); r.set_guide_lens(0)
    return seen


@pytest.mark.parametrize("prec", [32, 64])
def test_guides_on_the_cube(rt, prec):
    sc = volume_scene.cube(18, prec)
    params = preview_drive.history_defaults(rt)
    with contextlib.ExitStack() as stack:
        volume, twin = _pair(stack, rt, prec, sc)
        volume.accumulate_volume(2); twin.accumulate(2)
        _sources(rt, volume, twin)
        seen = _compare_guides(rt, volume, twin, prec)
        first = seen[rt.GUIDES_FIRST_HIT, 0]
        assert not _same_bits(seen[rt.GUIDES_FIRST_HIT, 2], first)      # the lens lattice is in effect at this camera
        assert np.abs(twin.guides()[2]).max() > 0                       # depths of hits, not a frame of sky
        # the filter reads what the _volume call left as it reads what the twin leaves
        volume.render_guides_volume(); twin.render_guides()
        assert _same_bits(volume.denoise(), twin.denoise()), prec
        # a committed base and an edit that moves nine spheres: the motion plane and the influence plane
        assert volume.history_update(*params) == twin.history_update(*params)
        volume.history_commit(); twin.history_commit()
        edit = _moved(sc)
        for r in (volume, twin):
            r.set_edit_influence(1.0); r.edit_scene(edit)
        volume.render_guides_volume(); twin.render_guides()
        _sources(rt, volume)
        assert volume.volume_grid()["registered"] == 18 ** 3            # the edit rebuilt the grid
        assert _same_tuple(volume.guides(), twin.guides()), prec
        motion = twin.scene_motion()
        assert _same_tuple(volume.scene_motion(), motion), prec
        lam = twin.edit_influence()
        assert _same_bits(volume.edit_influence(), lam), prec
        assert (motion[2] >= 0).any() and np.isfinite(lam).all()


@pytest.mark.parametrize("name", ["cube_no_ground", "with_bad"])
def test_guides_on_the_edge_scenes(rt, name):
    """cube_no_ground(14): sky pixels and an empty direct list; with_bad: spheres the plan cannot grid and the slow-division
    instantiation of the walk (never a picture: the guides alone)."""
    for prec in (32, 64):
        sc = volume_scene.cube_no_ground(14, prec) if name == "cube_no_ground" else volume_scene.with_bad(prec)
        assert volume_scene.scene_in_range(sc) == (name != "with_bad")
        with contextlib.ExitStack() as stack:
            volume, twin = _pair(stack, rt, prec, sc)
            _compare_guides(rt, volume, twin, (name, prec))
            depth = twin.guides()[2]
            assert (depth > 0).any()
            if name == "cube_no_ground":
                assert (depth == 0).any() and volume.volume_grid()["direct"] == 0


def _camera(rt, prec, where):
    """test_render_volume.py's cameras inside the cloud and below it, and one below the column looking up it."""
    if where == "centre":
        return rt.camera_look(prec, W, H, 1, B, lookfrom=(0.1, 7.2, 0.2), lookat=(5.0, 9.0, 3.0), vfov=60.0, defocus_angle=0.3, focus_dist=3.0)
    if where == "column":
        return rt.camera_look(prec, W, H, 1, B, lookfrom=(0.02, -3.0, 0.03), lookat=(0.0, 60.0, 0.0), vup=(1.0, 0.0, 0.0), vfov=20.0, defocus_angle=0.2, focus_dist=4.0)
    return rt.camera_look(prec, W, H, 1, B, lookfrom=(0.3, -0.5, 0.1), lookat=(0.5, 7.0, 0.4), vup=(1.0, 0.0, 0.0), vfov=50.0, defocus_angle=0.2, focus_dist=4.0)


@pytest.mark.parametrize("where", ["centre", "below_no_ground", "column"])
def test_guides_from_inside_below_and_along_the_column(rt, where):
    for prec in (32, 64):
        sc = {"centre": volume_scene.cube, "below_no_ground": volume_scene.cube_no_ground}[where](14, prec) if where != "column" else volume_scene.column(prec)
        with contextlib.ExitStack() as stack:
            volume, twin = _pair(stack, rt, prec, sc, cam=_camera(rt, prec, where))
            _compare_guides(rt, volume, twin, (where, prec))
            assert (twin.guides()[2] > 0).any(), (where, prec)
            if where == "column":
                assert volume.volume_grid()["ny"] > 128
            volume.accumulate_volume(2); twin.accumulate(2)
            assert _same_bits(volume.read_framebuffer(), twin.read_framebuffer()), (where, prec)


# ---- 6. coverage

@pytest.mark.parametrize("prec", [32, 64])
def test_coverage_layers_and_the_resolve_on_top(rt, prec):
    sc = volume_scene.cube(18, prec)
    with contextlib.ExitStack() as stack:
        volume, twin = _pair(stack, rt, prec, sc)
        volume.accumulate_volume(2); twin.accumulate(2)
        volume.render_guides_volume(); twin.render_guides()
        for grid in (2, 4):
            volume.denoise(); twin.denoise()
            volume.render_coverage_volume(grid); twin.render_coverage(grid)
            _sources(rt, volume)
            cov = twin.coverage()
            assert _same_tuple(volume.coverage(), cov), (prec, grid)
            assert (cov[0][..., 1] >= -1).any()                          # pixels that two spheres (or a sphere and the sky) share
            assert volume.resolve_edges() == twin.resolve_edges() > 0, (prec, grid)
            assert _same_bits(volume.read_denoised(), twin.read_denoised()), (prec, grid)


# ---- 8. frame edges and shards

@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (65, 9)])
def test_frame_sizes(rt, w, h):
    for prec in (32, 64):
        sc = volume_scene.cube(18, prec)
        with contextlib.ExitStack() as stack:
            volume, twin = _pair(stack, rt, prec, sc, w=w, h=h)
            for chunk in (1, 2):
                volume.accumulate_volume(chunk); twin.accumulate(chunk)
                assert _same_bits(volume.read_framebuffer(), twin.read_framebuffer()), (w, h, prec, chunk)
            _sources(rt, volume, twin)
            assert _same_bits(volume.read_linear(), twin.read_linear()), (w, h, prec)
            volume.render_guides_volume(); twin.render_guides()
            assert _same_tuple(volume.guides(), twin.guides()), (w, h, prec)


def test_shard_equals_the_rows_of_the_whole_frame(rt):
    sc = volume_scene.cube(18, 32)
    rows = rt.shard_rows(40, 1, 3, 8)
    with contextlib.ExitStack() as stack:
        full = _open(stack, rt, 32, sc, h=40)
        part = _open(stack, rt, 32, sc, h=40, shard=(1, 3, 8))
        for r in (full, part):
            r.accumulate_volume(2); r.accumulate_volume(1); r.render_guides_volume()
            _sources(rt, r)
        assert part.local_rows == len(rows) == 16
        assert _same_bits(part.read_framebuffer(), np.ascontiguousarray(full.read_framebuffer()[rows]))
        assert all(_same_bits(p, np.ascontiguousarray(f[rows])) for p, f in zip(part.guides(), full.guides()))


def test_a_rank_without_rows(rt):
    """set_shard(2, 3, 8) on a 48 x 8 frame: every call returns as its twin does and leaves the same state."""
    sc = volume_scene.cube(18, 32)
    with contextlib.ExitStack() as stack:
        volume, twin = _pair(stack, rt, 32, sc, h=8, shard=(2, 3, 8))
        assert volume.local_rows == twin.local_rows == 0
        assert volume.accumulate_volume(2) == twin.accumulate(2) == 0
        assert volume.accumulated_samples == twin.accumulated_samples == 2
        assert volume.render_guides_volume() == twin.render_guides() == 0
        assert volume.render_coverage_volume(2) == twin.render_coverage(2) == 0
        assert _same_tuple(volume.guides(), twin.guides()) and volume.guides()[0].shape[0] == 0
        code_v, text_v = _refusal(volume, "accumulate_adaptive_volume", 2, 0.0)     # a plain chunk is pending: the twin's refusal
        code_t, text_t = _refusal(twin, "accumulate_adaptive", 2, 0.0)
        assert code_v == code_t and text_v.replace("rtiow_accumulate_adaptive_volume", "rtiow_accumulate_adaptive") == text_t
        for r in (volume, twin):
            r.reset_accumulation()
        assert volume.accumulate_adaptive_volume(2, 0.0) == twin.accumulate_adaptive(2, 0.0) == (0, 0)
        assert volume.accumulated_samples == twin.accumulated_samples
        assert _same_tuple(volume.adaptive_state(), twin.adaptive_state())
        code_v, text_v = _refusal(volume, "accumulate_budget_volume", 2)
        code_t, text_t = _refusal(twin, "accumulate_budget", 2)
        assert code_v == code_t and text_v.replace("rtiow_accumulate_budget_volume", "rtiow_accumulate_budget") == text_t


# ---- 9. refusals

def test_refusals(rt):
    lib = rt.load_hip_library()
    with contextlib.ExitStack() as stack:
        volume, twin = stack.enter_context(rt.Renderer(0, 32)), stack.enter_context(rt.Renderer(0, 32))
        # before rtiow_set_scene / rtiow_set_camera / rtiow_init_rng: the twin's code and the twin's text under the new name
        def same_refusals(methods, where):
            for method in methods:
                call, twin_method, twin_call = CALLS[method]
                code_v, text_v = _refusal(volume, method, *ARGS[method])
                code_t, text_t = _refusal(twin, twin_method, *ARGS[method])
                assert code_v == code_t and call in text_v, (where, method, text_v)
                assert text_v.replace(call, twin_call) == text_t, (where, method)
        same_refusals(CALLS, "nothing set")
        for r in (volume, twin):
            r.set_camera(rt.camera(32, W, H, 1, B))
        same_refusals(CALLS, "a camera, no scene")
        for r in (volume, twin):
            r.set_scene(volume_scene.cube(14, 32))
        same_refusals(("accumulate_volume", "accumulate_adaptive_volume", "accumulate_budget_volume"), "no RNG states")
    with contextlib.ExitStack() as stack:
        r = _open(stack, rt, 32, volume_scene.ten_spheres())
        r.accumulate_adaptive(2, 0.0, min_samples=2); r.render_guides(); r.history_update(); r.history_commit()
        r.reset_accumulation(); r.init_rng(SEED); r.history_plan()     # a plan, so that the budget call gets as far as the scene
        for method, (call, twin_method, twin_call) in CALLS.items():
            code, text = _refusal(r, method, *ARGS[method])
            assert code == BADARG and text.count(call) == 1 and text.endswith("use " + twin_call), (method, text)
            assert "the volume grid does not suit this scene" in text
        assert not r.volume_grid()["usable"]
        assert r.accumulate_budget(2)[1] >= 0 and r.render_guides() > 0 and r.render_coverage(2) > 0     # ... and the twins do render them
        r.reset_accumulation(); r.init_rng(SEED)
        assert r.accumulate(2) > 0
    with contextlib.ExitStack() as stack:                             # a plain chunk after an adaptive one, and the reverse
        sc = volume_scene.cube(14, 32)
        volume, twin = _pair(stack, rt, 32, sc)
        volume.accumulate_adaptive_volume(2, 0.0); twin.accumulate_adaptive(2, 0.0)
        code_v, text_v = _refusal(volume, "accumulate_volume", 1)
        code_t, text_t = _refusal(twin, "accumulate", 1)
        assert code_v == code_t == STATE and text_v.replace("rtiow_accumulate_volume", "rtiow_accumulate") == text_t
        for r in (volume, twin):
            r.reset_accumulation(); r.init_rng(SEED)
        volume.accumulate_volume(2); twin.accumulate(2)
        code_v, text_v = _refusal(volume, "accumulate_adaptive_volume", 1, 0.0)
        code_t, text_t = _refusal(twin, "accumulate_adaptive", 1, 0.0)
        assert code_v == code_t == STATE and text_v.replace("rtiow_accumulate_adaptive_volume", "rtiow_accumulate_adaptive") == text_t
        assert _same_bits(volume.read_framebuffer(), twin.read_framebuffer())     # a refused call changed nothing
        assert lib.rtiow_accumulate_volume(volume._h, 0, None) == BADARG           # the twin's argument check under the new name
        assert "rtiow_accumulate_volume: samples must be > 0" in lib.rtiow_last_error_string(volume._h).decode()


# ---- 10. existing paths are left alone

def test_existing_paths_are_left_alone(rt):
    sc = volume_scene.cube(18, 32)
    S = 3
    with contextlib.ExitStack() as stack:
        fresh = _open(stack, rt, 32, sc, S=S)
        fresh.render(0)
        want_render = fresh.read_framebuffer()
        fresh.init_rng(SEED); fresh.accumulate(2)
        want_chunk = fresh.read_framebuffer()
        fresh.render_guides()
        want_guides = fresh.guides()
        fresh.denoise()
        want_count = fresh.upscale(2)
        want_upscaled = fresh.read_upscaled()

        r = _open(stack, rt, 32, sc, S=S)
        r.accumulate_volume(1); r.accumulate_volume(2); r.render_guides_volume(); r.render_coverage_volume(2)
        r.denoise(); r.upscale_volume(2); r.upscale_wide_volume(3)
        r.reset_accumulation(); r.init_rng(SEED)
        r.accumulate_adaptive_volume(2, 0.0)
        _sources(rt, r)
        r.init_rng(SEED); r.render(0)
        assert r.stats()["scene_source"] == rt.SCENE_SCALAR and _same_bits(r.read_framebuffer(), want_render)
        r.init_rng(SEED); r.render_large()
        assert r.stats()["scene_source"] == rt.SCENE_DEVICE_GRID and _same_bits(r.read_framebuffer(), want_render)
        r.init_rng(SEED); r.render_volume()
        assert r.stats()["scene_source"] == rt.SCENE_VOLUME_GRID and _same_bits(r.read_framebuffer(), want_render)
        r.reset_accumulation(); r.init_rng(SEED); r.accumulate_large(2)
        assert r.stats()["scene_source"] == rt.SCENE_DEVICE_GRID and _same_bits(r.read_framebuffer(), want_chunk)
        r.reset_accumulation(); r.init_rng(SEED); r.accumulate(2)
        assert r.stats()["scene_source"] == rt.SCENE_SCALAR and _same_bits(r.read_framebuffer(), want_chunk)
        r.set_camera(rt.camera(32, W, H, S, B)); r.init_rng(SEED)       # stale guides: rendered by rtiow_render_guides
        r.accumulate(2)
        r.render_guides()
        assert r.stats()["scene_source"] == rt.SCENE_SCALAR and _same_tuple(r.guides(), want_guides)
        r.denoise()
        assert r.upscale(2) == want_count and _same_bits(r.read_upscaled(), want_upscaled)
        assert r.stats()["scene_source"] == rt.SCENE_SCALAR
        with pytest.raises(rt.RtiowError) as e:                         # still no source a handle can be set to
            r.set_scene_source(rt.SCENE_VOLUME_GRID)
        assert e.value.code == BADARG
        # a second set_scene rebuilds the blob while chunks are pending (nothing waited for): the chunks after it see the new scene
        moved = _moved(sc, dx=0.45)
        r.reset_accumulation(); r.init_rng(SEED)
        r.accumulate_volume(2, sync=False); r.accumulate_volume(1, sync=False)
        r.set_scene(moved); r.init_rng(SEED)
        r.accumulate_volume(2)
        got = r.read_framebuffer()
        fresh.set_scene(moved); fresh.init_rng(SEED); fresh.accumulate(2)
        assert _same_bits(got, fresh.read_framebuffer()) and not _same_bits(got, want_chunk)
