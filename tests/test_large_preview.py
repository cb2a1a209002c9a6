"""The preview chain on large scenes on the GPU (-m gpu): rtiow_accumulate_large, rtiow_accumulate_adaptive_large,
rtiow_accumulate_budget_large, rtiow_render_guides_large and rtiow_render_coverage_large against their twins, bit for bit, on scenes beyond
a compute unit's LDS (tests/large_scene.py: the twin reads them through the exact loop over every sphere, the _large call through the
device grid of rtiow_render_large), against the CPU oracle, on the frame's edges and a shard, with their refusals, and with every existing
path left alone.  What the lattice scenes are (gridded almost whole) is checked without a GPU in tests/test_large_grid_plan.py."""
import contextlib

import numpy as np
import pytest

from tests import large_scene, preview_drive
from tests.test_gpu_parity import _same_bits

pytestmark = pytest.mark.gpu
BADARG, STATE = -1, -2
W, H, B, SEED = 48, 32, 8, 1227
CALLS = {                                                    # method -> (C call, twin method, twin's C call)
    "accumulate_large": ("rtiow_accumulate_large", "accumulate", "rtiow_accumulate"),
    "accumulate_adaptive_large": ("rtiow_accumulate_adaptive_large", "accumulate_adaptive", "rtiow_accumulate_adaptive"),
    "accumulate_budget_large": ("rtiow_accumulate_budget_large", "accumulate_budget", "rtiow_accumulate_budget"),
    "render_guides_large": ("rtiow_render_guides_large", "render_guides", "rtiow_render_guides"),
    "render_coverage_large": ("rtiow_render_coverage_large", "render_coverage", "rtiow_render_coverage"),
}
ARGS = {"accumulate_large": (2,), "accumulate_adaptive_large": (2, 0.0), "accumulate_budget_large": (2,), "render_guides_large": (),
        "render_coverage_large": (2,)}


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
    """(the handle of the _large calls, the handle of the twins), set up alike."""
    return _open(stack, rt, prec, scene, **kw), _open(stack, rt, prec, scene, **kw)


def _sources(rt, large, twin, lattice=True):
    """The twin read the scene through the exact loop -- it really is beyond the LDS -- and the _large call through the device grid."""
    if lattice:
        assert twin.stats()["scene_source"] == rt.SCENE_SCALAR
    st, grid = large.stats(), large.large_grid()
    assert st["scene_source"] == rt.SCENE_DEVICE_GRID
    assert (st["grid_nx"], st["grid_nz"], st["grid_registered"], st["grid_direct"]) == (grid["nx"], grid["nz"], grid["registered"], grid["direct"])


def _same_tuple(a, b):
    return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))


def _refusal(r, method, *args):
    with pytest.raises(Exception) as e:
        getattr(r, method)(*args)
    return e.value.code, str(e.value)


# ---- 1. chunks are the one-shot render

@pytest.mark.parametrize("n,prec", [(6000, 32), (6000, 64), (20000, 32)])
def test_chunks_are_the_one_shot_render(rt, oracle, n, prec):
    sc = large_scene.lattice(n, prec)
    with contextlib.ExitStack() as stack:
        large, twin = _pair(stack, rt, prec, sc)
        shot = _open(stack, rt, prec, sc)
        total = 0
        for chunk in (1, 2, 3):
            assert large.accumulate_large(chunk) > 0
            twin.accumulate(chunk)
            total += chunk
            _sources(rt, large, twin)
            assert large.accumulated_samples == total
            cam = rt.camera(prec, W, H, total, B)
            want, _ = oracle.render(prec, sc, cam, SEED)
            got = large.read_framebuffer()
            assert _same_bits(got, want), (n, prec, total)
            shot.set_camera(cam); shot.init_rng(SEED)
            shot.render_large()
            assert _same_bits(got, shot.read_framebuffer()), (n, prec, total)
            assert _same_bits(large.read_linear(), twin.read_linear()), (n, prec, total)
        assert float(np.asarray(got, np.float64).std()) > 0.01            # a picture, not a constant


# ---- 2. interchangeable

@pytest.mark.parametrize("prec", [32, 64])
def test_large_and_plain_chunks_interchange(rt, prec):
    """The chunk costs are the segments of the LAST chunk (on this scene in fp32: 12 148 in all after chunks of 2, 1 and 3 on either
    handle, 24 434 after one chunk of six), so they are compared with a handle that ran the same chunks through rtiow_accumulate alone;
    image, linear image and total also with a handle that ran one chunk of six."""
    sc = large_scene.lattice(6000, prec)
    with contextlib.ExitStack() as stack:
        mixed, plain = _pair(stack, rt, prec, sc, debug=True)
        once = _open(stack, rt, prec, sc)
        mixed.accumulate_large(2)
        assert mixed.stats()["scene_source"] == rt.SCENE_DEVICE_GRID
        mixed.accumulate(1)
        assert mixed.stats()["scene_source"] == rt.SCENE_SCALAR
        mixed.accumulate_large(3)
        for chunk in (2, 1, 3):
            plain.accumulate(chunk)
        once.accumulate(6)
        _sources(rt, mixed, plain)
        for other in (plain, once):
            assert _same_bits(mixed.read_framebuffer(), other.read_framebuffer()), prec
            assert _same_bits(mixed.read_linear(), other.read_linear()), prec
            assert mixed.accumulated_samples == other.accumulated_samples == 6
        costs = mixed.debug_read_chunk_costs()
        assert np.array_equal(costs, plain.debug_read_chunk_costs()) and costs.min() >= 3
        # ... and the other way round: a plain chunk first, the grid behind it
        mixed.reset_accumulation(); mixed.init_rng(SEED)
        mixed.accumulate(4); mixed.accumulate_large(2)
        assert _same_bits(mixed.read_framebuffer(), once.read_framebuffer()), prec


# ---- 3. adaptive

@pytest.mark.parametrize("prec", [32, 64])
def test_adaptive_chunks(rt, prec):
    """Three chunks of 2 samples with min_samples = 2; rel_error by the rule of tests/test_adaptive.py (preview_drive.run_mixed): the
    frame's median error after the first chunk, so that some pixels are carried and some sampled."""
    sc = large_scene.lattice(6000, prec)
    npix = W * H
    with contextlib.ExitStack() as stack:
        large, twin = _pair(stack, rt, prec, sc)
        thr, mixed = 0.0, 0
        for chunk in range(3):
            _, active_l = large.accumulate_adaptive_large(2, thr, min_samples=2)
            _, active_t = twin.accumulate_adaptive(2, thr, min_samples=2)
            _sources(rt, large, twin)
            assert active_l == active_t, (prec, chunk, active_l, active_t)
            assert _same_tuple(large.adaptive_state(), twin.adaptive_state()), (prec, chunk)
            assert _same_bits(large.read_framebuffer(), twin.read_framebuffer()), (prec, chunk)
            assert _same_bits(large.variance(), twin.variance()), (prec, chunk)
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
    sc = large_scene.lattice(6000, prec)
    cams = preview_drive.budget_moves(rt, prec, W, H, B)              # the dolly brings a border without history into view
    params = preview_drive.history_defaults(rt)
    with contextlib.ExitStack() as stack:
        large, twin = _pair(stack, rt, prec, sc, cam=cams["home"])
        code_t, text_t = _refusal(twin, "accumulate_budget", 2)       # no plan yet
        code_l, text_l = _refusal(large, "accumulate_budget_large", 2)
        assert code_l == code_t == STATE and "rtiow_accumulate_budget_large" in text_l
        assert text_l.replace("rtiow_accumulate_budget_large", "rtiow_accumulate_budget") == text_t
        large.accumulate_adaptive_large(4, 0.0, min_samples=4); large.render_guides_large()
        twin.accumulate_adaptive(4, 0.0, min_samples=4); twin.render_guides()
        assert large.history_update(*params) == twin.history_update(*params)
        large.history_commit(); twin.history_commit()
        preview_drive.move(large, cams["dolly"]); preview_drive.move(twin, cams["dolly"])
        large.render_guides_large()
        assert large.history_plan(*params) == twin.history_plan(*params)
        plan = twin.history_plan_lengths()
        assert _same_bits(large.history_plan_lengths(), plan) and 0 < (plan > 0).mean() < 1
        seen = []
        for chunk in range(3):
            _, active_l = large.accumulate_budget_large(2, 6.0, 1)
            _, active_t = twin.accumulate_budget(2, 6.0, 1)
            _sources(rt, large, twin)
            seen.append(active_t)
            assert active_l == active_t, (prec, chunk)
            assert _same_bits(large.adaptive_state()[0], twin.adaptive_state()[0]), (prec, chunk)
            assert _same_bits(large.read_framebuffer(), twin.read_framebuffer()), (prec, chunk)
        assert seen[0] == W * H and 0 < seen[-1] < W * H, seen        # the plan does decide: some pixels are done, some are not


# ---- 5. guides

def _moved(scene, dx=0.3):
    """The nine gridded spheres nearest a point in front of the camera, moved along x."""
    out = {k: np.array(v) for k, v in scene.items()}
    near = 4 + np.argsort(np.linalg.norm(scene["center_radius"][4:, :3] - np.array([6.0, 0.2, 1.4]), axis=1))[:9]
    out["center_radius"][near, 0] += dx
    return out


def _compare_guides(rt, large, twin, where):
    seen = {}
    for mode in (rt.GUIDES_FIRST_HIT, rt.GUIDES_SPECULAR):
        for lens in (0, 2):
            for r in (large, twin):
                r.set_guide_mode(mode); r.set_guide_lens(lens)
            large.render_guides_large(); twin.render_guides()
            assert large.stats()["scene_source"] == rt.SCENE_DEVICE_GRID
            assert _same_tuple(large.guides(), twin.guides()), (where, mode, lens)
            assert _same_tuple(large.filter_guides(), twin.filter_guides()), (where, mode, lens)
            seen[mode, lens] = twin.filter_guides()[0]
    for r in (large, twin):
        r.set_guide_mode(rt.GUIDES_FIRST_HIT); r.set_guide_lens(0)
    return seen


@pytest.mark.parametrize("prec", [32, 64])
def test_guides_on_the_lattice(rt, prec):
    sc = large_scene.lattice(6000, prec)
    params = preview_drive.history_defaults(rt)
    with contextlib.ExitStack() as stack:
        large, twin = _pair(stack, rt, prec, sc)
        large.accumulate_large(2); twin.accumulate(2)
        _sources(rt, large, twin)
        seen = _compare_guides(rt, large, twin, prec)
        first = seen[rt.GUIDES_FIRST_HIT, 0]
        assert not _same_bits(seen[rt.GUIDES_FIRST_HIT, 2], first)      # the lens lattice is in effect at this camera
        assert np.abs(twin.guides()[2]).max() > 0                       # depths of hits, not a frame of sky
        # the filter reads what the _large call left as it reads what the twin leaves
        large.render_guides_large(); twin.render_guides()
        assert _same_bits(large.denoise(), twin.denoise()), prec
        # a committed base and an edit that moves nine spheres: the motion plane and the influence plane
        assert large.history_update(*params) == twin.history_update(*params)
        large.history_commit(); twin.history_commit()
        edit = _moved(sc)
        for r in (large, twin):
            r.set_edit_influence(1.0); r.edit_scene(edit)
        large.render_guides_large(); twin.render_guides()
        assert large.stats()["scene_source"] == rt.SCENE_DEVICE_GRID
        assert _same_tuple(large.guides(), twin.guides()), prec
        motion = twin.scene_motion()
        assert _same_tuple(large.scene_motion(), motion), prec
        lam = twin.edit_influence()
        assert _same_bits(large.edit_influence(), lam), prec
        assert (motion[2] >= 0).any() and np.isfinite(lam).all()


@pytest.mark.parametrize("name", ["equal_no_ground", "mixed_with_bad"])
def test_guides_on_the_edge_scenes(rt, name):
    """equal_no_ground: sky pixels and an empty direct list; mixed_with_bad: spheres the plan cannot grid and the slow-division
    instantiation of the walk (never a picture: the guides alone)."""
    for prec in (32, 64):
        sc = large_scene.edge_scene(name, prec)
        with contextlib.ExitStack() as stack:
            large, twin = _pair(stack, rt, prec, sc)
            _compare_guides(rt, large, twin, (name, prec))
            depth = twin.guides()[2]
            assert (depth > 0).any()
            if name == "equal_no_ground":
                assert (depth == 0).any() and large.large_grid()["direct"] == 0


# ---- 6. coverage

@pytest.mark.parametrize("prec", [32, 64])
def test_coverage_layers_and_the_resolve_on_top(rt, prec):
    sc = large_scene.lattice(6000, prec)
    with contextlib.ExitStack() as stack:
        large, twin = _pair(stack, rt, prec, sc)
        large.accumulate_large(2); twin.accumulate(2)
        large.render_guides_large(); twin.render_guides()
        for grid in (2, 4):
            large.denoise(); twin.denoise()
            large.render_coverage_large(grid); twin.render_coverage(grid)
            assert large.stats()["scene_source"] == rt.SCENE_DEVICE_GRID
            cov = twin.coverage()
            assert _same_tuple(large.coverage(), cov), (prec, grid)
            assert (cov[0][..., 1] >= -1).any()                          # pixels that two spheres (or a sphere and the sky) share
            assert large.resolve_edges() == twin.resolve_edges() > 0, (prec, grid)
            assert _same_bits(large.read_denoised(), twin.read_denoised()), (prec, grid)


# ---- 7. frame edges

@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (65, 9)])
def test_frame_sizes(rt, w, h):
    for prec in (32, 64):
        sc = large_scene.lattice(6000, prec)
        with contextlib.ExitStack() as stack:
            large, twin = _pair(stack, rt, prec, sc, w=w, h=h)
            for chunk in (1, 2):
                large.accumulate_large(chunk); twin.accumulate(chunk)
                assert _same_bits(large.read_framebuffer(), twin.read_framebuffer()), (w, h, prec, chunk)
            _sources(rt, large, twin)
            assert _same_bits(large.read_linear(), twin.read_linear()), (w, h, prec)
            large.render_guides_large(); twin.render_guides()
            assert _same_tuple(large.guides(), twin.guides()), (w, h, prec)


def test_shard_equals_the_rows_of_the_whole_frame(rt):
    sc = large_scene.lattice(6000, 32)
    rows = rt.shard_rows(40, 1, 3, 8)
    with contextlib.ExitStack() as stack:
        full = _open(stack, rt, 32, sc, h=40)
        part = _open(stack, rt, 32, sc, h=40, shard=(1, 3, 8))
        for r in (full, part):
            r.accumulate_large(2); r.accumulate_large(1); r.render_guides_large()
            assert r.stats()["scene_source"] == rt.SCENE_DEVICE_GRID
        assert part.local_rows == len(rows) == 16
        assert _same_bits(part.read_framebuffer(), np.ascontiguousarray(full.read_framebuffer()[rows]))
        assert all(_same_bits(p, np.ascontiguousarray(f[rows])) for p, f in zip(part.guides(), full.guides()))


def test_a_rank_without_rows(rt):
    """set_shard(2, 3, 8) on a 48 x 8 frame: every call returns as its twin does and leaves the same state."""
    sc = large_scene.lattice(6000, 32)
    with contextlib.ExitStack() as stack:
        large, twin = _pair(stack, rt, 32, sc, h=8, shard=(2, 3, 8))
        assert large.local_rows == twin.local_rows == 0
        assert large.accumulate_large(2) == twin.accumulate(2) == 0
        assert large.accumulated_samples == twin.accumulated_samples == 2
        assert large.render_guides_large() == twin.render_guides() == 0
        assert large.render_coverage_large(2) == twin.render_coverage(2) == 0
        assert _same_tuple(large.guides(), twin.guides()) and large.guides()[0].shape[0] == 0
        code_l, text_l = _refusal(large, "accumulate_adaptive_large", 2, 0.0)      # a plain chunk is pending: the twin's refusal
        code_t, text_t = _refusal(twin, "accumulate_adaptive", 2, 0.0)
        assert code_l == code_t and text_l.replace("rtiow_accumulate_adaptive_large", "rtiow_accumulate_adaptive") == text_t
        for r in (large, twin):
            r.reset_accumulation()
        assert large.accumulate_adaptive_large(2, 0.0) == twin.accumulate_adaptive(2, 0.0) == (0, 0)
        assert large.accumulated_samples == twin.accumulated_samples
        assert _same_tuple(large.adaptive_state(), twin.adaptive_state())
        code_l, text_l = _refusal(large, "accumulate_budget_large", 2)
        code_t, text_t = _refusal(twin, "accumulate_budget", 2)
        assert code_l == code_t and text_l.replace("rtiow_accumulate_budget_large", "rtiow_accumulate_budget") == text_t


# ---- 8. refusals

def test_refusals(rt):
    lib = rt.load_hip_library()
    with contextlib.ExitStack() as stack:
        large, twin = stack.enter_context(rt.Renderer(0, 32)), stack.enter_context(rt.Renderer(0, 32))
        # before rtiow_set_scene / rtiow_set_camera / rtiow_init_rng: the twin's code and the twin's text under the new name
        def same_refusals(methods, where):
            for method in methods:
                call, twin_method, twin_call = CALLS[method]
                code_l, text_l = _refusal(large, method, *ARGS[method])
                code_t, text_t = _refusal(twin, twin_method, *ARGS[method])
                assert code_l == code_t and call in text_l, (where, method, text_l)
                assert text_l.replace(call, twin_call) == text_t, (where, method)
        same_refusals(CALLS, "nothing set")
        for r in (large, twin):
            r.set_camera(rt.camera(32, W, H, 1, B))
        same_refusals(CALLS, "a camera, no scene")
        for r in (large, twin):
            r.set_scene(large_scene.lattice(6000, 32))
        same_refusals(("accumulate_large", "accumulate_adaptive_large", "accumulate_budget_large"), "no RNG states")
    with contextlib.ExitStack() as stack:
        r = _open(stack, rt, 32, large_scene.ten_spheres())
        r.accumulate_adaptive(2, 0.0, min_samples=2); r.render_guides(); r.history_update(); r.history_commit()
        r.reset_accumulation(); r.init_rng(SEED); r.history_plan()     # a plan, so that the budget call gets as far as the scene
        for method, (call, twin_method, twin_call) in CALLS.items():
            code, text = _refusal(r, method, *ARGS[method])
            assert code == BADARG and text.count(call) == 1 and text.endswith("use " + twin_call), (method, text)
            assert "the device grid does not suit this scene" in text
        assert not r.large_grid()["usable"]
        assert r.accumulate_budget(2)[1] >= 0 and r.render_guides() > 0 and r.render_coverage(2) > 0     # ... and the twins do render them
        r.reset_accumulation(); r.init_rng(SEED)
        assert r.accumulate(2) > 0
    with contextlib.ExitStack() as stack:                             # a plain chunk after an adaptive one, and the reverse
        sc = large_scene.lattice(6000, 32)
        large, twin = _pair(stack, rt, 32, sc)
        large.accumulate_adaptive_large(2, 0.0); twin.accumulate_adaptive(2, 0.0)
        code_l, text_l = _refusal(large, "accumulate_large", 1)
        code_t, text_t = _refusal(twin, "accumulate", 1)
        assert code_l == code_t == STATE and text_l.replace("rtiow_accumulate_large", "rtiow_accumulate") == text_t
        for r in (large, twin):
            r.reset_accumulation(); r.init_rng(SEED)
        large.accumulate_large(2); twin.accumulate(2)
        code_l, text_l = _refusal(large, "accumulate_adaptive_large", 1, 0.0)
        code_t, text_t = _refusal(twin, "accumulate_adaptive", 1, 0.0)
        assert code_l == code_t == STATE and text_l.replace("rtiow_accumulate_adaptive_large", "rtiow_accumulate_adaptive") == text_t
        assert _same_bits(large.read_framebuffer(), twin.read_framebuffer())     # a refused call changed nothing
        assert lib.rtiow_accumulate_large(large._h, 0, None) == BADARG            # the twin's argument check under the new name
        assert "rtiow_accumulate_large: samples must be > 0" in lib.rtiow_last_error_string(large._h).decode()


# ---- 9. existing paths are left alone

def test_existing_paths_are_left_alone(rt):
    sc = large_scene.lattice(6000, 32)
    S = 3
    with contextlib.ExitStack() as stack:
        fresh = _open(stack, rt, 32, sc, S=S)
        fresh.render(0)
        want_render = fresh.read_framebuffer()
        fresh.init_rng(SEED); fresh.render_large()
        want_large = fresh.read_framebuffer()
        fresh.init_rng(SEED); fresh.accumulate(2)
        want_chunk = fresh.read_framebuffer()
        fresh.render_guides()
        want_guides = fresh.guides()
        assert _same_bits(want_render, want_large)

        r = _open(stack, rt, 32, sc, S=S)
        r.accumulate_large(1); r.accumulate_large(2); r.render_guides_large(); r.render_coverage_large(2)
        r.reset_accumulation(); r.init_rng(SEED)
        r.accumulate_adaptive_large(2, 0.0)
        assert r.stats()["scene_source"] == rt.SCENE_DEVICE_GRID
        r.init_rng(SEED); r.render(0)
        assert r.stats()["scene_source"] == rt.SCENE_SCALAR and _same_bits(r.read_framebuffer(), want_render)
        r.init_rng(SEED); r.render_large()
        assert _same_bits(r.read_framebuffer(), want_large)
        r.reset_accumulation(); r.init_rng(SEED); r.accumulate(2)
        assert r.stats()["scene_source"] == rt.SCENE_SCALAR and _same_bits(r.read_framebuffer(), want_chunk)
        r.set_camera(rt.camera(32, W, H, S, B)); r.init_rng(SEED)       # stale guides: rendered by rtiow_render_guides
        r.render_guides()
        assert _same_tuple(r.guides(), want_guides)
        # a second set_scene rebuilds the blob while chunks are pending (nothing waited for): the chunks after it see the new scene
        moved = _moved(sc, dx=0.45)
        r.accumulate_large(2, sync=False); r.accumulate_large(1, sync=False)
        r.set_scene(moved); r.init_rng(SEED)
        r.accumulate_large(2)
        got = r.read_framebuffer()
        fresh.set_scene(moved); fresh.init_rng(SEED); fresh.accumulate(2)
        assert _same_bits(got, fresh.read_framebuffer()) and not _same_bits(got, want_chunk)
