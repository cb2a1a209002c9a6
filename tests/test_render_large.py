"""rtiow_render_large on the GPU (-m gpu): the render through the grid walked in device memory is rtiow_render's image bit for bit --
against the CPU oracle on scenes beyond a compute unit's LDS, against the exact loop where both apply, ray by ray on adversarial rays,
on a shard -- and leaves every existing path alone.  What these tests assume of their scenes (gridded almost whole, at most two of the
random scenes refused, a line longer than any walk of the LDS grid) is checked without a GPU in tests/test_large_grid_plan.py."""
import numpy as np
import pytest

from tests import large_scene
from tests.test_gpu_parity import _adversarial_rays, _custom, _same_bits

pytestmark = pytest.mark.gpu
BADARG = -1


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _plan(rt, scene):
    return rt.debug_large_grid_plan(np.asarray(scene["center_radius"], np.float64), large_scene.centre(scene))


def _large(rt, prec, scene, W, H, S, B, shard=None):
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, W, H, S, B)); r.set_scene(scene)
        if shard:
            r.set_shard(*shard)
        r.init_rng(1227)
        ms = r.render_large()
        assert ms > 0
        return r.read_framebuffer(), r.stats(), r.large_grid()


@pytest.mark.parametrize("n,prec", [(6000, 32), (6000, 64), (20000, 32)])
def test_oracle_parity_beyond_the_lds(rt, oracle, n, prec):
    sc = large_scene.lattice(n, prec)
    W, H, S, B = 48, 32, 2, 8
    cam = rt.camera(prec, W, H, S, B)
    with rt.Renderer(0, prec) as r:
        r.set_camera(cam); r.set_scene(sc); r.init_rng(1227)
        r.render(0)
        assert r.stats()["scene_source"] == rt.SCENE_SCALAR          # the scene really is too large for the LDS
        plain = r.read_framebuffer()
        r.init_rng(1227)
        r.render_large()
        st, grid, got = r.stats(), r.large_grid(), r.read_framebuffer()
    assert st["scene_source"] == rt.SCENE_DEVICE_GRID and st["num_spheres"] == n + 4
    assert grid["usable"] and grid["registered"] >= 0.9 * n and grid["direct"] <= 8, grid
    assert (st["grid_nx"], st["grid_nz"], st["grid_registered"], st["grid_direct"]) == (grid["nx"], grid["nz"], grid["registered"], grid["direct"])
    assert st["scene_prepare_ms"] > 0
    want, _ = oracle.render(prec, sc, cam, 1227)
    assert _same_bits(got, want), (n, prec)
    assert _same_bits(plain, want), (n, prec)
    assert float(np.asarray(got, np.float64).std()) > 0.01            # a picture, not a constant


@pytest.mark.parametrize("case", large_scene.RANDOM_CASES)
def test_same_image_as_the_existing_paths(rt, case):
    for prec in (32, 64):
        sc = large_scene.random_case(case)[prec]
        W, H, S, B = 96, 56, 4, 12
        if not _plan(rt, sc)["usable"]:
            with rt.Renderer(0, prec) as r:
                r.set_camera(rt.camera(prec, W, H, S, B)); r.set_scene(sc); r.init_rng(1227)
                with pytest.raises(rt.RtiowError) as e:
                    r.render_large()
                assert e.value.code == BADARG and "rtiow_render_large" in str(e.value) and "rtiow_render" in str(e.value)
                assert not r.large_grid()["usable"]
            continue
        got, st, grid = _large(rt, prec, sc, W, H, S, B)
        assert st["scene_source"] == rt.SCENE_DEVICE_GRID and grid["usable"]
        want, st_w = _custom(rt, prec, sc, W, H, S, B, rt.SCENE_LDS_EXACT, sched=rt.SCHED_STATIC)
        assert st_w["scene_source"] == rt.SCENE_LDS_EXACT
        assert _same_bits(got, want), (case, prec)


def _bits_differ(t, t_ref):
    return (t.view(np.uint8).reshape(len(t), -1) != t_ref.view(np.uint8).reshape(len(t), -1)).any(axis=1)


@pytest.mark.parametrize("which,prec", [("lattice", 32), ("line", 32), ("line", 64)])
def test_ray_by_ray(rt, which, prec):
    """debug_hit_world_large against debug_hit_world of the same handle with the exact loop (RTIOW_SCENE_LDS_EXACT: the reference's
    12-operation test on every sphere, which these scenes' tables still fit the LDS for -- the 6 000-sphere scene in fp32 only), on the
    adversarial families: root bits and index equal.  Families a, c and e again in a call of their own, cut to the origins within the
    registration margin's reach (rfar around the recentring point): there every wave must walk, none may take the exact loop."""
    n_each = 20000
    sc = large_scene.lattice(6000, prec) if which == "lattice" else large_scene.line(2000, prec)
    cr = np.asarray(sc["center_radius"], np.float64)
    pl = _plan(rt, sc)
    assert pl["usable"]
    if which == "line":
        assert pl["nx"] + pl["nz"] > 128                             # longer than any walk of the LDS grid
    dt = np.float32 if prec == 32 else np.float64
    rays = _adversarial_rays(np.random.default_rng(7 + prec), cr, pl, n_each)
    with np.errstate(over="ignore", invalid="ignore"):
        rays = rays.astype(dt)
    # families a, c, e: _adversarial_rays stacks a, b, c, d, e (n_each rays each), then the degenerate ones
    near = np.vstack([rays[0:n_each], rays[2 * n_each:3 * n_each], rays[4 * n_each:5 * n_each]])
    reach = 0.99 * pl["rfar"]                                         # the kernel walks for |O - ctr|^2 <= 0.999 rfar^2
    dist = np.linalg.norm(near[:, :3].astype(np.float64) - large_scene.centre(sc), axis=1)
    near = near[dist <= reach]
    assert len(near) > 0.9 * 3 * n_each                               # the cut keeps the families, it does not empty them
    with rt.Renderer(0, prec, debug=True) as r:
        r.set_camera(rt.camera(prec, 64, 64, 1, 1)); r.set_scene(sc); r.set_scene_source(rt.SCENE_LDS_EXACT)
        t_ref, i_ref = r.debug_hit_world(rays)
        assert r.stats()["scene_source"] == rt.SCENE_LDS_EXACT
        t, i, cells = r.debug_hit_world_large(rays)
        tn_ref, in_ref = r.debug_hit_world(near)
        tn, inn, cells_near = r.debug_hit_world_large(near)
    assert 0.2 < float((i_ref >= 0).mean()) < 0.95                    # the families do hit things, and do miss
    bad = np.nonzero((i != i_ref) | _bits_differ(t, t_ref))[0]
    assert len(bad) == 0, (len(bad), rays[bad[:5]], t[bad[:5]], t_ref[bad[:5]], i[bad[:5]], i_ref[bad[:5]], cells[bad[:5]])
    bad = np.nonzero((inn != in_ref) | _bits_differ(tn, tn_ref))[0]
    assert len(bad) == 0, (len(bad), near[bad[:5]], tn[bad[:5]], tn_ref[bad[:5]], inn[bad[:5]], in_ref[bad[:5]], cells_near[bad[:5]])
    assert (cells_near >= 0).all(), int((cells_near < 0).sum())      # no wave took the exact loop
    assert cells_near.max() > 1 and (cells == -1).any()              # walks of several cells; the far and degenerate families do fall back
    if which == "line":
        assert cells_near.max() > 128, int(cells_near.max())         # a walk longer than the LDS grid allows


def test_shard_equals_the_rows_of_the_whole_frame(rt):
    sc = large_scene.lattice(6000, 32)
    W, H, S, B = 48, 40, 2, 8
    full, _, _ = _large(rt, 32, sc, W, H, S, B)
    part, st, _ = _large(rt, 32, sc, W, H, S, B, shard=(1, 3, 8))
    rows = rt.shard_rows(H, 1, 3, 8)
    assert len(rows) == 16 and st["local_rows"] == 16
    assert _same_bits(part, np.ascontiguousarray(full[rows]))


def test_existing_paths_are_left_alone(rt):
    sc = large_scene.lattice(400, 32)
    W, H, S, B = 64, 48, 3, 10
    fresh, st_fresh = _custom(rt, 32, sc, W, H, S, B, rt.SCENE_GRID)
    with rt.Renderer(0, 32) as r:
        r.set_camera(rt.camera(32, W, H, S, B)); r.set_scene(sc); r.init_rng(1227)
        r.render_large()
        large = r.read_framebuffer()
        assert r.stats()["scene_source"] == rt.SCENE_DEVICE_GRID
        r.init_rng(1227)
        r.render(0)
        assert r.stats()["scene_source"] == st_fresh["scene_source"] == rt.SCENE_GRID
        assert _same_bits(r.read_framebuffer(), fresh)
        with pytest.raises(rt.RtiowError) as e:
            r.set_scene_source(rt.SCENE_DEVICE_GRID)
        assert e.value.code == BADARG
        # a scene edit rebuilds the grid: the moved sphere is found where it is now
        moved = {k: np.array(v) for k, v in sc.items()}
        k = 4 + int(np.argmin(np.linalg.norm(sc["center_radius"][4:, :3] - np.array([6.0, 0.2, 1.4]), axis=1)))   # a gridded sphere in front of the camera
        moved["center_radius"][k, 0] += 0.3
        r.edit_scene(moved)
        r.init_rng(1227)
        r.render_large()
        after = r.read_framebuffer()
    assert _same_bits(large, fresh)
    want, _ = _custom(rt, 32, moved, W, H, S, B, rt.SCENE_GRID)
    assert _same_bits(after, want) and not _same_bits(after, fresh)


def test_refusals(rt):
    lib = rt.load_hip_library()
    with rt.Renderer(0, 32) as r:
        def refused():
            assert lib.rtiow_render_large(r._h, None) == BADARG
            text = lib.rtiow_last_error_string(r._h).decode()
            assert "rtiow_render_large" in text, text
            return text
        refused()                                                     # no scene, no camera
        r.set_scene(large_scene.lattice(400, 32))
        refused()                                                     # no camera
        r.set_camera(rt.camera(32, 32, 32, 1, 2))
        r.set_scene(large_scene.ten_spheres())
        r.init_rng(1227)
        assert "use rtiow_render" in refused()                        # the plan does not suit ten spheres: said so, no silent fall-back
        assert not r.large_grid()["usable"]
        r.render(0)                                                   # ... and rtiow_render does render them
        r.set_scene(large_scene.lattice(400, 32))
        r.init_rng(1227)
        assert r.render_large() > 0
    with rt.Renderer(0, 32) as r:
        r.set_camera(rt.camera(32, 32, 32, 1, 2))
        assert lib.rtiow_render_large(r._h, None) == BADARG           # a camera, no scene
        assert "rtiow_render_large" in lib.rtiow_last_error_string(r._h).decode()
