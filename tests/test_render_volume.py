"""rtiow_render_volume on the GPU (-m gpu): the render through the three-axis grid walked in device memory is rtiow_render's image bit for
bit -- against the CPU oracle on cubes beyond a compute unit's LDS, against the exact loop ray by ray on the families of
tests/volume_rays.py, with the camera inside and below the cloud, on a shard -- and leaves every existing path alone.  What these tests
assume of their scenes and rays is checked without a GPU in tests/test_volume_grid_plan.py."""
import numpy as np
import pytest

from tests import volume_rays, volume_scene
from tests.test_gpu_parity import _same_bits

pytestmark = pytest.mark.gpu
BADARG, STATE = -1, -2
UNSUITED = "rtiow_render_volume: the volume grid does not suit this scene (too few spheres, or too many too big for a cell); use rtiow_render"
PLAN_KEYS = ("nx", "ny", "nz", "registered", "direct", "index_entries", "occupied_cells", "longest_list")


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _differ(t, t_ref, index, index_ref):
    """Indices of the rays whose root bits or sphere index differ."""
    return np.nonzero((index != index_ref) | (t.view(np.uint8).reshape(len(t), -1) != t_ref.view(np.uint8).reshape(len(t), -1)).any(axis=1))[0]


def _describe(bad, rays, t, t_ref, index, index_ref, cells):
    return "%d rays differ; first: %s" % (len(bad), [(int(k), rays[k].tolist(), t[k], int(index[k]), int(cells[k]), t_ref[k], int(index_ref[k])) for k in bad[:5]])


@pytest.mark.parametrize("side,prec", [(18, 32), (18, 64), (27, 32)])
def test_oracle_parity_beyond_the_lds(rt, oracle, side, prec):
    sc = volume_scene.cube(side, prec)
    W, H, S, B = 48, 32, 2, 8
    cam = rt.camera(prec, W, H, S, B)
    with rt.Renderer(0, prec) as r:
        r.set_camera(cam); r.set_scene(sc); r.init_rng(1227)
        r.render(0)
        assert r.stats()["scene_source"] == rt.SCENE_SCALAR          # the scene really is too large for the LDS
        plain = r.read_framebuffer()
        r.init_rng(1227)
        assert r.render_volume() > 0
        st, grid, got = r.stats(), r.volume_grid(), r.read_framebuffer()
        r.init_rng(1227)
        r.render_large()
        large = r.read_framebuffer()
    assert st["scene_source"] == rt.SCENE_VOLUME_GRID and st["schedule"] == rt.SCHED_PERSISTENT and st["num_spheres"] == side ** 3 + 1
    assert grid["usable"] and grid["registered"] == side ** 3 and grid["direct"] == 1, grid
    assert (st["grid_nx"], st["grid_nz"], st["grid_registered"], st["grid_direct"]) == (grid["nx"], grid["nz"], grid["registered"], grid["direct"])
    assert st["grid_cell"] == grid["cell"] and st["scene_prepare_ms"] > 0
    pl = rt.debug_volume_grid_plan(np.asarray(sc["center_radius"], np.float64), volume_scene.centre(sc))
    assert {k: pl[k] for k in PLAN_KEYS} == {k: grid[k] for k in PLAN_KEYS}, (pl, grid)
    want, _ = oracle.render(prec, sc, cam, 1227)
    assert _same_bits(got, want), (side, prec)
    assert _same_bits(plain, want), (side, prec)
    assert _same_bits(large, want), (side, prec)
    assert float(np.asarray(got, np.float64).std()) > 0.01            # a picture, not a constant


@pytest.mark.parametrize("name,prec", [("cube14", 32), ("cube14", 64), ("with_bad", 32), ("with_bad", 64), ("column", 32)])
def test_ray_by_ray(rt, oracle, name, prec):
    """debug_hit_world_volume against debug_hit_world of the same handle under RTIOW_SCENE_LDS_EXACT (the reference's 12-operation test on
    every sphere), root bits and index, on the families of tests/volume_rays.py (20 000 rays each): once in family order and once
    shuffled; every seventh ray against the oracle's loop as well.  The walked families within rfar's reach again in a call of their own:
    there no wave may take the exact loop."""
    sc, cr, pl, rays, where = volume_rays.case(rt, name, prec)
    assert volume_scene.fits_lds(sc, prec)
    walked = volume_rays.within_reach(rays, where, cr, pl)
    near = rays[walked]
    mixed, perm = volume_rays.shuffled(rays, np.random.default_rng(99))
    with rt.Renderer(0, prec, debug=True) as r:
        r.set_camera(rt.camera(prec, 64, 64, 1, 1)); r.set_scene(sc); r.set_scene_source(rt.SCENE_LDS_EXACT)
        t_ref, i_ref = r.debug_hit_world(rays)
        assert r.stats()["scene_source"] == rt.SCENE_LDS_EXACT         # the tables still fit the LDS
        t, i, cells = r.debug_hit_world_volume(rays)
        t_m, i_m, cells_m = r.debug_hit_world_volume(mixed)
        t_n, i_n, cells_n = r.debug_hit_world_volume(near)
        grid = r.volume_grid()
    assert grid["usable"] and {k: pl[k] for k in PLAN_KEYS} == {k: grid[k] for k in PLAN_KEYS}, (pl, grid)     # the rays were built on the cells the kernel walks
    bad = _differ(t, t_ref, i, i_ref)
    assert len(bad) == 0, _describe(bad, rays, t, t_ref, i, i_ref, cells)
    bad = _differ(t_m, t_ref[perm], i_m, i_ref[perm])
    assert len(bad) == 0, _describe(bad, mixed, t_m, t_ref[perm], i_m, i_ref[perm], cells_m)
    bad = _differ(t_n, t_ref[walked], i_n, i_ref[walked])
    assert len(bad) == 0, _describe(bad, near, t_n, t_ref[walked], i_n, i_ref[walked], cells_n)
    pick = np.arange(0, len(rays), 7)
    t_o, i_o = oracle.hit_world(prec, sc["center_radius"], rays[pick])
    bad = _differ(t_o, t_ref[pick], i_o, i_ref[pick])
    assert len(bad) == 0, _describe(bad, rays[pick], t_o, t_ref[pick], i_o, i_ref[pick], cells[pick])
    # ---- what keeps the comparison from passing empty
    assert len(near) > 0.95 * 7 * volume_rays.N_EACH
    assert (cells_n >= 0).all(), int((cells_n < 0).sum())            # within rfar's reach no wave took the exact loop
    assert cells_n.max() > 1 and (cells[where["far"]] == -1).any()    # walks of several cells; the far and degenerate family does fall back
    assert (cells_m == -1).sum() > (cells == -1).sum()                # shuffled, the far rays drag their wave-mates along
    gridded = (i_ref >= 0) & ~np.isin(i_ref, pl["direct_list"])
    assert gridded[walked].mean() > 0.25
    for fam in volume_rays.WALKED:
        assert 0.20 <= float((i_ref[where[fam]] >= 0).mean()) <= 0.95, fam
    # with_bad alone is outside the range that allows FastDiv (range_flags bit 1, by handle.h's rule restated in volume_scene): its walks divide
    assert volume_scene.scene_in_range(sc) == (name != "with_bad")
    if name == "column":
        vertical = cells[where["vertical"]]
        assert pl["ny"] > 128 and vertical.max() > 128, int(vertical.max())          # a walk longer than any of the LDS grid


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("where", ["centre", "below", "below_no_ground"])
def test_camera_inside_the_cloud_and_below_it(rt, where, prec):
    """From y = -0.5 the camera of cube(14) sits inside the ground sphere: every path starts on the direct list's side of the walk and most
    end black inside the ground (the fp64 image is all zeros), so the same view is rendered again over cube_no_ground(14), where it sees
    the cloud from below."""
    sc = volume_scene.cube_no_ground(14, prec) if where == "below_no_ground" else volume_scene.cube(14, prec)
    W, H, S, B = 32, 24, 2, 6
    if where == "centre":
        cam = rt.camera_look(prec, W, H, S, B, lookfrom=(0.1, 7.2, 0.2), lookat=(5.0, 9.0, 3.0), vfov=60.0, defocus_angle=0.3, focus_dist=3.0)
    else:                                                             # looking up into the cloud
        cam = rt.camera_look(prec, W, H, S, B, lookfrom=(0.3, -0.5, 0.1), lookat=(0.5, 7.0, 0.4), vup=(1.0, 0.0, 0.0), vfov=50.0, defocus_angle=0.2, focus_dist=4.0)
    with rt.Renderer(0, prec) as r:
        r.set_camera(cam); r.set_scene(sc); r.set_scene_source(rt.SCENE_LDS_EXACT); r.set_schedule(rt.SCHED_STATIC)
        r.init_rng(1227)
        r.render(0)
        assert r.stats()["scene_source"] == rt.SCENE_LDS_EXACT
        want = r.read_framebuffer()
        r.init_rng(1227)
        r.render_volume()
        assert r.stats()["scene_source"] == rt.SCENE_VOLUME_GRID
        got = r.read_framebuffer()
    assert _same_bits(got, want), (where, prec)
    if where != "below":
        assert float(np.asarray(got, np.float64).std()) > 0.01


def test_shard_equals_the_rows_of_the_whole_frame(rt):
    sc = volume_scene.cube(18, 32)
    W, H, S, B = 48, 40, 2, 8
    def volume(shard=None):
        with rt.Renderer(0, 32) as r:
            r.set_camera(rt.camera(32, W, H, S, B)); r.set_scene(sc)
            if shard:
                r.set_shard(*shard)
            r.init_rng(1227)
            assert r.render_volume() > 0
            return r.read_framebuffer(), r.stats()
    full, _ = volume()
    part, st = volume((1, 3, 8))
    rows = rt.shard_rows(H, 1, 3, 8)
    assert len(rows) == 16 and st["local_rows"] == 16
    assert _same_bits(part, np.ascontiguousarray(full[rows]))


def test_existing_paths_are_left_alone(rt):
    sc = volume_scene.cube(14, 32)
    W, H, S, B = 64, 48, 3, 10
    cam = rt.camera(32, W, H, S, B)
    with rt.Renderer(0, 32) as r:
        r.set_camera(cam); r.set_scene(sc); r.init_rng(1227)
        r.render(0)
        fresh, st_fresh = r.read_framebuffer(), r.stats()
    with rt.Renderer(0, 32) as r:
        r.set_camera(cam); r.set_scene(sc); r.init_rng(1227)
        r.render_volume()
        volume = r.read_framebuffer()
        assert r.stats()["scene_source"] == rt.SCENE_VOLUME_GRID
        r.init_rng(1227)
        r.render_large()
        large = r.read_framebuffer()
        assert r.stats()["scene_source"] == rt.SCENE_DEVICE_GRID and r.large_grid()["usable"] and r.volume_grid()["usable"]      # both grids on one handle
        r.init_rng(1227)
        r.render(0)
        assert r.stats()["scene_source"] == st_fresh["scene_source"]
        plain = r.read_framebuffer()
        with pytest.raises(rt.RtiowError) as e:
            r.set_scene_source(rt.SCENE_VOLUME_GRID)
        assert e.value.code == BADARG
        # a scene edit rebuilds the grid: the moved sphere is found where it is now
        moved = {k: np.array(v) for k, v in sc.items()}
        k = 1 + int(np.argmin(np.linalg.norm(sc["center_radius"][1:, :3] - np.array([6.5, 1.0, 1.5]), axis=1)))   # a gridded sphere in front of the camera
        moved["center_radius"][k, 1] += 0.3
        r.edit_scene(moved)
        r.init_rng(1227)
        r.render_volume()
        after = r.read_framebuffer()
        assert r.volume_grid()["registered"] == 14 ** 3
    assert _same_bits(volume, fresh) and _same_bits(large, fresh) and _same_bits(plain, fresh)
    with rt.Renderer(0, 32) as r:
        r.set_camera(cam); r.set_scene(moved); r.init_rng(1227)
        r.render(0)
        want = r.read_framebuffer()
    assert _same_bits(after, want) and not _same_bits(after, fresh)


def test_refusals(rt):
    lib = rt.load_hip_library()
    with rt.Renderer(0, 32) as r:
        def refused(code=BADARG):
            assert lib.rtiow_render_volume(r._h, None) == code
            text = lib.rtiow_last_error_string(r._h).decode()
            assert "rtiow_render_volume" in text, text
            return text
        refused()                                                     # no scene, no camera
        r.set_scene(volume_scene.cube(14, 32))
        refused()                                                     # no camera
        r.set_camera(rt.camera(32, 32, 32, 1, 2))
        refused(STATE)                                                # before rtiow_init_rng
        r.set_scene(volume_scene.ten_spheres())
        r.init_rng(1227)
        assert refused() == UNSUITED                                  # the plan does not suit ten spheres: said so, no silent fall-back
        assert not r.volume_grid()["usable"]
        r.render(0)                                                   # ... and rtiow_render does render them
        r.set_scene(volume_scene.cube(14, 32))
        r.init_rng(1227)
        assert r.render_volume() > 0
    with rt.Renderer(0, 32) as r:
        r.set_camera(rt.camera(32, 32, 32, 1, 2))
        assert lib.rtiow_render_volume(r._h, None) == BADARG           # a camera, no scene
        assert "rtiow_render_volume" in lib.rtiow_last_error_string(r._h).decode()
    assert lib.rtiow_render_volume(None, None) == -1                  # a NULL handle
