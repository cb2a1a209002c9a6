"""The device grid's walk (rtiow_render_large; device/hit_device_grid.h) on the GPU (-m gpu) in the structural regimes that the lattice
and the line of tests/test_render_large.py do not reach: long lists of odd and even lengths with exact duplicates, an empty direct list,
a direct list that is no multiple of four and holds spheres the plan cannot grid, the faces of the y-slab, coarse coordinates -- ray by
ray against the exact loop and the oracle's loop, in family order and shuffled across waves -- then scenes beyond the LDS against the
oracle's loop alone, and the scene state around the call: after rtiow_edit_scene_mapped, with valid == 0 holes, twice from one init_rng.
Scenes: tests/large_scene.py; ray families: tests/large_rays.py; what these tests assume of either is shown without a GPU, for the
oracle alone, in tests/test_large_grid_plan.py."""
import numpy as np
import pytest

from tests import large_rays, large_scene
from tests.conftest import compact
from tests.test_gpu_parity import _same_bits

pytestmark = pytest.mark.gpu

PLAN_KEYS = ("nx", "nz", "cell", "registered", "direct", "index_entries", "longest_list")


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _differ(t, t_ref, index, index_ref):
    """Indices of the rays whose root bits or sphere index differ."""
    return np.nonzero((index != index_ref) | (t.view(np.uint8).reshape(len(t), -1) != t_ref.view(np.uint8).reshape(len(t), -1)).any(axis=1))[0]


def _unpermuted(v, perm):
    """The result of large_rays.shuffled's rays, back in the rays' own order."""
    out = np.empty_like(v)
    out[perm] = v
    return out


def _same_plan(pl, grid):
    """The hook's plan (around large_scene.centre: the centroid rounded to fp32) is the handle's (rounded to the handle's type): were it
    not, the ray families would be built on other cell edges than the kernel walks."""
    assert grid["usable"] and pl["usable"]
    assert {k: pl[k] for k in PLAN_KEYS} == {k: grid[k] for k in PLAN_KEYS}, (pl, grid)


def _every_seventh_against_the_oracle(oracle, prec, sc, rays, t_ref, i_ref):
    pick = np.arange(0, len(rays), 7)
    t_o, i_o = oracle.hit_world(prec, sc["center_radius"], rays[pick])
    bad = _differ(t_o, t_ref[pick], i_o, i_ref[pick])
    assert len(bad) == 0, (len(bad), rays[pick][bad[:5]], t_o[bad[:5]], t_ref[pick][bad[:5]], i_o[bad[:5]], i_ref[pick][bad[:5]])


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("name", large_scene.EDGE_SCENES)
def test_edge_scenes_ray_by_ray(rt, oracle, name, prec):
    """debug_hit_world_large against debug_hit_world of the same handle under RTIOW_SCENE_LDS_EXACT, root bits and index, on
    _adversarial_rays stacked with large_rays.edge_rays (20 000 rays a family, 185 128 in all); every seventh ray against the oracle's
    loop as well.  The rays within rfar's reach again in a call of their own: there no wave may take the exact loop."""
    sc, cr, pl, rays, where = large_rays.edge_case(rt, name, prec)
    near = rays[large_rays.within_reach(rays, where, cr, pl)]
    with rt.Renderer(0, prec, debug=True) as r:
        r.set_camera(rt.camera(prec, 64, 64, 1, 1)); r.set_scene(sc); r.set_scene_source(rt.SCENE_LDS_EXACT)
        t_ref, i_ref = r.debug_hit_world(rays)
        assert r.stats()["scene_source"] == rt.SCENE_LDS_EXACT
        t, i, cells = r.debug_hit_world_large(rays)
        tn_ref, in_ref = r.debug_hit_world(near)
        tn, inn, cells_near = r.debug_hit_world_large(near)
        grid = r.large_grid()
    _same_plan(pl, grid)
    bad = _differ(t, t_ref, i, i_ref)
    assert len(bad) == 0, large_rays.describe(bad, rays, t, t_ref, i, i_ref, cells, pl)
    bad = _differ(tn, tn_ref, inn, in_ref)
    assert len(bad) == 0, large_rays.describe(bad, near, tn, tn_ref, inn, in_ref, cells_near, pl)
    _every_seventh_against_the_oracle(oracle, prec, sc, rays, t_ref, i_ref)
    # ---- what keeps the comparison from passing empty
    assert len(near) > 0.8 * 8 * large_rays.N_EACH
    assert (cells_near >= 0).all(), int((cells_near < 0).sum())      # no wave took the exact loop
    assert cells_near.max() > 1 and (cells == -1).any()              # walks of several cells; the far and degenerate families do fall back
    large_rays.assert_floors(name, sc, pl, rays, where, i_ref)
    large_rays.assert_floors(name, sc, pl, rays, where, i)
    if name == "equal_no_ground":
        assert grid["direct"] == 0
    if name == "sparse_wide":
        assert cells[where["long_walk"]].max() >= 20, int(cells[where["long_walk"]].max())


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("name", ["clusters", "mixed_with_bad"])
def test_a_rays_result_does_not_depend_on_its_wave(rt, name, prec):
    """Four choices of hit_world_device_grid are made per wave by ballot (rho, the exact loop, fd.on, the pair loop of a cell's list);
    the probe hands lane k of wave w ray 64 w + k.  The same rays in family order, where almost every wave is of one family, and under a
    random permutation, where every wave is a mixture: (root bits, index) per ray must not change, and must be the exact loop's.  Under
    the permutation nearly every wave holds a far or degenerate ray and takes the exact loop (cells == -1: tests/test_large_grid_plan.py
    derives the floor of 1 000 from the kernel's text), so the rays within rfar's reach are shuffled again among themselves: there every
    wave walks, with lanes of lists of every length, lanes that are done, and squared lengths inside and outside fd's range."""
    sc, cr, pl, rays, where = large_rays.edge_case(rt, name, prec)
    mixed, perm = large_rays.shuffled(rays, np.random.default_rng(99))
    walked = large_rays.within_reach(rays, where, cr, pl)
    near_mixed, near_perm = large_rays.shuffled(rays[walked], np.random.default_rng(98))
    with rt.Renderer(0, prec, debug=True) as r:
        r.set_camera(rt.camera(prec, 64, 64, 1, 1)); r.set_scene(sc); r.set_scene_source(rt.SCENE_LDS_EXACT)
        t_ref, i_ref = r.debug_hit_world(rays)
        t, i, cells = r.debug_hit_world_large(rays)
        t_m, i_m, cells_m = r.debug_hit_world_large(mixed)
        t_n, i_n, cells_n = r.debug_hit_world_large(near_mixed)
        _same_plan(pl, r.large_grid())
    t_m, i_m, cells_m = (_unpermuted(v, perm) for v in (t_m, i_m, cells_m))
    bad = _differ(t, t_ref, i, i_ref)
    assert len(bad) == 0, large_rays.describe(bad, rays, t, t_ref, i, i_ref, cells, pl)
    bad = _differ(t_m, t, i_m, i)
    assert len(bad) == 0, large_rays.describe(bad, rays, t_m, t, i_m, i, cells_m, pl)
    t_n, i_n, cells_n = (_unpermuted(v, near_perm) for v in (t_n, i_n, cells_n))
    bad = _differ(t_n, t[walked], i_n, i[walked])
    assert len(bad) == 0, large_rays.describe(bad, rays[walked], t_n, t[walked], i_n, i[walked], cells_n, pl)
    # ---- the waves really mixed
    dragged = (cells >= 0) & (cells_m == -1)                          # near rays dragged through the exact loop by a far wave-mate
    assert dragged.sum() >= 1000, int(dragged.sum())
    assert (dragged | ~large_rays.dragged_along(rays, walked, perm)).all()                        # ... at least those the kernel's text names
    assert (cells_n >= 0).all() and (cells_n > 1).sum() >= 1000      # and among themselves every wave walked
    assert (i_n >= 0).mean() > 0.1 and (i_n < 0).mean() > 0.05


N_EACH_BEYOND = 4000       # 37 128 rays: the oracle's loop takes 1.8 s over the 20 004 spheres in fp32, 1.0 s over the 6 004 in fp64 (one core)


@pytest.mark.parametrize("n,prec", [(20000, 32), (6000, 64)])
def test_beyond_the_lds_ray_by_ray(rt, oracle, n, prec):
    """The scenes whose tables outgrow the LDS, where the exact loop's hook refuses: the oracle's loop on the CPU is the only reference.
    Root bits and index on every ray of all the families; within rfar's reach every wave walks."""
    sc = large_scene.lattice(n, prec)
    cr = np.asarray(sc["center_radius"], np.float64)
    pl = rt.debug_large_grid_plan(cr, large_scene.centre(sc), tables=True)
    rays, where = large_rays.stacked_rays(cr, pl, prec, N_EACH_BEYOND, 11 + prec)
    near = rays[large_rays.within_reach(rays, where, cr, pl)]
    with rt.Renderer(0, prec, debug=True) as r:
        r.set_camera(rt.camera(prec, 64, 64, 1, 1)); r.set_scene(sc)
        t, i, cells = r.debug_hit_world_large(rays)
        tn, inn, cells_near = r.debug_hit_world_large(near)
        _same_plan(pl, r.large_grid())
        r.init_rng(1227); r.render(0)
        assert r.stats()["scene_source"] == rt.SCENE_SCALAR           # beyond the LDS indeed
    t_o, i_o = oracle.hit_world(prec, sc["center_radius"], rays)
    bad = _differ(t, t_o, i, i_o)
    assert len(bad) == 0, large_rays.describe(bad, rays, t, t_o, i, i_o, cells, pl)
    picked = large_rays.within_reach(rays, where, cr, pl)
    bad = _differ(tn, t_o[picked], inn, i_o[picked])
    assert len(bad) == 0, large_rays.describe(bad, near, tn, t_o[picked], inn, i_o[picked], cells_near, pl)
    assert len(near) > 0.8 * 8 * N_EACH_BEYOND and (cells_near >= 0).all(), int((cells_near < 0).sum())
    assert (i_o >= 0).mean() >= 0.10 and (i_o < 0).mean() >= 0.05 and cells_near.max() > 8 and (cells == -1).any()
    assert (i_o[where["lists"]] >= 4).mean() >= 0.30                  # the long lists' family finds gridded spheres


# ---- scene state around the call: bit comparisons on small frames
W, H, S, B = 48, 32, 2, 8


def _render_large(rt, prec, scene, cam):
    with rt.Renderer(0, prec) as r:
        r.set_camera(cam); r.set_scene(scene); r.init_rng(1227)
        r.render_large()
        return r.read_framebuffer()


def _rows(scene, rows):
    return {k: np.ascontiguousarray(v[rows]) for k, v in scene.items()}


def test_after_edit_scene_mapped_across_the_lds_limit(rt, oracle):
    """INTEGRATION.md section 24's own case: a scene that rtiow_edit_scene_mapped grows past the LDS limit, then shrinks from the middle
    of its table.  After each edit render_large is a fresh handle's on the same scene and the oracle's image, and the grid was rebuilt."""
    full = large_scene.lattice(6000, 32)                              # 6 004 slots: the ground, three unit spheres, the lattice
    m = len(full["type"])
    start = _rows(full, np.arange(4504))
    cut = np.r_[0:2750, 3250:m]                                       # 500 lattice spheres leave the middle of the table
    cam = rt.camera(32, W, H, S, B)
    with rt.Renderer(0, 32) as r:
        r.set_camera(cam); r.set_scene(start); r.init_rng(1227)
        r.render(0)
        assert r.stats()["scene_source"] not in (rt.SCENE_SCALAR, rt.SCENE_DEVICE_GRID) and r.stats()["num_spheres"] == 4504      # inside the LDS
        before = r.large_grid()
        assert before["usable"] and before["registered"] == 4500
        origin = np.where(np.arange(m) < 4504, np.arange(m), -1)
        r.edit_scene_mapped(full, origin)
        r.init_rng(1227)
        r.render_large()
        grown, st, grid = r.read_framebuffer(), r.stats(), r.large_grid()
        assert st["scene_source"] == rt.SCENE_DEVICE_GRID and st["num_spheres"] == m and grid["registered"] == before["registered"] + 1500
        r.init_rng(1227); r.render(0)
        assert r.stats()["scene_source"] == rt.SCENE_SCALAR           # ... and past the LDS
        r.edit_scene_mapped(_rows(full, cut), cut)
        r.init_rng(1227)
        r.render_large()
        shrunk, st, grid2 = r.read_framebuffer(), r.stats(), r.large_grid()
        assert st["scene_source"] == rt.SCENE_DEVICE_GRID and st["num_spheres"] == m - 500 and grid2["registered"] == grid["registered"] - 500
    for got, scene in ((grown, full), (shrunk, _rows(full, cut))):
        assert _same_bits(got, _render_large(rt, 32, scene, cam))
        want, _ = oracle.render(32, scene, cam, 1227)
        assert _same_bits(got, want)
    assert not _same_bits(grown, shrunk)


def test_holes_at_set_scene(rt, oracle):
    """valid == 0 slots: the device grid indexes the kept spheres, compacted, and so does the shading that follows a hit."""
    sc = {k: np.array(v) for k, v in large_scene.lattice(6000, 32).items()}
    sc["valid"][4::7] = 0                                             # every 7th of the small spheres
    kept = int(sc["valid"].sum())
    assert kept == 6004 - 858
    cam = rt.camera(32, W, H, S, B)
    with rt.Renderer(0, 32) as r:
        r.set_camera(cam); r.set_scene(sc); r.init_rng(1227)
        r.render_large()
        got, st, grid = r.read_framebuffer(), r.stats(), r.large_grid()
    assert st["scene_source"] == rt.SCENE_DEVICE_GRID and st["num_spheres"] == kept and grid["registered"] == kept - 4
    want, _ = oracle.render(32, compact(sc), cam, 1227)
    assert _same_bits(got, want)
    assert not _same_bits(got, _render_large(rt, 32, large_scene.lattice(6000, 32), cam))      # the holes show


def test_rng_states_in_and_out(rt):
    """render_large takes the RNG states as render() takes them and leaves them as render() leaves them: a second frame without init_rng
    is the second frame of two render(0) calls after the same init_rng on another handle, and a render(0) behind the two is that
    handle's.  rtiow_render reads the states of rtiow_init_rng and does not advance them (include/rtiow.h: a repeated render is the same
    image bit for bit), so both second frames are the first again -- measured on an MI355X, for render(0) as for render_large -- and
    what shows that the states are read at all is the other seed."""
    sc = large_scene.lattice(6000, 32)
    cam = rt.camera(32, W, H, S, B)
    with rt.Renderer(0, 32) as r:
        r.set_camera(cam); r.set_scene(sc); r.init_rng(1227)
        r.render_large(); first = r.read_framebuffer()
        r.render_large(); second = r.read_framebuffer()
        assert r.stats()["scene_source"] == rt.SCENE_DEVICE_GRID
        r.render(0); third = r.read_framebuffer()
        r.init_rng(7)
        r.render_large(); other_seed = r.read_framebuffer()
    with rt.Renderer(0, 32) as r:
        r.set_camera(cam); r.set_scene(sc); r.init_rng(1227)
        r.render(0); plain_first = r.read_framebuffer()
        r.render(0); plain_second = r.read_framebuffer()
        r.render(0); plain_third = r.read_framebuffer()
    assert _same_bits(first, plain_first) and _same_bits(second, plain_second) and _same_bits(third, plain_third)
    assert not _same_bits(other_seed, first)
