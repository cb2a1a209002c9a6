"""The device grid's plan (csrc/library/device_grid.h) on the CPU.  tests/native/large_grid_plan_main.cpp is a stand-alone program, built
here with AddressSanitizer + UBSan and run directly: it holds plan and blob to the invariants that keep the kernel's gathers inside the
blob, on lattices of 6 000 to 100 000 spheres, lines of 2 000 and 200 000, one scene of each kind of large_scene.EDGE_SCENES and a scene
the plan refuses, and pins the reachable size of the grid.  Then the plan hook
(rtiow_debug_large_grid_plan: host arithmetic of the test build, no GPU) on the very scenes tests/test_render_large.py renders, so that
what those tests assume of their scenes is checked where no GPU is needed -- and, for tests/test_render_large_edges.py, of their rays:
every floor that file asserts of a ray family holds here for the oracle's loop alone, on the very rays."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import large_scene
from tests.conftest import ROOT


def test_large_grid_plan_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "large_grid_plan_main")
    inc = os.path.join(ROOT, "raytracingincuda_amd", "csrc", "library")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + inc, "-o", exe, os.path.join(ROOT, "tests", "native", "large_grid_plan_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    assert r.stdout.splitlines()[-1] == "0 large-grid-plan failure(s)"


def _plan(native, scene, tables=False):
    return native.debug_large_grid_plan(np.asarray(scene["center_radius"], np.float64), large_scene.centre(scene), tables=tables)


@pytest.mark.parametrize("n,prec", [(6000, 32), (6000, 64), (20000, 32)])
def test_lattices_are_gridded_almost_whole(native, n, prec):
    """What test_oracle_parity_beyond_the_lds asserts of large_grid(), and that the scene is beyond the LDS at all."""
    sc = large_scene.lattice(n, prec)
    pl = _plan(native, sc, tables=True)
    assert pl["usable"] and pl["registered"] >= 0.9 * n and pl["direct"] <= 8, pl
    assert sorted(pl["direct_list"]) == [0, 1, 2, 3]                   # the ground and the three unit spheres
    m = len(sc["type"])
    padded = (m + 4) // 4 * 4
    assert (prec // 8 + 4) * 4 * padded > 160 * 1024                  # layout_lds: the default source's tables do not fit
    cells, idx = pl["cells"].reshape(-1, 2).astype(np.int64), pl["indices"]
    assert (cells[:, 0] + cells[:, 1] <= len(idx)).all() and idx.max() < m and cells[:, 1].max() == pl["longest_list"]
    assert pl["nx"] * pl["nz"] > 4096                                  # more cells than the LDS grid may have


def test_at_most_two_of_the_random_scenes_are_refused(native):
    """test_same_image_as_the_existing_paths asserts the refusal of a scene the plan does not suit: it must not pass on refusals alone."""
    refused = [(case, prec) for case in large_scene.RANDOM_CASES for prec in (32, 64) if not _plan(native, large_scene.random_case(case)[prec])["usable"]]
    assert len({case for case, _ in refused}) <= 2, refused


def test_the_line_is_longer_than_any_walk_of_the_lds_grid(native):
    for prec in (32, 64):
        pl = _plan(native, large_scene.line(2000, prec))
        assert pl["usable"] and pl["nx"] + pl["nz"] > 128, pl


def test_ten_spheres_are_refused(native):
    assert not _plan(native, large_scene.ten_spheres())["usable"]


# ---- the edge scenes of tests/test_render_large_edges.py: each pinned to the property it exists for, and every floor that test asserts
# of its ray families shown here first for the reference alone (the oracle's loop on the CPU), on the very rays it traces
EDGE_CASES = [(name, prec) for name in large_scene.EDGE_SCENES for prec in (32, 64)]


@pytest.mark.parametrize("name,prec", EDGE_CASES)
def test_edge_scenes_have_the_structure_they_exist_for(native, name, prec):
    sc = large_scene.edge_scene(name, prec)
    m = len(sc["type"])
    assert (prec // 8 + 4) * 4 * ((m + 4) // 4 * 4) < 64 * 1024        # far inside the LDS: the exact loop's hook accepts the scene
    pl = _plan(native, sc, tables=True)
    assert pl["usable"], pl
    count = pl["cells"][:, :, 1].astype(np.int64)
    assert count.max() == pl["longest_list"] and pl["registered"] + pl["direct"] == m
    if name == "clusters":
        long = count[count >= 7]
        assert pl["longest_list"] >= 24 and len(long) >= 20 and (long % 2 == 0).any() and (long % 2 == 1).any() and pl["direct"] == 1, pl
        pairs = large_scene.twins(sc)
        assert len(pairs) >= 6
        def lists_with(low, high):                                     # the lengths of the lists that hold both copies
            return [int(count[c]) for c in zip(*np.nonzero(count >= 2)) if {low, high} <= set(pl["indices"][int(pl["cells"][c][0]):][:int(count[c])].tolist())]
        shared = [lists_with(low, high) for low, high in pairs]
        assert all(shared) and all(low < high for low, high in pairs) and max(max(s) for s in shared) >= 20, shared     # every pair in one list; one in a list of twenty or more
        cr = np.asarray(sc["center_radius"], np.float64)[601:]
        assert 0.15 <= cr[:, 3].min() < 0.16 and cr[:, 3].max() == pytest.approx(0.2) and np.ptp(cr[:, 1]) > 0.3     # mixed radii and heights
    elif name == "equal_no_ground":
        assert pl["direct"] == 0 and pl["registered"] == 900 and len(pl["direct_list"]) == 0, pl
        assert 3.4 < pl["yhi"] - pl["ylo"] < 3.6
    elif name == "mixed_with_bad":
        assert pl["direct"] % 4 != 0 and pl["direct"] >= 5, pl
        assert set(large_scene.MIXED_BAD.values()) <= set(pl["direct_list"].tolist())          # r < 0, r = NaN, cx = inf -- and r = 0
        assert {0, 1, 2, 3, 4} <= set(pl["direct_list"].tolist())
    elif name == "far_centre":
        assert pl["eps"] >= 0.04 and pl["eps"] > 0.2 * 0.2, pl        # a fifth of a radius and more
        assert abs(pl["x0"]) > 2900 and abs(pl["z0"]) > 1900
    else:
        assert pl["cell"] > 100 and pl["yhi"] - pl["ylo"] > 20 and pl["cell"] > 500 * 0.2, pl


@pytest.mark.parametrize("name,prec", EDGE_CASES)
def test_edge_ray_floors_hold_for_the_oracle_alone(native, oracle, name, prec):
    """0.3 to 0.9 s of the oracle's loop a case (185 128 rays against at most 1 001 spheres)."""
    from tests import large_rays
    sc, cr, pl, rays, where = large_rays.edge_case(native, name, prec)
    assert len(rays) > 9 * large_rays.N_EACH and set(where) == set(large_rays.ADVERSARIAL) | {"degenerate"} | set(large_rays.FAMILIES)
    _, index = oracle.hit_world(prec, sc["center_radius"], rays)
    large_rays.assert_floors(name, sc, pl, rays, where, index)
    near = large_rays.within_reach(rays, where, cr, pl)
    assert len(near) > 0.8 * 8 * large_rays.N_EACH                     # the cut to rfar's reach keeps the walked families
    for fam in large_rays.FAMILIES:                                    # ... every new one among them, with hits and misses of its own
        inside = near[(near >= where[fam].start) & (near < where[fam].stop)]
        assert len(inside) > 0.9 * large_rays.N_EACH, (fam, len(inside))
    assert (index[where["lists"]] >= 0).mean() > 0.5 and (index[where["long_walk"]] < 0).mean() > 0.9
    assert 0.05 < (index[where["slab"]] >= 0).mean() < 0.95 and 0.01 < (index[where["rim"]] >= 0).mean() < 0.95


def test_edge_ray_families_are_what_they_say(native):
    from tests import large_rays
    for name in ("equal_no_ground", "sparse_wide"):
        sc, cr, pl, rays, where = large_rays.edge_case(native, name, 64, 3000)
        ctr = large_scene.centre(sc)
        x0, z0, cell, nx, nz, ylo, yhi = (pl[k] for k in ("x0", "z0", "cell", "nx", "nz", "ylo", "yhi"))
        inside = lambda r, pad: (r[:, 0] >= x0 - pad) & (r[:, 0] <= x0 + nx * cell + pad) & (r[:, 2] >= z0 - pad) & (r[:, 2] <= z0 + nz * cell + pad)
        slab = rays[where["slab"]]
        assert inside(slab, 3 * cell).all() and (~inside(slab, 0.0)).sum() > 100
        vertical = (slab[:, 3] == 0) & (slab[:, 5] == 0)
        assert vertical.sum() == 1000 and (np.abs(slab[vertical, 4]) == 1).all() and {-1.0, 1.0} <= set(slab[vertical, 4].tolist())
        g_ylo, g_yhi = np.nextafter(np.float32(ylo), np.float32(-np.inf)), np.nextafter(np.float32(yhi), np.float32(np.inf))     # the kernel's faces
        for level in (ylo, yhi, float(g_ylo), float(g_yhi), ylo - pl["eps"], yhi + pl["eps"]):
            assert (slab[~vertical, 1] == level).sum() > 50, level
        assert {0.0, 1e-7, -1e-7, 1e-3, -1e-3, 1.0, -1.0} == set(slab[~vertical, 4].tolist())
        for fam in ("lists", "rim"):
            assert (np.linalg.norm(rays[where[fam], :3] - ctr, axis=1) <= 0.9 * pl["rfar"] + 1e-9).all(), fam
        rim = rays[where["rim"]]
        assert (~inside(rim, 0.0)).sum() > 1000 and inside(rim, -cell * (1 + 1e-9)).sum() == 0       # outside the rectangle, or in its outermost ring
        assert ((rim[:, 1] >= ylo) & (rim[:, 1] <= yhi)).all()
        walk = rays[where["long_walk"]]
        assert (np.abs(walk[:, 4]) <= 1e-4 * np.hypot(walk[:, 3], walk[:, 5]) * (1 + 1e-12)).all()
        top = (cr[pl["halfwidth"] > 0, 1] + cr[pl["halfwidth"] > 0, 3]).max()
        assert ((walk[:, 1] >= top) & (walk[:, 1] <= yhi)).all()
        assert np.median(large_rays.cells_crossed(walk, pl)) >= 0.9 * max(nx, nz)
        count = pl["cells"][:, :, 1]
        lists = rays[where["lists"]]
        tgt = lists[:, :3] + lists[:, 3:]
        ix, iz = np.floor((tgt[:, 0] - x0) / cell).astype(int), np.floor((tgt[:, 2] - z0) / cell).astype(int)
        ok = (ix >= 0) & (ix < nx) & (iz >= 0) & (iz < nz)
        assert ok.mean() > 0.99 and (count[iz[ok], ix[ok]] >= min(5, count.max()) - 1).mean() > 0.6           # aimed into the long lists (a centre may sit in a neighbour)
        shuffled, perm = large_rays.shuffled(rays, np.random.default_rng(3))
        assert sorted(perm.tolist()) == list(range(len(rays))) and np.array_equal(shuffled, rays[perm], equal_nan=True) and (perm != np.arange(len(rays))).mean() > 0.99


@pytest.mark.parametrize("name,prec", [(n, p) for n in ("clusters", "mixed_with_bad") for p in (32, 64)])
def test_the_shuffle_mixes_waves(native, name, prec):
    """test_a_rays_result_does_not_depend_on_its_wave asks for 1 000 rays that walk in family order and take the exact loop when shuffled.
    By the kernel's text alone: a wave all of whose rays are within rfar's reach and of ordinary length walks, and a wave with one ray
    whose squared length is NaN or outside (1e-30, 1e30) takes the exact loop, all 64 lanes."""
    from tests import large_rays
    sc, cr, pl, rays, where = large_rays.edge_case(native, name, prec)
    _, perm = large_rays.shuffled(rays, np.random.default_rng(99))
    dragged = large_rays.dragged_along(rays, large_rays.within_reach(rays, where, cr, pl), perm)
    assert dragged.sum() >= 1000, int(dragged.sum())
