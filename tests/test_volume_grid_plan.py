"""The volume grid's plan (csrc/library/volume_grid.h) on the CPU.  tests/native/volume_grid_plan_main.cpp is a stand-alone program, built
here with AddressSanitizer + UBSan and run directly: it holds plan and blob to the invariants that keep the kernel's gathers inside the
blob.  Then the plan hook (rtiow_debug_volume_grid_plan: host arithmetic of the test build, no GPU) on the very scenes
tests/test_render_volume.py renders, recomputed with numpy -- and, of that file's ray families, that they are what they say, for the
oracle's loop alone on the very rays."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import large_scene, volume_rays, volume_scene
from tests.conftest import ROOT


def test_volume_grid_plan_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "volume_grid_plan_main")
    inc = os.path.join(ROOT, "raytracingincuda_amd", "csrc", "library")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + inc, "-o", exe, os.path.join(ROOT, "tests", "native", "volume_grid_plan_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    assert r.stdout.splitlines()[-1] == "0 volume-grid-plan failure(s)"


def _plan(native, scene, tables=False, max_cells=0):
    return native.debug_volume_grid_plan(np.asarray(scene["center_radius"], np.float64), volume_scene.centre(scene), tables=tables, max_cells=max_cells)


def _check_invariants(scene, pl, max_cells=1 << 20):
    """Every finite sphere is direct or listed in every cell its inflated cube touches, against the fp32 edges; indices ascend within a
    cell; no sphere is in more than 8 cells; first and count tile the index array; nx ny nz <= max_cells."""
    cr = np.asarray(scene["center_radius"], np.float64)
    m = len(cr)
    nx, ny, nz = pl["nx"], pl["ny"], pl["nz"]
    assert 1 <= nx * ny * nz <= max_cells
    cells = pl["cells"].reshape(-1, 2).astype(np.int64)
    idx = pl["indices"].astype(np.int64)
    assert cells.shape[0] == nx * ny * nz
    first, count = cells[:, 0], cells[:, 1]
    assert first[0] == 0 and (first[1:] == first[:-1] + count[:-1]).all() and first[-1] + count[-1] == len(idx) == pl["index_entries"]
    assert count.max() == pl["longest_list"] and (count > 0).sum() == pl["occupied_cells"]
    assert idx.min() >= 0 and idx.max() < m
    owner = np.repeat(np.arange(len(cells)), count)                       # the cell of every index entry
    same_cell = owner[1:] == owner[:-1]
    assert (idx[1:][same_cell] > idx[:-1][same_cell]).all()               # ascending within a cell
    assert np.bincount(idx, minlength=m).max() <= 8
    direct = set(pl["direct_list"].tolist())
    assert pl["registered"] + pl["direct"] == m and len(direct) == pl["direct"]
    half = np.asarray(pl["halfwidth"])
    assert ((half > 0) == ~np.isin(np.arange(m), list(direct))).all()
    # the cube of every registered sphere against the edges the kernel uses: fp32 origin and width
    lo = np.array([np.float32(pl[k]) for k in ("x0", "y0", "z0")], np.float64)
    cell = float(np.float32(pl["cell"]))
    reg = np.nonzero(half > 0)[0]
    assert np.isfinite(cr[reg]).all()
    reach = (half[reg] + pl["eps"])[:, None]
    a = np.floor((cr[reg, :3] - reach - lo) / cell).astype(np.int64)
    b = np.floor((cr[reg, :3] + reach - lo) / cell).astype(np.int64)
    assert (a >= 0).all() and (b < np.array([nx, ny, nz])).all() and (b - a <= 1).all()
    listed = set(zip(owner.tolist(), idx.tolist()))
    want = 0
    for ex in (0, 1):
        for ey in (0, 1):
            for ez in (0, 1):
                c = np.minimum(a + np.array([ex, ey, ez]), b)            # the corner cells of the span (a span is at most 2 x 2 x 2)
                rec = (c[:, 1] * nz + c[:, 2]) * nx + c[:, 0]
                pairs = set(zip(rec.tolist(), reg.tolist()))
                assert pairs <= listed
                want = pairs if not want else want | pairs
    assert want == listed                                                  # ... and in no other cell
    return idx, count


@pytest.mark.parametrize("name", ["cube14", "cube18", "cube27", "cube18_f64", "with_bad", "column", "slab_of_layers", "cube_no_ground", "flat"])
def test_plan_invariants(native, name):
    sc = {"cube14": lambda: volume_scene.cube(14), "cube18": lambda: volume_scene.cube(18), "cube27": lambda: volume_scene.cube(27),
          "cube18_f64": lambda: volume_scene.cube(18, 64), "with_bad": volume_scene.with_bad, "column": volume_scene.column,
          "slab_of_layers": volume_scene.slab_of_layers, "cube_no_ground": lambda: volume_scene.cube_no_ground(12), "flat": volume_scene.flat}[name]()
    pl = _plan(native, sc, tables=True)
    assert pl["usable"], pl
    _check_invariants(sc, pl)
    if name == "with_bad":
        assert pl["direct"] == 7 and set(volume_scene.WITH_BAD.values()) | {0, 2745, 2746} == set(pl["direct_list"].tolist())
    if name == "column":
        assert pl["ny"] > 128 and pl["direct"] == 0
    if name == "cube_no_ground":
        assert pl["direct"] == 0
    if name == "flat":
        assert sorted(pl["direct_list"].tolist()) == [0, 1, 2, 3]         # the flat lattice is usable, not refused


def test_the_widening_loop_runs_under_a_small_cap(native):
    sc = volume_scene.cube(27)
    free = _plan(native, sc)
    assert free["nx"] * free["ny"] * free["nz"] > 4096
    pl = _plan(native, sc, tables=True, max_cells=4096)
    assert pl["usable"] and pl["cell"] > free["cell"] and pl["registered"] == free["registered"]
    _check_invariants(sc, pl, max_cells=4096)


@pytest.mark.parametrize("side", [14, 18, 27])
def test_cubes_have_short_lists(native, side):
    """Spheres per occupied cell: at most 6, and at most 0.4 of the two-axis device grid's on the same scene (cube(14): 2.6 against
    10.5; cube(18): 2.8 against 13.6; cube(27): 3.0 against 24.6).  The bound 0.4 holds for every cell-size constant the plan may be given
    (K = 2.0: about 4.1 and 4.7 on cube(18) and cube(27))."""
    sc = volume_scene.cube(side)
    pl = _plan(native, sc, tables=True)
    assert pl["usable"] and pl["direct"] <= 1, pl
    mean = pl["index_entries"] / pl["occupied_cells"]
    flat = native.debug_large_grid_plan(np.asarray(sc["center_radius"], np.float64), large_scene.centre(sc), tables=True)
    assert flat["usable"]
    flat_mean = flat["index_entries"] / int((flat["cells"][:, :, 1] > 0).sum())
    print("cube(%d): %d x %d x %d, mean %.2f, longest %d; device grid %d x %d, mean %.2f, longest %d"
          % (side, pl["nx"], pl["ny"], pl["nz"], mean, pl["longest_list"], flat["nx"], flat["nz"], flat_mean, flat["longest_list"]))
    assert mean <= 6.0 and mean <= 0.4 * flat_mean, (mean, flat_mean)


def test_ten_spheres_are_refused(native):
    assert not _plan(native, volume_scene.ten_spheres())["usable"]


def test_a_cap_above_the_librarys_is_refused(native):
    """A record's byte offset is computed in 32 bits: the hook takes no cap above 2^20 cells."""
    sc = volume_scene.cube(14)
    assert _plan(native, sc, max_cells=1 << 20)["usable"]
    with pytest.raises(native.RtiowError) as e:
        _plan(native, sc, max_cells=(1 << 20) + 1)
    assert e.value.code == -1


def test_gauss_cloud_is_reported(native):
    pl = _plan(native, volume_scene.gauss_cloud())
    print("gauss_cloud: usable %s, %d x %d x %d, mean %.2f, longest %d" % (pl["usable"], pl["nx"], pl["ny"], pl["nz"],
                                                                        pl["index_entries"] / max(1, pl["occupied_cells"]), pl["longest_list"]))


def test_ray_scenes_fit_the_lds(native):
    """A pin of what tests/test_render_volume.py assumes of its scenes, not a test of the library: it runs none of the feature's code and
    passes without it.  The exact loop (RTIOW_SCENE_LDS_EXACT) still applies to the ray-by-ray scenes in both precisions, the cubes of
    the oracle test are beyond the LDS, and with_bad is the one scene outside the range that allows FastDiv (range_flags bit 1)."""
    for prec in (32, 64):
        for sc in (volume_scene.cube(14, prec), volume_scene.with_bad(prec), volume_scene.column(prec)):
            assert volume_scene.fits_lds(sc, prec)
        assert volume_scene.scene_in_range(volume_scene.cube(14, prec)) and volume_scene.scene_in_range(volume_scene.column(prec))
        assert not volume_scene.scene_in_range(volume_scene.with_bad(prec))
    for prec, sc in ((32, volume_scene.cube(18, 32)), (64, volume_scene.cube(18, 64)), (32, volume_scene.cube(27, 32))):
        m = len(sc["type"])
        assert (prec // 8 + 4) * 4 * ((m + 4) // 4 * 4) > 160 * 1024      # layout_lds: the default source's tables do not fit


# ---- the ray families of tests/volume_rays.py: what they say, for the oracle alone
@pytest.mark.parametrize("name,prec", [("cube14", 32), ("cube14", 64), ("with_bad", 32), ("with_bad", 64), ("column", 32)])
def test_walked_families_hit_and_miss(native, oracle, name, prec):
    sc, cr, pl, rays, where = volume_rays.case(native, name, prec)
    assert len(rays) == 8 * volume_rays.N_EACH and tuple(where) == volume_rays.FAMILIES
    _, index = oracle.hit_world(prec, sc["center_radius"], rays)
    for fam in volume_rays.WALKED:
        share = float((index[where[fam]] >= 0).mean())
        print(name, prec, fam, "hits %.3f" % share)
        assert 0.20 <= share <= 0.95, (fam, share)
    near = volume_rays.within_reach(rays, where, cr, pl)
    assert len(near) > 0.95 * 7 * volume_rays.N_EACH                    # the cut to rfar's reach keeps the walked families
    gridded = (index >= 0) & ~np.isin(index, pl["direct_list"])
    assert gridded[near].mean() > 0.25                                   # ... and they hit gridded spheres, not the ground alone


def test_families_are_what_they_say(native):
    for name in ("cube14", "column"):
        sc, cr, pl, rays, where = volume_rays.case(native, name, 64, 3000)
        r = rays.astype(np.float64)
        lo = np.array([pl["x0"], pl["y0"], pl["z0"]])
        dims = np.array([pl["nx"], pl["ny"], pl["nz"]])
        hi = lo + dims * pl["cell"]
        ctr = volume_scene.centre(sc)
        assert np.array_equal(rays, rays.astype(np.float32).astype(np.float64), equal_nan=True)     # fp32 numbers
        # faces: one coordinate within two fp32 steps of a face of its axis, every axis and every step served
        f = r[where["faces"]]
        seen = set()
        for k, ray in enumerate(f[:600]):
            a = k % 3
            j = int(round((ray[a] - lo[a]) / pl["cell"]))
            face = np.float32(lo[a]) + np.float32(j) * np.float32(pl["cell"])
            steps = [s for s in (-2, -1, 0, 1, 2) if np.float32(ray[a]) == np.float32(volume_rays._f32_steps(face, s))]
            assert steps, (k, ray)
            seen.add((a, steps[0]))
        assert seen == {(a, s) for a in range(3) for s in (-2, -1, 0, 1, 2)}
        # parallel: one or two components that never step, exact zeros among them
        d = r[where["parallel"], 3:]
        still = (np.abs(d) < 1e-30).sum(axis=1)
        assert set(still.tolist()) == {1, 2} and (d == 0).any() and ((d != 0) & (np.abs(d) < 1e-30)).any()
        # ties: equal leaving parameters in fp32 for at least half the family
        assert volume_rays.tied(r[where["ties"]], pl).mean() >= 0.5
        t3 = r[where["ties"]]
        off = t3[:, :3].astype(np.float32) - lo.astype(np.float32)
        assert ((off[:, 0] == off[:, 1]) & (off[:, 1] == off[:, 2]) & (t3[:, 3] == t3[:, 4]) & (t3[:, 4] == t3[:, 5])).sum() > 100     # three-way ties
        # diagonals: across the whole grid
        g = r[where["diagonals"]]
        end = g[:, :3] + g[:, 3:] / np.abs(g[:, 3:]).max(axis=1, keepdims=True) * (hi - lo).max()
        assert (np.abs(g[:, 3:]) > 0).sum(axis=1).min() >= 2 and np.median(np.abs(end - g[:, :3]).max(axis=1)) >= 0.9 * (hi - lo).max()
        # entering: outside the box, through each of the six faces, within reach of the walk
        e = r[where["entering"]]
        outside_lo, outside_hi = e[:, :3] < lo, e[:, :3] > hi
        assert (outside_lo | outside_hi).any(axis=1).mean() > 0.9
        assert outside_lo.any(axis=0).all() and outside_hi.any(axis=0).all()
        assert (np.linalg.norm(e[:, :3] - ctr, axis=1) <= 0.9 * pl["rfar"]).all()
        # inside: within the box, a third inside a sphere
        i = r[where["inside"]]
        assert ((i[:, :3] >= lo - 0.3) & (i[:, :3] <= hi + 0.3)).all()
        reg = np.nonzero(pl["halfwidth"] > 0)[0]
        d2 = ((i[::3, None, :3] - cr[None, reg[:4000], :3]) ** 2).sum(axis=2) if len(reg) <= 4000 else None
        if d2 is not None:
            assert (d2.min(axis=1) < 0.2 ** 2).mean() > 0.95
        # vertical: straight up and straight down
        v = r[where["vertical"]]
        assert (v[:, 3] == 0).all() and (v[:, 5] == 0).all() and set(v[:, 4].tolist()) == {-1.0, 1.0}
        # far: beyond rfar or not finite or huge
        far = r[where["far"]]
        with np.errstate(invalid="ignore", over="ignore"):
            beyond = np.linalg.norm(far[:, :3] - ctr, axis=1) > 1.04 * pl["rfar"]
            odd = ~np.isfinite(far).all(axis=1) | ((far[:, 3:] ** 2).sum(axis=1) > 1e31)
        assert (beyond | odd).all() and odd.sum() > 100 and (~np.isfinite(far)).any()
        shuffled, perm = volume_rays.shuffled(rays, np.random.default_rng(3))
        assert sorted(perm.tolist()) == list(range(len(rays))) and np.array_equal(shuffled, rays[perm], equal_nan=True) and (perm != np.arange(len(rays))).mean() > 0.99


def test_the_columns_verticals_cross_the_whole_height(native, oracle):
    """test_ray_by_ray asks the column's up and down rays for walks of more than 128 cells: some of them start beyond an end, run the whole
    height and, by the oracle, hit nothing on the way."""
    sc, cr, pl, rays, where = volume_rays.case(native, "column", 32)
    v = rays[where["vertical"]].astype(np.float64)
    _, index = oracle.hit_world(32, sc["center_radius"], rays[where["vertical"]])
    lo, hi = pl["y0"], pl["y0"] + pl["ny"] * pl["cell"]
    whole = ((v[:, 1] < lo) & (v[:, 4] > 0)) | ((v[:, 1] > hi) & (v[:, 4] < 0))
    assert pl["ny"] > 128 and (whole & (index < 0)).sum() > 100 and (index >= 0).sum() > 100
