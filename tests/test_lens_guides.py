"""Lens-sampled filter guides on the GPU (rtiow_set_guide_lens, guide_lens_kernel).  The guides are defined
operation by operation in T with plain * + - / and sqrt, so all four planes of rtiow_read_filter_guides are checked BIT FOR BIT against
tests/lens_guides_model.py's lens_guides_np, which calls the CPU oracle's hit_world; the five calls that steer by the filter guides are
checked against tests/preview_model.py's functions fed the lens planes; the first-hit guides, the history, the plan, the coverage
layers and the next chunk keep their bits; the knob at 0 and a pinhole camera are exact no-ops."""
import numpy as np
import pytest

from tests.lattice import lattice_scene
from tests.lens_guides_model import lens_guides_np
from tests.preview_drive import E_BADARG, E_STATE, INF
from tests.preview_model import (LATTICE, chain_np, feedback_np, filter_np, guides_np, same_bits, temporal_noise_np,
                                 variance_filter_np)

pytestmark = pytest.mark.gpu

FIRST_HIT, SPECULAR = 0, 1
# the smallest frames at which the kernel can still go wrong: one pixel, a ragged tile, tiles in both directions plus a ragged edge, and
# several whole tiles in both directions
FRAMES = ((1, 1), (7, 5), (33, 17), (64, 40))
MAIN = FRAMES[2]
WIDE = 10.0                                   # degrees of defocus: lens rays of one pixel see different spheres at these sizes
MODES = ((FIRST_HIT, 0), (SPECULAR, 1), (SPECULAR, 8))       # (guide mode, max_bounces); max_fuzz = +inf
SIG = (0.5, 0.1, 0.1, 1.0)
SOURCES = (0, 1, 2, 3)                        # LDS, SCALAR, LDS_EXACT, GRID


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def wide(rt, prec, W, H):
    return rt.camera_look(prec, W, H, 1, 10, defocus_angle=WIDE)


def start(r, rt, prec, scene_id, cam, source=3, shard=None, seed=1227):
    r.set_camera(cam)
    r.set_scene(lattice_scene(prec) if scene_id == LATTICE else rt.build_scene(scene_id, prec))
    r.set_scene_source(source)
    if shard:
        r.set_shard(*shard)
    r.init_rng(seed)


def set_mode(r, mode, max_bounces):
    if mode == SPECULAR:
        r.set_guide_mode(SPECULAR, max_bounces, INF)
    else:
        r.set_guide_mode(FIRST_HIT)


def check_planes(got, want, where):
    n, a, z, b = got
    wn, wa, wz, wb = want
    assert b.dtype == np.int32 and np.array_equal(b, wb), (where, int((b != wb).sum()))
    assert same_bits(z, wz), (where, "depth", int((z != wz).sum()))
    assert same_bits(n, wn), (where, "normal", int((n != wn).any(-1).sum()))
    assert same_bits(a, wa), (where, "albedo", int((a != wa).any(-1).sum()))


# ---- 1. the filter guides are the definition, bit for bit

@pytest.mark.parametrize("scene_id", [1, 3, LATTICE])
@pytest.mark.parametrize("prec", [32, 64])
def test_filter_guides_are_the_definition(rt, oracle, prec, scene_id):
    """The cross product on 33 x 17: both lattices, the three chains, through the 10-degree aperture (in the material lattice that camera
    sits inside a glass sphere).  One handle walks through the six settings, so every change of a knob is followed by a fresh render."""
    W, H = MAIN
    cam = wide(rt, prec, W, H)
    rows = np.arange(H)
    with rt.Renderer(0, prec) as r:
        start(r, rt, prec, scene_id, cam)
        for G in (2, 4):
            for mode, mb in MODES:
                set_mode(r, mode, mb)
                r.set_guide_lens(G)
                got = r.filter_guides()
                want = lens_guides_np(rt, oracle, prec, scene_id, cam, rows, G, mb, INF)
                check_planes(got, want, (prec, scene_id, G, mode, mb))
                if mode == SPECULAR:
                    assert want[3].max() >= 1, (scene_id, G, mb)          # the case meets a specular surface
                    assert int(want[3].max()) <= mb
                else:
                    assert not want[3].any()


@pytest.mark.parametrize("size", [FRAMES[0], FRAMES[1], FRAMES[3]], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("prec", [32, 64])
def test_spot_frames(rt, oracle, prec, size):
    W, H = size
    cam = wide(rt, prec, W, H)
    rows = np.arange(H)
    with rt.Renderer(0, prec) as r:
        start(r, rt, prec, 3, cam)
        for G, (mode, mb) in ((4, MODES[2]), (2, MODES[0])):
            set_mode(r, mode, mb)
            r.set_guide_lens(G)
            check_planes(r.filter_guides(), lens_guides_np(rt, oracle, prec, 3, cam, rows, G, mb, INF), (prec, size, G, mode))


@pytest.mark.parametrize("prec", [32, 64])
def test_every_scene_source_and_a_shard(rt, oracle, prec):
    W, H = MAIN
    cam = wide(rt, prec, W, H)
    want = lens_guides_np(rt, oracle, prec, 3, cam, np.arange(H), 4, 8, INF)
    for source in SOURCES:
        with rt.Renderer(0, prec) as r:
            start(r, rt, prec, 3, cam, source=source)
            r.set_guide_mode(SPECULAR, 8, INF)
            r.set_guide_lens(4)
            check_planes(r.filter_guides(), want, (prec, "source", source))
    # rank 1 of 3, strips of 4 rows: the rows are global
    with rt.Renderer(0, prec) as r:
        start(r, rt, prec, 3, cam, shard=(1, 3, 4))
        r.set_guide_mode(SPECULAR, 8, INF)
        r.set_guide_lens(4)
        rows = r.local_row_map()
        assert 0 < len(rows) < H and rows[0] == 4
        part = r.filter_guides()
        check_planes(part, lens_guides_np(rt, oracle, prec, 3, cam, rows, 4, 8, INF), (prec, "shard"))
        check_planes(part, tuple(np.ascontiguousarray(a[rows]) for a in want), (prec, "shard of the whole"))


@pytest.mark.parametrize("prec", [32, 64])
def test_the_default_lens_and_the_sky(rt, oracle, prec):
    W, H = MAIN
    rows = np.arange(H)
    cam = rt.camera(prec, W, H, 1, 10)                   # the reference's 0.6 degrees
    assert float(cam.defocus_angle) > 0
    sky = rt.camera_look(prec, W, H, 1, 10, lookat=(13.0, 50.0, 3.0), vup=(1.0, 0.0, 0.0), defocus_angle=WIDE)
    with rt.Renderer(0, prec) as r:
        start(r, rt, prec, 3, cam)
        for G in (2, 4):
            r.set_guide_lens(G)
            check_planes(r.filter_guides(), lens_guides_np(rt, oracle, prec, 3, cam, rows, G, 0, INF), (prec, "default lens", G))
        r.set_guide_mode(SPECULAR, 8, INF)
        r.set_camera(sky); r.init_rng(1227)
        want = lens_guides_np(rt, oracle, prec, 3, sky, rows, 4, 8, INF)
        assert not any(a.any() for a in want)            # nothing but sky: every plane is zero
        got = r.filter_guides()
        check_planes(got, want, (prec, "sky"))
        assert not any(a.view(np.uint8).any() for a in got)


# ---- 2. the test is not vacuous (asserted on the model alone)

@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("size", [FRAMES[2], FRAMES[3]], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("prec", [32, 64])
def test_the_wide_lens_sees_different_spheres(rt, oracle, prec, size, scene_id):
    W, H = size
    cam = wide(rt, prec, W, H)
    lens = lens_guides_np(rt, oracle, prec, scene_id, cam, np.arange(H), 2, 0, INF)
    first = guides_np(rt, oracle, prec, scene_id, cam, np.arange(H))
    differ = (lens[1] != first[1]).any(-1)
    assert differ.mean() >= 0.10, (prec, size, scene_id, float(differ.mean()))


# ---- 3. the filters read them

@pytest.mark.parametrize("mode", [FIRST_HIT, SPECULAR])
@pytest.mark.parametrize("prec", [32, 64])
def test_the_filters_read_the_lens_guides(rt, oracle, prec, mode):
    W, H = MAIN
    levels, radius = 3, 2
    cam = wide(rt, prec, W, H)
    mb = 8 if mode == SPECULAR else 0
    sv = (4.5,) + SIG[1:]
    where = (prec, mode)
    with rt.Renderer(0, prec) as r:
        start(r, rt, prec, 3, cam)
        set_mode(r, mode, mb)
        r.accumulate_adaptive(4, 0.0, min_samples=4)     # a 4-sample adaptive chunk: every pixel active
        lin, var, counts = r.read_linear(), r.variance(), r.adaptive_state()[0]
        plain = r.denoise(levels, *SIG)
        r.set_guide_lens(2)
        n, a, z, b = r.filter_guides()
        check_planes((n, a, z, b), lens_guides_np(rt, oracle, prec, 3, cam, np.arange(H), 2, mb, INF), where)
        got = r.denoise(levels, *SIG)
        assert same_bits(got, filter_np(lin, n, a, z, levels, *SIG)), where
        assert not same_bits(got, plain), where          # fails without the feature
        assert same_bits(r.denoise_variance(levels, *sv), variance_filter_np(lin, var, n, a, z, levels, *sv)), where
        r.history_update()
        C, M = r.history()
        assert same_bits(C, lin), where                  # no base: the temporal image is the accumulation
        assert same_bits(r.denoise_history(levels, *SIG), filter_np(C, n, a, z, levels, *SIG)), where
        got = r.denoise_history_variance(levels, *sv, radius)
        v0 = temporal_noise_np(C, M, counts, var, radius)
        assert same_bits(r.history_variance(), v0), where
        assert same_bits(got, variance_filter_np(C, v0, n, a, z, levels, *sv)), where
        sf = (0.05,) + SIG[1:]
        r.history_commit_filtered(*sf, feedback=0.5)
        rgb, length = r.history_base()
        want, want_m = feedback_np(C, M, n, a, z, sf, 0.5)
        assert same_bits(rgb, want) and same_bits(length, want_m), where


# ---- 4. everything else keeps its bits

def _walk(r, rt, prec, cam, cam2, lens):
    """What the knob must leave alone, from one handle: the first-hit guides, both updates, the plan, the coverage layers, a commit and
    the next camera's chunk and update.  lens: the knob's value, set before anything is computed."""
    out = {}
    start(r, rt, prec, 3, cam)
    if lens:
        r.set_guide_lens(lens)
    r.accumulate_adaptive(4, 0.0, min_samples=4)
    r.denoise(2, *SIG)                                   # renders the guides, both sets
    out["normal"], out["albedo"], out["depth"] = r.guides()
    out["count"] = r.history_update()
    out["history"], out["length"] = r.history()
    r.render_coverage(2)
    out["ids"], out["counts"], out["cov_normal"], out["cov_depth"] = r.coverage()
    r.history_commit()
    r.set_camera(cam2); r.init_rng(7)
    r.history_plan()
    out["plan"] = r.history_plan_lengths()
    r.accumulate_adaptive(4, 0.0, min_samples=4)
    out["framebuffer"] = r.read_framebuffer()
    out["linear"] = r.read_linear()
    out["adaptive_counts"] = r.adaptive_state()[0]
    out["count2"], out["clipped2"] = r.history_update_clipped()
    out["history2"], out["length2"] = r.history()
    out["count3"] = r.history_update()
    out["history3"], out["length3"] = r.history()
    out["normal2"], out["albedo2"], out["depth2"] = r.guides()
    return out


@pytest.mark.parametrize("prec", [32, 64])
def test_everything_else_keeps_its_bits(rt, prec):
    W, H = MAIN
    cam = wide(rt, prec, W, H)
    cam2 = rt.camera_look(prec, W, H, 1, 10, lookfrom=(12.9, 2.0, 3.3), defocus_angle=WIDE)
    runs = {}
    for lens in (0, 2, 4):
        with rt.Renderer(0, prec) as r:
            runs[lens] = _walk(r, rt, prec, cam, cam2, lens)
    want = runs[0]
    assert want["count2"] > 0 and want["count3"] > 0 and (want["plan"] > 0).any() and (want["ids"][..., 1] != -2).any()
    for lens in (2, 4):
        for key, value in want.items():
            got = runs[lens][key]
            if isinstance(value, np.ndarray):
                assert same_bits(got, value), (prec, lens, key)
            else:
                assert got == value, (prec, lens, key)


# ---- 5. off and pinhole are exact no-ops

@pytest.mark.parametrize("prec", [32, 64])
def test_off_is_the_original(rt, prec):
    W, H = MAIN
    cam = wide(rt, prec, W, H)
    with rt.Renderer(0, prec) as r:
        start(r, rt, prec, 3, cam)
        r.accumulate(4)
        first = r.filter_guides()
        plain = r.denoise(3, *SIG)
        assert r.set_guide_lens(0) is None and r._lib.rtiow_read_guides(r._h, None, None, None, W * H) == 0     # nothing changed
        r.set_guide_lens(4)
        lens = r.filter_guides()
        assert not same_bits(lens[0], first[0]) and not same_bits(r.denoise(3, *SIG), plain)
        r.set_guide_lens(0)
        for got, want in zip(r.filter_guides(), first):
            assert same_bits(got, want), prec
        for got, want in zip(r.filter_guides()[:3], r.guides()):
            assert same_bits(got, want), prec
        assert same_bits(r.denoise(3, *SIG), plain), prec


@pytest.mark.parametrize("mode", [FIRST_HIT, SPECULAR])
@pytest.mark.parametrize("prec", [32, 64])
def test_a_pinhole_camera_makes_the_knob_inert(rt, oracle, prec, mode):
    W, H = MAIN
    cam = rt.camera_look(prec, W, H, 1, 10, defocus_angle=0.0)
    with rt.Renderer(0, prec) as r:
        start(r, rt, prec, 3, cam)
        set_mode(r, mode, 8)
        r.accumulate(4)
        first = r.filter_guides()
        plain = r.denoise(3, *SIG)
        r.set_guide_lens(4)
        assert r._lib.rtiow_read_filter_guides(r._h, None, None, None, None, W * H) == E_STATE      # the knob changed: stale all the same
        got = r.filter_guides()
        for x, y in zip(got, first):
            assert same_bits(x, y), (prec, mode)
        assert same_bits(r.denoise(3, *SIG), plain), (prec, mode)
        if mode == SPECULAR:
            want = chain_np(rt, oracle, prec, 3, cam, np.arange(H), 8, INF)
            check_planes(got, want[:4], (prec, "pinhole chain"))
            assert got[3].any()
        else:
            assert not got[3].any()
            for x, y in zip(got[:3], r.guides()):
                assert same_bits(x, y), prec
        # a lens on the same handle brings the lattice into effect
        r.set_camera(wide(rt, prec, W, H)); r.init_rng(1227)
        mb = 8 if mode == SPECULAR else 0
        check_planes(r.filter_guides(), lens_guides_np(rt, oracle, prec, 3, wide(rt, prec, W, H), np.arange(H), 4, mb, INF), (prec, mode, "lens again"))


# ---- 6. states and error codes

def test_states_and_error_codes(rt):
    W, H = MAIN
    npix = W * H
    cam = wide(rt, 32, W, H)
    with rt.Renderer(0, 32) as r:
        lib = r._lib
        read_guides = lambda: lib.rtiow_read_guides(r._h, None, None, None, npix)
        read_filter = lambda: lib.rtiow_read_filter_guides(r._h, None, None, None, None, npix)
        read_denoised = lambda: lib.rtiow_read_denoised(r._h, None, 0)
        assert lib.rtiow_set_guide_lens(r._h, 2) == 0 and lib.rtiow_set_guide_lens(r._h, 0) == 0    # a knob: no scene or camera needed
        start(r, rt, 32, 3, cam)
        for value in (-1, 1, 3, 5):
            assert lib.rtiow_set_guide_lens(r._h, value) == E_BADARG, value
        assert read_filter() == E_STATE                  # never rendered
        plan = np.zeros((H, W), np.float32)
        r.accumulate(2)
        r.history_update()
        r.history_commit()
        r.accumulate(2)
        r.history_update()
        r.history_plan()
        r.render_coverage(2)
        r.denoise(2)
        assert read_guides() == 0 and read_filter() == 0 and read_denoised() != E_STATE
        assert lib.rtiow_set_guide_lens(r._h, 0) == 0    # unchanged: everything stays
        assert read_guides() == 0 and read_filter() == 0 and read_denoised() != E_STATE
        for value in (2, 4, 2, 0):
            r.render_guides()
            r.denoise(2)
            assert read_guides() == 0
            assert lib.rtiow_set_guide_lens(r._h, value) == 0, value
            assert read_guides() == E_STATE and read_filter() == E_STATE and read_denoised() == E_STATE, value
            # the accumulation, the temporal image, the base, the plan and the coverage layers still answer
            assert r.accumulated_samples == 4
            assert lib.rtiow_read_history(r._h, None, None, npix) == 0
            assert lib.rtiow_read_history_base(r._h, None, None, npix) == 0
            assert lib.rtiow_read_history_plan(r._h, plan.ctypes.data, npix) == 0
            assert lib.rtiow_read_coverage(r._h, None, None, None, None, npix) == 0
        r.set_guide_lens(4)
        kept = r.filter_guides()
        assert lib.rtiow_set_guide_lens(r._h, 4) == 0    # the same value again keeps the guides
        assert read_guides() == 0 and read_filter() == 0
        # the knob survives set_camera, set_scene and set_shard (the guides go stale with each, as ever)
        r.set_camera(cam)
        assert read_filter() == E_STATE
        r.set_scene(rt.build_scene(3, 32))
        r.set_shard(0, 1, 8)
        for got, want in zip(r.filter_guides(), kept):
            assert same_bits(got, want)
        # orthogonal to the guide mode: mode 2 is still refused, and a change of mode keeps the lattice
        assert lib.rtiow_set_guide_mode(r._h, 2, 8, 1.0) == E_BADARG
        r.set_guide_mode(SPECULAR, 8, INF)
        assert read_filter() == E_STATE
        assert r.filter_guides()[3].any()
        r.set_guide_mode(FIRST_HIT)
        for got, want in zip(r.filter_guides(), kept):
            assert same_bits(got, want)
