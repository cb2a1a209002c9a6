"""Filter guides that follow mirrors and glass to the first diffuse surface (rtiow_set_guide_mode,
rtiow_read_filter_guides, guide_chain_kernel).  The chain is defined operation by operation in T with plain * + - / and sqrt, so all
four planes are checked BIT FOR BIT against tests/preview_model.py's chain_np, which calls the CPU oracle's hit_world once per bounce
level; the three filters are checked against the model's filters fed with the filter guides; the first-hit guides, the history and every output
of the default mode keep their bits."""
import ctypes

import numpy as np
import pytest

from tests.lattice import lattice_scene
from tests.preview_drive import E_BADARG, E_STATE, INF
from tests.preview_drive import setup as _setup    # not a bare `setup`: older pytests take that name for a module hook
from tests.preview_model import LATTICE, chain_np, filter_np, same_bits, variance_filter_np

pytestmark = pytest.mark.gpu

FIRST_HIT, SPECULAR = 0, 1
SIG = (0.5, 0.1, 0.1, 1.0)


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


# ---- 1. the definition, bit for bit

_references = {}


def _reference(rt, oracle, prec, scene_id, W, H, max_bounces, max_fuzz):
    """The restatement of one case on the whole frame, computed once and shared (read-only) by the tests that need it."""
    key = (prec, scene_id, W, H, max_bounces, max_fuzz)
    if key not in _references:
        out = chain_np(rt, oracle, prec, scene_id, rt.camera(prec, W, H, 1, 10), np.arange(H), max_bounces, max_fuzz)
        for a in out[:4]:
            a.setflags(write=False)
        _references[key] = out
    return _references[key]


CASES = [(3, 67, 41, 1, INF), (3, 67, 41, 2, INF), (3, 67, 41, 8, INF), (1, 96, 54, 8, INF), (3, 67, 41, 8, 0.25), (LATTICE, 67, 41, 8, INF)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "s%s_%dx%d_b%d_f%s" % c)
@pytest.mark.parametrize("prec", [32, 64])
def test_filter_guides_are_the_definition(rt, oracle, prec, case):
    scene_id, W, H, max_bounces, max_fuzz = case
    wn, wa, wz, wb, facts = _reference(rt, oracle, prec, scene_id, W, H, max_bounces, max_fuzz)
    # the case meets what it is there for (counted on the restatement)
    npix = W * H
    assert (wb >= 1).sum() >= 0.15 * npix, (case, int((wb >= 1).sum()))
    if max_bounces == 8 and max_fuzz == INF:
        assert (wb >= 2).sum() >= 0.02 * npix, (case, int((wb >= 2).sum()))
    if max_bounces in (1, 2):
        assert facts["specular_at_cap"] >= 1 and int(wb.max()) == max_bounces, (case, facts)
    if scene_id in (1, LATTICE):
        assert facts["tir"] >= 1, (case, facts)
    if max_fuzz != INF:
        assert facts["rough_metal_first_hit"] >= 1, (case, facts)
    for source in (3, 1):                                # GRID, SCALAR
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3 if scene_id == LATTICE else scene_id, W, H, B=10, source=source)
            if scene_id == LATTICE:
                r.set_scene(lattice_scene(prec))
            r.set_guide_mode(SPECULAR, max_bounces, max_fuzz)
            n, a, z, b = r.filter_guides()
        where = (prec, case, source)
        assert b.dtype == np.int32 and np.array_equal(b, wb), (where, int((b != wb).sum()))
        assert same_bits(z, wz), (where, int((z != wz).sum()))
        assert same_bits(n, wn), (where, int((n != wn).any(-1).sum()))
        assert same_bits(a, wa), (where, int((a != wa).any(-1).sum()))


# ---- 2. shards

@pytest.mark.parametrize("prec", [32, 64])
def test_shards_hold_their_rows(rt, prec):
    W, H = 67, 41
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H, B=10)
        r.set_guide_mode(SPECULAR, 8, INF)
        whole = r.filter_guides()
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H, B=10, shard=(1, 3, 4))
        r.set_guide_mode(SPECULAR, 8, INF)
        rows = r.local_row_map()
        part = r.filter_guides()
        first = r.guides()
    assert 0 < len(rows) < H and (whole[3][rows] >= 1).any()
    for got, want in zip(part, whole):
        assert same_bits(got, np.ascontiguousarray(want[rows])), prec
    assert first[2].shape == (len(rows), W)


# ---- 3. the first-hit guides are untouched

@pytest.mark.parametrize("prec", [32, 64])
def test_first_hit_guides_keep_their_bits(rt, prec):
    W, H = 67, 41
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H, B=10)
        first = r.guides()
        fn, fa, fz, fb = r.filter_guides()               # FIRST_HIT: the first-hit planes, bounces 0
        for got, want in zip((fn, fa, fz), first):
            assert same_bits(got, want), prec
        assert fb.dtype == np.int32 and not fb.any()
        r.set_guide_mode(SPECULAR, 8, INF)
        for got, want in zip(r.guides(), first):
            assert same_bits(got, want), prec
        sn, sa, sz, sb = r.filter_guides()
        assert sb.any() and not same_bits(sz, fz)
        # a pixel whose first hit is not specular has the first-hit guides in both sets
        same = sb == 0
        assert same.any() and same_bits(sz[same], fz[same]) and same_bits(sn[same], fn[same]) and same_bits(sa[same], fa[same])


# ---- 4. the filters read the filter guides

@pytest.mark.parametrize("prec", [32, 64])
def test_the_filters_read_the_filter_guides(rt, prec):
    W, H, levels = 67, 41, 3
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H, B=10)
        r.accumulate(4)
        lin = r.read_linear()
        first_out = r.denoise(levels, *SIG)
        r.history_update()
        rgb, _ = r.history()
        first_hist = r.denoise_history(levels, *SIG)
        r.set_guide_mode(SPECULAR, 8, INF)
        n, a, z, b = r.filter_guides()
        got = r.denoise(levels, *SIG)
        assert same_bits(got, filter_np(lin, n, a, z, levels, *SIG)), prec
        assert not same_bits(got, first_out)             # fails without the feature
        assert same_bits(r.history()[0], rgb)            # the temporal image survived the switch
        got = r.denoise_history(levels, *SIG)
        assert same_bits(got, filter_np(rgb, n, a, z, levels, *SIG)), prec
        assert not same_bits(got, first_hist)
    sv = (4.5,) + SIG[1:]
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H, B=10)
        r.accumulate_with_variance(4)
        lin, var = r.read_linear(), r.variance()
        first_out = r.denoise_variance(levels, *sv)
        r.set_guide_mode(SPECULAR, 8, INF)
        n, a, z, b = r.filter_guides()
        got = r.denoise_variance(levels, *sv)
        assert same_bits(got, variance_filter_np(lin, var, n, a, z, levels, *sv)), prec
        assert not same_bits(got, first_out)


# ---- 5. the default behaviour is preserved

def _walk(r, rt, prec, W, H, switch):
    """denoise, history and filtered history of one frame, a commit, and the next camera's history; `switch` chooses where the
    handle visits SPECULAR mode: "never", "and_back" (before anything is computed) or "commit" (across the commit)."""
    cam2 = rt.camera_look(prec, W, H, 1, 10, lookfrom=(12.9, 2.0, 3.3))
    out = {}
    _setup(r, rt, prec, 3, W, H, B=10)
    if switch == "and_back":
        r.set_guide_mode(SPECULAR, 8, INF)
        r.accumulate(4)
        r.denoise(3, *SIG)                                # the chain buffers exist and have been filtered by
        r.set_guide_mode(FIRST_HIT)
    else:
        r.accumulate(4)
    out["denoise"] = r.denoise(3, *SIG)
    r.history_update()
    out["history"], out["length"] = r.history()
    out["denoise_history"] = r.denoise_history(3, *SIG)
    if switch == "commit":
        r.set_guide_mode(SPECULAR, 8, INF)
        r.denoise(3, *SIG)                                # renders both sets of guides before the commit takes the first-hit ones
    r.history_commit()
    r.set_camera(cam2); r.init_rng(7)
    r.accumulate(4)
    out["reprojected"] = r.history_update()
    out["history2"], out["length2"] = r.history()
    return out


@pytest.mark.parametrize("prec", [32, 64])
def test_the_default_mode_and_the_history_keep_their_bits(rt, prec):
    W, H = 67, 41
    runs = {}
    for switch in ("never", "and_back", "commit"):
        with rt.Renderer(0, prec) as r:
            runs[switch] = _walk(r, rt, prec, W, H, switch)
    want = runs["never"]
    assert want["reprojected"] > 0
    for key in ("denoise", "history", "length", "denoise_history", "history2", "length2"):
        assert same_bits(runs["and_back"][key], want[key]), (prec, key)
    for key in ("denoise", "history", "length", "denoise_history", "history2", "length2"):      # history does not depend on the mode
        assert same_bits(runs["commit"][key], want[key]), (prec, key)
    assert runs["commit"]["reprojected"] == want["reprojected"] == runs["and_back"]["reprojected"]


# ---- 6. state and arguments

def test_states_and_error_codes(rt):
    W, H = 67, 41
    npix = W * H
    with rt.Renderer(0, 32) as r:
        lib = r._lib
        _setup(r, rt, 32, 3, W, H, B=10)
        for mode in (-1, 2, 7):
            assert lib.rtiow_set_guide_mode(r._h, mode, 8, 1.0) == E_BADARG, mode
        for bounces in (0, -1, 17):
            assert lib.rtiow_set_guide_mode(r._h, SPECULAR, bounces, 1.0) == E_BADARG, bounces
        for fuzz in (-0.5, float("nan"), -INF):
            assert lib.rtiow_set_guide_mode(r._h, SPECULAR, 8, fuzz) == E_BADARG, fuzz
        assert lib.rtiow_set_guide_mode(r._h, FIRST_HIT, -5, float("nan")) == 0          # mode 0 ignores the rest
        assert lib.rtiow_read_filter_guides(r._h, None, None, None, None, npix) == E_STATE   # never rendered
        r.accumulate(2)
        r.denoise(2)
        assert lib.rtiow_read_filter_guides(r._h, None, None, None, None, npix) == 0
        assert lib.rtiow_read_filter_guides(r._h, None, None, None, None, npix + 1) == E_BADARG
        assert lib.rtiow_set_guide_mode(r._h, FIRST_HIT, 3, 0.5) == 0                    # changes nothing: everything stays
        assert lib.rtiow_read_filter_guides(r._h, None, None, None, None, npix) == 0
        r.read_denoised()
        for args in ((SPECULAR, 8, INF), (SPECULAR, 4, INF), (SPECULAR, 4, 0.25), (FIRST_HIT, 4, 0.25)):
            r.render_guides()
            r.denoise(2)
            assert lib.rtiow_set_guide_mode(r._h, *args) == 0, args
            assert lib.rtiow_read_filter_guides(r._h, None, None, None, None, npix) == E_STATE, args
            assert lib.rtiow_read_guides(r._h, None, None, None, npix) == E_STATE, args
            assert lib.rtiow_read_denoised(r._h, None, 0) == E_STATE, args
            assert r.accumulated_samples == 2
        r.set_guide_mode(SPECULAR, 4, 0.25)
        kept = r.filter_guides()
        assert lib.rtiow_set_guide_mode(r._h, SPECULAR, 4, 0.25) == 0                    # the same values again keep the guides
        assert lib.rtiow_read_filter_guides(r._h, None, None, None, None, npix) == 0
        # only the planes asked for are written
        b = np.full((H, W), -1, np.int32)
        assert lib.rtiow_read_filter_guides(r._h, None, None, None, b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), npix) == 0
        assert np.array_equal(b, kept[3]) and b.max() >= 1
        # the knob survives set_camera (and the guides go stale with the camera, as ever)
        r.set_camera(rt.camera(32, W, H, 1, 10))
        assert lib.rtiow_read_filter_guides(r._h, None, None, None, None, npix) == E_STATE
        r.set_scene(rt.build_scene(3, 32))
        again = r.filter_guides()
        for got, want in zip(again, kept):
            assert same_bits(got, want)
