"""Edge resolve on the GPU: rtiow_render_coverage finds the first-hit spheres that share each pixel from a
small lattice of primary rays, and rtiow_resolve_edges rebuilds the mixed pixels of the denoised image, in place, from what the filter
produced on the pure pixels of each layer nearby.  Every value is defined operation by operation in T with plain * + - / and sqrt, so
the layers and the resolved image are checked BIT FOR BIT, every pixel, against tests/edge_resolve_model.py."""
import ctypes

import numpy as np
import pytest

from tests.edge_resolve_model import INF, NO_LAYER, SKY, coverage_np, resolve_np, scene_of
from tests.lattice import lattice_scene
from tests.preview_drive import E_BADARG, E_STATE, history_defaults, move, moves, sample
from tests.preview_model import LATTICE, same_bits

pytestmark = pytest.mark.gpu

# 1 x 1; partial 8 x 8 and 16 x 16 tiles with the window clipped on all four sides; more than one workgroup of the resolve
FRAMES = ((1, 1), (7, 5), (33, 17), (64, 40))
BIG = FRAMES[-1]
LATTICE_LOOKFROM = (9.0, 3.0, 9.0)       # outside the glass sphere that surrounds the default camera of tests/lattice.py
# (subsamples_per_side, radius, sigma_normal, sigma_depth, prior)
SETTINGS = ((4, 1, 0.3, 0.5, 8.0), (2, 3, INF, 2.0, 2.5), (4, 3, 0.3, INF, INF), (2, 1, 0.05, 0.05, 0.5))


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def view(rt, prec, scene_id, W, H, B=10):
    """The camera of the exactness cases: the reference's view, and for the lattice one from outside its glass sphere."""
    if scene_id == LATTICE:
        return rt.camera_look(prec, W, H, 1, B, lookfrom=LATTICE_LOOKFROM)
    return rt.camera(prec, W, H, 1, B)


def start(r, rt, prec, scene_id, cam, source=3, shard=None, seed=1227):
    r.set_camera(cam)
    r.set_scene(lattice_scene(prec) if scene_id == LATTICE else rt.build_scene(scene_id, prec))
    r.set_scene_source(source)
    if shard:
        r.set_shard(*shard)
    r.init_rng(seed)


def check_layers(r, rt, oracle, prec, scene_id, cam, G, where):
    """render_coverage(G) and coverage() against the model; returns the model's layers and surface counts."""
    ms = r.render_coverage(G)
    assert ms > 0, where
    got = r.coverage()
    want = coverage_np(oracle, prec, scene_of(rt, scene_id, prec), cam, r.local_row_map(), G)
    for name, a, b in zip(("ids", "counts", "normal", "depth"), got, want):
        assert same_bits(a, b), (where, name, int((a != b).sum()))
    return want


def check_resolve(r, layers, n_eff, setting, where):
    """resolve_edges at `setting` on the denoised image the handle holds, against the model, every pixel; returns (before, after, count)."""
    G, radius, sn, sz, prior = setting
    g = r.read_denoised()
    N, _, Z = r.guides()
    count = r.resolve_edges(radius, sn, sz, prior)
    out = r.read_denoised()
    want, wrote = resolve_np(g, *layers[:4], N, Z, n_eff, G * G, radius, sn, sz, prior)
    assert same_bits(out, want), (where, setting, int((out != want).any(axis=-1).sum()))
    assert count == int(wrote.sum()), (where, setting, count, int(wrote.sum()))
    mixed = layers[0][..., 1] != NO_LAYER
    assert same_bits(np.ascontiguousarray(out[~mixed]), np.ascontiguousarray(g[~mixed])), where         # pure pixels keep their bits
    return g, out, count


# ---- 1. the layers

@pytest.mark.parametrize("scene_id", [1, 3, LATTICE])
@pytest.mark.parametrize("prec", [32, 64])
def test_layers_are_exact(rt, oracle, prec, scene_id):
    for W, H in FRAMES:
        cam = view(rt, prec, scene_id, W, H)
        with rt.Renderer(0, prec) as r:
            start(r, rt, prec, scene_id, cam)
            for G in (4, 2, 4):                              # a different G renders again, and so does the same
                ids, counts, _, _, surfaces = check_layers(r, rt, oracle, prec, scene_id, cam, G, (prec, scene_id, W, H, G))
                assert ((counts.sum(-1) == G * G) == (surfaces <= 2)).all()
            if (W, H) == BIG:                                # what the resolve's cases rely on
                mixed = ids[..., 1] != NO_LAYER
                assert (surfaces >= 3).any() and (mixed & (ids == SKY).any(-1)).any() and (~mixed & (ids[..., 0] == SKY)).any()


@pytest.mark.parametrize("prec", [32, 64])
def test_layers_from_every_scene_source_and_on_a_shard(rt, oracle, prec):
    W, H = 33, 17
    for scene_id in (1, 3):
        cam = view(rt, prec, scene_id, W, H)
        for source in (rt.SCENE_LDS, rt.SCENE_SCALAR, rt.SCENE_LDS_EXACT, rt.SCENE_GRID):
            with rt.Renderer(0, prec) as r:
                start(r, rt, prec, scene_id, cam, source)
                check_layers(r, rt, oracle, prec, scene_id, cam, 4, (prec, scene_id, "source", source))
    cam = view(rt, prec, 3, W, H)
    with rt.Renderer(0, prec) as r:                          # rows are global: strips 1, 4, ... of 3 rows each
        start(r, rt, prec, 3, cam, shard=(1, 3, 3))
        assert 0 < r.local_rows < H
        for G in (2, 4):
            check_layers(r, rt, oracle, prec, 3, cam, G, (prec, "shard", G))


# ---- 2. the resolve

@pytest.mark.parametrize("scene_id", [1, 3, LATTICE])
@pytest.mark.parametrize("prec", [32, 64])
def test_resolve_of_a_plain_accumulation_is_exact(rt, oracle, prec, scene_id):
    for W, H in FRAMES:
        cam = view(rt, prec, scene_id, W, H)
        with rt.Renderer(0, prec) as r:
            start(r, rt, prec, scene_id, cam)
            r.accumulate(3)
            n = np.full((H, W), 3, np.int32)
            rewritten = 0
            for setting in SETTINGS:
                where = (prec, scene_id, W, H)
                layers = check_layers(r, rt, oracle, prec, scene_id, cam, setting[0], where)
                plain = r.denoise()
                g, out, count = check_resolve(r, layers, n, setting, where)
                assert same_bits(g, plain), where            # read_denoised before the call is the plain filter's
                rewritten += count
            if (W, H) == BIG:
                assert rewritten > 0 and not same_bits(out, g)


def _budget_frame(r, rt, prec, scene_id, W, H):
    """An adaptive base at the home view, then a budget chunk at the orbit view that samples only where the plan is short: pixels with
    0, 2 and more samples in one accumulation."""
    cams = moves(rt, prec, W, H)
    start(r, rt, prec, scene_id, cams["home"])
    sample(r, True)
    r.history_update(); r.history_commit()
    move(r, cams["orbit"], 1228)
    r.history_plan()
    r.accumulate_budget(2, 6.0, 0)
    return cams["orbit"]


@pytest.mark.parametrize("scene_id", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_resolve_after_every_filter_is_exact(rt, oracle, prec, scene_id):
    """The count behind the image: the pixel's own samples after denoise() and denoise_variance() of an adaptive accumulation that holds
    pixels without a sample, the history length after denoise_history() and denoise_history_variance()."""
    for (W, H), setting in (((33, 17), SETTINGS[1]), (BIG, SETTINGS[0])):
        where = (prec, scene_id, W, H)
        with rt.Renderer(0, prec) as r:
            cam = _budget_frame(r, rt, prec, scene_id, W, H)
            layers = check_layers(r, rt, oracle, prec, scene_id, cam, setting[0], where)
            counts = r.adaptive_state()[0]
            if (W, H) == BIG:
                assert (counts == 0).any() and (counts > 0).any(), where
            r.denoise()
            check_resolve(r, layers, counts, setting, where + ("denoise",))
            r.denoise_variance()
            check_resolve(r, layers, counts, setting, where + ("denoise_variance",))
            r.history_update_clipped()
            M = r.history()[1]
            assert not same_bits(M, counts.astype(M.dtype)), where
            r.denoise_history()
            check_resolve(r, layers, M, setting, where + ("denoise_history",))
            r.denoise_history_variance()
            _, out, count = check_resolve(r, layers, M, setting, where + ("denoise_history_variance",))
            # the asynchronous form: the same image, read after the fact
            r.denoise_history_variance()
            assert r.resolve_edges(*setting[1:], sync=False) is None
            assert same_bits(r.read_denoised(), out), where
            r.history_commit()                               # the commit takes the temporal image: its resolve comes before it


@pytest.mark.parametrize("prec", [32, 64])
def test_a_frame_without_silhouettes_is_left_alone(rt, oracle, prec):
    W, H = 33, 17
    inside = rt.camera(prec, W, H, 1, 10)                    # the lattice's glass sphere of radius 2 surrounds the reference's camera
    sky = rt.camera_look(prec, W, H, 1, 10, lookat=(13.0, 50.0, 3.0), vup=(0.0, 0.0, 1.0))
    for scene_id, cam, pid in ((LATTICE, inside, 2), (3, sky, SKY)):
        with rt.Renderer(0, prec) as r:
            start(r, rt, prec, scene_id, cam)
            r.accumulate(2)
            for G in (2, 4):
                ids, counts, _, _, _ = check_layers(r, rt, oracle, prec, scene_id, cam, G, (prec, scene_id))
                assert (ids[..., 0] == pid).all() and (ids[..., 1] == NO_LAYER).all() and (counts[..., 0] == G * G).all()
                g = r.denoise()
                assert r.resolve_edges() == 0
                assert same_bits(r.read_denoised(), g)


# ---- 3. what the call leaves alone

def _everything(r):
    out = {"fb": r.read_framebuffer(), "linear": r.read_linear(), "temporal": r.history()[0], "length": r.history()[1], "base": r.history_base()[0],
           "base_length": r.history_base()[1], "plan": r.history_plan_lengths()}
    out["counts"], out["err"] = r.adaptive_state()
    out["normal"], out["albedo"], out["depth"] = r.guides()
    return out


@pytest.mark.parametrize("prec", [32, 64])
def test_the_resolve_touches_nothing_but_the_denoised_image(rt, prec):
    W, H = BIG
    states = []
    for resolve in (False, True):
        with rt.Renderer(0, prec) as r:
            _budget_frame(r, rt, prec, 3, W, H)
            r.history_update()
            r.history_plan()
            plain = r.denoise_history()
            if resolve:
                assert r.resolve_edges() > 0                 # renders the layers itself, 4 x 4
                assert not same_bits(r.read_denoised(), plain)
                assert (r.coverage()[1].sum(-1) <= 16).all() and (r.coverage()[1][..., 0] > 0).all()
            s = _everything(r)
            s["plain"] = plain
            r.accumulate_budget(2, INF, 0)                   # the next chunk's bits
            s["next_fb"], s["next_linear"] = r.read_framebuffer(), r.read_linear()
            states.append(s)
    for name in states[0]:
        assert same_bits(states[0][name], states[1][name]), name


# ---- 4. states and refusals

def test_states_and_error_codes(rt):
    W, H, prec = 33, 17, 32
    npix = W * H
    nan = float("nan")
    good = (2, 0.3, 0.5, 8.0)
    with rt.Renderer(0, prec) as r:
        lib, h = r._lib, r._h
        resolve = lambda *a: lib.rtiow_resolve_edges(h, *a, None, None)
        read = lambda n=npix: lib.rtiow_read_coverage(h, None, None, None, None, n)
        assert lib.rtiow_render_coverage(h, 4, None) == E_STATE and read() == E_STATE          # before scene and camera
        start(r, rt, prec, 3, rt.camera(prec, W, H, 1, 10))
        for G in (-1, 0, 1, 3, 5, 8, 16):
            assert lib.rtiow_render_coverage(h, G, None) == E_BADARG, G
        assert read() == E_STATE                                                                # the bad calls rendered nothing
        assert resolve(*good) == E_STATE                                                        # no denoised image
        r.accumulate(2)
        plain = r.denoise()
        ms, n = ctypes.c_float(-1), ctypes.c_uint64(7)
        for bad in ((0,) + good[1:], (4,) + good[1:], (-1,) + good[1:]) + tuple(good[:k] + (v,) + good[k + 1:] for k in (1, 2, 3) for v in (0.0, -1.0, nan)):
            assert lib.rtiow_resolve_edges(h, *bad, ctypes.byref(ms), ctypes.byref(n)) == E_BADARG and ms.value == 0 and n.value == 0, bad
        assert same_bits(r.read_denoised(), plain) and read() == E_STATE                        # the failing calls left the handle as it was
        assert lib.rtiow_resolve_edges(h, *good, None, ctypes.byref(n)) == 0 and n.value > 0 and read() == 0   # stale layers are rendered first:
        assert (r.coverage()[1].sum(-1) > 4).any()                                              # 4 x 4 when the C call was never told a lattice
        assert read(npix + 1) == E_BADARG and read(0) == E_BADARG
        resolved = r.read_denoised()
        assert resolve(*good) == E_STATE and same_bits(r.read_denoised(), resolved)             # already resolved
        assert "already resolved" in lib.rtiow_last_error_string(h).decode()
        r.denoise()
        r.accumulate(1)
        assert resolve(*good) == E_STATE                                                        # a chunk since the filter
        r.denoise()
        r.reset_accumulation()
        assert resolve(*good) == E_STATE                                                        # a reset since the filter
        r.accumulate(2)
        r.render_coverage(2)
        r.denoise()
        r.history_update()
        r.history_commit()
        assert resolve(*good) == 0                                                              # a commit is nothing to a filtered accumulation
        # ... and the layers survive it, with chunks, resets and the guide mode; the resolve used the 2 x 2 lattice it was given
        assert read() == 0 and (r.coverage()[1].sum(-1) <= 4).all()
        r.set_guide_mode(rt.GUIDES_SPECULAR)
        assert read() == 0 and resolve(*good) == E_STATE                                        # a new guide mode: no denoised image
        r.set_guide_mode(rt.GUIDES_FIRST_HIT)
        r.history_update()
        r.denoise_history()
        r.history_commit()
        assert resolve(*good) == E_STATE                                                        # the temporal image it came from is gone
        assert "resolve before rtiow_history_commit" in lib.rtiow_last_error_string(h).decode()
        r.history_update()
        r.denoise_history()
        assert resolve(*good) == 0
        # stale after set_scene, set_camera and set_shard; the next resolve renders them again at the last lattice
        for change in (lambda: r.set_scene(rt.build_scene(3, prec)), lambda: r.set_camera(rt.camera(prec, W, H, 1, 10)), lambda: r.set_shard(0, 1, 8)):
            assert read() == 0
            change()
            assert read() == E_STATE
            r.init_rng(1227)
            r.accumulate(1)
            r.denoise()
            assert r.resolve_edges() >= 0 and read() == 0 and (r.coverage()[1].sum(-1) <= 4).all()
    with rt.Renderer(0, prec) as r:                          # the wrapper renders stale layers at its own default lattice
        start(r, rt, prec, 3, rt.camera(prec, W, H, 1, 10))
        r.accumulate(2)
        r.denoise()
        G = rt.api.COVERAGE_GRID
        assert r.resolve_edges() > 0 and (r.coverage()[1].sum(-1) <= G * G).all() and (r.coverage()[1].sum(-1) == G * G).any()
    with rt.Renderer(0, prec) as r:                          # a sharded handle: layers yes, resolve no
        start(r, rt, prec, 3, rt.camera(prec, W, H, 1, 10), shard=(1, 3, 8))
        r.accumulate(2)
        assert r.render_coverage(2) >= 0 and r.coverage()[0].shape == (r.local_rows, W, 2)
        assert r._lib.rtiow_resolve_edges(r._h, *good, None, None) == E_STATE
        assert "sharded" in r._lib.rtiow_last_error_string(r._h).decode()


# ---- 5. it pays where it was proposed to

@pytest.fixture(scope="module")
def references(rt):
    """The 1024-sample linear images of scenes 1 and 3 at 320 x 180 and 50 bounces: the set-up of tests/test_denoise.py, rendered once."""
    W, H, B, prec = 320, 180, 50, 32
    out = {}
    for scene_id in (1, 3):
        with rt.Renderer(0, prec) as r:
            start(r, rt, prec, scene_id, rt.camera(prec, W, H, 1, B))
            r.accumulate(1024)
            out[scene_id] = r.read_linear().astype(np.float64)
    return out


@pytest.mark.parametrize("samples", [4, 16])
@pytest.mark.parametrize("scene_id", [1, 3])
def test_it_lowers_the_error_of_denoise(rt, references, capsys, scene_id, samples):
    """A sign condition, not a tuned threshold: at the defaults the linear MSE of the resolved denoise() is below that of plain denoise(),
    over the whole frame and over the mixed pixels alone."""
    W, H, B, prec = 320, 180, 50, 32
    ref = references[scene_id]
    with rt.Renderer(0, prec) as r:
        start(r, rt, prec, scene_id, rt.camera(prec, W, H, 1, B))
        r.accumulate(samples)
        plain = r.denoise().astype(np.float64) ** 2
        count = r.resolve_edges()
        resolved = r.read_denoised().astype(np.float64) ** 2
        mixed = r.coverage()[0][..., 1] != NO_LAYER
    mse = lambda img, sel: float(np.mean((img - ref)[sel] ** 2))
    frame = np.ones_like(mixed)
    whole, edges = mse(resolved, frame) / mse(plain, frame), mse(resolved, mixed) / mse(plain, mixed)
    with capsys.disabled():
        print("\nedge resolve, scene %d, %d samples: MSE resolved / plain %.4f (whole frame), %.4f (the %d mixed pixels, %d rewritten)"
              % (scene_id, samples, whole, edges, int(mixed.sum()), count))
    assert whole < 1 and edges < 1, (scene_id, samples, whole, edges)
