"""Progressive rendering (rtiow_accumulate) on the GPU.  The bar is the project's usual one, BIT-EXACT: after chunks k1, ..., ki the
framebuffer holds the very bits rtiow_render leaves with samples_per_pixel = k1 + ... + ki -- whatever the chunk sizes, schedule, scene
source or shard layout -- because a pixel's samples are one sequential RNG chain summed in sample order and every chunk resumes each
pixel from its exact state."""
import functools
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

from tests import preview_drive
from tests.conftest import compact
from tests.preview_drive import one_shot
from tests.preview_model import same_bits

pytestmark = pytest.mark.gpu

SCHEDULES = (0, 1, 2)        # RTIOW_SCHED_STATIC, PERSISTENT, SORTED
SOURCES = (0, 1, 2, 3)       # RTIOW_SCENE_LDS, SCALAR, LDS_EXACT, GRID
_setup = functools.partial(preview_drive.setup, B=50, sched=2)


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def test_previews_equal_one_shot_renders(rt):
    W, H, B, chunks = 320, 192, 50, [1, 2, 7, 10]          # >= 4096 pixels: chunks 2..4 are ranked by the previous chunk's costs
    for prec in (32, 64):
        for scene_id in (3, 1):
            with rt.Renderer(0, prec) as r:
                _setup(r, rt, prec, scene_id, W, H, B=B)
                assert r.accumulated_samples == 0
                total = 0
                for k in chunks:
                    ms = r.accumulate(k)
                    total += k
                    assert ms > 0 and r.accumulated_samples == total
                    got = r.read_framebuffer()
                    assert same_bits(got, one_shot(rt, prec, scene_id, W, H, total, B)), (prec, scene_id, total)
                st = r.stats()
                assert st["phases"] == 1 and st["prepass_samples"] == 0 and st["primary_rays"] == W * H * chunks[-1]


def test_previews_equal_the_oracle(rt, oracle):
    W, H, B = 64, 40, 50
    for prec in (32, 64):
        sc = compact(oracle.build_scene(3, prec))
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3, W, H, B=B)
            total = 0
            for k in (1, 3):
                r.accumulate(k)
                total += k
                want, _ = oracle.render(prec, sc, rt.camera(prec, W, H, total, B), 1227)
                assert same_bits(r.read_framebuffer(), want), (prec, total)


def test_schedule_and_source_do_not_change_the_bits(rt):
    W, H, B = 96, 72, 25                                      # 6912 pixels: the sorted schedule ranks the second chunk
    for prec in (32, 64):
        want = one_shot(rt, prec, 3, W, H, 10, B)
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3, W, H, B=B)
            for sched in SCHEDULES:
                for source in SOURCES:
                    r.set_schedule(sched, 0)
                    r.set_scene_source(source)
                    r.reset_accumulation()
                    r.accumulate(5, threads=8)
                    r.accumulate(5)
                    assert same_bits(r.read_framebuffer(), want), (prec, sched, source)
            # the schedule switched between two chunks, without a reset
            for first, second in ((0, 2), (2, 1), (1, 0), (2, 0)):
                r.set_scene_source(3)
                r.set_schedule(first, 0)
                r.reset_accumulation()
                r.accumulate(5)
                r.set_schedule(second, 0)
                r.accumulate(5)
                assert r.accumulated_samples == 10
                assert same_bits(r.read_framebuffer(), want), (prec, first, second)


@pytest.mark.parametrize("name,chunks", [("config3_headline_scene3_1920x1080_100spp_50b_f32", [1, 9, 40, 50]),
                                         ("scene3_1920x1080_100spp_50b_f64", [25, 25, 25, 25])])
def test_full_frames_accumulated_match_the_goldens(rt, golden_dir, name, chunks):
    """tests/golden/full_frame_crcs.json: one CRC-32 per row of the oracle's full frame and its SHA-256."""
    g = json.load(open(os.path.join(golden_dir, "full_frame_crcs.json")))[name]
    assert sum(chunks) == g["samples"]
    with rt.Renderer(0, g["precision"]) as r:
        _setup(r, rt, g["precision"], g["scene_id"], g["width"], g["height"], B=g["bounces"], seed=g["seed"])
        for k in chunks:
            r.accumulate(k)
        img = r.read_framebuffer()
    assert img.shape == (g["height"], g["width"], 3)
    crcs = [zlib.crc32(np.ascontiguousarray(img[j]).view(np.uint8).tobytes()) & 0xffffffff for j in range(img.shape[0])]
    bad = [j for j in range(img.shape[0]) if crcs[j] != g["row_crc32"][j]]
    assert not bad, "%s: %d rows differ from the oracle, first %s" % (name, len(bad), bad[:8])
    assert hashlib.sha256(np.ascontiguousarray(img).view(np.uint8).tobytes()).hexdigest() == g["sha256"]


def test_sharded_chunks_assemble_to_the_one_shot_image(rt):
    W, H, B, nranks, strip = 322, 183, 25, 3, 2
    for prec in (32, 64):
        want = one_shot(rt, prec, 3, W, H, 8, B)
        full = np.zeros_like(want)
        rows = 0
        for rank in range(nranks):
            with rt.Renderer(0, prec) as r:
                _setup(r, rt, prec, 3, W, H, B=B, shard=(rank, nranks, strip))
                r.accumulate(4)
                r.accumulate(4)
                part = r.read_framebuffer()
            rows += part.shape[0]
            rt.place_rows(full, part, rank, nranks, strip)
        assert rows == H and same_bits(full, want), prec


def test_render_and_count_between_chunks_leave_the_accumulation_alone(rt):
    W, H, B = 96, 72, 25
    for prec in (32, 64):
        with rt.Renderer(0, prec) as r:
            _setup(r, rt, prec, 3, W, H, S=5, B=B)              # the camera's own 5 spp: what render / count_segments use
            r.accumulate(3)
            r.render(0)                                          # the sorted schedule's own prepass records and hand-over
            assert same_bits(r.read_framebuffer(), one_shot(rt, prec, 3, W, H, 5, B))
            r.count_segments(0)
            r.accumulate(4)
            assert r.accumulated_samples == 7
            assert same_bits(r.read_framebuffer(), one_shot(rt, prec, 3, W, H, 7, B)), prec


def test_what_resets_the_accumulation(rt):
    W, H, B = 96, 72, 25
    prec = 32
    want1 = one_shot(rt, prec, 3, W, H, 1, B)
    cam = rt.camera(prec, W, H, 1, B)
    resets = {
        "set_camera": lambda r: r.set_camera(cam),
        "set_scene": lambda r: r.set_scene(rt.build_scene(3, prec)),
        "set_shard": lambda r: r.set_shard(0, 1, 8),
        "init_rng": lambda r: r.init_rng(1227),
        "reset_accumulation": lambda r: r.reset_accumulation(),
    }
    with rt.Renderer(0, prec) as r:
        _setup(r, rt, prec, 3, W, H, B=B)
        for name, reset in resets.items():
            r.accumulate(2)
            assert r.accumulated_samples > 0
            reset(r)
            assert r.accumulated_samples == 0, name
            r.init_rng(1227)                                     # set_camera / set_shard ask for it again
            r.accumulate(1)
            assert same_bits(r.read_framebuffer(), want1), name
        # a new scene source, schedule or framebuffer does not change the image: the total goes on
        r.reset_accumulation()
        r.accumulate(2)
        r.set_scene_source(0)
        r.set_schedule(1, 0)
        assert r.accumulated_samples == 2
        r.accumulate(3)
        assert r.accumulated_samples == 5
        assert same_bits(r.read_framebuffer(), one_shot(rt, prec, 3, W, H, 5, B))


def test_errors_and_a_bound_torch_framebuffer(rt, oracle):
    with rt.Renderer(0, 32) as r:
        with pytest.raises(rt.RtiowError) as e:
            r.accumulate(1)
        assert e.value.code == -2                                # no camera, no scene
        r.set_camera(rt.camera(32, 16, 16, 1, 4))
        r.set_scene(rt.build_scene(3, 32))
        with pytest.raises(rt.RtiowError) as e:
            r.accumulate(1)
        assert e.value.code == -2                                # RNG not initialised
        r.init_rng(1227)
        for bad in (0, -3):
            with pytest.raises(rt.RtiowError) as e:
                r.accumulate(bad)
            assert e.value.code == -1
        r.accumulate(1)
        with pytest.raises(rt.RtiowError) as e:
            r.accumulate(2 ** 31 - 1)                            # the total would pass INT32_MAX
        assert e.value.code == -1 and r.accumulated_samples == 1

    import torch
    from raytracingincuda_amd.distributed import StripGather
    W, H, S, B = 80, 48, 2, 8
    want, _ = oracle.render(32, compact(oracle.build_scene(3, 32)), rt.camera(32, W, H, S, B), 1227)
    g = StripGather(W, H, 0, 1, 8, torch.float32, "cuda:0")
    stream = torch.cuda.Stream()
    with rt.Renderer(0, 32) as r, torch.cuda.stream(stream):
        r.set_stream(stream.cuda_stream)
        r.set_camera(rt.camera(32, W, H, 1, B)); r.set_scene(rt.build_scene(3, 32)); r.init_rng(1227)
        view = g.local_view()
        r.bind_framebuffer(view.data_ptr(), view.numel() * 4)
        r.accumulate(1, sync=False)
        r.accumulate(1, sync=False)
        full = g.gather()
        stream.synchronize()
        assert r.accumulated_samples == S
    assert same_bits(full.cpu().numpy(), want)
