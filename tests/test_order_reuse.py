"""The carried hand-out order of RTIOW_SCHED_SORTED (-m gpu): after a handle's first two-phase render, further renders of the same frame
skip prepass and ranking and launch once, from sample 0, in the order the first one left.  The order is a
scheduling hint, so every image must equal the static schedule's bit for bit; what is checked here is that, the state machine
(which calls keep the order, which drop it) and the stats of a reused render."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, compact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _setup(rt, r, prec, scene_id, cam, shard=None, sched=None, source=None, seed=1227):
    r.set_camera(cam); r.set_scene(rt.build_scene(scene_id, prec))
    if shard:
        r.set_shard(*shard)
    if sched is not None:
        r.set_schedule(sched)
    if source is not None:
        r.set_scene_source(source)
    r.init_rng(seed)


_REFS = {}


def _reference(rt, oracle, prec, scene_id, cam, cam_key, shard=None, seed=1227):
    """The static schedule's image (threads = 8: one lane per pixel, no hand-out at all) of a fresh handle, and the oracle's rows
    0, H/2 and H - 1 of the local image.  Computed once per configuration and left alone."""
    key = (prec, scene_id, cam_key, shard, seed)
    if key not in _REFS:
        with rt.Renderer(0, prec) as r:
            _setup(rt, r, prec, scene_id, cam, shard, rt.SCHED_STATIC, seed=seed)
            r.render(8)
            img = r.read_framebuffer()
            row_map = r.local_row_map()
        sc = compact(oracle.build_scene(scene_id, prec))
        rows = {}
        for jl in (0, img.shape[0] // 2, img.shape[0] - 1):
            j = int(row_map[jl])
            rows[jl] = oracle.render(prec, sc, cam, seed, j, j + 1)[0]
        img.setflags(write=False)
        _REFS[key] = (img, rows)
    return _REFS[key]


def _check_image(got, ref):
    img, rows = ref
    assert _same_bits(got, img)
    for jl, want in rows.items():
        assert _same_bits(got[jl:jl + 1], want), jl


def _check_reused(st, ms):
    assert st["phases"] == 1 and st["prepass_samples"] == 0 and st["prepass_ms"] == 0 and st["staged_stores"] == 1 and st["order_reused"] == 1, st
    assert st["prepass_clock_mhz"] == 0
    assert 0 < st["main_ms"] and 0 < st["place_ms"] and st["main_ms"] + st["place_ms"] <= st["render_ms"] * 1.001, st
    assert abs(st["render_ms"] - ms) < 1e-6


def _check_two_phase(st):
    assert st["phases"] == 2 and st["prepass_samples"] > 0 and st["staged_stores"] == 1 and st["order_reused"] == 0, st


@pytest.mark.parametrize("prec,scene_id,W,H,S,B,shard,solo", [
    (32, 1, 64, 64, 24, 40, None, True),            # the smallest frame the schedule sorts: the solo kernel with clamped waves
    (64, 3, 96, 48, 24, 8, None, False),            # persistent kernel, rotated trip (fp64); the 64-byte records are no longer read
    (32, 3, 72, 60, 64, 20, None, False),           # 4320 pixels: a padded last pool, -1 slots in the order
    (32, 3, 128, 96, 24, 50, (1, 2, 4), True),      # strips plus solo waves
    (32, 2, 200, 100, 64, 50, None, True),
])
def test_four_renders_one_ranking(rt, oracle, prec, scene_id, W, H, S, B, shard, solo):
    cam = rt.camera(prec, W, H, S, B)
    ref = _reference(rt, oracle, prec, scene_id, cam, (W, H, S, B), shard)
    with rt.Renderer(0, prec) as r:
        _setup(rt, r, prec, scene_id, cam, shard)
        for k in range(4):
            ms = r.render(0)
            st = r.stats()
            _check_image(r.read_framebuffer(), ref)
            assert (st["solo_waves"] > 0) == solo, st
            if k == 0:
                _check_two_phase(st)
                first = st
            else:
                _check_reused(st, ms)
                # the same launch as the first render's main launch
                assert [st[f] for f in ("grid_blocks", "solo_waves", "solo_lanes", "vgprs", "lds_bytes")] == [first[f] for f in ("grid_blocks", "solo_waves", "solo_lanes", "vgprs", "lds_bytes")]


@pytest.mark.parametrize("W,H,S,sched", [
    (64, 64, 8, 2),          # too few samples for a prepass
    (60, 60, 24, 2),         # below 4096 pixels
    (96, 64, 24, 1),         # RTIOW_SCHED_PERSISTENT
])
def test_unsorted_renders_carry_nothing(rt, oracle, W, H, S, sched):
    cam = rt.camera(32, W, H, S, 20)
    ref = _reference(rt, oracle, 32, 3, cam, (W, H, S, 20))
    with rt.Renderer(0, 32) as r:
        _setup(rt, r, 32, 3, cam, sched=sched)
        for _ in range(4):
            ms = r.render(0)
            st = r.stats()
            assert st["phases"] == 1 and st["order_reused"] == 0 and st["staged_stores"] == 0 and st["prepass_ms"] == 0 and st["place_ms"] == 0, st
            assert abs(st["main_ms"] - ms) < 1e-6
            _check_image(r.read_framebuffer(), ref)


BASE = (96, 64, 24, 12)      # the invalidation cases start after two renders of this frame, scene 3, fp32


def _invalidation_cases(rt):
    """name -> (change(r), configuration rendered afterwards {scene_id, cam_key, shard}, order reused on the first render afterwards)."""
    def other_view(r):
        r.set_camera(rt.camera_look(32, 96, 64, 24, 12, lookfrom=(-6.0, 3.0, 9.0), vfov=30.0)); r.init_rng(1227)

    def larger_then_smaller(r):
        r.set_camera(rt.camera(32, 128, 96, 24, 12)); r.init_rng(1227)
        r.render(0)
        _check_two_phase(r.stats())
        r.set_camera(rt.camera(32, 64, 64, 24, 12)); r.init_rng(1227)

    def scene(r):
        r.set_scene(rt.build_scene(1, 32))

    def shard(r):
        r.set_shard(0, 2, 48); r.init_rng(1227)      # rows 0..47: 4608 local pixels, still sorted (an even split of this frame is below 4096)

    def static_and_back(r):
        r.set_schedule(rt.SCHED_STATIC); r.render(8)
        assert r.stats()["phases"] == 1 and r.stats()["order_reused"] == 0
        r.set_schedule(rt.SCHED_SORTED)

    def source(r):
        r.set_scene_source(rt.SCENE_LDS)

    def count(r):
        assert r.count_segments(0) > 0

    def accumulate(r):
        r.accumulate(12); r.accumulate(12)
        assert r.stats()["order_reused"] == 0

    return {
        "camera_other_view": (other_view, dict(cam_key="other_view"), False),
        "camera_larger_then_smaller": (larger_then_smaller, dict(cam_key=(64, 64, 24, 12)), False),
        "scene": (scene, dict(scene_id=1), False),
        "shard": (shard, dict(shard=(0, 2, 48)), False),
        "schedule_static_and_back": (static_and_back, {}, True),     # the static render reads and writes none of the order's buffers
        "scene_source": (source, {}, False),                         # another launch: the key differs
        "count_segments": (count, {}, False),                        # a counting run ranks into the same buffers
        "accumulate": (accumulate, {}, False),                       # the second chunk ranks into h->order
    }


@pytest.mark.parametrize("name", ["camera_other_view", "camera_larger_then_smaller", "scene", "shard", "schedule_static_and_back", "scene_source",
                                  "count_segments", "accumulate"])
def test_what_drops_the_order(rt, oracle, name):
    change, after, keeps = _invalidation_cases(rt)[name]
    scene_id, shard, cam_key = after.get("scene_id", 3), after.get("shard"), after.get("cam_key", BASE)
    cam = rt.camera_look(32, 96, 64, 24, 12, lookfrom=(-6.0, 3.0, 9.0), vfov=30.0) if cam_key == "other_view" else rt.camera(32, *cam_key)
    ref = _reference(rt, oracle, 32, scene_id, cam, cam_key, shard)
    with rt.Renderer(0, 32) as r:
        _setup(rt, r, 32, 3, rt.camera(32, *BASE))
        r.render(0); r.render(0)
        assert r.stats()["order_reused"] == 1
        change(r)
        ms = r.render(0)
        st = r.stats()
        _check_image(r.read_framebuffer(), ref)
        if keeps:
            _check_reused(st, ms)
        else:
            _check_two_phase(st)
        ms = r.render(0)                              # and the new frame's order is carried in its turn
        _check_reused(r.stats(), ms)
        _check_image(r.read_framebuffer(), ref)


def test_what_keeps_the_order(rt, oracle):
    cam = rt.camera(32, *BASE)
    with rt.Renderer(0, 32) as r:
        _setup(rt, r, 32, 3, cam)
        r.render(0)
        _check_two_phase(r.stats())
        r.init_rng(7)                                 # a new seed: the same cost distribution
        ms = r.render(0)
        _check_reused(r.stats(), ms)
        _check_image(r.read_framebuffer(), _reference(rt, oracle, 32, 3, cam, BASE, seed=7))
        r.set_camera(rt.camera(32, *BASE)); r.init_rng(1227)     # the identical camera
        ms = r.render(0)
        _check_reused(r.stats(), ms)
        _check_image(r.read_framebuffer(), _reference(rt, oracle, 32, 3, cam, BASE))


_CHILD = r"""
import json, sys
import numpy as np
import raytracingincuda_amd as rt
with rt.Renderer(0, 32) as r:
    r.set_camera(rt.camera(32, 96, 64, 24, 12)); r.set_scene(rt.build_scene(3, 32)); r.init_rng(1227)
    out = []
    for _ in range(4):
        r.render(0)
        st = r.stats()
        out.append({"phases": st["phases"], "order_reused": st["order_reused"], "prepass_ms": st["prepass_ms"]})
    np.save(sys.argv[1], r.read_framebuffer())
print(json.dumps(out))
"""


def test_switch_off(rt, oracle, tmp_path):
    """RTIOW_ORDER_REUSE=0 is read at rtiow_create: a child process, every render in two phases."""
    img = str(tmp_path / "img.npy")
    env = dict(os.environ, RTIOW_ORDER_REUSE="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", _CHILD, img], capture_output=True, text=True, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(rows) == 4 and all(row["phases"] == 2 and row["order_reused"] == 0 and row["prepass_ms"] > 0 for row in rows), rows
    _check_image(np.load(img), _reference(rt, oracle, 32, 3, rt.camera(32, *BASE), BASE))


def test_async_pair_and_two_member_group(rt, oracle):
    import ctypes
    cam = rt.camera(32, *BASE)
    ref = _reference(rt, oracle, 32, 3, cam, BASE)
    with rt.Renderer(0, 32) as r:
        _setup(rt, r, 32, 3, cam)
        r.render(0)
        r._check(r._lib.rtiow_render_async(r._h, 0))
        ms = ctypes.c_float(0)
        r._check(r._lib.rtiow_render_wait(r._h, ctypes.byref(ms)))
        _check_reused(r.stats(), ms.value)
        _check_image(r.read_framebuffer(), ref)
    # two ranks on device 0, 4-row strips.  At 96 x 64 a rank holds 3072 pixels and does not sort: three steps, the same image.  A frame
    # twice as tall sorts on both ranks: each carries its own order from the second step on.
    for H, sorts in ((64, False), (128, True)):
        W, _, S, B = BASE
        cam = rt.camera(32, W, H, S, B)
        whole = _reference(rt, oracle, 32, 3, cam, (W, H, S, B))
        with rt.RendererGroup(2, 32, 4, rt.GATHER_AUTO, [0, 0]) as g:
            g.set_camera(cam); g.set_scene(rt.build_scene(3, 32)); g.init_rng(1227)
            for step in range(3):
                g.render(0)
                g.gather()
                _check_image(g.read_framebuffer(), whole)
                for k in range(2):
                    st = g.member(k).stats()
                    if not sorts:
                        assert st["phases"] == 1 and st["order_reused"] == 0, st
                    elif step == 0:
                        _check_two_phase(st)
                    else:
                        assert st["phases"] == 1 and st["order_reused"] == 1 and st["prepass_ms"] == 0 and st["staged_stores"] == 1, st
