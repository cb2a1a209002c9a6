"""Parity tests proper (-m gpu): the HIP render path, called through the C-ABI, against the
CPU oracle on the same seeded inputs.  The bar is BIT-EXACT: kernel and oracle share one
floating-point contract (IEEE + - * / sqrt, explicit fma placements, no other contraction;
see DESIGN.md), so every pixel's float bits must agree, in fp32 and in fp64.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import compact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _render(rt, prec, scene_id, W, H, S, B, threads=8, source=3, shard=None, seed=1227, sched=2, wps=0):
    sc = rt.build_scene(scene_id, prec)
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, W, H, S, B))
        r.set_scene(sc)
        r.set_scene_source(source)
        r.set_schedule(sched, wps)
        if shard:
            r.set_shard(*shard)
        r.init_rng(seed)
        ms = r.render(threads)
        assert ms > 0 or r.local_rows == 0
        return r.read_framebuffer()


def _render_stats(rt, prec, scene_id, W, H, S, B):
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, W, H, S, B)); r.set_scene(rt.build_scene(scene_id, prec)); r.init_rng(1227)
        r.render(0)
        return r.stats()


def _oracle(oracle, rt, prec, scene_id, W, H, S, B, seed=1227, rows=None):
    sc = compact(oracle.build_scene(scene_id, prec))
    cam = rt.camera(prec, W, H, S, B)
    if rows is None:
        return oracle.render(prec, sc, cam, seed)
    return oracle.render(prec, sc, cam, seed, rows[0], rows[1])


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------------------
def test_native_library_is_what_runs(rt):
    rt.load_host_library()
    with rt.Renderer(0, 32) as r:
        assert r._lib.rtiow_abi_version() == rt.ABI_VERSION
    maps = open("/proc/self/maps").read()
    assert "librtiow_hip.so" in maps and "librtiow_host.so" in maps
    # the product library carries no test hooks (include/rtiow_debug.h lives in librtiow_hip_debug.so only)
    with rt.Renderer(0, 32) as r:
        assert not hasattr(r._lib, "rtiow_debug_ops")
        with pytest.raises(rt.RtiowError):
            r.debug_read_rng()


def test_device_arithmetic_is_ieee_like_the_host(rt, oracle):
    rng = np.random.default_rng(7)
    for prec, dt in ((32, np.float32), (64, np.float64)):
        n = 1 << 16
        mk = lambda: (rng.standard_normal(n) * 10.0 ** rng.uniform(-18, 18, n)).astype(dt)
        a, b, c = mk(), mk(), mk()
        # include denormal results / operands
        a[:64] = np.array(np.finfo(dt).tiny, dt) * rng.uniform(0.01, 4, 64).astype(dt)
        with rt.Renderer(0, prec, debug=True) as r, np.errstate(all="ignore"):
            assert _same_bits(r.debug_ops(0, a, b), (a / b).astype(dt))
            assert _same_bits(r.debug_ops(1, np.abs(a)), np.sqrt(np.abs(a)).astype(dt))
            fma = np.array([np.float64(x) * np.float64(y) + np.float64(z) for x, y, z in zip(a[:2048], b[:2048], c[:2048])])
            got = r.debug_ops(2, a[:2048], b[:2048], c[:2048])
            if prec == 32:   # double holds a float product exactly; one rounding left
                assert _same_bits(got, fma.astype(np.float32))
            # unfused a*b+c must NOT be contracted (-ffp-contract=off)
            assert _same_bits(r.debug_ops(4, a, b, c), ((a * b).astype(dt) + c).astype(dt))
    # u32 -> (0,1] float conversion, incl. the ends of the range
    xs = np.concatenate([np.array([0, 1, 2, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff], np.uint32),
                         rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)])
    with rt.Renderer(0, 32, debug=True) as r:
        got = r.debug_ops(3, xs.view(np.float32))
    want = (xs.astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)).astype(np.float32)
    assert _same_bits(got, want) and got.min() > 0 and got.max() <= 1.0


def test_rng_init_matches_curand_init_semantics(rt, oracle):
    # rtweekend.h:49: curand_init(1227, pixel_index, 0); also under sharding (GLOBAL index)
    for W, H, shard in [(64, 40, None), (37, 19, None), (48, 40, (1, 3, 8)), (33, 21, (2, 4, 4))]:
        with rt.Renderer(0, 32, debug=True) as r:
            r.set_camera(rt.camera(32, W, H, 1, 1))
            if shard:
                r.set_shard(*shard)
            r.init_rng(1227)
            rows = r.local_row_map()
            got = r.debug_read_rng()
        seqs = (rows[:, None].astype(np.int64) * W + np.arange(W)[None, :]).ravel()
        assert np.array_equal(got, oracle.xorwow_states(1227, seqs))
    with rt.Renderer(0, 32, debug=True) as r:          # another seed, high subsequence bits
        r.set_camera(rt.camera(32, 2048, 1100, 1, 1))
        r.set_shard(7, 8, 8)
        r.init_rng(0x1234567890ABCDEF)
        rows = r.local_row_map()
        got = r.debug_read_rng().reshape(len(rows), 2048, 6)
    for (k, i) in [(0, 0), (5, 17), (len(rows) - 1, 2047)]:
        st = oracle.xorwow_init(0x1234567890ABCDEF, int(rows[k]) * 2048 + i, 0)
        assert np.array_equal(got[k, i], st)


def test_render_matches_committed_golden_images(rt, golden_dir):
    from tests.golden.make_golden import CUDA_SEM_CONFIGS
    for name, prec, sid, W, H, S, B in CUDA_SEM_CONFIGS:
        gold = np.load(os.path.join(golden_dir, name + ".npy"))
        assert _same_bits(_render(rt, prec, sid, W, H, S, B), gold), name


@pytest.mark.parametrize("prec,scene_id,W,H,S,B", [
    (32, 1, 320, 192, 10, 25),      # BASELINE configs[1]
    (32, 3, 320, 192, 10, 25),
    (32, 2, 160, 96, 6, 50),
    (64, 3, 160, 96, 4, 25),
    (64, 1, 96, 64, 2, 50),
    (32, 3, 101, 67, 3, 8),         # ragged: not a multiple of any tile
    (32, 3, 1, 1, 5, 5),
    (32, 3, 7, 3, 1, 1),
    (32, 3, 64, 8, 7, 0),           # zero bounces: ray_color returns black at once
    (64, 2, 33, 9, 2, 3),
    (32, 3, 128, 72, 64, 12),       # two-phase sorted schedule: 4 ranking samples + 60
    (64, 3, 96, 48, 24, 8),         # two-phase, 2 ranking samples, fp64 state carried between phases
    (32, 1, 96, 64, 24, 50),
    (32, 3, 131, 67, 70, 6),        # two-phase with ragged pools (npix not a multiple of 64)
])
def test_render_bit_exact_vs_oracle(rt, oracle, prec, scene_id, W, H, S, B):
    want, stats = _oracle(oracle, rt, prec, scene_id, W, H, S, B)
    for sched in (rt.SCHED_SORTED, rt.SCHED_PERSISTENT, rt.SCHED_STATIC):
        got = _render(rt, prec, scene_id, W, H, S, B, sched=sched)
        assert _same_bits(got, want), sched
    assert np.isfinite(got).all()


def test_block_shapes_and_scene_sources_give_the_same_image(rt, oracle):
    want, _ = _oracle(oracle, rt, 32, 3, 100, 60, 3, 12)
    for threads in (0, 1, 4, 8, 16, 32):
        for source in (rt.SCENE_GRID, rt.SCENE_LDS, rt.SCENE_SCALAR, rt.SCENE_LDS_EXACT):
            for sched, wps in ((rt.SCHED_SORTED, 0), (rt.SCHED_PERSISTENT, 0), (rt.SCHED_PERSISTENT, 1), (rt.SCHED_STATIC, 0)):
                got = _render(rt, 32, 3, 100, 60, 3, 12, threads, source, sched=sched, wps=wps)
                assert _same_bits(got, want), (threads, source, sched, wps)
    want64, _ = _oracle(oracle, rt, 64, 3, 50, 30, 2, 12)
    for threads in (0, 8, 16):
        assert _same_bits(_render(rt, 64, 3, 50, 30, 2, 12, threads, rt.SCENE_SCALAR), want64)


def test_scene_larger_than_lds_falls_back_to_scalar_loads(rt, oracle):
    """6000 spheres need 192 KB of fp32 tables: more than a CU's LDS.  The default source then reads
    the tables through the scalar cache (stats say so) and the image still equals the oracle's."""
    rng = np.random.default_rng(7)
    n = 6000
    base = compact(oracle.build_scene(3, 32))
    cr = np.zeros((n, 4), np.float32); af = np.zeros((n, 4), np.float32)
    cr[0] = base["center_radius"][0]; af[0] = base["albedo_fuzz"][0]                  # the ground
    cr[1:, 0] = rng.uniform(-40, 40, n - 1); cr[1:, 2] = rng.uniform(-40, 40, n - 1); cr[1:, 1] = 0.2; cr[1:, 3] = 0.2
    af[1:, :3] = rng.uniform(0.1, 0.9, (n - 1, 3)); af[1:, 3] = rng.uniform(0, 0.5, n - 1)
    ty = rng.choice([0, 1, 2], n, p=[0.8, 0.15, 0.05]).astype(np.int32); ty[0] = 0
    scene = {"center_radius": cr, "albedo_fuzz": af, "refraction_index": np.full(n, 1.5, np.float32), "type": ty,
             "valid": np.ones(n, np.int32)}
    W, H, S, B = 48, 32, 2, 8
    cam = rt.camera(32, W, H, S, B)
    want, _ = oracle.render(32, scene, cam, 1227)
    for sched in (rt.SCHED_SORTED, rt.SCHED_STATIC):
        with rt.Renderer(0, 32) as r:
            r.set_camera(cam); r.set_scene(scene); r.set_schedule(sched); r.init_rng(1227)
            r.render(0)
            assert r.stats()["scene_source"] == rt.SCENE_SCALAR and r.stats()["num_spheres"] == n
            assert _same_bits(r.read_framebuffer(), want), sched


def test_threads_shapes_only_the_static_schedule(rt):
    with rt.Renderer(0, 32) as r:
        r.set_camera(rt.camera(32, 96, 64, 2, 8)); r.set_scene(rt.build_scene(3, 32)); r.init_rng(1227)
        for T in (4, 24, 32):
            r.set_schedule(rt.SCHED_SORTED); r.render(T)
            assert (r.stats()["block_x"], r.stats()["block_y"]) == (16, 16)
            r.set_schedule(rt.SCHED_STATIC); r.render(T)
            assert (r.stats()["block_x"], r.stats()["block_y"]) == (T, T)


def test_per_launch_timing_and_segment_counts(rt):
    """The sorted schedule's two launches are timed and counted separately (bench.py's roofline is
    the main launch): event times nest inside the render time, segment counts add up."""
    W, H, S, B = 256, 144, 64, 20
    with rt.Renderer(0, 32) as r:
        r.set_camera(rt.camera(32, W, H, S, B)); r.set_scene(rt.build_scene(3, 32)); r.init_rng(1227)
        r.set_schedule(rt.SCHED_SORTED)
        ms = r.render(0)
        total = r.count_segments(0)
        st = r.stats()
        assert st["phases"] == 2 and st["prepass_samples"] == 3
        assert 0 < st["prepass_ms"] and 0 < st["main_ms"] and st["prepass_ms"] + st["main_ms"] <= ms * 1.001
        # finished pixels are staged in slot order and place_pixels_kernel writes the image (its own event pair, inside render_ms)
        assert st["staged_stores"] == 1 and 0 < st["place_ms"] < 0.5 and st["prepass_ms"] + st["main_ms"] + st["place_ms"] <= ms * 1.001
        assert st["scene_prepare_ms"] > 0            # screening table + grid plan of this scene, host time before the first start event
        assert st["segments_prepass"] + st["segments_main"] == total
        assert 0.02 < st["segments_prepass"] / total < 0.10            # 3 of 64 samples
        r.set_schedule(rt.SCHED_PERSISTENT)
        ms = r.render(0)
        assert r.count_segments(0) == total
        st = r.stats()
        assert st["phases"] == 1 and st["prepass_samples"] == 0 and st["segments_prepass"] == 0 and st["segments_main"] == total
        assert abs(st["main_ms"] - ms) < 1e-6 and st["prepass_ms"] == 0 and st["staged_stores"] == 0 and st["place_ms"] == 0


def test_segment_count_matches_oracle(rt, oracle):
    for prec, sid, W, H, S, B in [(32, 3, 96, 56, 5, 25), (32, 1, 64, 40, 3, 50), (64, 2, 40, 24, 4, 10), (32, 3, 128, 64, 30, 25)]:
        want, stats = _oracle(oracle, rt, prec, sid, W, H, S, B)
        with rt.Renderer(0, prec) as r:
            r.set_camera(rt.camera(prec, W, H, S, B)); r.set_scene(rt.build_scene(sid, prec)); r.init_rng(1227)
            assert r.count_segments(0) == stats[1]
            assert _same_bits(r.read_framebuffer(), want)


def test_sharded_render_assembles_to_the_single_gpu_image(rt, oracle):
    W, H, S, B = 96, 75, 3, 10
    want, _ = _oracle(oracle, rt, 32, 3, W, H, S, B)
    for nranks, strip in [(2, 8), (3, 8), (8, 8), (4, 16), (5, 1)]:
        full = np.zeros((H, W, 3), np.float32)
        total = 0
        for rank in range(nranks):
            part = _render(rt, 32, 3, W, H, S, B, threads=0, shard=(rank, nranks, strip))
            total += part.shape[0]
            rt.place_rows(full, part, rank, nranks, strip)
        assert total == H and _same_bits(full, want), (nranks, strip)


def test_external_framebuffer_and_torch_stream(rt, oracle):
    import torch
    from raytracingincuda_amd.distributed import StripGather
    W, H, S, B = 80, 48, 2, 8
    want, _ = _oracle(oracle, rt, 32, 3, W, H, S, B)
    g = StripGather(W, H, 0, 1, 8, torch.float32, "cuda:0")
    stream = torch.cuda.Stream()
    with rt.Renderer(0, 32) as r, torch.cuda.stream(stream):
        r.set_stream(stream.cuda_stream)
        r.set_camera(rt.camera(32, W, H, S, B)); r.set_scene(rt.build_scene(3, 32)); r.init_rng(1227)
        view = g.local_view()
        r.bind_framebuffer(view.data_ptr(), view.numel() * 4)
        r.render(0, sync=False)
        full = g.gather()
        stream.synchronize()
    assert _same_bits(full.cpu().numpy(), want)


def test_call_order_and_argument_errors(rt):
    with rt.Renderer(0, 32) as r:
        with pytest.raises(rt.RtiowError) as e:
            r.render(8)
        assert e.value.code == -2
        r.set_camera(rt.camera(32, 16, 16, 1, 1))
        r.set_scene(rt.build_scene(3, 32))
        with pytest.raises(rt.RtiowError):
            r.render(8)                    # RNG not initialised (main.cu:326-330 must come first)
        r.init_rng(1227)
        with pytest.raises(rt.RtiowError):
            r.render(33)
        with pytest.raises(rt.RtiowError):
            r.set_shard(3, 2, 8)
        r.render(8)
    with pytest.raises(rt.RtiowError):
        rt.Renderer(99, 32)
    with pytest.raises((rt.RtiowError, ValueError)):
        rt.Renderer(0, 16)


def test_executable_is_a_drop_in(rt, oracle, tmp_path):
    """stdout bytes, file name and P3 text of global-float-hip-raytrace (main.cu:342-343,
    349-358, 368-379, 397-398) on BASELINE configs[1] geometry (reduced spp for the oracle)."""
    exe = os.path.join(os.path.dirname(rt.lib_paths()["hip"]), "..", "bin", "global-float-hip-raytrace")
    r = subprocess.run([exe, "--scene_id", "1", "--width=160", "--height", "96", "--samples", "4", "--bounces=25", "--threads", "8"],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert re.fullmatch(r" *\d+\.\d{8}, *\d+\.\d{8}\n", r.stdout) and len(r.stdout) == 32
    render_ms, e2e_ms = (float(x) for x in r.stdout.split(","))
    assert 0 < render_ms < e2e_ms
    name = "global_float_scene1_160x96_4samples_25bounces_8threadsPerBlockRow.ppm"
    assert os.listdir(str(tmp_path)) == [name]
    want, _ = _oracle(oracle, rt, 32, 1, 160, 96, 4, 25)
    assert open(str(tmp_path / name), "rb").read() == rt.format_ppm(want)
    # optional binary output: same file name, P6, same levels (ppm_diff of the two is all zeros)
    sub = tmp_path / "p6"; sub.mkdir()
    r6 = subprocess.run([exe, "--scene_id", "1", "--width=160", "--height", "96", "--samples", "4", "--bounces=25", "--threads", "8",
                         "--ppm_format", "p6"], capture_output=True, text=True, cwd=str(sub))
    assert r6.returncode == 0, r6.stderr
    raw = open(str(sub / name), "rb").read()
    assert raw.startswith(b"P6\n160 96\n255\n") and len(raw) == 14 + 160 * 96 * 3
    levels = np.array(rt.format_ppm(want).split()[4:], dtype=np.uint8)
    assert np.array_equal(np.frombuffer(raw[14:], np.uint8), levels)
    (tmp_path / "p6" / name).unlink(); sub.rmdir()
    # --schedule static = the reference's launch geometry (one lane per pixel of a --threads^2 block): same file
    sub = tmp_path / "static"; sub.mkdir()
    rs = subprocess.run([exe, "--scene_id", "1", "--width=160", "--height", "96", "--samples", "4", "--bounces=25", "--threads", "8",
                         "--schedule", "static"], capture_output=True, text=True, cwd=str(sub))
    assert rs.returncode == 0, rs.stderr
    assert open(str(sub / name), "rb").read() == rt.format_ppm(want)
    (sub / name).unlink(); sub.rmdir()
    # --stats: one JSON line on stderr, stdout untouched; since round 5 with the launches' own event times and the effective shader clock the
    # launches stamped themselves (rtiow_stats.main_clock_mhz: what tells a 1.7 GHz render from a 2.3 GHz one, profiles/r05/cold_process_study.md)
    sub = tmp_path / "stats"; sub.mkdir()
    rs = subprocess.run([exe, "--scene_id", "3", "--width=640", "--height", "360", "--samples", "64", "--bounces=50", "--threads", "8", "--stats", "--ppm_format", "p6"],
                        capture_output=True, text=True, cwd=str(sub))
    assert rs.returncode == 0, rs.stderr
    assert re.fullmatch(r" *\d+\.\d{8}, *\d+\.\d{8}\n", rs.stdout)
    import json
    st = json.loads([l for l in rs.stderr.splitlines() if l.startswith("{")][-1])
    assert st["launch_ms"]["main"] > 0 and st["launch_ms"]["prepass"] > 0 and abs(sum(st["launch_ms"].values()) - st["render_ms"]) < 0.3
    assert 500 < st["clock_mhz"]["main"] < 3500 and 500 < st["clock_mhz"]["prepass"] < 3500 and st["clock_mhz"]["nominal"] > 0
    assert 0 < st["clock_mhz"]["main_wave0_ms"] <= st["launch_ms"]["main"] * 1.05
    for f in os.listdir(str(sub)): (sub / f).unlink()
    sub.rmdir()
    # the same figures through the C-ABI
    with rt.Renderer(0, 32) as r:
        r.set_camera(rt.camera(32, 640, 360, 64, 50)); r.set_scene(rt.build_scene(3, 32)); r.init_rng(1227)
        r.render(0)
        s2 = r.stats()
        assert 500 < s2["main_clock_mhz"] < 3500 and 500 < s2["prepass_clock_mhz"] < 3500 and 0 < s2["main_wave0_ms"] <= s2["main_ms"] * 1.05
        r.set_schedule(rt.SCHED_STATIC); r.render(8)
        assert r.stats()["main_clock_mhz"] == 0          # the static schedule has no persistent wave to stamp
    # defaults (main.cu:45-54) and the double variant's name (GlobalDouble main.cu:351)
    exe64 = exe.replace("float", "double")
    r = subprocess.run([exe64, "--scene_id=3", "--samples=1", "--bounces=2"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0
    assert os.path.exists(str(tmp_path / "global_double_scene3_320x192_1samples_2bounces_8threadsPerBlockRow.ppm"))


def test_benchmark_harness_csv_round_trip(rt, tmp_path):
    """tools/hip_benchmark.sh (global_float_benchmark.sh's loop) -> reference CSV schema -> bin/csv_avg."""
    from tests.conftest import ROOT
    csv = str(tmp_path / "bench.csv")
    env = dict(os.environ, SCENE_IDS="3", WIDTHS="64 96", HEIGHTS="40 56", SAMPLES="2", BOUNCES="5", THREADS="8 16", RUNS="2")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "hip_benchmark.sh"), "float", csv], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = open(csv).read().splitlines()
    assert lines[0] == "scene_id,width,height,samples,bounces,threads,run,render_only_time_ms,end_to_end_time_ms"
    assert len(lines) == 1 + 2 * 2 * 2
    for line in lines[1:]:
        assert re.fullmatch(r"3,(64,40|96,56),2,5,(8|16),[12], *\d+\.\d{8}, *\d+\.\d{8}", line), line
    avg = str(tmp_path / "avg.csv")
    exe = os.path.join(os.path.dirname(rt.lib_paths()["hip"]), "..", "bin", "csv_avg")
    assert subprocess.run([exe, csv, avg], capture_output=True).returncode == 0
    assert len(open(avg).read().splitlines()) == 1 + 4
    # the same loop with a JSON line per run next to the CSV, and the BASELINE.json preset
    side = str(tmp_path / "stats.jsonl")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "hip_benchmark.sh"), "float", csv], env=dict(env, STATS_JSONL=side, RUNS="1"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(l) for l in open(side)]
    assert len(rows) == 4 and all(row["stats"]["mrays_per_s"] > 0 and row["stats"]["wall_ms"]["end_to_end"] > 0 for row in rows)
    assert [(row["width"], row["threads"]) for row in rows] == [(64, 8), (96, 8), (64, 16), (96, 16)]
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "hip_benchmark.sh"), "float", csv], env=dict(os.environ, BASELINE_CONFIGS="1", RUNS="1", STATS_JSONL=side), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [l.split(",")[:5] for l in open(csv).read().splitlines()[1:]] == [["1", "320", "192", "10", "25"], ["3", "1280", "720", "100", "50"], ["3", "1920", "1080", "100", "50"]]
    assert [json.loads(l)["stats"]["solo_waves"] for l in open(side)] == [0, 256, 0]


def _custom(rt, prec, scene, W, H, S, B, source, sched=2):
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, W, H, S, B)); r.set_scene(scene); r.set_scene_source(source); r.set_schedule(sched)
        r.init_rng(1227)
        r.render(0)
        return r.read_framebuffer(), r.stats()


def test_grid_walk_equals_exact_loop_on_the_reference_scenes(rt):
    """RTIOW_SCENE_GRID (default: per-lane walk over a uniform grid of the small spheres + direct
    list) vs the reference's 12-operation test on every sphere, bit for bit, on mid-size frames of
    all three scenes in both precisions; the stats must say the grid was really used."""
    for prec, scene_id, W, H, S in ((32, 3, 1280, 720, 20), (32, 1, 1280, 720, 20), (32, 2, 640, 360, 20),
                                    (64, 3, 640, 360, 20), (64, 1, 640, 360, 10)):
        sc = rt.build_scene(scene_id, prec)
        a, st = _custom(rt, prec, sc, W, H, S, 50, rt.SCENE_GRID)
        assert st["scene_source"] == rt.SCENE_GRID, (prec, scene_id)
        # the ground and the three unit spheres are the direct list, every small sphere sits in a cell
        assert st["grid_direct"] == 4 and st["grid_registered"] == st["num_spheres"] - 4 and 0.9 < st["grid_cell"] < 1.3, st
        lo, hi = {1: (21, 25), 2: (6, 9), 3: (11, 14)}[scene_id]                  # the reference's own 22 / 6 / 11-cell grids, plus margins
        assert lo <= st["grid_nx"] <= hi and lo <= st["grid_nz"] <= hi, st
        b, st_b = _custom(rt, prec, sc, W, H, S, 50, rt.SCENE_LDS_EXACT, sched=rt.SCHED_STATIC)
        assert st_b["grid_nx"] == 0 and st_b["grid_direct"] == 0
        assert st_b["scene_source"] == rt.SCENE_LDS_EXACT
        assert _same_bits(a, b), (prec, scene_id)
        c, _ = _custom(rt, prec, sc, W, H, S, 50, rt.SCENE_LDS)
        assert _same_bits(a, c), (prec, scene_id)


def _random_field(rng, prec, n, x_range, z_range, radius, y_of, ground=True, big=()):
    """A scene of n small spheres scattered over a rectangle, optionally with the ground and a few big ones."""
    dt = np.float32 if prec == 32 else np.float64
    rows = []
    if ground:
        rows.append((0.0, -1000.0, 0.0, 1000.0))
    rows += list(big)
    for _ in range(n):
        r = radius(rng)
        rows.append((rng.uniform(*x_range), y_of(rng, r), rng.uniform(*z_range), r))
    cr = np.array(rows, dt)
    m = len(rows)
    af = np.zeros((m, 4), dt)
    af[:, :3] = rng.uniform(0.1, 0.9, (m, 3)); af[:, 3] = rng.uniform(0, 0.5, m)
    ty = rng.choice([0, 1, 2], m, p=[0.6, 0.2, 0.2]).astype(np.int32)
    if ground:
        ty[0] = 0
    return {"center_radius": cr, "albedo_fuzz": af, "refraction_index": np.full(m, 1.5, dt), "type": ty, "valid": np.ones(m, np.int32)}


@pytest.mark.parametrize("case", ["dense_clusters", "mixed_radii_and_heights", "far_from_the_camera", "tiny_spheres", "stacked_no_ground", "touching_pairs"])
def test_grid_walk_equals_exact_loop_on_random_scenes(rt, oracle, case):
    """Scenes the grid was not tuned for: full cells that overflow into the direct list, radii near
    half a cell, spheres at many heights, a field far away from the camera (rays whose origin lies
    beyond the registration margin's reach: the per-ray clip and the brute-force fallback), tiny
    spheres (registration margin >> radius), no ground, and touching pairs (equal roots: the
    lower index must win, hittable.h:54)."""
    rng = np.random.default_rng({"dense_clusters": 1, "mixed_radii_and_heights": 2, "far_from_the_camera": 3, "tiny_spheres": 4,
                                 "stacked_no_ground": 5, "touching_pairs": 6}[case])
    for prec in (32, 64):
        if case == "dense_clusters":
            sc = _random_field(rng, prec, 300, (-6, 6), (-6, 6), lambda g: 0.2, lambda g, r: r)
        elif case == "mixed_radii_and_heights":
            sc = _random_field(rng, prec, 200, (-10, 8), (-10, 8), lambda g: g.choice([0.1, 0.2, 0.3, 0.45]), lambda g, r: g.uniform(r, 2.0),
                               big=[(0.0, 1.0, 0.0, 1.0), (4.0, 1.0, 0.0, 1.0)])
        elif case == "far_from_the_camera":
            sc = _random_field(rng, prec, 200, (-130, -105), (-32, -18), lambda g: g.uniform(0.1, 0.25), lambda g, r: r)   # 10x its own size away: camera rays are 'far'
        elif case == "tiny_spheres":
            sc = _random_field(rng, prec, 250, (-8, 8), (-8, 8), lambda g: g.choice([0.002, 0.01, 0.05]), lambda g, r: g.uniform(0.0, 1.5))
        elif case == "stacked_no_ground":
            sc = _random_field(rng, prec, 150, (-4, 6), (-4, 6), lambda g: 0.25, lambda g, r: g.uniform(-3, 4), ground=False)
        else:
            sc = _random_field(rng, prec, 240, (-12, 12), (-12, 12), lambda g: 0.2, lambda g, r: r)
            twin = sc["center_radius"][1:41].copy()
            sc["center_radius"][201:241] = twin                                    # 40 exact duplicates at higher indices
            sc["center_radius"][201:221, 0] += np.float32(0.4) if prec == 32 else 0.4   # 20 of them shifted to touch their twin
        W, H, S, B = 320, 192, 6, 20
        a, st = _custom(rt, prec, sc, W, H, S, B, rt.SCENE_GRID)
        assert st["scene_source"] == rt.SCENE_GRID, (case, prec)
        b, _ = _custom(rt, prec, sc, W, H, S, B, rt.SCENE_LDS_EXACT, sched=rt.SCHED_STATIC)
        assert _same_bits(a, b), (case, prec)
        want, _ = oracle.render(prec, sc, rt.camera(prec, 96, 56, 4, 12), 1227)
        got, _ = _custom(rt, prec, sc, 96, 56, 4, 12, rt.SCENE_GRID)
        assert _same_bits(got, want), (case, prec)


@pytest.mark.parametrize("seed", range(10))
def test_grid_walk_equals_exact_loop_random_sweep(rt, seed):
    """Ten more scenes drawn at random (count, extent, radius law, height spread, with or without the
    ground and big spheres, scene centre on or off the camera axis): grid walk == exact loop, bit for
    bit.  Whether a scene gets a grid at all is the builder's choice; at least the common ones must."""
    rng = np.random.default_rng(1000 + seed)
    prec = 32 if seed % 2 == 0 else 64
    n = int(rng.integers(60, 700))
    half = float(rng.uniform(3, 25))
    cx, cz = (0.0, 0.0) if seed % 3 else (float(rng.uniform(-30, 5)), float(rng.uniform(-20, 10)))
    rlaw = [lambda g: 0.2, lambda g: float(g.uniform(0.05, 0.5)), lambda g: float(g.choice([0.1, 0.35])), lambda g: float(np.exp(g.uniform(np.log(0.02), np.log(0.6))))][seed % 4]
    yspread = float(rng.choice([0.0, 0.5, 3.0]))
    big = [(cx, 1.0, cz, 1.0), (cx - 4.0, 1.0, cz, 1.0)] if seed % 2 else []
    sc = _random_field(rng, prec, n, (cx - half, cx + half), (cz - half, cz + half), rlaw, lambda g, r: r + float(g.uniform(0, yspread)) if yspread else r,
                       ground=seed % 5 != 4, big=big)
    W, H, S, B = 200, 120, 4, 16
    a, st = _custom(rt, prec, sc, W, H, S, B, rt.SCENE_GRID)
    b, _ = _custom(rt, prec, sc, W, H, S, B, rt.SCENE_LDS_EXACT, sched=rt.SCHED_STATIC)
    assert _same_bits(a, b), (seed, st)
    c, _ = _custom(rt, prec, sc, W, H, S, B, rt.SCENE_GRID, sched=rt.SCHED_STATIC)
    assert _same_bits(c, b), (seed, st)
    print("seed %d: n=%d source=%d grid %dx%d registered %d direct %d" % (seed, n, st["scene_source"], st["grid_nx"], st["grid_nz"], st["grid_registered"], st["grid_direct"]))
    if seed in (0, 2, 3, 5, 6, 7, 8):            # the other three are too dense for 4-entry cells and keep the screened loop
        assert st["scene_source"] == rt.SCENE_GRID and st["grid_registered"] >= 16, (seed, st)


def _crafted_camera(rt, prec, W, H, S, B, center, direction, spread=0.0):
    """A camera whose primary rays all leave `center` along `direction` (pixel deltas `spread` x unit steps in the plane
    across it; 0 = every ray identical), no defocus: the degenerate rays a perspective view never produces exactly."""
    cam = rt.camera(prec, W, H, S, B)
    d = np.array(direction, np.float64)
    c = np.array(center, np.float64)
    u = np.cross(d, [0.0, 1.0, 0.0]) if abs(d[1]) < 0.9 * np.linalg.norm(d) else np.cross(d, [1.0, 0.0, 0.0])
    u = u / np.linalg.norm(u) * spread
    v = np.cross(d, u); v = v / (np.linalg.norm(v) or 1.0) * spread
    for k in range(3):
        cam.center[k] = c[k]; cam.pixel00_loc[k] = c[k] + d[k] - (W // 2) * u[k] - (H // 2) * v[k]
        cam.pixel_delta_u[k] = u[k]; cam.pixel_delta_v[k] = v[k]
        cam.defocus_disk_u[k] = 0.0; cam.defocus_disk_v[k] = 0.0
    cam.defocus_angle = 0.0
    return cam


def _render_cam(rt, prec, scene, cam, source, sched=2):
    with rt.Renderer(0, prec) as r:
        r.set_camera(cam); r.set_scene(scene); r.set_scene_source(source); r.set_schedule(sched); r.init_rng(1227)
        r.render(0)
        return r.read_framebuffer(), r.stats()


@pytest.mark.parametrize("prec", [32, 64])
def test_grid_walk_on_degenerate_rays(rt, oracle, prec):
    """Rays a perspective camera never produces exactly: parallel to a grid axis (zero direction components: the
    clip's parallel case, a DDA that never steps on one axis), straight down and up, exactly diagonal (both
    boundary crossings tie at every step), starting exactly ON a cell boundary and running along it, starting
    inside a sphere, and far outside the scene looking in.  Every pixel gets the same primary ray (zero pixel
    deltas, no defocus) and its own random stream, so the bounces differ.  Grid == exact loop, and == oracle."""
    from tests.test_grid_plan import _plan
    sc = rt.build_scene(3, prec)
    keep = sc["valid"] != 0
    pl = _plan(rt, sc["center_radius"][keep].astype(np.float64))
    assert pl["usable"]
    x0, z0, cell = float(np.float32(pl["x0"])), float(np.float32(pl["z0"])), float(np.float32(pl["cell"]))
    first = sc["center_radius"][keep][1].astype(np.float64)                  # a small sphere
    W, H, S, B = 32, 8, 6, 12
    cases = [((20.0, 0.2, first[2]), (-1.0, 0.0, 0.0)),                       # along -x through a row of spheres, inside the slab
             ((first[0], 0.2, -30.0), (0.0, 0.0, 1.0)),                       # along +z
             ((first[0], 5.0, first[2]), (0.0, -1.0, 0.0)),                   # straight down onto a sphere
             ((first[0], 0.2, first[2]), (0.0, 1.0, 0.0)),                    # straight up from a sphere's centre (origin inside it)
             ((-12.0, 0.2, -12.0), (1.0, 0.0, 1.0)),                          # exactly diagonal: tx == tz at every cell
             ((x0 + 3 * cell, 0.2, 10.0), (0.0, 0.0, -1.0)),                  # on a cell boundary, along it
             ((x0 + 3 * cell, 0.25, z0 + 2 * cell), (1.0, 0.0, -1.0)),        # from a cell corner, diagonally
             ((300.0, 0.2, -5.5), (-1.0, 0.0, 0.0)),                          # a far origin skimming the field (fallback loop)
             ((300.0, 40.0, -5.5), (-1.0, 0.0, 0.0)),                         # a far origin passing over it (no walk, no fallback)
             ((-5.5, 0.2, -5.5), (1e-30, -1.0, 1e-30))]                       # denormal-small components
    for center, direction in cases:
        cam = _crafted_camera(rt, prec, W, H, S, B, center, direction)
        a, st = _render_cam(rt, prec, sc, cam, rt.SCENE_GRID)
        assert st["scene_source"] == rt.SCENE_GRID
        b, _ = _render_cam(rt, prec, sc, cam, rt.SCENE_LDS_EXACT, sched=rt.SCHED_STATIC)
        assert _same_bits(a, b), (center, direction)
        want, _ = oracle.render(prec, compact(sc), cam, 1227)
        assert _same_bits(a, want), (center, direction)
    # the same views with a little spread (nearly axis-parallel bundles)
    for center, direction in cases[:5]:
        cam = _crafted_camera(rt, prec, 64, 32, 4, 12, center, direction, spread=1e-4)
        a, _ = _render_cam(rt, prec, sc, cam, rt.SCENE_GRID)
        b, _ = _render_cam(rt, prec, sc, cam, rt.SCENE_LDS_EXACT, sched=rt.SCHED_STATIC)
        assert _same_bits(a, b), (center, direction, "spread")


@pytest.mark.parametrize("S,B,defocus", [(3, 6, True), (2, 8, False), (1, 1, True), (24, 5, True)])
def test_rotated_fp64_trip_matches_the_oracle(rt, oracle, S, B, defocus):
    """The fp64 kernels run a ROTATED trip (one rejection loop for lens samples and unit vectors) while the launch fills
    every lane -- frames of at least 64 pixels per resident wave, which the small parametrised frames above are not.  640 x 448 takes it
    (4 480 pools for 4 096 resident waves); with and without a lens (no lens: the loop serves unit vectors only and a new sample starts
    without a draw), one sample of one segment (every lane starts a sample in every trip), and a two-phase frame (prepass and main launch
    both rotated, the state parked between them)."""
    W, H = 640, 448
    sc = rt.build_scene(3, 64)
    cam = rt.camera(64, W, H, S, B)
    if not defocus:
        for k in range(3):
            cam.defocus_disk_u[k] = 0.0; cam.defocus_disk_v[k] = 0.0
        cam.defocus_angle = 0.0
    got, st = _render_cam(rt, 64, sc, cam, rt.SCENE_GRID)
    assert W * H // 64 >= 256 * 4 * 4        # at least one 64-pixel pool per resident fp64 wave (four per SIMD): every lane takes pixels
    want, _ = oracle.render(64, compact(sc), cam, 1227)
    assert _same_bits(got, want), (S, B, defocus)
    again, _ = _render_cam(rt, 64, sc, cam, rt.SCENE_GRID, sched=rt.SCHED_STATIC)       # the reference's own launch geometry: no persistent loop at all
    assert _same_bits(again, want)


@pytest.mark.parametrize("prec", [32, 64])
def test_render_on_the_material_lattice(rt, oracle, prec):
    """The material lattice (tests/lattice.py: fuzz 0 ... 4 unclamped, refraction indices 1e-3 ... 1e3 with 1 and 2/3 among them, albedo
    components 0 ... 1.5 and a denormal, radii 1e-3 ... 1000, two hollow glass spheres of negative inner radius, a glass sphere around the
    camera) renders to the oracle's bits from all three scene sources under the static and the sorted schedule."""
    from tests.lattice import lattice_scene
    sc = lattice_scene(prec)
    assert 40 <= len(sc["type"]) <= 60
    cam = rt.camera(prec, 96, 56, 4, 12)
    want, _ = oracle.render(prec, sc, cam, 1227)
    assert np.isfinite(want).all() and float(np.asarray(want, np.float64).std()) > 0.05
    for source in (rt.SCENE_GRID, rt.SCENE_LDS, rt.SCENE_LDS_EXACT):
        for sched in (rt.SCHED_STATIC, rt.SCHED_SORTED):
            got, _ = _render_cam(rt, prec, sc, cam, source, sched=sched)
            assert _same_bits(got, want), (prec, source, sched, int((got != want).any(axis=2).sum()))


def test_rotated_fp64_trip_on_the_material_lattice(rt, oracle):
    """The lattice at 640 x 448 in fp64, which takes the rotated trip (test_rotated_fp64_trip_matches_the_oracle), against oracle rows
    from the top, the middle and the bottom of the frame."""
    from tests.lattice import lattice_scene
    W, H = 640, 448
    sc = lattice_scene(64)
    cam = rt.camera(64, W, H, 2, 12)
    got, _ = _render_cam(rt, 64, sc, cam, rt.SCENE_GRID)
    for row0 in (0, 216, 300, 440):
        want, _ = oracle.render(64, sc, cam, 1227, row0=row0, row1=row0 + 8)
        assert _same_bits(got[row0:row0 + 8], want), row0


def test_primary_ray_normalisation_paths_match_the_oracle(rt, oracle):
    """gen_primary takes 1/sqrt(|D|^2) through the short in-range sequence when the host can bound |D| for the
    whole frame (primary_rays_in_range) and through the compiler's full IEEE sequence otherwise.  The same view
    with the pixel plane 2^-35 ... 2^35 away from the lens (the rays are the same lines; |D|^2 runs from 2^-70 to
    2^70 and out of the range the host accepts at both ends) must give the oracle's bits on either path."""
    sc = rt.build_scene(3, 32)
    W, H, S, B = 48, 24, 3, 8
    for log2_len in (-35, -25, -8, 0, 9, 25, 35):
        cam = _crafted_camera(rt, 32, W, H, S, B, (13.0, 2.0, 3.0), tuple(np.array([-13.0, -2.0, -3.0]) / 13.49 * 2.0 ** log2_len),
                              spread=2.0 ** log2_len * 0.01)
        a, _ = _render_cam(rt, 32, sc, cam, rt.SCENE_GRID)
        want, _ = oracle.render(32, compact(sc), cam, 1227)
        assert _same_bits(a, want), log2_len


@pytest.mark.parametrize("prec", [32, 64])
def test_short_ieee_forms_on_a_far_translated_scene(rt, oracle, prec):
    """The root quotients use one reciprocal per segment only while the host can vouch for the operand ranges
    (every coordinate of spheres and lens below 2^18).  Scene 3 and its camera moved by
    1e5 (inside that bound: short forms, on coordinates where fp32 has lost five digits) and by 3e5 (outside:
    the compiler's sequences) must both give the oracle's bits."""
    W, H, S, B = 64, 40, 3, 10
    for shift in (1.0e5, 3.0e5):
        sc = rt.build_scene(3, prec)
        off = np.array([shift, 0.0, -shift])
        sc["center_radius"][:, 0] += np.asarray(off[0], sc["center_radius"].dtype)
        sc["center_radius"][:, 2] += np.asarray(off[2], sc["center_radius"].dtype)
        cam = rt.camera(prec, W, H, S, B)
        for k in range(3):
            cam.center[k] += off[k]; cam.pixel00_loc[k] += off[k]
        a, _ = _render_cam(rt, prec, sc, cam, rt.SCENE_GRID)
        want, _ = oracle.render(prec, compact(sc), cam, 1227)
        assert _same_bits(a, want), (prec, shift)
        assert float(np.asarray(a, np.float64).std()) > 0.01           # a picture, not a constant


def _adversarial_rays(rng, cr, plan, n_each):
    """Ray families a render rarely or never produces, around the grid of `plan` (tests/test_grid_plan._plan)."""
    x0, z0, cell, nx, nz = plan["x0"], plan["z0"], plan["cell"], plan["nx"], plan["nz"]
    xs, zs = (x0, x0 + nx * cell), (z0, z0 + nz * cell)
    def unit(n):
        v = rng.normal(size=(n, 3)); return v / np.linalg.norm(v, axis=1, keepdims=True)
    fam = []
    # a. anywhere in and around the field, any direction, any length
    o = np.column_stack([rng.uniform(xs[0] - 3, xs[1] + 3, n_each), rng.uniform(-0.5, 4, n_each), rng.uniform(zs[0] - 3, zs[1] + 3, n_each)])
    fam.append(np.hstack([o, unit(n_each) * np.exp(rng.uniform(-3, 3, (n_each, 1)))]))
    # b. from the ground plane, grazing
    o = np.column_stack([rng.uniform(xs[0] - 20, xs[1] + 20, n_each), rng.choice([0.0, 1e-4, -1e-4], n_each), rng.uniform(zs[0] - 20, zs[1] + 20, n_each)])
    d = unit(n_each); d[:, 1] = rng.choice([0.0, 1e-6, -1e-6, 1e-3, 0.02], n_each) * rng.choice([1, 1, 1, -1], n_each)
    fam.append(np.hstack([o, d]))
    # c. on cell boundaries and corners, axis-parallel, diagonal and random directions
    o = np.column_stack([x0 + rng.integers(0, nx + 1, n_each) * cell, rng.uniform(0, 0.45, n_each), z0 + rng.integers(0, nz + 1, n_each) * cell])
    o[: n_each // 2, 2] = rng.uniform(zs[0], zs[1], n_each // 2)                        # half of them on an x boundary only
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [1, 0, 1], [1, 0, -1], [-1, 0, 1], [-1, 0, -1], [0, 1, 0], [0, -1, 0]], np.float64)
    d = np.where(rng.random((n_each, 1)) < 0.6, axes[rng.integers(0, len(axes), n_each)], unit(n_each))
    fam.append(np.hstack([o, d]))
    # d. far origins: aimed at the field (the brute-force fallback), past it, and away from it
    far = unit(n_each) * np.exp(rng.uniform(np.log(50), np.log(5000), (n_each, 1))); far[:, 1] = np.abs(far[:, 1]) * rng.choice([1.0, 1e-3, 0.0], n_each)
    centre = np.array([(xs[0] + xs[1]) / 2, 0.2, (zs[0] + zs[1]) / 2])
    tgt = centre + np.column_stack([rng.uniform(-1, 1, n_each) * (xs[1] - xs[0]), rng.choice([0.0, 0.2, 3.0, 50.0], n_each), rng.uniform(-1, 1, n_each) * (zs[1] - zs[0])])
    fam.append(np.hstack([centre + far, (tgt - centre - far) * rng.choice([1.0, -1.0], (n_each, 1), p=[0.85, 0.15])]))
    # e. on sphere surfaces: outward, inward, tangent (self-intersection against tmin)
    k = rng.integers(0, len(cr), n_each)
    nrm = unit(n_each)
    o = cr[k, :3] + nrm * cr[k, 3:4] * rng.choice([1.0, 1.0 + 1e-6, 1.0 - 1e-6, 0.5], (n_each, 1))
    tang = np.cross(nrm, unit(n_each))
    d = np.where(rng.random((n_each, 1)) < 0.4, tang, nrm * rng.choice([1.0, -1.0], (n_each, 1)) + 0.3 * unit(n_each))
    fam.append(np.hstack([o, d]))
    # f. degenerate numbers
    r = fam[0][: n_each // 4].copy()
    r[:, 3:] *= rng.choice([1e-25, 1e-12, 1e12, 1e25], (len(r), 1))
    z = fam[0][: 64].copy(); z[:, 3:] = 0.0
    bad = fam[0][: 64].copy(); bad[::2, 3] = np.nan; bad[1::4, 0] = np.inf; bad[3::4, 4] = -np.inf
    fam += [r, z, bad]
    return np.vstack(fam)


@pytest.mark.parametrize("prec,scene_id", [(32, 3), (32, 1), (64, 3), (64, 1), (32, 2)])
def test_hit_world_ray_by_ray_grid_vs_exact(rt, oracle, prec, scene_id):
    """hit_world alone (rtiow_debug_hit_world) on ~1.3 million adversarial rays: the grid walk returns the same
    (root bits, sphere index) as the 12-operation loop over every sphere, ray by ray."""
    from tests.test_grid_plan import _plan
    sc = rt.build_scene(scene_id, prec)
    keep = sc["valid"] != 0
    cr = sc["center_radius"][keep].astype(np.float64)
    pl = _plan(rt, cr)
    assert pl["usable"]
    rays = _adversarial_rays(np.random.default_rng(100 * scene_id + prec), cr, pl, 200000)
    dt = np.float32 if prec == 32 else np.float64
    with np.errstate(over="ignore", invalid="ignore"):
        rays = rays.astype(dt)
    out = {}
    for source in (rt.SCENE_GRID, rt.SCENE_LDS_EXACT, rt.SCENE_LDS):
        with rt.Renderer(0, prec, debug=True) as r:
            r.set_camera(rt.camera(prec, 64, 64, 1, 1)); r.set_scene(sc); r.set_scene_source(source)
            out[source] = r.debug_hit_world(rays)
            if source == rt.SCENE_GRID:
                assert r.stats()["scene_source"] == rt.SCENE_GRID
    t_ref, i_ref = out[rt.SCENE_LDS_EXACT]
    hit_frac = float((i_ref >= 0).mean())
    assert 0.2 < hit_frac < 0.95, hit_frac                                  # the families do hit things, and do miss
    for source in (rt.SCENE_GRID, rt.SCENE_LDS):
        t, i = out[source]
        bad = np.nonzero((i != i_ref) | (t.view(np.uint8).reshape(len(t), -1) != t_ref.view(np.uint8).reshape(len(t), -1)).any(axis=1))[0]
        assert len(bad) == 0, (source, len(bad), rays[bad[:5]], t[bad[:5]], t_ref[bad[:5]], i[bad[:5]], i_ref[bad[:5]])
    # and the oracle's in-order loop (hittable.h:80-98 restated on the CPU), ray by ray, on a slice of every family
    pick = np.arange(0, len(rays), 7)
    t_o, i_o = oracle.hit_world(prec, cr.astype(dt), rays[pick])
    bad = np.nonzero((i_o != i_ref[pick]) | (t_o.view(np.uint8).reshape(len(pick), -1) != t_ref[pick].view(np.uint8).reshape(len(pick), -1)).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), rays[pick][bad[:5]], t_o[bad[:5]], t_ref[pick][bad[:5]], i_o[bad[:5]], i_ref[pick][bad[:5]])


def test_screen_equals_exact_on_the_488_sphere_scene(rt):
    """Scene 1 at 1280x720x20: the screened loop (default) vs the exact loop, bit for bit."""
    a = _render(rt, 32, 1, 1280, 720, 20, 50, threads=0, source=rt.SCENE_LDS)
    b = _render(rt, 32, 1, 1280, 720, 20, 50, threads=0, source=rt.SCENE_LDS_EXACT)
    assert _same_bits(a, b)


def test_screen_equals_exact_fp64(rt, oracle):
    """fp64 screen vs the exact loop on a mid-size frame, and both against oracle rows."""
    W, H, S, B = 640, 360, 20, 50
    a = _render(rt, 64, 3, W, H, S, B, threads=0, source=rt.SCENE_LDS)
    b = _render(rt, 64, 3, W, H, S, B, threads=0, source=rt.SCENE_LDS_EXACT, sched=rt.SCHED_STATIC)
    assert _same_bits(a, b)
    want, _ = _oracle(oracle, rt, 64, 3, W, H, S, B, rows=(200, 202))
    assert _same_bits(a[200:202], want)
    # the fp64 kernel screens in packed fp32 (rays rounded to fp32 for the screen only): also on
    # the 488-sphere scene, whose centres lie up to 16 units from the recentring point
    a1 = _render(rt, 64, 1, 320, 192, 10, 25, threads=0, source=rt.SCENE_LDS)
    b1 = _render(rt, 64, 1, 320, 192, 10, 25, threads=0, source=rt.SCENE_LDS_EXACT, sched=rt.SCHED_STATIC)
    assert _same_bits(a1, b1)


def test_baseline_config3_1280x720(rt, oracle):
    """BASELINE configs[2]: scene 3, 1280x720, 100 spp, 50 bounces -- oracle rows + shard invariance."""
    W, H, S, B = 1280, 720, 100, 50
    a = _render(rt, 32, 3, W, H, S, B, threads=8)
    for row in (5, 400, 719):
        want, _ = _oracle(oracle, rt, 32, 3, W, H, S, B, rows=(row, row + 1))
        assert _same_bits(a[row:row + 1], want), row
    full = np.zeros_like(a)
    for rank in range(2):
        rt.place_rows(full, _render(rt, 32, 3, W, H, S, B, threads=0, shard=(rank, 2, 8)), rank, 2, 8)
    assert _same_bits(full, a)


def test_scene1_at_config3_and_config4_geometry_vs_oracle(rt, oracle):
    """"additionally run C3/C4 geometry on scene 1" (487 spheres, the only scene
    the reference published numbers for): oracle rows at 1280x720 and 1920x1080, 100 spp, 50 bounces."""
    for W, H, rows in ((1280, 720, (3, 377, 719)), (1920, 1080, (540, 1001))):
        a = _render(rt, 32, 1, W, H, 100, 50, threads=0)
        assert np.isfinite(a).all() and a.min() >= 0 and a.max() <= 1.0 + 1e-6
        for row in rows:
            want, _ = _oracle(oracle, rt, 32, 1, W, H, 100, 50, rows=(row, row + 1))
            assert _same_bits(a[row:row + 1], want), (W, H, row)


def _render_scene(rt, prec, scene, cam, sched=2, seed=1227):
    with rt.Renderer(0, prec) as r:
        r.set_camera(cam); r.set_scene(scene); r.set_schedule(sched); r.init_rng(seed)
        r.render(0)
        segs = r.count_segments(0)
        return r.read_framebuffer(), segs


@pytest.mark.parametrize("prec", [32, 64])
def test_sky_comes_from_the_primary_ray_known_answer_on_the_gpu(rt, oracle, prec):
    """camera.h:121 on the HIP path itself, with NO oracle in the comparison: in front of a perfect
    mirror every path is hit -> reflect -> miss with attenuation exactly 1, and the CUDA program
    shades the miss with the PRIMARY ray, so at 1 sample per pixel the mirror image must be
    bit-identical to the image of the empty scene (see tests/test_oracle_pins.py for the CPU twin,
    which also checks that sky-from-the-current-ray gives a different picture).  Then the analytic
    gradient and, last, the oracle."""
    from tests.test_oracle_pins import probe_scene
    W, H = 64, 40
    cam = rt.camera(prec, W, H, 1, 10)
    for sched in (rt.SCHED_SORTED, rt.SCHED_STATIC):
        empty, seg_e = _render_scene(rt, prec, probe_scene(prec, "empty"), cam, sched)
        mirror, seg_m = _render_scene(rt, prec, probe_scene(prec, "mirror"), cam, sched)
        assert seg_e == W * H and seg_m == 2 * W * H
        assert _same_bits(empty, mirror), sched
    p00, du, dv, c = (np.array(list(x), np.float64) for x in (cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v, cam.center))
    jj, ii = np.mgrid[0:H, 0:W]
    d = p00 + ii[..., None] * du + jj[..., None] * dv - c
    a = 0.5 * (d[..., 1] / np.linalg.norm(d, axis=-1) + 1.0)
    want = (1.0 - a)[..., None] * np.ones(3) + a[..., None] * np.array([0.5, 0.7, 1.0])
    slack = 0.25 * (np.linalg.norm(dv) + np.linalg.norm(du) + 0.06) / 10.0
    assert np.abs(empty.astype(np.float64) ** 2 - want).max() <= slack
    ref, _ = oracle.render(prec, probe_scene(prec, "mirror"), cam, 1227)
    assert _same_bits(mirror, ref)
    # many samples: later samples start from different RNG states in the two scenes (the metal
    # scatter draws a random_unit_vector even at fuzz 0, material.h:56), so only statistics agree
    cam16 = rt.camera(prec, W, H, 16, 10)
    e16, _ = _render_scene(rt, prec, probe_scene(prec, "empty"), cam16)
    m16, _ = _render_scene(rt, prec, probe_scene(prec, "mirror"), cam16)
    assert not _same_bits(e16, m16) and np.abs(e16.astype(np.float64) - m16).max() < 2e-3


def test_baseline_config5_fp64_500spp_and_float_vs_double(rt, oracle, tmp_path):
    """BASELINE configs[4]: fp64, scene 3, 1920x1080, 500 spp, 50 bounces.  Oracle row spot check,
    and the reference's own acceptance procedure (README.md:101-116): ppm_diff of the float and the
    double image must be 'rather dark' -- here quantified against the calibrated noise floor of
    SURVEY A.5 (two independent 100-spp renders differ by mean 1.41 levels; at 500 spp ~0.63)."""
    W, H, S, B = 1920, 1080, 500, 50
    d = _render(rt, 64, 3, W, H, S, B, threads=0)
    assert np.isfinite(d).all() and d.min() >= 0
    want, _ = _oracle(oracle, rt, 64, 3, W, H, S, B, rows=(700, 701))
    assert _same_bits(d[700:701], want)
    f = _render(rt, 32, 3, W, H, S, B, threads=0)
    pf, pd = str(tmp_path / "f.ppm"), str(tmp_path / "d.ppm")
    rt.write_ppm(pf, f); rt.write_ppm(pd, d)
    exe = os.path.join(os.path.dirname(rt.lib_paths()["hip"]), "..", "bin", "ppm_diff")
    r = subprocess.run([exe, pf, pd, str(tmp_path / "diff.ppm"), "--max-mean", "1.0", "--max-p99", "8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    lf = np.floor(256 * np.clip(f.astype(np.float64), 0, 0.999)); ld = np.floor(256 * np.clip(d, 0, 0.999))
    # per-channel bias: fp32 comes out ~0.33 levels (0.2 %) darker than fp64 -- the algorithm's own
    # precision effect (fp32 self-intersections at tmin against the radius-1000 ground sphere), the
    # bit-exact oracle shows the same; anything beyond a fraction of a level would be a bug
    assert np.all(np.abs(lf.mean(axis=(0, 1)) - ld.mean(axis=(0, 1))) < 0.6)


@pytest.mark.parametrize("prec,scene_id,W,H,S,B,shard", [
    (32, 3, 640, 360, 32, 50, None),          # 0.7 pools per wave: 128 solo waves
    (64, 3, 640, 360, 32, 50, None),
    (32, 3, 1920, 1080, 24, 50, (1, 4, 2)),   # a quarter of the headline frame in 2-row strips: 256 solo waves
    (32, 1, 64, 64, 24, 40, None),            # the smallest frame the sorted schedule sorts: solo waves clamped to the 64 workgroups
    (32, 2, 200, 100, 64, 50, None),          # scene 2 (4 spheres)
])
def test_solo_waves_leave_the_image_alone(rt, oracle, prec, scene_id, W, H, S, B, shard):
    """On a partly filled GPU the main launch of the sorted schedule is render_solo_kernel: the top-ranked pixels
    two per wave.  A schedule only: same image as the static schedule (one lane per pixel, no hand-out at all),
    bit for bit, and as the oracle on a few rows."""
    sc = rt.build_scene(scene_id, prec)
    with rt.Renderer(0, prec) as r:
        r.set_camera(rt.camera(prec, W, H, S, B)); r.set_scene(sc)
        if shard:
            r.set_shard(*shard)
        r.init_rng(1227)
        r.render(0)
        got = r.read_framebuffer()
        st = r.stats()
    assert st["phases"] == 2 and st["solo_waves"] > 0 and st["solo_lanes"] == 2, st
    if not shard and prec == 32 and scene_id == 3:          # the rule needs a bounce limit that lets outlier chains exist
        few = _render_stats(rt, prec, scene_id, W, H, S, 10)
        assert few["phases"] == 2 and few["solo_waves"] == 0, few
    assert st["solo_waves"] == min(256 if shard else 128, st["grid_blocks"]), st
    assert _same_bits(got, _render(rt, prec, scene_id, W, H, S, B, threads=8, shard=shard, sched=rt.SCHED_STATIC))
    if not shard:
        for row in (0, H // 2, H - 1):
            want, _ = _oracle(oracle, rt, prec, scene_id, W, H, S, B, rows=(row, row + 1))
            assert _same_bits(got[row:row + 1], want), row


@pytest.mark.parametrize("W,H,shard", [(640, 360, None), (333, 217, None), (1920, 1080, (3, 8, 2)), (700, 300, (1, 3, 5))])
def test_sort_key_is_the_neighbourhood_mean_of_the_prepass_cost(rt, W, H, shard):
    """cost_smooth_kernel (LDS tiles) against the definition: the mean of the prepass cost over the 13 x 13 window
    clipped to the image and to the pixel's own row strip, in quarter segments, rounded to nearest."""
    with rt.Renderer(0, 32, debug=True) as r:
        r.set_camera(rt.camera(32, W, H, 32, 50)); r.set_scene(rt.build_scene(3, 32))
        strip = H                                            # one rank: its strips are adjacent, the window crosses them
        if shard:
            r.set_shard(*shard); strip = shard[2]
        r.init_rng(1227)
        r.render(0)
        assert r.stats()["phases"] == 2
        own, smoothed = r.debug_read_costs()
    rows = own.shape[0]
    assert own.min() >= 2 and own.max() <= 2 * 50            # two prepass samples of 1..50 segments each
    hw = 6
    csum = np.zeros((rows + 1, W + 1), np.int64)
    csum[1:, 1:] = own.astype(np.int64).cumsum(0).cumsum(1)
    jl = np.arange(rows)[:, None]; i = np.arange(W)[None, :]
    s0 = (jl // strip) * strip
    j0 = np.maximum(jl - hw, s0); j1 = np.minimum(np.minimum(jl + hw, s0 + strip - 1), rows - 1)
    i0 = np.maximum(i - hw, 0); i1 = np.minimum(i + hw, W - 1)
    total = csum[j1 + 1, i1 + 1] - csum[j0, i1 + 1] - csum[j1 + 1, i0] + csum[j0, i0]
    cells = (j1 - j0 + 1) * (i1 - i0 + 1)
    want = (4 * total + cells // 2) // cells
    assert np.array_equal(smoothed.astype(np.int64), want)


def test_full_size_properties(rt, oracle):
    """BASELINE headline config (scene 3, 1920x1080, 100 spp, 50 bounces): too big for the
    oracle in full, so: (1) run-to-run determinism, (2) 8-way sharded == whole image,
    (3) oracle spot check of whole rows, (4) value range / no NaN, (5) segment statistics."""
    W, H, S, B = 1920, 1080, 100, 50
    sc = rt.build_scene(3, 32)
    with rt.Renderer(0, 32) as r:
        r.set_camera(rt.camera(32, W, H, S, B)); r.set_scene(sc); r.init_rng(1227)
        r.render(0)
        a = r.read_framebuffer()
        r.render(8)
        b = r.read_framebuffer()
        assert r.stats()["solo_waves"] == 0          # a full GPU keeps the plain kernel
        segs = r.count_segments(0)
    assert _same_bits(a, b)
    # the fp32 screen in front of the exact sphere test (default) vs the exact test on every
    # sphere: 6e10 sphere tests must not differ in a single bit
    assert _same_bits(a, _render(rt, 32, 3, W, H, S, B, threads=0, source=rt.SCENE_LDS_EXACT, sched=rt.SCHED_STATIC))
    assert np.isfinite(a).all() and a.min() >= 0 and a.max() <= 1.0 + 1e-6
    assert 2.0 < segs / (W * H * S) < 2.6          # 2.24 segments per primary ray
    full = np.zeros_like(a)
    for rank in range(8):
        rt.place_rows(full, _render(rt, 32, 3, W, H, S, B, threads=0, shard=(rank, 8, 8)), rank, 8, 8)
    assert _same_bits(full, a)
    for row in (0, 611, 1079):
        want, _ = _oracle(oracle, rt, 32, 3, W, H, S, B, rows=(row, row + 1))
        assert _same_bits(a[row:row + 1], want), row


def _full_frame_names():
    from tests.golden.make_full_frame_crcs import CONFIGS
    return [c[0] for c in CONFIGS]


@pytest.mark.parametrize("name", _full_frame_names())
def test_full_frames_match_the_oracle_row_by_row(rt, golden_dir, name):
    """Every pixel of the BASELINE.json frames (configs[2], [3] = headline, [4], the fp64 headline and the
    487-sphere scene at 1080p / at the reference grid's largest frame) against the oracle's full render of
    the same frame: tests/golden/full_frame_crcs.json holds one CRC-32 per row of the raw float bits and the
    SHA-256 of the image (tests/golden/make_full_frame_crcs.py, minutes of CPU per frame).  Default
    schedule and scene source, i.e. exactly what bench.py and the executables run."""
    import hashlib
    import zlib
    gold = json.load(open(os.path.join(golden_dir, "full_frame_crcs.json")))
    if name not in gold:
        pytest.skip("no golden for %s yet (tests/golden/make_full_frame_crcs.py %s)" % (name, name))
    g = gold[name]
    img = _render(rt, g["precision"], g["scene_id"], g["width"], g["height"], g["samples"], g["bounces"], threads=0, seed=g["seed"])
    assert img.shape == (g["height"], g["width"], 3) and img.dtype == (np.float32 if g["precision"] == 32 else np.float64)
    crcs = [zlib.crc32(np.ascontiguousarray(img[j]).view(np.uint8).tobytes()) & 0xffffffff for j in range(img.shape[0])]
    bad = [j for j in range(img.shape[0]) if crcs[j] != g["row_crc32"][j]]
    assert not bad, "%s: %d rows differ from the oracle, first %s" % (name, len(bad), bad[:8])
    assert hashlib.sha256(np.ascontiguousarray(img).view(np.uint8).tobytes()).hexdigest() == g["sha256"]


def test_levels_quantised_on_the_device_equal_the_host_writers(rt):
    """rtiow_read_levels: int(256 * clamp(c, 0, 0.999)) per channel on the device == the host's to_level on the read-back framebuffer
    (main.cu:367, 374-376), fp32 and fp64, full frame and shard; a NaN channel is counted."""
    for prec in (32, 64):
        with rt.Renderer(0, prec) as r:
            r.set_camera(rt.camera(prec, 322, 183, 8, 10)); r.set_scene(rt.build_scene(3, prec)); r.init_rng(1227)
            for shard in (None, (1, 3, 2)):
                if shard:
                    r.set_shard(*shard); r.init_rng(1227)
                r.render(0)
                fb = r.read_framebuffer()
                lev, nans = r.read_levels()
                want, host_nans = rt.levels(fb)
                assert nans == 0 and host_nans == 0 and lev.shape == fb.shape and np.array_equal(lev, want)
                assert lev.max() > 200 and lev.min() < 50


def test_bench_prints_one_contract_line(rt):
    """bench.py's contract with the driver: exactly one JSON line on stdout with the agreed fields,
    the roofline of the dominant launch and the CPU baseline (small frame so the CPU leg takes a second)."""
    import json, sys
    from tests.conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--width", "256", "--height", "144",
                        "--samples", "64", "--bounces", "10"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["unit"] == "Mrays/s" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - 256 * 144 * 64 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-3 * d["value"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["unit"] == "TFLOP/s" and 0 < rf["launch_ms_mean"] <= d["kernel_ms_mean"] and rf["device"]["cus"] > 0 and rf["device"]["clock_mhz"] > 0
    assert "practical_peak" not in rf and rf["algorithmic_frac"] > 0 and d["step"]["scene_prepare_ms"] > 0
    # frac is EXECUTED work: the vector-issue fraction from rocprofv3 --pmc passes this very run made over the loaded build.  bench.py is built to
    # degrade to null where the profiler cannot run (no permission, counter slots busy): the contract line must survive that (the live leg has its
    # own test below, which skips there)
    if rf["frac"] is None:
        assert "live passes failed" in rf["counters_from"] or "no record" in rf["counters_from"], rf["counters_from"]
    else:
        assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and 0 < rf["frac"] < 1
        assert rf["build_id"] == rt.build_id() and rf["issue_saturation"]["simd_cycles_busy_per_valu_inst"] > 2.0
    # the other configurations of the round's claims ride along, rendered by the same library after the timed region
    ex = {e["name"]: e for e in d["extra_configs"]}
    assert set(ex) == {"fp64_headline", "scene1_487_spheres_1080p", "baseline_config2_scene1_320x192_10spp_25b"}
    for e in ex.values():
        assert e["ms_per_step"] > 0 and e["value"] > 0 and e["unit"] == "Mrays/s" and e["main_launch_ms"] <= e["ms_per_step"]
        assert e["frac"] is None or 0 < e["frac"] < 1.2
    if ex["fp64_headline"]["frac"] is not None:       # the fp64 figure charges what EXECUTED at the double-precision rate (this run's own "f64" pass)
        assert ex["fp64_headline"]["dp_cycles_from"].startswith("executed")
    cb = d["cpu_baseline"]
    assert cb["kind"] in ("reference", "port") and cb["cores"] == 1 and cb["value"] > 0 and cb["unit"] == "Mrays/s" and cb["sample"]


@pytest.mark.parametrize("prec", [32, 64])
def test_bench_dump_outputs_is_the_rendered_image(rt, oracle, tmp_path, prec):
    """bench.py --dump-outputs DIR writes the image its timed path left after the last step.  The RNG state is not written
    back, so every step renders the same image: bit for bit the oracle's render of the same scene, camera and seed."""
    import sys
    from tests.conftest import ROOT
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--width", "96", "--height", "64",
                        "--samples", "4", "--bounces", "12", "--precision", str(prec), "--pmc", "off", "--no-cpu-baseline", "--no-extra-configs",
                        "--no-scaling-probe", "--dump-outputs", str(out)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["image.npy"]
    got = np.load(out / "image.npy")
    assert got.dtype == (np.float32 if prec == 32 else np.float64) and got.shape == (64, 96, 3)
    want, _ = oracle.render(prec, compact(rt.build_scene(3, prec)), rt.camera(prec, 96, 64, 4, 12), 1227)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_bench_live_counter_passes(rt):
    """The live leg of roofline.frac: rocprofv3 --pmc child passes over the loaded library (skips where the profiler cannot collect counters)."""
    import json, sys
    from tests.conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--width", "256", "--height", "144", "--samples", "64",
                        "--bounces", "10", "--pmc", "live", "--no-cpu-baseline", "--no-extra-configs", "--no-scaling-probe"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    rf = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])["roofline"]
    if rf["frac"] is None and "live passes failed" in rf["counters_from"]:
        pytest.skip("rocprofv3 --pmc is not usable here: " + rf["counters_from"][:200])
    assert rf["frac"] is not None and "rocprofv3" in rf["counters_from"] and rf["build_id"] == rt.build_id()
    iss = rf["issued"]
    assert iss["valu_wave_insts_per_launch"] > 1e6 and abs(iss["valu_issue_frac"] - rf["frac"]) < 1e-3 and 0 < iss["active_lane_frac"] <= 1
    assert rf["traffic"] > 0 and rf["write_bytes"] >= 256 * 144 * 12 * 0.9


def test_bench_two_rank_rehearsal(rt):
    """bench.py --gpus 2 launched the way the driver launches it (torch.distributed.run, one rank per
    process); with a single GPU the ranks share device 0 and gather over gloo (RTIOW_BENCH_BACKEND).
    Checks the rank-0 line: whole-job value, strong scaling, sharding description, no traffic figure."""
    import json, sys
    from tests.conftest import ROOT
    env = dict(os.environ, RTIOW_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--width", "256", "--height", "144", "--samples", "64", "--bounces", "10"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["backend"] == "gloo" and "strips" in d["config"]["sharding"]
    assert abs(d["value"] - 256 * 144 * 64 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-3 * d["value"]
    assert d["roofline"]["traffic"] is None and "cpu_baseline" not in d
    assert 1.5 < d["segments_per_ray"] < 3.5            # summed over both ranks' shards


def test_degenerate_sizes_and_depths(rt, oracle):
    """Frames smaller than a tile or a wave, one sample, no bounces: every schedule still equals the
    oracle bit for bit (lane cap, padded pools and the unsorted / sorted switch all depend on the size)."""
    cases = [(1, 1, 1, 0), (1, 1, 3, 1), (1, 70, 2, 5), (70, 1, 2, 5), (9, 9, 1, 50), (65, 3, 24, 2), (8, 8, 64, 3), (33, 17, 70, 1)]
    for prec in (32, 64):
        for W, H, S, B in cases:
            want, _ = _oracle(oracle, rt, prec, 3, W, H, S, B)
            for sched in (rt.SCHED_SORTED, rt.SCHED_PERSISTENT, rt.SCHED_STATIC):
                got = _render(rt, prec, 3, W, H, S, B, threads=8, sched=sched)
                assert _same_bits(got, want), (prec, W, H, S, B, sched)
    # odd shard splits of a small frame: more ranks than strips, one-row strips
    want, _ = _oracle(oracle, rt, 32, 3, 40, 11, 30, 8)
    for n, strip in ((5, 8), (3, 1), (11, 1), (4, 3)):
        full = np.zeros_like(want)
        for rank in range(n):
            with rt.Renderer(0, 32) as r:
                r.set_camera(rt.camera(32, 40, 11, 30, 8)); r.set_scene(rt.build_scene(3, 32)); r.set_shard(rank, n, strip); r.init_rng(1227)
                r.render(0)
                if r.local_rows:
                    rt.place_rows(full, r.read_framebuffer(), rank, n, strip)
        assert _same_bits(full, want), (n, strip)
