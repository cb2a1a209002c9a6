"""Pins of the CPU oracle itself (no GPU): before the oracle may judge the HIP path it is
checked against the reference's own outputs and against third-party known answers.

 * serial semantics  == the reference's serial tracer (src/InOneWeekend) byte for byte:
   hashes in tests/golden/serial_ref.json were produced by the reference's sources built
   by oracle/Makefile (tests/golden/make_golden.py), and whole P3 texts of small configs in
   tests/golden/ref_serial_small.npz; when oracle/_ref/ is present the binary is also run live.
 * XORWOW engine + 2^67 jump matrices == rocRAND's host engine (salt=1 known answers).
 * scene tables == the entries SURVEY.md A.3 dumped from the reference's structs.
 * analytic known answers for hit_sphere / reflect / refract / Schlick.
"""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests.oracle_lib import ROOT


def test_glibc_rand_restatement_matches_libc(oracle):
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(1)
    want = np.array([libc.rand() for _ in range(20000)], np.int32)
    assert np.array_equal(oracle.glibc_rand(20000), want)
    # first glibc rand()/(RAND_MAX+1.0f) values
    first = oracle.glibc_rand(3).astype(np.float32) / np.float32(2147483648.0)
    assert np.allclose(first, [0.840187728, 0.394382924, 0.783099234], rtol=0, atol=1e-9)


def test_serial_semantics_matches_reference_hashes(oracle, golden_dir):
    gold = json.load(open(os.path.join(golden_dir, "serial_ref.json")))
    assert len(gold["driver"]) >= 4
    for g in gold["driver"]:
        p3, stats = oracle.render_serial(g["scene_id"], g["width"], g["height"], g["samples"], g["depth"])
        assert len(p3) == g["bytes"]
        assert hashlib.md5(p3).hexdigest() == g["md5"], g
        assert stats[0] == g["width"] * g["height"] * g["samples"]


def test_serial_semantics_matches_reference_binary_live(oracle, golden_dir):
    """Byte for byte against the P3 text the reference's serial tracer printed (tests/golden/ref_serial_small.npz);
    with oracle/_ref built, the binary is also run and must print the same text."""
    gold = np.load(os.path.join(golden_dir, "ref_serial_small.npz"))
    configs = [(3, 48, 27, 2, 7), (2, 40, 24, 3, 50), (1, 64, 36, 1, 5)]
    assert gold["configs"].tolist() == [list(c) for c in configs]
    drv = os.path.join(ROOT, "oracle", "_ref", "ref_serial_driver")
    for k, cfg in enumerate(configs):
        want = gold["p3_%d" % k].tobytes()
        got, _ = oracle.render_serial(*cfg)
        assert got == want, cfg
        if os.path.exists(drv):
            assert subprocess.run([drv] + [str(x) for x in cfg], capture_output=True, check=True).stdout == want, cfg


def test_unmodified_reference_binary_hash_is_recorded(golden_dir):
    # The 55 s run of the reference's unmodified main.cc (scene 1, 1280x768, 10 spp, depth 20)
    # was compared with oracle.render_serial(1, 1280, 768, 10, 20) when the fixture was made
    # (make_golden.py --full); here only the recorded hash is checked against SURVEY A.1.
    gold = json.load(open(os.path.join(golden_dir, "serial_ref.json")))["unmodified_binary"]
    assert gold["md5"] == "73e0404ea185d32ec6a4e8f4ec158eb6"


@pytest.mark.skipif(not os.environ.get("RTIOW_SLOW"), reason="35 s; set RTIOW_SLOW=1")
def test_serial_semantics_full_reference_config(oracle, golden_dir):
    gold = json.load(open(os.path.join(golden_dir, "serial_ref.json")))["unmodified_binary"]
    p3, _ = oracle.render_serial(1, 1280, 768, 10, 20)
    assert hashlib.md5(p3).hexdigest() == gold["md5"]


def test_xorwow_engine_and_jumps_match_rocrand(oracle, golden_dir):
    kats = json.load(open(os.path.join(golden_dir, "xorwow_rocrand_kat.json")))
    assert len(kats) > 100
    for k in kats:
        st = oracle.xorwow_init(k["seed"], k["subsequence"], k["offset"], salt=1)
        got = [oracle.xorwow_next(st) for _ in range(4)]
        assert got == k["u32"], k


def test_xorwow_survey_known_answers(oracle):
    # SURVEY.md A.6 (rocRAND 7.2 host engine, rocrand_init(1227, seq, 0))
    kat = {0: [2182705537, 3856141749, 3955497083, 4166789925], 1: [3494376245, 2768503877, 2850426799, 3590630605],
           61439: [2618532050, 3083497680, 1039127971, 2346679302], 2073599: [2168410605, 4244404003, 2045635238, 3563087961]}
    for seq, want in kat.items():
        st = oracle.xorwow_init(1227, seq, 0, salt=1)
        assert [oracle.xorwow_next(st) for _ in range(4)] == want


def test_xorwow_offset_equals_discarding_draws(oracle):
    for salt in (0, 1):
        for seq, off in [(0, 3), (5, 17), (123456, 4099)]:
            a = oracle.xorwow_init(1227, seq, off, salt)
            b = oracle.xorwow_init(1227, seq, 0, salt)
            for _ in range(off):
                oracle.xorwow_next(b)
            assert np.array_equal(a, b)


def test_xorwow_curand_salt_initial_state(oracle):
    # curand_init's published scrambling for seed 1227, subsequence 0 (state before any draw).
    seed = 1227
    s0 = (seed ^ 0xaad26b49) & 0xffffffff
    s1 = 0xf7dcefdd
    t0 = (1099087573 * s0) & 0xffffffff
    t1 = (2591861531 * s1) & 0xffffffff
    want = [(123456789 + t0) & 0xffffffff, 362436069 ^ t0, (521288629 + t1) & 0xffffffff, 88675123 ^ t1,
            (5783321 + t0) & 0xffffffff, (6615241 + t1 + t0) & 0xffffffff]
    assert list(oracle.xorwow_init(seed, 0, 0, salt=0)) == want


def test_uniform_float_range_and_formula(oracle):
    st = oracle.xorwow_init(1227, 9, 0)
    st2 = st.copy()
    for _ in range(2000):
        x = oracle.xorwow_next(st2)
        u = oracle.uniform(32, st)
        want = np.float32(np.float32(x) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33))
        assert np.float32(u) == want and 0.0 < u <= 1.0
    st = oracle.xorwow_init(1227, 9, 0)
    st2 = st.copy()
    for _ in range(500):
        x = oracle.xorwow_next(st2); y = oracle.xorwow_next(st2)
        z = x ^ (y << 21)
        assert oracle.uniform(64, st) == z * 2.0 ** -53 + 2.0 ** -54


def test_scene_tables_match_survey_fixture_and_golden(oracle, golden_dir):
    sc = oracle.build_scene(3, 32)
    assert len(sc["type"]) == 125 and sc["valid"].all()
    # SURVEY.md A.3 (reference GlobalFloat structs, g++ evaluation order)
    assert np.allclose(sc["center_radius"][1, :3], [-10.2952108, 0.2, -10.6450558], rtol=0, atol=5e-7)
    assert sc["type"][1] == 1
    assert np.allclose(sc["albedo_fuzz"][1], [0.5987757, 0.9558237, 0.8992200, 0.1676114], rtol=0, atol=5e-7)
    assert np.allclose(sc["center_radius"][2, :3], [-10.5014267, 0.2, -9.7500029], rtol=0, atol=5e-7)
    assert np.allclose(sc["albedo_fuzz"][2, :3], [0.3342138, 0.5988296, 0.2450961], rtol=0, atol=5e-7)
    assert np.allclose(sc["albedo_fuzz"][3, :3], [0.0380553, 0.0131085, 0.0832953], rtol=0, atol=5e-7)
    counts = {1: (488, [341], [394, 64, 29]), 2: (40, [], [29, 8, 3]), 3: (125, [], [96, 23, 6])}
    gold = np.load(os.path.join(golden_dir, "scene_tables.npz"))
    for prec in (32, 64):
        for sid, (n, invalid, types) in counts.items():
            sc = oracle.build_scene(sid, prec)
            assert len(sc["type"]) == n
            assert list(np.where(sc["valid"] == 0)[0]) == invalid
            assert list(np.bincount(sc["type"][sc["valid"] == 1], minlength=3)) == types
            for k in ("center_radius", "albedo_fuzz", "refraction_index", "type", "valid"):
                assert np.array_equal(sc[k], gold["s%d_f%d_%s" % (sid, prec, k)])
    # any other id falls into the default: branch (main.cu:241)
    assert np.array_equal(oracle.build_scene(42, 32)["center_radius"], oracle.build_scene(3, 32)["center_radius"])


def test_camera_initialize_analytic(oracle):
    for prec, tol in ((32, 2e-5), (64, 1e-12)):
        ints, f = oracle.camera_flat(prec, 320, 192, 10, 25)
        assert list(ints) == [320, 192, 10, 25]
        pss, center, p00, du, dv = f[0], f[1:4], f[4:7], f[7:10], f[10:13]
        dang, ddu, ddv = f[13], f[14:17], f[17:20]
        assert abs(pss - 0.1) < tol and np.allclose(center, [13, 2, 3])
        w = np.array([13, 2, 3.0]); w /= np.linalg.norm(w)
        u = np.cross([0, 1.0, 0], w); u /= np.linalg.norm(u)
        v = np.cross(w, u)
        vh = 2 * np.tan(np.radians(20) / 2) * 10
        vw = vh * 320 / 192
        assert np.allclose(du, vw * u / 320, atol=tol) and np.allclose(dv, -vh * v / 192, atol=tol)
        ul = np.array([13, 2, 3.0]) - 10 * w - vw * u / 2 + vh * v / 2
        assert np.allclose(p00, ul + 0.5 * (vw * u / 320 - vh * v / 192), atol=10 * tol)
        rad = 10 * np.tan(np.radians(0.3))
        assert abs(dang - 0.6) < 1e-6 and np.allclose(ddu, rad * u, atol=tol) and np.allclose(ddv, rad * v, atol=tol)


def _hit(oracle, c, r, o, d, tmin=0.001, tmax=np.inf):
    c = np.array(c, np.float64); o = np.array(o, np.float64); d = np.array(d, np.float64)
    t = ctypes.c_double(); p = np.zeros(3); n = np.zeros(3); front = ctypes.c_int()
    ok = oracle.L.oracle_hit_sphere_f64(c.ctypes.data, r, o.ctypes.data, d.ctypes.data, tmin, tmax,
                                        ctypes.addressof(t), p.ctypes.data, n.ctypes.data, ctypes.addressof(front))
    return (ok, t.value, p, n, front.value) if ok else (0, None, None, None, None)


def test_hit_sphere_known_answers(oracle):
    # axis-aligned ray at a unit sphere: roots 4 and 6, outward normal, front face
    ok, t, p, n, front = _hit(oracle, [0, 0, -5], 1.0, [0, 0, 0], [0, 0, -1])
    assert ok and t == 4.0 and np.array_equal(p, [0, 0, -4]) and np.array_equal(n, [0, 0, 1]) and front == 1
    # un-normalised direction: t scales with 1/|d|
    ok, t, *_ = _hit(oracle, [0, 0, -5], 1.0, [0, 0, 0], [0, 0, -2])
    assert ok and t == 2.0
    # from inside: near root negative, far root taken, normal flipped, back face
    ok, t, p, n, front = _hit(oracle, [0, 0, 0], 2.0, [0, 0, 0], [1, 0, 0])
    assert ok and t == 2.0 and np.array_equal(n, [-1, 0, 0]) and front == 0
    # tangent ray: discriminant 0, single root
    ok, t, *_ = _hit(oracle, [0, 1, -5], 1.0, [0, 0, 0], [0, 0, -1])
    assert ok and t == 5.0
    # miss; sphere behind; open interval at both ends (interval.h:21-23)
    assert _hit(oracle, [0, 3, -5], 1.0, [0, 0, 0], [0, 0, -1])[0] == 0
    assert _hit(oracle, [0, 0, 5], 1.0, [0, 0, 0], [0, 0, -1])[0] == 0
    assert _hit(oracle, [0, 0, -5], 1.0, [0, 0, 0], [0, 0, -1], tmin=4.0, tmax=6.0)[0] == 0
    ok, t, *_ = _hit(oracle, [0, 0, -5], 1.0, [0, 0, 0], [0, 0, -1], tmin=4.0, tmax=6.5)
    assert ok and t == 6.0
    # t < 0.001 rejected (shadow-acne guard, camera.h:87): origin on the surface, leaving
    assert _hit(oracle, [0, 0, -1], 1.0, [0, 0, 0], [0, 0, 1])[0] == 0


def test_reflect_refract_schlick_known_answers(oracle):
    out = np.zeros(3)
    v = np.array([1.0, -1.0, 0.0]); n = np.array([0.0, 1.0, 0.0])
    oracle.L.oracle_reflect_f64(v.ctypes.data, n.ctypes.data, out.ctypes.data)
    assert np.array_equal(out, [1.0, 1.0, 0.0])
    # normal incidence: refract passes straight through for any eta
    uv = np.array([0.0, -1.0, 0.0])
    oracle.L.oracle_refract_f64(uv.ctypes.data, n.ctypes.data, 1.0 / 1.5, out.ctypes.data)
    assert np.allclose(out, [0, -1, 0], atol=1e-15)
    # Snell: sin(theta_t) = eta * sin(theta_i)
    th = np.radians(40.0)
    uv = np.array([np.sin(th), -np.cos(th), 0.0])
    oracle.L.oracle_refract_f64(uv.ctypes.data, n.ctypes.data, 1.0 / 1.5, out.ctypes.data)
    assert abs(np.linalg.norm(out) - 1) < 1e-12 and abs(out[0] - np.sin(th) / 1.5) < 1e-12 and out[1] < 0
    # Schlick: r0 at normal incidence, 1 at grazing; powf is evaluated in float
    r0 = ((1 - 1.5) / (1 + 1.5)) ** 2
    assert abs(oracle.L.oracle_reflectance_f64(1.0, 1.5) - r0) < 1e-15
    assert abs(oracle.L.oracle_reflectance_f64(0.0, 1.5) - 1.0) < 1e-15
    c = 0.3
    assert abs(oracle.L.oracle_reflectance_f64(c, 1.5) - (r0 + (1 - r0) * (1 - c) ** 5)) < 1e-6


def test_cuda_semantics_golden_images_regress(oracle, golden_dir, native):
    """The committed oracle renders (what -m gpu compares the HIP path with) are reproducible."""
    from tests.golden.make_golden import CUDA_SEM_CONFIGS
    from tests.conftest import compact
    for name, prec, sid, W, H, S, B in CUDA_SEM_CONFIGS:
        gold = np.load(os.path.join(golden_dir, name + ".npy"))
        img, stats = oracle.render(prec, compact(oracle.build_scene(sid, prec)), native.camera(prec, W, H, S, B), 1227)
        assert np.array_equal(img.view(np.uint8), gold.view(np.uint8)), name
        assert stats[0] == W * H * S and stats[1] >= stats[0]


def test_cuda_semantics_row_ranges_and_thread_independence(oracle, native):
    """Row subsets equal the same rows of the full render (streams are keyed by the global
    pixel index), whatever the number of host threads the oracle uses."""
    from tests.conftest import compact
    sc = compact(oracle.build_scene(3, 32))
    cam = native.camera(32, 96, 56, 8, 20)
    full, st = oracle.render(32, sc, cam, 1227)
    part, _ = oracle.render(32, sc, cam, 1227, 16, 40)
    assert np.array_equal(full[16:40], part)
    assert np.isfinite(full).all() and full.min() >= 0 and full.max() <= 1.0 + 1e-6
    oracle.set_threads(1)
    try:
        one, st1, seg = oracle.render(32, sc, cam, 1227, segments=True)
    finally:
        oracle.set_threads(0)
    assert np.array_equal(full.view(np.uint8), one.view(np.uint8)) and st == st1
    assert int(seg.sum()) == st1[1]


# ---------------------------------------------------------------------------------------
# Pins of the CUDA-semantics corner of the oracle -- the one the HIP kernel is compared with.
#
# oracle/rtiow_oracle.cpp has ONE scatter / sky / ray_color implementation, parameterised by a
# policy (serial: fp64, rand(), unfused | CUDA: T, XORWOW, explicit fma) and two run-time
# switches (loop form, sky mode).  The corner {serial, recursive, sky=current} is the reference's
# serial program and is pinned byte for byte above.  The tests below walk from that corner to
# {CUDA, iterative, sky=primary} one switch at a time, each step against reference-run output:
#   1. loop form        recursive -> iterative with IDENTICAL random numbers: same P3 bytes;
#   2. policy           serial -> CUDA (sky still from the current ray) against the images the
#                       reference's own serial tracer printed (tests/golden/ref_serial_*.npz),
#                       gated with SURVEY.md A.5's ppm_diff noise floors;
#   3. sky mode         current -> primary: the blue channel of the sky blend is 1.0 for every
#                       direction (camera.h:123: (1-a)*1 + a*1), so the FINAL oracle -- the exact
#                       code path the GPU is judged by -- must still match the reference images
#                       in blue within the floor, while red/green get whiter (SURVEY §0 finding 2);
#                       plus known answers for the sky term and a mirror scene that separates the
#                       two sky modes exactly.
# What stays "parity unpinned": cuRAND's bit stream and nvcc's contraction choices (no CUDA
# toolchain here) -- they change the noise, not these statistics.
# ---------------------------------------------------------------------------------------
from tests.oracle_lib import ITERATIVE, RECURSIVE, SKY_CURRENT, SKY_PRIMARY, diff_stats, p3_levels, to_levels  # noqa: E402


def _ref_images(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "ref_serial_320x192_100spp_50b.json")))
    imgs = np.load(os.path.join(golden_dir, "ref_serial_320x192_100spp_50b.npz"))
    return meta, imgs


def _p3_text(levels):
    """uint8 [H, W, 3] -> the P3 text the reference's serial tracer prints for it (header, one pixel per line)."""
    H, W, _ = levels.shape
    return ("P3\n%d %d\n255\n" % (W, H) + "".join("%d %d %d\n" % tuple(p) for p in levels.reshape(-1, 3).tolist())).encode()


def test_reference_image_fixtures_are_what_the_reference_prints(golden_dir):
    """The fixture images are outputs of the reference's serial tracer (make_golden.py): each one, printed
    back as P3 text, has the md5 and length recorded from that tracer's output.  When the binary built
    from the reference's sources is here, one of them is also regenerated and compared."""
    meta, imgs = _ref_images(golden_dir)
    assert sorted(meta["scenes"]) == ["1", "2", "3"] and imgs["s1"].shape == (192, 320, 3)
    # SURVEY.md A.5 measured the same floors with the reference's ppm_diff (1.408 / 2.490)
    assert abs(meta["scenes"]["3"]["floor_mean"] - 1.408) < 0.05 and abs(meta["scenes"]["1"]["floor_mean"] - 2.490) < 0.08
    for sid in ("1", "2", "3"):
        text = _p3_text(imgs["s" + sid])
        assert len(text) == meta["scenes"][sid]["bytes"] and hashlib.md5(text).hexdigest() == meta["scenes"][sid]["md5"], sid
    drv = os.path.join(ROOT, "oracle", "_ref", "ref_serial_driver")
    if os.path.exists(drv):
        out = subprocess.run([drv, "2", "320", "192", "100", "50"], capture_output=True, check=True).stdout
        assert hashlib.md5(out).hexdigest() == meta["scenes"]["2"]["md5"]
        assert np.array_equal(p3_levels(out), imgs["s2"])


def test_loop_form_is_neutral_with_identical_random_numbers(oracle):
    """camera.h:84-127 (iterative: running attenuation, then * sky) against the recursion of the
    serial program (src/InOneWeekend/camera.h:137-156), SAME policy, SAME rand() stream: the draws
    happen in the same order, only the association of the colour product differs (rounding far
    below a level).  Pins the loop structure of the CUDA form -- depth limit, absorb -> black,
    order of scatter and attenuation -- against the byte-exact corner."""
    for cfg in [(3, 160, 96, 10, 50), (1, 120, 72, 4, 25), (2, 80, 48, 8, 50), (3, 64, 36, 6, 2), (2, 40, 24, 9, 1)]:
        rec, st_r = oracle.render_serial(*cfg)
        it, st_i = oracle.render_serial(*cfg, loop_form=ITERATIVE)
        a, b = p3_levels(rec), p3_levels(it)
        assert st_r == st_i, cfg                                   # same rays, same hit_world calls
        assert np.abs(a.astype(int) - b.astype(int)).max() <= 1 and (a != b).mean() < 1e-3, cfg


@pytest.mark.parametrize("scene_id", [1, 2, 3])
def test_cuda_policy_with_current_ray_sky_matches_reference_images(oracle, native, golden_dir, scene_id):
    """CUDA policy (per-pixel XORWOW, (0,1] draws, explicit fma, powf-Schlick, x,y,z cube points),
    iterative loop, fp64, with the sky switched to the CURRENT ray == the reference serial
    tracer's image up to Monte-Carlo noise: SURVEY.md §8c gates (1.25 x / 1.5 x the noise floor
    between two independent renders, per-channel bias <= 0.3 level).  A wrong fuzz factor,
    Schlick term, refraction index choice or absorb rule moves the bias by levels.
    Measured: mean 2.46 / 1.26 / 1.41 (floors 2.47 / 1.25 / 1.40), |bias| <= 0.034."""
    from tests.conftest import compact
    meta, imgs = _ref_images(golden_dir)
    m = meta["scenes"][str(scene_id)]
    ref = imgs["s%d" % scene_id]
    img, _ = oracle.render(64, compact(oracle.build_scene(scene_id, 64)), native.camera(64, 320, 192, 100, 50), 1227, sky_mode=SKY_CURRENT)
    d = diff_stats(to_levels(img), ref)
    assert d["mean"] <= 1.25 * m["floor_mean"], d
    assert d["p99"] <= 1.5 * m["floor_p99"], d
    assert max(abs(b) for b in d["bias"]) <= 0.3, d


def test_cuda_policy_fp32_with_current_ray_sky_vs_reference_images(oracle, native, golden_dir):
    """Same for the fp32 policy (GlobalFloat).  fp32 differs from the fp64 reference image by a
    real effect of the reference's own float arithmetic: hit points on the radius-1000 ground
    sphere carry ~6e-5 of rounding, so some scattered rays re-hit it beyond tmin = 0.001 (shadow
    acne: 2.42 instead of 2.24 hit_world calls per ray on scene 3), which darkens the GROUND
    rows by ~0.45 level and leaves sky rows alone.  Gate: floor gates as above, bias within 0.5
    level and negative on the ground only."""
    from tests.conftest import compact
    meta, imgs = _ref_images(golden_dir)
    m, ref = meta["scenes"]["3"], imgs["s3"]
    img, st = oracle.render(32, compact(oracle.build_scene(3, 32)), native.camera(32, 320, 192, 100, 50), 1227, sky_mode=SKY_CURRENT)
    lv = to_levels(img)
    d = diff_stats(lv, ref)
    assert d["mean"] <= 1.25 * m["floor_mean"] and d["p99"] <= 1.5 * m["floor_p99"], d
    assert max(abs(b) for b in d["bias"]) <= 0.5, d
    sky_rows = diff_stats(lv[:40], ref[:40])
    assert max(abs(b) for b in sky_rows["bias"]) <= 0.15, sky_rows
    assert 2.3 < st[1] / st[0] < 2.55


@pytest.mark.parametrize("scene_id", [1, 2, 3])
def test_final_cuda_oracle_matches_reference_images_in_the_sky_invariant_channel(oracle, native, golden_dir, scene_id):
    """The oracle exactly as the GPU tests use it (primary-ray sky, camera.h:121) against the
    reference-run images.  The blue weight of the sky blend is (1-a)*1.0 + a*1.0 = 1 for every
    direction, so the blue channel does not depend on WHICH ray feeds the sky term: it must match
    the reference image within the noise floor.  Red and green must be brighter (the primary ray
    of a ground pixel looks down: whiter sky), by the amounts SURVEY §0 finding 2 describes
    (measured +17.6 / +9.6 levels on scene 3, +13.6 / +7.3 on scene 1)."""
    from tests.conftest import compact
    meta, imgs = _ref_images(golden_dir)
    m = meta["scenes"][str(scene_id)]
    ref = imgs["s%d" % scene_id]
    img, _, seg = oracle.render(64, compact(oracle.build_scene(scene_id, 64)), native.camera(64, 320, 192, 100, 50), 1227, segments=True)
    lv = to_levels(img)
    blue = diff_stats(lv[..., 2], ref[..., 2])
    assert blue["mean"] <= 1.25 * m["floor_mean_blue"] and blue["p99"] <= 1.5 * m["floor_p99_blue"], blue
    d = diff_stats(lv, ref)
    assert abs(d["bias"][2]) <= 0.3, d
    assert 5.0 < d["bias"][1] < d["bias"][0] < 25.0, d           # whiter: red gains most (sky red weight 1 - a/2)
    # pixels whose 100 samples all missed (one hit_world call each) are the same in both modes:
    # the primary ray IS the ray that missed
    pure = seg == 100
    assert pure.sum() > 2000
    top = diff_stats(lv[pure], ref[pure])
    assert max(abs(b) for b in top["bias"]) <= 0.3 and top["mean"] <= 0.6, top


def test_policies_agree_when_only_the_policy_differs(oracle, native):
    """Serial policy vs CUDA policy with the SAME loop form and the SAME (primary-ray) sky at
    converged sample counts: block means agree to ~1 level (independent noise only)."""
    from tests.conftest import compact
    W, H, S, B = 48, 28, 1500, 50
    ser = p3_levels(oracle.render_serial(3, W, H, S, B, loop_form=ITERATIVE, sky_mode=SKY_PRIMARY)[0]).astype(np.float64)
    img, _ = oracle.render(64, compact(oracle.build_scene(3, 64)), native.camera(64, W, H, S, B), 1227)
    cud = to_levels(img).astype(np.float64)
    assert np.abs(ser - cud).mean() < 0.8
    blocks = (ser - cud).reshape(4, H // 4, 4, W // 4, 3).mean(axis=(1, 3))
    assert np.abs(blocks).max() < 1.0, blocks
    assert np.abs((ser - cud).mean(axis=(0, 1))).max() < 0.25


def test_sky_term_known_answers(oracle):
    """camera.h:121-123: a = 0.5*(unit(dir).y + 1); colour = (1-a)*(1,1,1) + a*(0.5,0.7,1.0),
    for un-normalised directions, in every policy."""
    rng = np.random.default_rng(5)
    dirs = [[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, -3], [3, 4, 0], [-13, -2, -3]] + list(rng.normal(size=(40, 3)) * rng.uniform(0.1, 50, (40, 1)))
    for policy, tol in ((0, 1e-15), (64, 1e-15), (32, 3e-7)):
        for d in dirs:
            d = np.asarray(d, np.float64)
            a = 0.5 * (d[1] / np.linalg.norm(d) + 1.0)
            want = (1.0 - a) * np.ones(3) + a * np.array([0.5, 0.7, 1.0])
            got = oracle.sky(policy, d)
            assert np.allclose(got, want, rtol=0, atol=tol), (policy, d, got, want)
            assert abs(got[2] - 1.0) <= tol                        # blue weight is 1 for every direction
    assert np.array_equal(oracle.sky(0, [0, 1, 0]), [0.5, 0.7, 1.0]) and np.array_equal(oracle.sky(32, [0, -2, 0]), [1, 1, 1])


def probe_scene(prec, kind):
    """Two hand-made scenes for the sky-mode known answers: 'empty' = one tiny far-away sphere that
    no ray meets (the C-ABI wants a non-empty table); 'mirror' = the same plus a perfect mirror
    (metal, albedo 1, fuzz 0) of radius 6 at the look-at point, which covers the whole 20-degree
    view from (13,2,3) (angular radius 26 degrees against 18 for the frame's corner)."""
    dt = np.float32 if prec == 32 else np.float64
    cr = [[2000.0, 3000.0, 500.0, 0.01]]
    af = [[0.5, 0.5, 0.5, 0.0]]
    ty = [0]
    if kind == "mirror":
        cr.append([0.0, 0.0, 0.0, 6.0]); af.append([1.0, 1.0, 1.0, 0.0]); ty.append(1)
    n = len(ty)
    return {"center_radius": np.array(cr, dt), "albedo_fuzz": np.array(af, dt), "refraction_index": np.zeros(n, dt),
            "type": np.array(ty, np.int32), "valid": np.ones(n, np.int32)}


@pytest.mark.parametrize("prec", [32, 64])
def test_sky_comes_from_the_primary_ray_mirror_known_answer(oracle, native, prec):
    """camera.h:121 shades a miss with the PRIMARY ray r, not the ray that missed.  Known answer:
    in front of a perfect mirror every path is hit -> reflect -> miss, attenuation exactly 1, so
    with 1 sample per pixel the CUDA program's image of the mirror is BIT-IDENTICAL to the image
    of the empty scene (same jitter and lens draws come first), while the serial program's rule
    (sky from the current = reflected ray) gives a different picture.  Also checks the empty
    image against the analytic gradient of the pixel-centre directions."""
    W, H = 64, 40
    cam = native.camera(prec, W, H, 1, 10)
    empty, st_e = oracle.render(prec, probe_scene(prec, "empty"), cam, 1227)
    mirror, st_m = oracle.render(prec, probe_scene(prec, "mirror"), cam, 1227)
    assert st_e[1] == W * H and st_m[1] == 2 * W * H               # miss | hit + miss, for every pixel
    assert np.array_equal(empty.view(np.uint8), mirror.view(np.uint8))
    cur, _ = oracle.render(prec, probe_scene(prec, "mirror"), cam, 1227, sky_mode=SKY_CURRENT)
    assert np.abs(cur.astype(np.float64) - mirror).mean() > 0.02    # the reflected rays see another part of the sky
    # analytic: pixel^2 = sky(unit(pixel centre - camera centre)) up to jitter (half a pixel) and lens (radius 0.052)
    p00, du, dv, c = (np.array(list(x), np.float64) for x in (cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v, cam.center))
    jj, ii = np.mgrid[0:H, 0:W]
    d = p00 + ii[..., None] * du + jj[..., None] * dv - c
    a = 0.5 * (d[..., 1] / np.linalg.norm(d, axis=-1) + 1.0)
    want = (1.0 - a)[..., None] * np.ones(3) + a[..., None] * np.array([0.5, 0.7, 1.0])
    # |d sky / d uy| <= 0.25 per unit of uy; a pixel is |dv|/10 of uy, the lens 0.052/10
    slack = 0.25 * (np.linalg.norm(dv) + np.linalg.norm(du) + 0.06) / 10.0
    assert np.abs(empty.astype(np.float64) ** 2 - want).max() <= slack


def test_full_frame_goldens_are_what_the_oracle_renders(oracle, native, golden_dir):
    """tests/golden/full_frame_crcs.json (the -m gpu full-frame parity test compares the HIP path with it) is the
    oracle's output: structure, and three whole rows of every frame re-rendered here (sky / glass band / ground)."""
    import zlib
    from tests.conftest import compact
    from tests.golden.make_full_frame_crcs import CONFIGS
    gold = json.load(open(os.path.join(golden_dir, "full_frame_crcs.json")))
    assert set(gold) <= {c[0] for c in CONFIGS} and len(gold) >= 3
    for name, prec, scene_id, W, H, S, B in CONFIGS:
        if name not in gold:
            continue
        g = gold[name]
        assert (g["precision"], g["scene_id"], g["width"], g["height"], g["samples"], g["bounces"], g["seed"]) == (prec, scene_id, W, H, S, B, 1227)
        assert len(g["row_crc32"]) == H and len(g["sha256"]) == 64 and g["oracle_stats"][0] == W * H * S
        if S > 100:
            continue                                           # the 500 spp frame: structure only (a row is 1e6 rays)
        scene = compact(oracle.build_scene(scene_id, prec))
        cam = native.camera(prec, W, H, S, B)
        for row in (3, (H * 57) // 100, H - 2):
            img, _ = oracle.render(prec, scene, cam, 1227, row, row + 1)
            assert zlib.crc32(img.view(np.uint8).tobytes()) & 0xffffffff == g["row_crc32"][row], (name, row)
