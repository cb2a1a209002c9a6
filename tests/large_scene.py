"""Scenes for the large-scene tests and probe (rtiow_render_large): the jittered lattice beyond a compute unit's LDS, the line whose grid
is longer than any walk of the LDS grid, and the six random scenes of tests/test_gpu_parity.py's
test_grid_walk_equals_exact_loop_on_random_scenes, restated (that test builds them inline)."""
import functools

import numpy as np

RANDOM_CASES = ("dense_clusters", "mixed_radii_and_heights", "far_from_the_camera", "tiny_spheres", "stacked_no_ground", "touching_pairs")


def _materials(rng, m, dt, ground_rows=1):
    af = np.zeros((m, 4), dt)
    af[:, :3] = rng.uniform(0.1, 0.9, (m, 3)); af[:, 3] = rng.uniform(0, 0.5, m)
    ty = rng.choice([0, 1, 2], m, p=[0.7, 0.2, 0.1]).astype(np.int32)
    ty[:ground_rows] = 0
    return af, ty


def _scene(cr, rng, dt):
    cr = np.asarray(cr, dt)
    af, ty = _materials(rng, len(cr), dt)
    return {"center_radius": cr, "albedo_fuzz": af, "refraction_index": np.full(len(cr), 1.5, dt), "type": ty, "valid": np.ones(len(cr), np.int32)}


@functools.lru_cache(maxsize=None)
def lattice(n, prec=32, seed=11):
    """n spheres (r = 0.2, pitch 1, jittered by a quarter pitch) on the ground, behind the ground and three unit spheres: n + 4 in all."""
    dt = np.float32 if prec == 32 else np.float64
    rng = np.random.default_rng(seed + n)
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    cr = np.zeros((n + 4, 4))
    cr[0] = (0, -1000, 0, 1000)
    cr[1:4] = [(0, 1, 0, 1), (-4, 1, 0, 1), (4, 1, 0, 1)]
    cr[4:, 0] = k % side - 0.5 * side + rng.uniform(-0.25, 0.25, n)
    cr[4:, 2] = k // side - 0.5 * side + rng.uniform(-0.25, 0.25, n)
    cr[4:, 1] = 0.2; cr[4:, 3] = 0.2
    return _scene(cr, rng, dt)


@functools.lru_cache(maxsize=None)
def line(n, prec=32):
    """n spheres (r = 0.2, pitch 1) along x on the ground: a grid of thousands of units by a few."""
    dt = np.float32 if prec == 32 else np.float64
    rng = np.random.default_rng(5)
    cr = np.zeros((n + 1, 4))
    cr[0] = (0, -1000, 0, 1000)
    cr[1:, 0] = np.arange(n) - 0.5 * n; cr[1:, 1] = 0.2; cr[1:, 3] = 0.2
    return _scene(cr, rng, dt)


def ten_spheres(prec=32):
    dt = np.float32 if prec == 32 else np.float64
    cr = np.zeros((10, 4))
    cr[0] = (0, -1000, 0, 1000)
    cr[1:, 0] = np.arange(9) - 4; cr[1:, 1] = 0.2; cr[1:, 3] = 0.2
    return _scene(cr, np.random.default_rng(1), dt)


def centre(scene):
    """The library's recentring point for the device grid: the centroid of the finite spheres with r < 100, rounded to fp32."""
    cr = np.asarray(scene["center_radius"], np.float64)
    keep = (cr[:, 3] < 100.0) & np.isfinite(cr[:, :3]).all(axis=1)
    return cr[keep, :3].mean(axis=0).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def random_case(case):
    """{32: scene, 64: scene} of one of RANDOM_CASES, drawn as test_grid_walk_equals_exact_loop_on_random_scenes draws them (same
    generator, same order: fp32 first)."""
    from tests.test_gpu_parity import _random_field
    rng = np.random.default_rng({"dense_clusters": 1, "mixed_radii_and_heights": 2, "far_from_the_camera": 3, "tiny_spheres": 4,
                                 "stacked_no_ground": 5, "touching_pairs": 6}[case])
    out = {}
    for prec in (32, 64):
        if case == "dense_clusters":
            sc = _random_field(rng, prec, 300, (-6, 6), (-6, 6), lambda g: 0.2, lambda g, r: r)
        elif case == "mixed_radii_and_heights":
            sc = _random_field(rng, prec, 200, (-10, 8), (-10, 8), lambda g: g.choice([0.1, 0.2, 0.3, 0.45]), lambda g, r: g.uniform(r, 2.0),
                               big=[(0.0, 1.0, 0.0, 1.0), (4.0, 1.0, 0.0, 1.0)])
        elif case == "far_from_the_camera":
            sc = _random_field(rng, prec, 200, (-130, -105), (-32, -18), lambda g: g.uniform(0.1, 0.25), lambda g, r: r)
        elif case == "tiny_spheres":
            sc = _random_field(rng, prec, 250, (-8, 8), (-8, 8), lambda g: g.choice([0.002, 0.01, 0.05]), lambda g, r: g.uniform(0.0, 1.5))
        elif case == "stacked_no_ground":
            sc = _random_field(rng, prec, 150, (-4, 6), (-4, 6), lambda g: 0.25, lambda g, r: g.uniform(-3, 4), ground=False)
        else:
            sc = _random_field(rng, prec, 240, (-12, 12), (-12, 12), lambda g: 0.2, lambda g, r: r)
            twin = sc["center_radius"][1:41].copy()
            sc["center_radius"][201:241] = twin
            sc["center_radius"][201:221, 0] += np.float32(0.4) if prec == 32 else 0.4
        out[prec] = sc
    return out
