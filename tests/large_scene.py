"""Scenes for the large-scene tests and probe (rtiow_render_large): the jittered lattice beyond a compute unit's LDS, the line whose grid
is longer than any walk of the LDS grid, the six random scenes of tests/test_gpu_parity.py's
test_grid_walk_equals_exact_loop_on_random_scenes, restated (that test builds them inline), and five scenes for the regimes of the
device grid's walk that those do not reach (EDGE_SCENES)."""
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


def centre_of(cr):
    """centre() of a table [n, 4] = {cx, cy, cz, r}."""
    cr = np.asarray(cr, np.float64)
    with np.errstate(invalid="ignore"):
        keep = (cr[:, 3] < 100.0) & np.isfinite(cr[:, :3]).all(axis=1)
    return cr[keep, :3].mean(axis=0).astype(np.float32).astype(np.float64)


def centre(scene):
    """The library's recentring point for the device grid: the centroid of the finite spheres with r < 100, rounded to fp32."""
    return centre_of(scene["center_radius"])


# ---- scenes for the structural regimes of the device grid's walk that the lattice and the line do not reach (tests/test_render_large_edges.py).
# Each stays far inside the LDS in both precisions, so the exact loop (RTIOW_SCENE_LDS_EXACT) is a reference for it on the GPU, and each
# is pinned to the property it exists for, without a GPU, in tests/test_large_grid_plan.py.
EDGE_SCENES = ("clusters", "equal_no_ground", "mixed_with_bad", "far_centre", "sparse_wide")
CLUSTER_SIZES = tuple(range(1, 25))
CLUSTERS_WITH_TWINS = (2, 5, 8, 11, 14, 17, 20, 23)                 # sizes of the clusters whose last sphere repeats their first
MIXED_BAD = {"negative_radius": 105, "nan_radius": 305, "inf_centre": 505, "zero_radius": 705}


@functools.lru_cache(maxsize=None)
def clusters(prec=32):
    """The ground, 600 spheres (r = 0.2) scattered over 40 x 40 and 24 clusters of 1, 2, ..., 24 spheres within 0.05 of a common point
    (r in [0.15, 0.2], heights spread over 0.3): long lists of odd and even lengths, mixed radii and heights.  In eight clusters the last
    sphere is an exact copy of the first, the cluster's largest and highest: equal roots, of which the lower index must win."""
    dt = np.float32 if prec == 32 else np.float64
    rng = np.random.default_rng(2401)
    rows = [(0.0, -1000.0, 0.0, 1000.0)]
    rows += [(x, 0.2, z, 0.2) for x, z in rng.uniform(-20, 20, (600, 2))]
    for k in CLUSTER_SIZES:
        px, pz = rng.uniform(-18, 18, 2)
        first = len(rows)
        for _ in range(k):
            r = rng.uniform(0.15, 0.2)
            rows.append((px + rng.uniform(-0.035, 0.035), r + rng.uniform(0.0, 0.3), pz + rng.uniform(-0.035, 0.035), r))
        if k in CLUSTERS_WITH_TWINS:
            x, _, z, _ = rows[first]
            rows[first] = (x, 0.5, z, 0.2)
            rows[-1] = rows[first]
    return _scene(np.array(rows), rng, dt)


def twins(scene):
    """[(lower index, higher index)] of the spheres of `scene` that are exact copies of one another in centre and radius."""
    cr = np.asarray(scene["center_radius"])
    seen, out = {}, []
    for i, row in enumerate(cr):
        key = row.tobytes()
        if key in seen:
            out.append((seen[key], i))
        else:
            seen[key] = i
    return out


@functools.lru_cache(maxsize=None)
def equal_no_ground(prec=32):
    """900 spheres (r = 0.2) on a jittered 30 x 30 lattice at heights in [0, 3] and nothing else: an empty direct list, a thick slab."""
    dt = np.float32 if prec == 32 else np.float64
    rng = np.random.default_rng(2402)
    k = np.arange(900)
    cr = np.zeros((900, 4))
    cr[:, 0] = k % 30 - 15 + rng.uniform(-0.25, 0.25, 900)
    cr[:, 2] = k // 30 - 15 + rng.uniform(-0.25, 0.25, 900)
    cr[:, 1] = rng.uniform(0.0, 3.0, 900); cr[:, 3] = 0.2
    return _scene(cr, rng, dt)


@functools.lru_cache(maxsize=None)
def mixed_with_bad(prec=32):
    """The ground, four big spheres and 800 of r in [0.05, 0.35] at heights in [-1, 3] over 30 x 30; four of the small ones overwritten
    with r = -0.3, r = NaN, cx = +inf and r = 0 (MIXED_BAD): a direct list that is no multiple of four and holds spheres the plan cannot
    grid.  For the ray-by-ray tests only: never a picture."""
    dt = np.float32 if prec == 32 else np.float64
    rng = np.random.default_rng(2403)
    cr = np.zeros((805, 4))
    cr[0] = (0, -1000, 0, 1000)
    cr[1:5] = [(0, 1, 0, 1), (-6, 1, 3, 1), (7, 1, -4, 1), (2, 1.5, 9, 1.5)]
    cr[5:, 0] = rng.uniform(-15, 15, 800); cr[5:, 2] = rng.uniform(-15, 15, 800)
    cr[5:, 1] = rng.uniform(-1.0, 3.0, 800); cr[5:, 3] = rng.uniform(0.05, 0.35, 800)
    cr[MIXED_BAD["negative_radius"], 3] = -0.3
    cr[MIXED_BAD["nan_radius"], 3] = np.nan
    cr[MIXED_BAD["inf_centre"], 0] = np.inf
    cr[MIXED_BAD["zero_radius"], 3] = 0.0
    return _scene(cr, rng, dt)


@functools.lru_cache(maxsize=None)
def far_centre(prec=32):
    """900 spheres (r = 0.2) on a jittered 30 x 30 lattice on a ground, all of it translated by (3000, 0, -2000): eps, which grows with
    the largest coordinate, is a quarter of a radius."""
    dt = np.float32 if prec == 32 else np.float64
    rng = np.random.default_rng(2404)
    k = np.arange(900)
    cr = np.zeros((901, 4))
    cr[0] = (0, -1000, 0, 1000)
    cr[1:, 0] = k % 30 - 15 + rng.uniform(-0.25, 0.25, 900)
    cr[1:, 2] = k // 30 - 15 + rng.uniform(-0.25, 0.25, 900)
    cr[1:, 1] = 0.2; cr[1:, 3] = 0.2
    cr[:, 0] += 3000.0; cr[:, 2] -= 2000.0
    return _scene(cr, rng, dt)


@functools.lru_cache(maxsize=None)
def sparse_wide(prec=32):
    """The ground and 1 000 spheres (r = 0.2) scattered over 4000 x 4000: cells hundreds of radii wide, a slab tens of radii thick."""
    dt = np.float32 if prec == 32 else np.float64
    rng = np.random.default_rng(2405)
    cr = np.zeros((1001, 4))
    cr[0] = (0, -1000, 0, 1000)
    cr[1:, 0] = rng.uniform(-2000, 2000, 1000); cr[1:, 2] = rng.uniform(-2000, 2000, 1000)
    cr[1:, 1] = 0.2; cr[1:, 3] = 0.2
    return _scene(cr, rng, dt)


def edge_scene(name, prec=32):
    return {"clusters": clusters, "equal_no_ground": equal_no_ground, "mixed_with_bad": mixed_with_bad, "far_centre": far_centre,
            "sparse_wide": sparse_wide}[name](prec)


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
