"""Scenes for the volume-scene tests and probe (rtiow_render_volume): jittered cubic lattices that fill a volume, with and without a
ground, a stack of layers, a column taller than any walk of the LDS grid, a Gaussian cloud, the flat lattice of the large-scene tests, a
cube with spheres the plan cannot grid, and a scene the plan refuses."""
import functools

import numpy as np

from tests import large_scene
from tests.large_scene import _scene, centre, centre_of, ten_spheres  # noqa: F401  (the recentring point is the device grid's)

WITH_BAD = {"negative_radius": 105, "nan_radius": 305, "inf_centre": 505, "zero_radius": 705}


def _dt(prec):
    return np.float32 if prec == 32 else np.float64


def _lattice3(rng, side):
    """side^3 centres at pitch 1, jittered by +-0.3, centred in x and z, y from 0.5 up."""
    k = np.arange(side ** 3)
    c = np.column_stack([k % side - 0.5 * (side - 1), k // (side * side) + 0.5, (k // side) % side - 0.5 * (side - 1)]).astype(np.float64)
    return c + rng.uniform(-0.3, 0.3, c.shape)


@functools.lru_cache(maxsize=None)
def cube(side, prec=32):
    """The ground (r = 1000) and side^3 spheres of r = 0.2 on a jittered cubic lattice above it: side^3 + 1 in all."""
    rng = np.random.default_rng(3000 + side)
    cr = np.zeros((side ** 3 + 1, 4))
    cr[0] = (0, -1000, 0, 1000)
    cr[1:, :3] = _lattice3(rng, side); cr[1:, 3] = 0.2
    return _scene(cr, rng, _dt(prec))


@functools.lru_cache(maxsize=None)
def cube_no_ground(side, prec=32):
    rng = np.random.default_rng(3100 + side)
    cr = np.zeros((side ** 3, 4))
    cr[:, :3] = _lattice3(rng, side); cr[:, 3] = 0.2
    return _scene(cr, rng, _dt(prec))


@functools.lru_cache(maxsize=None)
def slab_of_layers(prec=32):
    """The ground and 3 layers of a jittered 40 x 40 lattice (r = 0.2) at y = 0.5, 1.5, 2.5."""
    rng = np.random.default_rng(3200)
    k = np.arange(3 * 1600)
    cr = np.zeros((len(k) + 1, 4))
    cr[0] = (0, -1000, 0, 1000)
    cr[1:, 0] = k % 40 - 19.5; cr[1:, 1] = k // 1600 + 0.5; cr[1:, 2] = (k // 40) % 40 - 19.5
    cr[1:, :3] += rng.uniform(-0.3, 0.3, (len(k), 3)); cr[1:, 3] = 0.2
    return _scene(cr, rng, _dt(prec))


@functools.lru_cache(maxsize=None)
def column(prec=32):
    """2 000 spheres (r = 0.2) stacked along y at pitch 0.5 and nothing else: more than 128 cells along y."""
    rng = np.random.default_rng(3300)
    cr = np.zeros((2000, 4))
    cr[:, 1] = 0.5 * np.arange(2000); cr[:, 3] = 0.2
    cr[:, [0, 2]] = rng.uniform(-0.05, 0.05, (2000, 2))
    return _scene(cr, rng, _dt(prec))


@functools.lru_cache(maxsize=None)
def gauss_cloud(prec=32):
    """The ground and 20 000 spheres (r = 0.2) drawn from a Gaussian of sigma = 6 around (0, 20, 0): where a uniform grid stops helping."""
    rng = np.random.default_rng(3400)
    cr = np.zeros((20001, 4))
    cr[0] = (0, -1000, 0, 1000)
    cr[1:, :3] = rng.normal(0.0, 6.0, (20000, 3)) + np.array([0.0, 20.0, 0.0]); cr[1:, 3] = 0.2
    return _scene(cr, rng, _dt(prec))


def flat(prec=32, n=6000):
    return large_scene.lattice(n, prec)


@functools.lru_cache(maxsize=None)
def with_bad(prec=32):
    """cube(14) with four of its spheres overwritten with r = -0.3, r = NaN, cx = +inf and r = 0 (WITH_BAD) and two unit spheres added:
    a direct list of seven with the ground, more than one packed trip.  The non-finite coordinate clears range_flags bit 1 (the walk
    then divides instead of multiplying by one reciprocal).  For the ray-by-ray tests only: never a picture."""
    rng = np.random.default_rng(3500)
    base = np.asarray(cube(14, 64)["center_radius"], np.float64)
    cr = np.vstack([base, [(-3.0, 16.0, 2.0, 1.0), (4.0, 7.5, -9.5, 1.0)]])
    cr[WITH_BAD["negative_radius"], 3] = -0.3
    cr[WITH_BAD["nan_radius"], 3] = np.nan
    cr[WITH_BAD["inf_centre"], 0] = np.inf
    cr[WITH_BAD["zero_radius"], 3] = 0.0
    return _scene(cr, rng, _dt(prec))


def scene_in_range(scene):
    """library/handle.h's scene_in_range over the spheres (range_flags bit 1; the test cameras' lenses lie within a few units of the
    origin): every |coordinate| + |radius| finite and below 2^18, a NaN passed over as std::fmax passes it over.  Where it is False the
    walks divide by a instead of multiplying by one refined reciprocal (FastDiv off)."""
    cr = np.asarray(scene["center_radius"], np.float64)
    with np.errstate(invalid="ignore"):
        reach = np.nanmax(np.abs(cr[:, :3]) + np.abs(cr[:, 3:4]))
    return bool(np.isfinite(reach) and reach < 2.0 ** 18)


def fits_lds(scene, prec):
    """layout_lds: the exact loop's table of the scene fits a compute unit's LDS with room to spare (RTIOW_SCENE_LDS_EXACT applies)."""
    m = len(scene["type"])
    return (prec // 8) * 4 * ((m + 4) // 4 * 4) <= 128 * 1024
