"""Scenes at the ends of the number range: scene 3 with albedos alone edited, so that rays, hits, RNG draws and segment counts stay
scene 3's and only COLOURS overflow, go NaN or go subnormal (tests/test_number_range.py).  No geometry and no refraction index is
touched, and no loop's exit depends on an albedo.

range_scene(): the small lambertian spheres (type 0, r < 1) in index order, in four interleaved groups -- albedo NaN, +inf, `bright`,
`dark` --, the big lambertian (r == 1) `dark`, every second small metal `bright`.  bright / dark are 1e7 / 1e-40 in fp32 (1e7 overflows
after six bounces, 1e-40 is subnormal) and 1e40 / 1e-310 in fp64.

valid_range_scene(): valid input only -- every albedo finite and >= 0 -- with the ground at 1e7: fp32 overflows along a 50-bounce path,
fp64 does not.

classes() sorts a gamma-encoded frame's pixels: the framebuffer shows a NaN sum as 0, an overflowed sum as +inf and a subnormal linear
value as a value below sqrt(tiny)."""
import numpy as np

from tests.conftest import compact

LAMBERTIAN, METAL = 0, 1
BRIGHT = {32: 1e7, 64: 1e40}
DARK = {32: 1e-40, 64: 1e-310}
SETTINGS = ((2, 50), (4, 12))                # (samples, bounces)
FRAMES = ((64, 40), (33, 17))


def _dtype(prec):
    return np.float32 if prec == 32 else np.float64


def plain_scene(rt, prec):
    """compact(scene 3): what both variants edit."""
    sc = compact(rt.build_scene(3, prec))
    return {k: (v.copy() if hasattr(v, "shape") else v) for k, v in sc.items()}


def range_scene(rt, prec):
    sc = plain_scene(rt, prec)
    af, r, ty = sc["albedo_fuzz"], sc["center_radius"][:, 3], sc["type"]
    small = np.flatnonzero((ty == LAMBERTIAN) & (r < 1))
    for group, value in enumerate((np.nan, np.inf, BRIGHT[prec], DARK[prec])):
        af[small[group::4], :3] = value
    af[np.flatnonzero((ty == LAMBERTIAN) & (r == 1)), :3] = DARK[prec]
    af[np.flatnonzero((ty == METAL) & (r < 1))[::2], :3] = BRIGHT[prec]
    assert af.dtype == _dtype(prec)
    sc["name"] = "range"                             # what caches of CPU results keep these tables under
    return sc


def valid_range_scene(rt, prec):
    sc = plain_scene(rt, prec)
    ground = np.flatnonzero(sc["center_radius"][:, 3] == 1000)
    assert len(ground) == 1
    sc["albedo_fuzz"][ground, :3] = 1e7
    a = sc["albedo_fuzz"][:, :3]
    assert np.isfinite(a).all() and (a >= 0).all()
    sc["name"] = "valid_range"
    return sc


def classes(fb):
    """Pixels of a gamma-encoded frame by class: {"inf", "zero", "subnormal", "normal"}.  A pixel counts once, in the first class one of
    its channels falls in."""
    tiny = np.finfo(fb.dtype).tiny
    root = np.sqrt(fb.dtype.type(tiny))
    inf = np.isinf(fb).any(axis=-1)
    zero = ~inf & (fb == 0).any(axis=-1)
    sub = ~inf & ~zero & ((fb > 0) & (fb < root)).any(axis=-1)
    normal = ~inf & ~zero & ~sub
    return {"inf": int(inf.sum()), "zero": int(zero.sum()), "subnormal": int(sub.sum()), "normal": int(normal.sum())}


def linear_classes(lin):
    """Channels of a linear image by class: NaN, +inf, -inf, subnormal (non-zero, below tiny), zero, normal."""
    tiny = np.finfo(lin.dtype).tiny
    with np.errstate(invalid="ignore"):
        mag = np.abs(lin)
        return {"nan": int(np.isnan(lin).sum()), "+inf": int((lin == np.inf).sum()), "-inf": int((lin == -np.inf).sum()),
                "subnormal": int(((mag > 0) & (mag < tiny)).sum()), "zero": int((lin == 0).sum()),
                "normal": int(((mag >= tiny) & np.isfinite(lin)).sum())}
