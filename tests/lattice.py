"""The material lattice: one scene that holds every material parameter the reference scenes never feed the shade step
(tests/test_scatter.py, test_render_on_the_material_lattice).  52 spheres, all valid:

  0        the ground (radius 1000, lambertian)
  1        a lambertian unit sphere at the origin (the near_zero fallback is crafted on it)
  2        a glass sphere of radius 2 around the default camera (13, 2, 3)
  3, 4     a hollow glass sphere: outer radius 1, inner radius -0.9, same centre; 5, 6: another, index 2.417, radius 0.5 / -0.45
  7        a big distant metal sphere (radius 25)
  8, 9     two small spheres of radius 1e-3 and 0.05
  10 ...   a 7 x 6 field: one glass sphere per refraction index of INDEX (radii 0.25 / 0.5: exact reciprocals), one metal per fuzz of
           FUZZ, lambertians for the rest; albedo components drawn from ALBEDO.

Every centre is a multiple of 1/64, so that crafted hit points C + r n on an axis are exact in both precisions."""
import numpy as np

FUZZ = [0.0, 1e-7, 0.3, 1.0 - 2.0 ** -24, 1.0, 1.5, 4.0]
INDEX = [1.5, 1.0, 1.0 + 2.0 ** -20, 1.33, 2.417, 2.0 / 3.0, 0.1, 10.0, 1e3, 1e-3]
ALBEDO = [0.0, 0.5, 1.0, 1.5, 1e-40]
LAMBERTIAN, METAL, DIELECTRIC = 0, 1, 2
UNIT_LAMBERTIAN = 1


def lattice_scene(prec):
    dt = np.float32 if prec == 32 else np.float64
    rng = np.random.default_rng(20240611)
    cr, af, ri, ty = [], [], [], []

    def add(c, r, t, albedo=(0.0, 0.0, 0.0), fuzz=0.0, index=0.0):
        cr.append((c[0], c[1], c[2], r)); af.append((albedo[0], albedo[1], albedo[2], fuzz)); ri.append(index); ty.append(t)

    add((0, -1000, 0), 1000.0, LAMBERTIAN, (0.5, 0.5, 0.5))
    add((0, 0, 0), 1.0, LAMBERTIAN, (0.5, 1.0, 1.5))
    add((13, 2, 3), 2.0, DIELECTRIC, index=1.5)
    add((-4, 1, 0), 1.0, DIELECTRIC, index=1.5); add((-4, 1, 0), -0.9, DIELECTRIC, index=1.5)
    add((4, 0.5, 1.5), 0.5, DIELECTRIC, index=2.417); add((4, 0.5, 1.5), -0.45, DIELECTRIC, index=2.417)
    add((-30, 20, -40), 25.0, METAL, (1.0, 0.5, 1.5), fuzz=0.3)
    add((2.5, 0.5, 2.25), 1e-3, LAMBERTIAN, (1.0, 1.0, 1.0)); add((3.0, 0.75, -0.5), 0.05, METAL, (0.5, 0.5, 1.0), fuzz=0.0)
    kinds = [(DIELECTRIC, i) for i in INDEX] + [(METAL, f) for f in FUZZ] + [(LAMBERTIAN, None)] * 25
    order = rng.permutation(len(kinds))
    cells = [(ix, iz) for ix in range(7) for iz in range(6)]
    for (ix, iz), k in zip(cells, order):
        t, v = kinds[k]
        r = float(rng.choice([0.25, 0.5])) if t == DIELECTRIC else float(rng.choice([0.05, 0.2, 0.3, 0.45]))
        jitter = rng.integers(-16, 17, 2) / 64.0
        c = (-4.5 + 1.5 * ix + jitter[0], r, -3.75 + 1.5 * iz + jitter[1])
        albedo = tuple(float(a) for a in rng.choice(ALBEDO, 3))
        if t == DIELECTRIC:
            add(c, r, t, index=v)
        elif t == METAL:
            add(c, r, t, albedo, fuzz=v)
        else:
            add(c, r, t, albedo)
    n = len(ty)
    return {"center_radius": np.array(cr, np.float64).astype(dt), "albedo_fuzz": np.array(af, np.float64).astype(dt),
            "refraction_index": np.array(ri, np.float64).astype(dt), "type": np.array(ty, np.int32), "valid": np.ones(n, np.int32)}
