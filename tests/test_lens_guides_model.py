"""tests/lens_guides_model.py pinned on the CPU: the CRC-32 of its planes on two small frames; the model against a scalar restatement of
INTEGRATION.md section 18 written ray by ray; the lattice's stated properties; a chain that ends at its first hit, from a lattice
collapsed to the lens point (0, 0), is tests/preview_model.py's guides_np bit for bit, and with bounces its chain_np; and the cameras
and frames of tests/test_lens_guides.py see what that test relies on -- lens rays of one pixel that meet different spheres.
tests/test_lens_guides.py compares the library with the model bit for bit; this keeps the model itself from moving where there is no GPU."""
import zlib

import numpy as np
import pytest

from tests.lens_guides_model import KAPPA, chain_from, lens_guides_np, lens_points, lens_ray_np, scene_of, targets
from tests.preview_model import LATTICE, chain_np, guides_np, same_bits

INF = float("inf")
WIDE = 10.0                     # degrees of defocus: lens rays of one pixel see different spheres even on frames a few pixels wide
# (scene, W, H, G, max_bounces_eff) -> precision -> CRC-32 of normal | albedo | depth | bounces
PINS = {
    (3, 13, 9, 2, 0): {32: "d7d0b2dc", 64: "0eb12294"},
    (3, 13, 9, 4, 8): {32: "1365462f", 64: "f26e3ea1"},
    (1, 11, 7, 4, 0): {32: "c8160c03", 64: "c296b4f2"},
    (LATTICE, 11, 7, 2, 8): {32: "cceb9f28", 64: "176ea48c"},
}


def _crc(planes):
    return "%08x" % (zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in planes)) & 0xffffffff)


def wide(rt, prec, W, H):
    """The reference's view through a 10-degree aperture; in the material lattice that camera sits inside a glass sphere."""
    return rt.camera_look(prec, W, H, 1, 10, defocus_angle=WIDE)


def scalar_chain(T, oracle, prec, sc, O, D, max_bounces, max_fuzz):
    """Section 12's chain of ONE ray on scalars of T: the second statement the vectorised model is held to."""
    cr = np.asarray(sc["center_radius"], T).reshape(-1, 4)
    af = np.asarray(sc["albedo_fuzz"], T).reshape(-1, 4)
    eta = np.asarray(sc["refraction_index"], T).reshape(-1)
    ty = np.asarray(sc["type"]).reshape(-1)
    d3 = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    A, Z, b = [T(1)] * 3, T(0), 0
    zero = [T(0)] * 3
    with np.errstate(all="ignore"):
        while True:
            t, k = oracle.hit_world(prec, cr, np.array([list(O) + list(D)], T))
            t, k = T(t[0]), int(k[0])
            if k < 0:
                return (zero, zero, T(0), 0) if b == 0 else (zero, A, Z, b)
            P = [O[c] + t * D[c] for c in range(3)]
            inv_r = T(1) / cr[k, 3]
            out = [(P[c] - cr[k, c]) * inv_r for c in range(3)]
            front = d3(D, out) < 0
            N = out if front else [-v for v in out]
            glass, metal = ty[k] == 2, ty[k] == 1
            specular = glass or (metal and float(af[k, 3]) <= max_fuzz)
            An = A if glass else [A[c] * af[k, c] for c in range(3)]
            Zn = Z + t
            if not specular or b == max_bounces:
                return N, An, Zn, b
            A, Z, O, b = An, Zn, P, b + 1
            if not glass:
                c2 = T(2) * d3(D, N)
                D = [D[c] - c2 * N[c] for c in range(3)]
            else:
                ln = np.sqrt(d3(D, D))
                il = T(1) / ln
                u = [D[c] * il for c in range(3)]
                m = -d3(u, N)
                ct = m if m < 1 else T(1)
                st = np.sqrt(T(1) - ct * ct)
                ri = T(1) / eta[k] if front else eta[k]
                if ri * st > 1:
                    c2 = T(2) * -ct
                    r = [u[c] - c2 * N[c] for c in range(3)]
                else:
                    perp = [ri * (u[c] + ct * N[c]) for c in range(3)]
                    kk = -np.sqrt(np.abs(T(1) - d3(perp, perp)))
                    r = [perp[c] + kk * N[c] for c in range(3)]
                D = [r[c] * ln for c in range(3)]


def scalar_lens_guides(T, oracle, prec, sc, cam, rows, G, max_bounces_eff, max_fuzz):
    """INTEGRATION.md section 18 pixel by pixel and ray by ray on scalars of T."""
    W = cam.img_width
    C, U, V, p00, du, dv = ([T(x) for x in v[:]] for v in (cam.center, cam.defocus_disk_u, cam.defocus_disk_v, cam.pixel00_loc,
                                                          cam.pixel_delta_u, cam.pixel_delta_v))
    kappa = T(1) if G == 2 else T(0.8944271909999159)
    normal = np.zeros((len(rows), W, 3), T); albedo = np.zeros((len(rows), W, 3), T); depth = np.zeros((len(rows), W), T)
    bounces = np.zeros((len(rows), W), np.int32)
    for jl, j in enumerate(rows):
        for i in range(W):
            ps = [(p00[c] + T(i) * du[c]) + T(j) * dv[c] for c in range(3)]
            Ns, As, Zs, bm = [T(0)] * 3, [T(0)] * 3, T(0), 0
            for s in range(G * G):
                a, b = s % G, s // G
                lx = kappa * (T(2 * a + 1) / T(G) - T(1))
                ly = kappa * (T(2 * b + 1) / T(G) - T(1))
                Os = [(C[c] + lx * U[c]) + ly * V[c] for c in range(3)]
                Ds = [ps[c] - Os[c] for c in range(3)]
                n, al, z, bs = scalar_chain(T, oracle, prec, sc, Os, Ds, max_bounces_eff, max_fuzz)
                Ns = [Ns[c] + n[c] for c in range(3)]; As = [As[c] + al[c] for c in range(3)]; Zs = Zs + z
                bm = max(bm, bs)
            q = T(1) / T(G * G)
            normal[jl, i] = [v * q for v in Ns]; albedo[jl, i] = [v * q for v in As]; depth[jl, i] = Zs * q
            bounces[jl, i] = bm
    return normal, albedo, depth, bounces


@pytest.mark.parametrize("prec", [32, 64])
def test_the_lattice_is_as_stated(prec):
    T = np.float32 if prec == 32 else np.float64
    assert [float(x) for x, _ in lens_points(T, 2)[:2]] == [-0.5, 0.5]
    assert [float(y) for _, y in lens_points(T, 2)] == [-0.5, -0.5, 0.5, 0.5]            # b is the outer index
    k = float(T(KAPPA[4]))
    assert [float(x) for x, _ in lens_points(T, 4)[:4]] == [float(T(k) * T(o)) for o in (-0.75, -0.25, 0.25, 0.75)]
    for G in (2, 4):
        pts = np.array(lens_points(T, G), np.float64)
        assert len(pts) == G * G and np.hypot(pts[:, 0], pts[:, 1]).max() < 1            # every point inside the unit disk
        assert np.array_equal(np.sort(pts, axis=0), np.sort(-pts, axis=0))       # symmetric about the lens centre
    # the 4 x 4 lattice has the uniform unit disk's second moment per axis, 1/4; the 2 x 2 lattice has it exactly
    assert (np.array(lens_points(T, 2), np.float64) ** 2).mean(0).tolist() == [0.25, 0.25]
    np.testing.assert_allclose((np.array(lens_points(T, 4), np.float64) ** 2).mean(0), 0.25, rtol=1e-6)
    assert float(T(1) / T(4)) == 0.25 and float(T(1) / T(16)) == 0.0625


@pytest.mark.parametrize("case", list(PINS), ids=lambda c: "s%s_%dx%d_g%d_b%d" % c)
@pytest.mark.parametrize("prec", [32, 64])
def test_the_model_keeps_its_bits_and_is_the_scalar_statement(native, oracle, prec, case):
    scene, W, H, G, mb = case
    T = np.float32 if prec == 32 else np.float64
    cam = wide(native, prec, W, H)
    rows = np.arange(H)
    got = lens_guides_np(native, oracle, prec, scene, cam, rows, G, mb, INF)
    assert [a.dtype for a in got] == [T, T, T, np.int32] and all(np.isfinite(a).all() for a in got)
    want = scalar_lens_guides(T, oracle, prec, scene_of(native, scene, prec), cam, rows, G, mb, INF)
    for name, a, b in zip(("normal", "albedo", "depth", "bounces"), got, want):
        assert same_bits(a, b), (case, name)
    # a blurred normal is no longer than a unit normal, and some are visibly shorter; a first-hit chain has no bounces
    length = np.sqrt((got[0].astype(np.float64) ** 2).sum(-1))
    assert length.max() <= 1 + 1e-6 and (length[got[2] > 0] < 0.99).any()
    assert (got[3] == 0).all() if mb == 0 else got[3].max() >= 1
    assert _crc(got) == PINS[case][prec], (case, prec, _crc(got))


@pytest.mark.parametrize("scene", [1, 3])
@pytest.mark.parametrize("prec", [32, 64])
def test_a_collapsed_lattice_is_the_centre_ray(native, oracle, prec, scene):
    """Lens point (0, 0): O_s = (O + 0 U) + 0 V = O, so with max_bounces_eff = 0 the per-ray values are guides_np's, and with bounces
    chain_np's, bit for bit."""
    W, H = 29, 19
    rows = np.arange(H)
    sc = scene_of(native, scene, prec)
    for cam in (native.camera(prec, W, H, 1, 10), wide(native, prec, W, H)):
        n, a, z, b = lens_ray_np(oracle, prec, sc, cam, rows, 0.0, 0.0, 0, INF)
        wn, wa, wz, hit = guides_np(native, oracle, prec, scene, cam, rows)
        assert hit.any() and not hit.all() and not b.any()
        assert same_bits(n, wn) and same_bits(a, wa) and same_bits(z, wz)
        got = lens_ray_np(oracle, prec, sc, cam, rows, 0.0, 0.0, 8, INF)
        want = chain_np(native, oracle, prec, scene, cam, rows, 8, INF)
        assert want[3].max() >= 1
        for x, y in zip(got, want[:4]):
            assert same_bits(x, y)


@pytest.mark.parametrize("scene", [1, 3])
@pytest.mark.parametrize("size", [(33, 17), (64, 40)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("prec", [32, 64])
def test_the_wide_lens_sees_different_spheres(native, oracle, prec, size, scene):
    """What keeps tests/test_lens_guides.py from being vacuous, asserted on the model alone: with the 10-degree camera the G = 2 albedo
    plane differs from the first-hit albedo plane in at least 10 % of the pixels (20 to 67 % at these frames)."""
    W, H = size
    cam = wide(native, prec, W, H)
    rows = np.arange(H)
    lens = lens_guides_np(native, oracle, prec, scene, cam, rows, 2, 0, INF)
    first = guides_np(native, oracle, prec, scene, cam, rows)
    differ = (lens[1] != first[1]).any(-1)
    assert differ.mean() >= 0.10, (prec, size, scene, float(differ.mean()))
    assert not same_bits(lens[2], first[2])
