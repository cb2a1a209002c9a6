"""The scatter step call by call (rtiow_debug_scatter against oracle_scatter): every material branch and every statement of the step.

One call is everything that follows hit_world in a trip of the path loop -- sky on a miss, else hit record and lambertian / metal /
dielectric scatter -- from a caller-supplied (closest, hit), so the tests feed hit records and generator states no render produces.  Every
comparison is on bits (status, colour, O, D, attenuation, depth, the six state words), every family runs in both precisions and in every
form the precision has (0 shade_step<T, false>, 1 the bounded shade_step<T, true>, 2 fp64's shade_front / merged_rounds / shade_back), and
every family first asserts FROM THE ORACLE'S RESULTS that the branches it is about are really taken (the class shares below)."""
import numpy as np
import pytest

from tests.conftest import compact
from tests.lattice import DIELECTRIC, LAMBERTIAN, METAL, UNIT_LAMBERTIAN, lattice_scene

gpu = pytest.mark.gpu
INV_STEP = pow(362437, -1, 2 ** 32)                 # the Weyl word d advances by 362437 per generator step
MIN_SHARE = 0.02
E_BADARG = -1                                       # include/rtiow.h


def _dt(prec):
    return np.float32 if prec == 32 else np.float64


def _forms(prec):
    return (0, 1) if prec == 32 else (0, 1, 2)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _steps(calls, out):
    """Generator steps every call consumed, from the state's d word."""
    return ((out["states"][:, 5].astype(np.uint64) - calls["states"][:, 5].astype(np.uint64)) * INV_STEP) % (2 ** 32)


def _calls(prec, O, D, closest, hit, states, rng, atten=None, sky_uy=None, depth=None):
    dt = _dt(prec)
    n = len(hit)
    with np.errstate(over="ignore"):
        return {"O": np.asarray(O, np.float64).astype(dt), "D": np.asarray(D, np.float64).astype(dt), "closest": np.asarray(closest, np.float64).astype(dt),
                "hit": np.asarray(hit, np.int32), "atten": (rng.uniform(0.0, 2.0, (n, 3)) if atten is None else np.asarray(atten, np.float64)).astype(dt),
                "sky_uy": (rng.uniform(-1.0, 1.0, n) if sky_uy is None else np.asarray(sky_uy, np.float64)).astype(dt),
                "depth": rng.integers(0, 12, n).astype(np.int32) if depth is None else np.asarray(depth, np.int32),
                "states": np.ascontiguousarray(states, np.uint32)}


def _cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _take(calls, idx):
    return {k: v[idx] for k, v in calls.items()}


_STATE_POOL = {}


def _init_states(oracle, n, salt):
    """n states of curand_init over many subsequences and offsets (a pool of 8192 of them, dealt round robin from `salt`)."""
    if "pool" not in _STATE_POOL:
        rng = np.random.default_rng(77)
        seq = rng.integers(0, 2 ** 31, 8192); off = rng.choice([0, 1, 2, 3, 17, 1000, 2 ** 20 + 5, 2 ** 31 + 11], 8192)
        _STATE_POOL["pool"] = np.array([oracle.xorwow_init(1227 + (k & 3), int(seq[k]), int(off[k])) for k in range(8192)], np.uint32)
    return _STATE_POOL["pool"][(np.arange(n) * 13 + salt) % 8192]


def _geometry(scene, calls):
    """In float64, from the inputs: material type, face and shading normal of every call that hits (class counting only)."""
    cr = scene["center_radius"].astype(np.float64)
    hit = calls["hit"]; k = np.maximum(hit, 0)
    O, D, t = calls["O"].astype(np.float64), calls["D"].astype(np.float64), calls["closest"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        P = O + np.where(hit >= 0, t, 0.0)[:, None] * D
        outward = (P - cr[k, :3]) / cr[k, 3:4]
        front = (D * outward).sum(axis=1) < 0
    nrm = np.where(front[:, None], outward, -outward)
    ty = np.where(hit >= 0, scene["type"][k], -1)
    return ty, front, nrm


def _material_classes(scene, calls, out):
    ty, front, nrm = _geometry(scene, calls)
    steps = _steps(calls, out)
    side = (out["D"].astype(np.float64) * nrm).sum(axis=1)
    glass = ty == DIELECTRIC
    return {"miss": ty < 0, "lambertian": ty == LAMBERTIAN,
            "metal kept": (ty == METAL) & (out["status"] == 0), "metal absorbed": (ty == METAL) & (out["status"] == 1),
            "glass total internal reflection": glass & (steps == 0), "glass reflected": glass & (steps > 0) & (side > 0),
            "glass refracted": glass & (steps > 0) & (side < 0)}, front


def _assert_shares(classes, n, floor=MIN_SHARE, counts=None):
    for name, mask in classes.items():
        need = (counts or {}).get(name, int(np.ceil(floor * n)))
        assert int(mask.sum()) >= need, (name, int(mask.sum()), need, n)


def _assert_finite(out):
    for k in ("col", "O", "D", "atten"):
        assert np.isfinite(out[k]).all(), k


def _aimed(rng, scene, k, cos_in, inside, length=None):
    """Hit records on the spheres k [n]: a random point Q of the sphere, a direction that meets the geometric normal there at cos_in
    (from outside, or from inside), the origin a little way back along it and closest the way to Q.  Crafted, not traced."""
    cr = scene["center_radius"].astype(np.float64)
    n = len(k)
    g = _unit(rng, n)
    tang = np.cross(g, _unit(rng, n)); tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    cos_in = np.asarray(cos_in, np.float64) * np.ones(n)
    d = np.where(inside, 1.0, -1.0)[:, None] * cos_in[:, None] * g + np.sqrt(np.maximum(0.0, 1.0 - cos_in ** 2))[:, None] * tang
    length = np.exp(rng.uniform(-2, 2, n)) if length is None else np.asarray(length, np.float64) * np.ones(n)
    D = d * length[:, None]
    r = np.abs(cr[k, 3])
    t = rng.uniform(0.05, 0.9, n) * r * np.where(inside, 2.0 * np.maximum(cos_in, 1e-3), 1.0) / length
    Q = cr[k, :3] + r[:, None] * g
    return Q - t[:, None] * D, D, t, k.astype(np.int32)


# ----------------------------------------------------------------------------------------------------------------------------------
# The twin is the oracle's render (CPU)
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["scene3", "lattice"])
@pytest.mark.parametrize("prec", [32, 64])
def test_the_twin_is_the_oracles_render(native, oracle, prec, which):
    """oracle_hit_world and oracle_scatter chained from the oracle's own primary rays rebuild oracle.render bit for bit (16 x 10, 3 samples,
    12 bounces): the twin the GPU hook is compared with is the arithmetic of the render that every image test trusts."""
    rt = native
    dt = _dt(prec)
    W, H, S, B = 16, 10, 3, 12
    scene = compact(rt.build_scene(3, prec)) if which == "scene3" else lattice_scene(prec)
    cam = rt.camera(prec, W, H, S, B)
    want, _ = oracle.render(prec, scene, cam, 1227)
    npix = W * H
    ij = np.array([(i, j) for j in range(H) for i in range(W)], np.int32)
    states = oracle.xorwow_states(1227, np.arange(npix))
    acc = np.zeros((npix, 3), dt)
    for _ in range(S):
        rays, uy, states = oracle.primary_rays(prec, cam, ij, states)
        O, D = rays[:, :3].copy(), rays[:, 3:].copy()
        atten = np.ones((npix, 3), dt); depth = np.zeros(npix, np.int32)
        col = np.zeros((npix, 3), dt)                                        # camera.h:127: black at the depth limit
        live = np.arange(npix)
        for _bounce in range(B):
            if len(live) == 0:
                break
            t, idx = oracle.hit_world(prec, scene["center_radius"], np.hstack([O[live], D[live]]))
            out = oracle.scatter(prec, scene, O[live], D[live], t, idx, atten[live], uy[live], depth[live], states[live])
            assert (out["depth"] == depth[live] + (out["status"] == 0)).all()
            O[live], D[live], atten[live], depth[live], states[live] = out["O"], out["D"], out["atten"], out["depth"], out["states"]
            ended = out["status"] == 1
            col[live[ended]] = out["col"][ended]
            live = live[~ended]
        acc = acc + col                                                      # camera.h:160
    scale = dt(cam.pixel_samples_scale)
    pc = scale * acc                                                         # camera.h:167
    with np.errstate(invalid="ignore"):
        got = np.where(pc > 0, np.sqrt(pc), dt(0)).astype(dt).reshape(H, W, 3)   # color.h:10-13
    assert np.array_equal(_bits(got.reshape(-1, 3)), _bits(want.reshape(-1, 3)))
    assert float(want.std()) > 0.01


# ----------------------------------------------------------------------------------------------------------------------------------
# The families
# ----------------------------------------------------------------------------------------------------------------------------------
def family_real_hits(oracle, prec, scene, hit_world, n_each=6000):
    """a. Rays like the hit_world test's families a, b and e (anywhere, grazing the ground, on sphere surfaces) plus rays aimed at every
    sphere from outside and from inside at any incidence; (closest, hit) from hit_world."""
    from tests.test_gpu_parity import _adversarial_rays
    rng = np.random.default_rng(1000 + prec)
    cr = scene["center_radius"].astype(np.float64)
    plan = {"x0": -6.5, "z0": -5.5, "cell": 1.5, "nx": 9, "nz": 8}
    adv = _adversarial_rays(rng, cr, plan, n_each)
    rays = [adv[0:n_each], adv[n_each:2 * n_each], adv[4 * n_each:5 * n_each]]
    weight = np.array([1.0, 4.0, 2.0])[scene["type"]]          # lambertians fill their class anyway: aim more rays at metal and glass
    weight[0] = 0.0
    for inside in (False, True):
        k = rng.choice(len(cr), 2 * n_each, p=weight / weight.sum())
        O, D, _, _ = _aimed(rng, scene, k, rng.uniform(0.0, 1.0, len(k)), np.full(len(k), inside))
        rays.append(np.hstack([O, D]))
    rays = np.vstack(rays).astype(_dt(prec))
    rays = rays[rng.permutation(len(rays))]
    rays = rays[: len(rays) // 64 * 64]
    t, idx = hit_world(rays)
    return _calls(prec, rays[:, :3], rays[:, 3:], t, idx, _init_states(oracle, len(rays), prec), rng)


def _check_real_hits(scene, calls, want):
    classes, front = _material_classes(scene, calls, want)
    _assert_shares(classes, len(calls["hit"]))
    for name, mask in classes.items():
        if name == "miss":
            continue
        assert int((mask & front).sum()) >= 50, (name, "front face")
        if name.startswith("glass"):
            assert int((mask & ~front).sum()) >= 50, (name, "back face")


def family_lambertian_fallback(oracle, prec, scene):
    """b. On the unit sphere at the origin: D = v, O = -2 v, closest = 1 for the unit vector v the state will produce, so the hit point is
    -v exactly, the normal cancels v and near_zero fires; O moved by 0.5, 0.9, 1.1 and 2 near_zero on one, two and three components."""
    rng = np.random.default_rng(2000 + prec)
    e = 1e-6 if prec == 32 else 1e-8
    base = 64
    states = _init_states(oracle, base, 5 + prec)
    v, _, _ = oracle.random_unit_vector(prec, states)
    v = v.astype(np.float64)
    moves = [np.zeros(3)]
    for f in (0.5, 0.9, 1.1, 2.0):
        for comps in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)):
            for sign in (1.0, -1.0):
                m = np.zeros(3); m[list(comps)] = sign * f * e
                moves.append(m)
    O = np.concatenate([-2.0 * v + m for m in moves])
    n = len(O)
    reps = len(moves)
    return _calls(prec, O, np.tile(v, (reps, 1)), np.ones(n), np.full(n, UNIT_LAMBERTIAN), np.tile(states, (reps, 1)), rng)


def _fallback_classes(want):
    # centre 0, radius 1: the normal is the hit point itself, and the fallback returns the normal
    taken = (_bits(want["D"]) == _bits(want["O"])).all(axis=1)
    return {"fallback taken": taken, "fallback not taken": ~taken}


def family_metal_grazing(oracle, prec, scene):
    """c. Directions within 1e-3 of the tangent plane on every metal sphere (fuzz 0 ... 4), from outside and from inside."""
    rng = np.random.default_rng(3000 + prec)
    metals = np.nonzero(scene["type"] == METAL)[0]
    n = 64 * 96
    k = metals[rng.integers(0, len(metals), n)]
    cos_in = rng.choice([0.0, 1e-9, 1e-6, 1e-4, 1e-3], n) * rng.uniform(0.5, 1.0, n)
    O, D, t, hit = _aimed(rng, scene, k, cos_in, rng.random(n) < 0.3)
    return _calls(prec, O, D, t, hit, _init_states(oracle, n, 9 + prec), rng)


def _axis_records(scene, prec):
    """Records on every glass sphere whose hit point C + |r| g lies exactly on an axis g through the centre."""
    dt = _dt(prec)
    cr = scene["center_radius"].astype(np.float64)
    eta = scene["refraction_index"].astype(np.float64)
    glass = np.nonzero(scene["type"] == DIELECTRIC)[0]
    axes = np.vstack([np.eye(3), -np.eye(3)])
    recs = []                                         # (O, D, closest, hit)

    def step(x, k):                                   # k units in the last place of dt
        x = dt(x)
        for _ in range(abs(k)):
            x = np.nextafter(x, dt(np.inf) if k > 0 else dt(-np.inf))
        return float(x)

    for s in glass:
        C, r = cr[s, :3], cr[s, 3]
        for a, g in enumerate(axes):
            h = axes[(a + 1) % 6]
            P = C + abs(r) * g
            for sgn in (-1.0, 1.0):                   # from outside / from inside (geometrically)
                # exact normal incidence, at three lengths
                for length in (1.0, 0.125, 32.0):
                    D = sgn * g * length
                    recs.append((P - D, D, 1.0, s))
                    recs.append((P - D, D, 1.0 - 2.0 ** -10 if sgn < 0 else 1.0 + 2.0 ** -10, s))   # the hit point outside the sphere: the dot product exceeds 1
                # the critical angle of this face, when it has one
                front = (sgn < 0) == (r > 0)
                ri = 1.0 / eta[s] if front else eta[s]
                if ri > 1.0:
                    sc = float(dt(1.0 / ri)); cc = float(dt(np.sqrt(max(0.0, 1.0 - sc * sc))))
                    for ulps in (0, 1, -1, 2, -2, 8, -8):
                        D = sgn * cc * g + step(sc, ulps) * h
                        recs.append((P.astype(dt).astype(np.float64) - D, D, 1.0, s))
                # grazing
                for eps in (1e-3, 1e-5, 2.0 ** -30, 2.0 ** -50):
                    D = sgn * eps * g + h
                    recs.append((P - D, D, 1.0, s))
    O = np.array([q[0] for q in recs]); D = np.array([q[1] for q in recs])
    return O, D, np.array([q[2] for q in recs]), np.array([q[3] for q in recs], np.int32)


def family_glass_edges(oracle, prec, scene):
    """d. Exact normal incidence (cos = 1, sin = sqrt(0)), a dot product above 1 (the fmin clamp), the critical angle of every index
    +- 0, 1, 2, 8 units in the last place from inside and -- index below 1 -- from outside, grazing incidence, index exactly 1; every
    record with four generator states, plus near-critical and near-normal incidence at random points."""
    rng = np.random.default_rng(4000 + prec)
    O, D, t, hit = _axis_records(scene, prec)
    reps = 4
    O, D, t, hit = np.tile(O, (reps, 1)), np.tile(D, (reps, 1)), np.tile(t, reps), np.tile(hit, reps)
    glass = np.nonzero(scene["type"] == DIELECTRIC)[0]
    eta = scene["refraction_index"].astype(np.float64); r = scene["center_radius"][:, 3].astype(np.float64)
    n = 4096
    k = glass[rng.integers(0, len(glass), n)]
    inside = rng.random(n) < 0.5
    ri = np.where(inside == (r[k] > 0), eta[k], 1.0 / eta[k])
    sin_c = np.where(ri > 1.0, 1.0 / np.maximum(ri, 1.0), rng.uniform(0, 1, n)) * (1.0 + rng.choice([0.0, 1e-7, -1e-7, 1e-3, -1e-3, 0.1, -0.3, 1.0, 1.0], n))
    cos_in = np.sqrt(np.maximum(0.0, 1.0 - np.minimum(sin_c, 1.0) ** 2))
    O2, D2, t2, hit2 = _aimed(rng, scene, k, cos_in, inside)
    k3 = glass[rng.integers(0, len(glass), 1024)]
    O3, D3, t3, hit3 = _aimed(rng, scene, k3, np.ones(1024), rng.random(1024) < 0.5)
    t3 = t3 * (1.0 - 1e-4)                                  # short of the surface from outside, past it from inside: |normal| > 1, the clamp
    O, D, t, hit = np.vstack([O, O2, O3]), np.vstack([D, D2, D3]), np.concatenate([t, t2, t3]), np.concatenate([hit, hit2, hit3])
    n = len(hit) // 64 * 64
    return _calls(prec, O[:n], D[:n], t[:n], hit[:n], _init_states(oracle, n, 21 + prec), rng)


def _check_glass_edges(prec, scene, calls, want):
    classes, _ = _material_classes(scene, calls, want)
    n = len(calls["hit"])
    _assert_shares({k: v for k, v in classes.items() if k.startswith("glass")}, n)
    # draw counts: a total internal reflection consumes nothing, anything else one number (one generator step in fp32, two in fp64).
    # Which is which is decided here in float64 from the inputs, away from the threshold.
    steps = _steps(calls, want)
    assert set(np.unique(steps)) <= {0, 1 if prec == 32 else 2}
    ty, front, nrm = _geometry(scene, calls)
    eta = scene["refraction_index"].astype(np.float64)[calls["hit"]]
    D = calls["D"].astype(np.float64)
    ud = D / np.linalg.norm(D, axis=1, keepdims=True)
    cos = np.minimum(-(ud * nrm).sum(axis=1), 1.0)
    ri = np.where(front, 1.0 / eta, eta)
    x = ri * np.sqrt(np.maximum(0.0, 1.0 - cos * cos))
    sure = (np.abs(x - 1.0) > 0.5) & ((prec == 64) | (ri <= 100.0)) & (cos > 1e-4)      # (cos ~ 0: which face it is depends on the last bit)
    assert sure.mean() > 0.3
    assert (steps[sure & (x > 1.0)] == 0).all() and (steps[sure & (x < 1.0)] > 0).all()
    assert int((sure & (x > 1.0)).sum()) >= 200 and int((sure & (x < 1.0)).sum()) >= 200


ROUND_BINS = (("1 round", 1, 1), ("2-3 rounds", 2, 3), ("4-6 rounds", 4, 6), ("7-12 rounds", 7, 12), ("more than 12 rounds", 13, 10 ** 9))


def family_long_rejection(oracle, prec, scene):
    """e. States whose random_unit_vector runs 1, 2-3, 4-6, 7-12 and more than 12 rounds (found with the oracle among 600 000 random
    states), on lambertian and metal hit records."""
    rng = np.random.default_rng(5000 + prec)
    pool = rng.integers(0, 2 ** 32, (600000, 6), dtype=np.uint64).astype(np.uint32)
    _, _, rounds = oracle.random_unit_vector(prec, pool)
    pick = []
    for _, lo, hi in ROUND_BINS:
        idx = np.nonzero((rounds >= lo) & (rounds <= hi))[0]
        pick.append(idx[:400])
    pick = np.concatenate(pick)
    pick = pick[: len(pick) // 64 * 64]
    pick = pick[rng.permutation(len(pick))]
    n = len(pick)
    diffuse = np.nonzero(scene["type"] != DIELECTRIC)[0]
    k = diffuse[rng.integers(0, len(diffuse), n)]
    O, D, t, hit = _aimed(rng, scene, k, rng.uniform(0.05, 1.0, n), np.zeros(n, bool))
    return _calls(prec, O, D, t, hit, pool[pick], rng), rounds[pick]


def _spoilers(scene, prec):
    """f. One-lane spoilers on a glass and on a metal sphere, hit point exactly on the +x axis of the sphere: |D|^2 at both ends of
    [2^-80, 2^80], just outside, well outside (2^+-92, 2^+-100), and exact normal incidence at an ordinary length."""
    dt = _dt(prec)
    cr = scene["center_radius"].astype(np.float64)
    ty = scene["type"]
    glass = [s for s in np.nonzero(ty == DIELECTRIC)[0] if cr[s, 3] in (0.25, 0.5)][0]
    metal = np.nonzero(ty == METAL)[0][-1]
    up = lambda x: float(np.nextafter(dt(x), dt(np.inf)))
    down = lambda x: float(np.nextafter(dt(x), dt(0)))
    lengths = [2.0 ** 40, 2.0 ** -40, up(2.0 ** 40), down(2.0 ** -40), 2.0 ** 40 * 1.001, 2.0 ** -40 * 0.999, 2.0 ** 46, 2.0 ** -46, 2.0 ** 50, 2.0 ** -50, 1.0]
    recs = []
    g = np.array([1.0, 0.0, 0.0])
    for s in (glass, metal):
        P = cr[s, :3] + abs(cr[s, 3]) * g
        for length in lengths:
            D = -g * length
            t = 0.25 / length                               # a power of two times 1 / length: O = P + 0.25 g exactly
            recs.append((P + 0.25 * g, D, t, s))
    return recs


def family_mixed_waves(oracle, prec, scene, real_hits):
    """f. 64 waves of family a (all in range) as they are, then once per (spoiler, lane) with that lane of every wave replaced."""
    rng = np.random.default_rng(6000 + prec)
    base = _take(real_hits, np.arange(64 * 64))
    parts, lanes_of = [base], [np.full(64 * 64, -1)]
    for q, (O, D, t, s) in enumerate(_spoilers(scene, prec)):
        for lane in (0, 31, 32, 63):
            c = {k: v.copy() for k, v in base.items()}
            sel = np.arange(lane, 64 * 64, 64)
            sp = _calls(prec, np.tile(O, (64, 1)), np.tile(D, (64, 1)), np.full(64, t), np.full(64, s), c["states"][sel], rng)
            for key in c:
                c[key][sel] = sp[key]
            parts.append(c); lanes_of.append(np.where(np.arange(64 * 64) % 64 == lane, q, -1))
    return _cat(parts), np.concatenate(lanes_of)


def _f32_edges():
    one = np.float32(1.0)
    e = [one, -one, np.float32(0.0), np.float32(-0.0), np.nextafter(one, np.float32(0)), -np.nextafter(one, np.float32(0)),
         np.nextafter(np.float32(0), one), -np.nextafter(np.float32(0), one), np.float32(1e-40), np.float32(-1e-40), np.float32(1.1754942e-38), np.float32(-1.1754942e-38),
         np.float32(2.0 ** -24), np.float32(-2.0 ** -24), np.float32(2.0 ** -25), np.float32(-2.0 ** -25), np.float32(2.0 ** -26), np.float32(0.5), np.float32(-0.5)]
    return np.array(e, np.float32)


def _sky_values(prec, chunk):
    """g. fp32: every float of [0.5, 1) and its negatives, in 16 chunks; fp64: 4 000 000 random values, in 4 chunks; the edges ride in chunk 0."""
    if prec == 32:
        half = np.arange(chunk * 2 ** 19, (chunk + 1) * 2 ** 19, dtype=np.uint32)
        u = np.uint32(0x3f000000) + half
        v = np.concatenate([u.view(np.float32), (u | np.uint32(0x80000000)).view(np.float32)])
        edges = _f32_edges()
    else:
        rng = np.random.default_rng(7000 + chunk)
        v = np.concatenate([rng.uniform(-1.0, 1.0, 500000), np.sign(rng.uniform(-1, 1, 300000)) * np.exp2(rng.uniform(-1080.0, 0.0, 300000)),
                            np.nextafter(1.0, 0.0) - rng.integers(0, 2 ** 20, 200000) * 2.0 ** -53])
        one = 1.0
        edges = np.array([one, -one, 0.0, -0.0, np.nextafter(one, 0), -np.nextafter(one, 0), 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308,
                          2.0 ** -53, -2.0 ** -53, 2.0 ** -54, 2.0 ** -55, 0.5, -0.5, 1.0 - 2.0 ** -24, 2.0 ** -25])
    if chunk == 0:
        v = np.concatenate([edges.astype(v.dtype), v])
    return v


SKY_CHUNKS = {32: 16, 64: 4}


def family_sky(prec, chunk):
    rng = np.random.default_rng(7100 + chunk)
    uy = _sky_values(prec, chunk)
    n = len(uy)
    atten = np.ones((n, 3)); atten[n // 2:] = rng.uniform(0.0, 2.0, (n - n // 2, 3))
    z = np.zeros(n)
    states = np.tile(np.arange(1, 7, dtype=np.uint32), (n, 1))
    D = np.tile([0.0, 1.0, 0.0], (n, 1))
    return _calls(prec, np.zeros((n, 3)), D, z + np.inf, np.full(n, -1), states, rng, atten=atten, sky_uy=uy, depth=np.zeros(n, np.int32))


# ----------------------------------------------------------------------------------------------------------------------------------
# Class shares on the CPU: the generators fill their classes whatever the GPU does (and the GPU tests assert the same again)
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [32, 64])
def test_the_families_fill_their_classes(oracle, prec):
    scene = lattice_scene(prec)
    a = family_real_hits(oracle, prec, scene, lambda rays: oracle.hit_world(prec, scene["center_radius"], rays))
    want = oracle.scatter(prec, scene, **a); _assert_finite(want); _check_real_hits(scene, a, want)
    b = family_lambertian_fallback(oracle, prec, scene)
    want = oracle.scatter(prec, scene, **b); _assert_finite(want); _assert_shares(_fallback_classes(want), len(b["hit"]))
    c = family_metal_grazing(oracle, prec, scene)
    want = oracle.scatter(prec, scene, **c); _assert_finite(want)
    cl, _ = _material_classes(scene, c, want); _assert_shares({k: cl[k] for k in ("metal kept", "metal absorbed")}, len(c["hit"]))
    d = family_glass_edges(oracle, prec, scene)
    want = oracle.scatter(prec, scene, **d); _assert_finite(want); _check_glass_edges(prec, scene, d, want)
    e, rounds = family_long_rejection(oracle, prec, scene)
    _assert_shares({name: (rounds >= lo) & (rounds <= hi) for name, lo, hi in ROUND_BINS}, len(rounds), counts={"more than 12 rounds": 50})
    f, _ = family_mixed_waves(oracle, prec, scene, a)
    want = oracle.scatter(prec, scene, **f); _assert_finite(want)


# ----------------------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


@pytest.fixture(scope="module")
def probe(rt):
    """One debug renderer per precision with the lattice scene, and the scene."""
    made = {}
    for prec in (32, 64):
        r = rt.Renderer(0, prec, debug=True)
        sc = lattice_scene(prec)
        r.set_camera(rt.camera(prec, 64, 64, 1, 1)); r.set_scene(sc); r.set_scene_source(rt.SCENE_LDS_EXACT)
        made[prec] = (r, sc)
    yield made
    for r, _ in made.values():
        r.close()


_FIELDS = ("col", "O", "D", "atten", "states")


def _differs(got, want):
    bad = (got["status"] != want["status"]) | (got["depth"] != want["depth"])
    for k in _FIELDS:
        bad |= (_bits(got[k]) != _bits(want[k])).any(axis=1)
    return np.nonzero(bad)[0]


def _run_forms(probe, oracle, prec, calls, want=None, trips=None):
    """Every form of the precision on `calls`: each equals the oracle bit for bit (so they equal each other), no retry touched the path
    state, and the trip count is what the family states (default: one trip in form 0, any number otherwise)."""
    r, scene = probe[prec]
    if want is None:
        want = oracle.scatter(prec, scene, **calls)
        _assert_finite(want)
    outs = {}
    for form in _forms(prec):
        got = r.debug_scatter(form, **calls)
        bad = _differs(got, want)
        assert len(bad) == 0, (prec, form, len(bad), {k: v[bad[:3]] for k, v in calls.items()}, {k: got[k][bad[:3]] for k in _FIELDS + ("status",)},
                               {k: want[k][bad[:3]] for k in _FIELDS + ("status",)})
        assert not got["flags"].any(), (prec, form, "a retry changed O, D, atten or depth")
        if form == 0:
            assert (got["trips"] == 1).all()
        elif trips is not None:
            want_trips = trips(got["rounds_per_trip"])
            bad = np.nonzero(got["trips"] != want_trips)[0]
            assert len(bad) == 0, (prec, form, got["trips"][bad[:5]], want_trips[bad[:5]])
        outs[form] = got
    return want, outs


@pytest.fixture(scope="module")
def real_hits(probe, oracle):
    """Family a of both precisions, (closest, hit) from rtiow_debug_hit_world under RTIOW_SCENE_LDS_EXACT."""
    return {prec: family_real_hits(oracle, prec, probe[prec][1], probe[prec][0].debug_hit_world) for prec in (32, 64)}


@gpu
def test_form_two_is_fp64_only(rt, probe):
    r, _ = probe[32]
    one = _calls(32, np.zeros((1, 3)), [[0.0, 1.0, 0.0]], [1.0], [-1], np.ones((1, 6), np.uint32), np.random.default_rng(0))
    with pytest.raises(rt.RtiowError) as e:
        r.debug_scatter(2, **one)
    assert e.value.code == E_BADARG
    with pytest.raises(rt.RtiowError) as e:                                     # a hit index beyond the scene is refused, not read
        r.debug_scatter(0, **dict(one, hit=np.array([10 ** 6], np.int32)))
    assert e.value.code == E_BADARG


@gpu
@pytest.mark.parametrize("prec", [32, 64])
def test_real_hits(probe, oracle, real_hits, prec):
    """a. Miss, lambertian, metal kept and absorbed, glass reflected, refracted and totally reflected, on front faces and (glass) back faces."""
    calls = real_hits[prec]
    t, idx = oracle.hit_world(prec, probe[prec][1]["center_radius"], np.hstack([calls["O"], calls["D"]]))
    assert np.array_equal(idx, calls["hit"]) and np.array_equal(_bits(t), _bits(calls["closest"]))
    want, _ = _run_forms(probe, oracle, prec, calls)
    _check_real_hits(probe[prec][1], calls, want)


@gpu
@pytest.mark.parametrize("prec", [32, 64])
def test_shade_records_read_from_memory(rt, probe, oracle, real_hits, prec):
    """The lattice's 52 shade records ride in LDS (layout_lds keeps them there up to 32 KB a workgroup).  Behind 800 more spheres the table
    is 852 x 12 reals -- 40 KB in fp32, 80 KB in fp64 -- and the step reads its record from memory instead: the same calls (they name the
    first 52 spheres only), the same bits."""
    scene = probe[prec][1]
    big = {k: (np.concatenate([v, np.tile(v[-1:], (800,) + (1,) * (v.ndim - 1))]) if hasattr(v, "shape") else v) for k, v in scene.items()}
    big["center_radius"][len(scene["type"]):, :3] += np.asarray(1.0e4, big["center_radius"].dtype)
    calls = _take(real_hits[prec], np.arange(64 * 128))
    want = oracle.scatter(prec, scene, **calls)
    _assert_finite(want)
    with rt.Renderer(0, prec, debug=True) as r:
        r.set_camera(rt.camera(prec, 64, 64, 1, 1)); r.set_scene(big); r.set_scene_source(rt.SCENE_LDS_EXACT)
        for form in _forms(prec):
            got = r.debug_scatter(form, **calls)
            assert len(_differs(got, want)) == 0 and not got["flags"].any(), (prec, form)


@gpu
@pytest.mark.parametrize("prec", [32, 64])
def test_lambertian_fallback(probe, oracle, prec):
    """b. The near_zero fallback (nd = normal), on both sides of its test."""
    calls = family_lambertian_fallback(oracle, prec, probe[prec][1])
    want, _ = _run_forms(probe, oracle, prec, calls)
    _assert_shares(_fallback_classes(want), len(calls["hit"]))


@gpu
@pytest.mark.parametrize("prec", [32, 64])
def test_metal_at_grazing_incidence(probe, oracle, prec):
    """c. Kept and absorbed within 1e-3 of the tangent plane, fuzz 0 ... 4."""
    scene = probe[prec][1]
    calls = family_metal_grazing(oracle, prec, scene)
    want, _ = _run_forms(probe, oracle, prec, calls)
    cl, _ = _material_classes(scene, calls, want)
    _assert_shares({k: cl[k] for k in ("metal kept", "metal absorbed")}, len(calls["hit"]))


@gpu
@pytest.mark.parametrize("prec", [32, 64])
def test_glass_at_the_edges(probe, oracle, prec):
    """d. Normal incidence, the clamp, critical angles, grazing, index 1; a total internal reflection draws nothing."""
    scene = probe[prec][1]
    calls = family_glass_edges(oracle, prec, scene)
    want, _ = _run_forms(probe, oracle, prec, calls)
    _check_glass_edges(prec, scene, calls, want)


@gpu
@pytest.mark.parametrize("prec", [32, 64])
def test_long_rejection_loops(probe, oracle, prec):
    """e. 1 ... more than 12 rounds: one trip in form 0, ceil(rounds / rounds per trip) in the bounded forms, retries clean."""
    calls, rounds = family_long_rejection(oracle, prec, probe[prec][1])
    _assert_shares({name: (rounds >= lo) & (rounds <= hi) for name, lo, hi in ROUND_BINS}, len(rounds), counts={"more than 12 rounds": 50})
    want, _ = _run_forms(probe, oracle, prec, calls, trips=lambda per_trip: -(-rounds // per_trip))
    per_round = 3 if prec == 32 else 6
    assert np.array_equal(_steps(calls, want), rounds.astype(np.uint64) * per_round)


@gpu
@pytest.mark.parametrize("prec", [32, 64])
def test_mixed_waves(probe, oracle, real_hits, prec):
    """f. One lane of a wave outside the range of the short IEEE forms: every lane equals the oracle, and the lanes that were not
    replaced keep the bits they had in the unspoiled wave."""
    scene = probe[prec][1]
    calls, spoiler_of = family_mixed_waves(oracle, prec, scene, real_hits[prec])
    dd = (calls["D"][:64 * 64].astype(np.float64) ** 2).sum(axis=1)
    assert ((dd >= 2.0 ** -70) & (dd <= 2.0 ** 70)).all()                     # the unspoiled waves are in range
    ty = np.where(calls["hit"][:64 * 64] >= 0, scene["type"][np.maximum(calls["hit"][:64 * 64], 0)], -1).reshape(64, 64)
    assert ((ty == DIELECTRIC).sum(axis=1) >= 2).all() and ((ty == METAL).sum(axis=1) >= 2).all()   # every wave has lanes to spoil
    want, outs = _run_forms(probe, oracle, prec, calls)
    base = 64 * 64
    for form, got in outs.items():
        for v in range(1, len(spoiler_of) // base):
            keep = spoiler_of[v * base:(v + 1) * base] < 0
            for k in _FIELDS:
                assert np.array_equal(_bits(got[k][v * base:(v + 1) * base])[keep], _bits(got[k][:base])[keep]), (prec, form, v, k)


@gpu
@pytest.mark.parametrize("prec", [32, 64])
def test_sky(probe, oracle, prec):
    """g. The sky blend for every float of [0.5, 1) and its negatives (fp32), 4 000 000 random values (fp64), +-1, +-0, their neighbours and
    denormals, attenuation 1 and random, against the oracle's double blend (camera.h:121-123): the evidence for fp32's four-operation form."""
    total = 0
    for chunk in range(SKY_CHUNKS[prec]):
        calls = family_sky(prec, chunk)
        total += len(calls["hit"])
        want, _ = _run_forms(probe, oracle, prec, calls)
        assert (want["status"] == 1).all() and np.array_equal(want["states"], calls["states"])
    assert total >= (2 ** 24 if prec == 32 else 4 * 10 ** 6)
