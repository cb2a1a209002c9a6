"""Ray families for the device grid's walk (rtiow_render_large; device/hit_device_grid.h), beside tests/test_gpu_parity._adversarial_rays:
the faces of the y-slab, the long lists, the rim of the grid's rectangle with the clip that enters through it, and walks across the whole
grid.  Plain numpy over a plan of api.debug_large_grid_plan(..., tables=True); tests/test_large_grid_plan.py checks on the CPU, against
the oracle alone, that the families reach what tests/test_render_large_edges.py asserts of them."""
import functools

import numpy as np

from tests import large_scene

FAMILIES = ("slab", "lists", "rim", "long_walk")
N_EACH = 20000                                                           # rays per family in the ray-by-ray tests of the edge scenes


def _headings(rng, n):
    th = rng.uniform(0, 2 * np.pi, n)
    return np.column_stack([np.cos(th), np.zeros(n), np.sin(th)])


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _f32_steps(v, k):
    """v rounded to fp32 and moved k fp32 steps (k < 0: down)."""
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return float(v)


def _slab(rng, cr, pl, n, finite):
    x0, z0, cell, nx, nz, ylo, yhi, eps = pl["x0"], pl["z0"], pl["cell"], pl["nx"], pl["nz"], pl["ylo"], pl["yhi"], pl["eps"]
    # the faces as the plan has them, as the kernel has them (fp32, one step outward: _f32_steps(ylo, -1)) and a step or two to either side
    levels = np.array([ylo, yhi, ylo - eps, yhi + eps, 0.5 * (ylo + yhi)] + [_f32_steps(ylo, k) for k in (-2, -1, 0, 1)] + [_f32_steps(yhi, k) for k in (-1, 0, 1, 2)])
    nv = n // 3                                                          # verticals
    ns = n - nv
    o = np.column_stack([rng.uniform(x0 - 3 * cell, x0 + (nx + 3) * cell, ns), rng.choice(levels, ns), rng.uniform(z0 - 3 * cell, z0 + (nz + 3) * cell, ns)])
    d = _headings(rng, ns)
    d[:, 1] = rng.choice([0.0, 1e-7, -1e-7, 1e-3, -1e-3, 1.0, -1.0], ns)
    # dx = dz = 0, dy = +-1, through sphere centres, cell centres and cell corners; from above and from below, towards the slab and away
    k = rng.integers(0, len(finite), nv)
    ix, iz = rng.integers(0, nx, nv), rng.integers(0, nz, nv)
    kind = rng.integers(0, 3, nv)
    x = np.where(kind == 0, cr[finite[k], 0], x0 + (ix + np.where(kind == 1, 0.5, 0.0)) * cell)
    z = np.where(kind == 0, cr[finite[k], 2], z0 + (iz + np.where(kind == 1, 0.5, 0.0)) * cell)
    above = rng.random(nv) < 0.5
    y = np.where(above, yhi + rng.uniform(0.0, 5.0, nv), ylo - rng.uniform(0.0, 5.0, nv))
    y[: nv // 8] = rng.choice(levels, nv // 8)                          # ... and from the faces themselves
    dy = np.where(above, -1.0, 1.0) * rng.choice([1.0, 1.0, 1.0, -1.0], nv)
    ov = np.column_stack([x, y, z])
    dv = np.column_stack([np.zeros(nv), dy, np.zeros(nv)])
    return np.vstack([np.hstack([o, d]), np.hstack([ov, dv])])


def _lists(rng, cr, pl, n, ctr):
    x0, z0, cell = pl["x0"], pl["z0"], pl["cell"]
    cells, indices = np.asarray(pl["cells"], np.int64), np.asarray(pl["indices"], np.int64)
    count = cells[:, :, 1]
    iz, ix = np.nonzero(count >= min(5, count.max()))                   # the cells with five entries or more, or the fullest the scene has
    c = rng.integers(0, len(iz), n)
    iz, ix = iz[c], ix[c]
    first, cnt = cells[iz, ix, 0], cells[iz, ix, 1]
    listed = indices[first + rng.integers(0, 1 << 30, n) % cnt]         # the sphere whose height the ray is aimed at
    inside = indices[first + rng.integers(0, 1 << 30, n) % cnt]         # the sphere a third of the rays start in
    tgt = np.column_stack([x0 + (ix + 0.5 + rng.uniform(-0.5, 0.5, n)) * cell, cr[listed, 1], z0 + (iz + 0.5 + rng.uniform(-0.5, 0.5, n)) * cell])
    o = ctr + _unit(rng, n) * (0.9 * pl["rfar"] * rng.random((n, 1)) ** (1.0 / 3.0))
    third = np.arange(n) % 3
    tgt[third == 0] = cr[listed[third == 0], :3]                        # exactly at a listed sphere's centre
    o[third == 1] = (cr[inside, :3] + _unit(rng, n) * cr[inside, 3:4] * rng.uniform(0.0, 0.9, (n, 1)))[third == 1]
    return np.hstack([o, tgt - o])


def _rim(rng, pl, n, ctr):
    x0, z0, cell, nx, nz, ylo, yhi = pl["x0"], pl["z0"], pl["cell"], pl["nx"], pl["nz"], pl["ylo"], pl["yhi"]
    lo, hi = np.array([x0, z0]), np.array([x0 + nx * cell, z0 + nz * cell])
    corner = np.max(np.abs(np.array([[lo[0], lo[1]], [lo[0], hi[1]], [hi[0], lo[1]], [hi[0], hi[1]]]) - ctr[[0, 2]]), axis=0)
    room = 0.9 * pl["rfar"] - np.hypot(*corner) - max(abs(ylo - ctr[1]), abs(yhi - ctr[1]))     # how far outside the rectangle 0.9 rfar still reaches
    assert room > cell
    side = rng.integers(0, 4, n)                                         # the face the ray is on: x low, x high, z low, z high
    axis, sign = side // 2, np.where(side % 2 == 0, -1.0, 1.0)
    outward = np.zeros((n, 2)); outward[np.arange(n), axis] = sign
    along = np.zeros((n, 2)); along[np.arange(n), 1 - axis] = 1.0
    face = np.where(side % 2 == 0, lo[axis], hi[axis])
    span = rng.uniform(0, 1, n) * (hi - lo)[1 - axis] + lo[1 - axis]
    outside = np.arange(n) % 2 == 1
    depth = np.where(outside, rng.uniform(0, 1, n) ** 2 * 0.7 * room, -rng.uniform(0, 1, n) * cell)      # inside: within the outermost ring of cells
    depth[rng.random(n) < 0.1] = 0.0                                      # on the face itself
    p = np.zeros((n, 2))
    p[np.arange(n), axis] = face + sign * depth
    p[np.arange(n), 1 - axis] = span
    heading = np.where(outside[:, None], -outward, outward)              # outside: inward, through the clip; inside: outward
    kind = rng.integers(0, 3, n)
    diag = heading + along * rng.choice([-1.0, 1.0], (n, 1))
    th = rng.uniform(-0.49 * np.pi, 0.49 * np.pi, n)
    rand = heading * np.cos(th)[:, None] + along * np.sin(th)[:, None]
    d2 = np.where((kind == 0)[:, None], heading, np.where((kind == 1)[:, None], diag, rand))
    dy = np.where(kind == 2, rng.uniform(-0.2, 0.2, n), 0.0)
    o = np.column_stack([p[:, 0], rng.uniform(ylo, yhi, n), p[:, 1]])
    assert (np.linalg.norm(o - ctr, axis=1) <= 0.9 * pl["rfar"]).all()
    return np.hstack([o, np.column_stack([d2[:, 0], dy, d2[:, 1]])])


def _long_walk(rng, cr, pl, n, registered):
    x0, z0, cell, nx, nz, ylo, yhi = pl["x0"], pl["z0"], pl["cell"], pl["nx"], pl["nz"], pl["ylo"], pl["yhi"]
    lo, hi = np.array([x0, z0]), np.array([x0 + nx * cell, z0 + nz * cell])
    top = float((cr[registered, 1] + cr[registered, 3]).max())          # above every gridded sphere and still inside the slab (yhi = top + w - r)
    y = rng.uniform(top, yhi, n) if yhi > top else rng.uniform(ylo, yhi, n)
    diagonal = np.arange(n) % 2 == 0
    # corner to opposite corner: from within a cell and a half of one corner (inside or just outside) to within as much of the opposite one
    cx, cz = rng.integers(0, 2, n), rng.integers(0, 2, n)
    a = np.column_stack([np.where(cx == 0, lo[0], hi[0]), np.where(cz == 0, lo[1], hi[1])]) + rng.uniform(-1.5, 1.5, (n, 2)) * cell
    b = np.column_stack([np.where(cx == 0, hi[0], lo[0]), np.where(cz == 0, hi[1], lo[1])]) + rng.uniform(-1.5, 1.5, (n, 2)) * cell
    # along the long axis: from one end to the other, at any position across
    long_axis = 0 if nx >= nz else 1
    end = rng.integers(0, 2, n)
    a2, b2 = np.zeros((n, 2)), np.zeros((n, 2))
    a2[:, long_axis] = np.where(end == 0, lo[long_axis], hi[long_axis]) + rng.uniform(-0.5, 0.5, n) * cell
    b2[:, long_axis] = np.where(end == 0, hi[long_axis], lo[long_axis])
    a2[:, 1 - long_axis] = rng.uniform(lo[1 - long_axis], hi[1 - long_axis], n)
    b2[:, 1 - long_axis] = a2[:, 1 - long_axis] + rng.choice([0.0, 1.0], n) * rng.uniform(-1, 1, n) * cell
    a, b = np.where(diagonal[:, None], a, a2), np.where(diagonal[:, None], b, b2)
    d2 = b - a
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    dy = rng.choice([0.0, 1.0, -1.0], n) * rng.uniform(0, 1e-4, n)      # |dy| <= 1e-4 of the horizontal length
    scale = np.exp(rng.uniform(-2, 2, (n, 1)))
    return np.hstack([np.column_stack([a[:, 0], y, a[:, 1]]), np.column_stack([d2[:, 0], dy, d2[:, 1]]) * scale])


def edge_rays(rng, cr, plan, n_each):
    """(rays [4 n_each, 6], {family: slice}) around the device grid of `plan` (with tables) for the spheres cr [n, 4]."""
    cr = np.asarray(cr, np.float64)
    ctr = large_scene.centre_of(cr)
    with np.errstate(invalid="ignore"):
        finite = np.nonzero(np.isfinite(cr).all(axis=1) & (cr[:, 3] > 0) & (cr[:, 3] < 100.0))[0]
    registered = np.nonzero(np.asarray(plan["halfwidth"]) > 0)[0]
    fam = [_slab(rng, cr, plan, n_each, finite), _lists(rng, cr, plan, n_each, ctr), _rim(rng, plan, n_each, ctr), _long_walk(rng, cr, plan, n_each, registered)]
    assert all(len(f) == n_each for f in fam)
    return np.vstack(fam), {name: slice(k * n_each, (k + 1) * n_each) for k, name in enumerate(FAMILIES)}


ADVERSARIAL = ("a", "b", "c", "d", "e")                                  # _adversarial_rays' families of n_each rays; its degenerate ones follow
WALKED = ("a", "b", "c", "e") + FAMILIES                                 # every family but the far origins and the degenerate numbers


def stacked_rays(cr, plan, prec, n_each, seed):
    """_adversarial_rays stacked with edge_rays, in the type of a handle of `prec`: (rays, {family: slice})."""
    from tests.test_gpu_parity import _adversarial_rays
    cr = np.asarray(cr, np.float64)
    rng = np.random.default_rng(seed)
    with np.errstate(invalid="ignore"):
        adv = _adversarial_rays(rng, cr, plan, n_each)
    edge, fam = edge_rays(rng, cr, plan, n_each)
    where = {name: slice(k * n_each, (k + 1) * n_each) for k, name in enumerate(ADVERSARIAL)}
    where["degenerate"] = slice(5 * n_each, len(adv))
    where.update({name: slice(len(adv) + s.start, len(adv) + s.stop) for name, s in fam.items()})
    with np.errstate(over="ignore", invalid="ignore"):
        rays = np.vstack([adv, edge]).astype(np.float32 if prec == 32 else np.float64)
    return rays, where


@functools.lru_cache(maxsize=4)
def edge_case(rt, name, prec, n_each=N_EACH):
    """(scene, cr as fp64, plan with tables, rays, {family: slice}) of one of large_scene.EDGE_SCENES: the very rays the GPU tests trace,
    so that what tests/test_large_grid_plan.py shows of them for the oracle alone holds there."""
    sc = large_scene.edge_scene(name, prec)
    cr = np.asarray(sc["center_radius"], np.float64)
    pl = rt.debug_large_grid_plan(cr, large_scene.centre(sc), tables=True)
    rays, where = stacked_rays(cr, pl, prec, n_each, 7 + prec)
    return sc, cr, pl, rays, where


def within_reach(rays, where, cr, plan):
    """Indices of the rays of the WALKED families whose origin lies within 0.99 rfar of the recentring point (the kernel walks for
    |O - ctr|^2 <= 0.999 rfar^2) and whose squared length is an ordinary number: every wave made of these alone must walk."""
    pick = np.concatenate([np.arange(where[name].start, where[name].stop) for name in WALKED])
    r = rays[pick].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        a = (r[:, 3:] ** 2).sum(axis=1)
        ok = (np.linalg.norm(r[:, :3] - large_scene.centre_of(cr), axis=1) <= 0.99 * plan["rfar"]) & (a > 1e-29) & (a < 1e29)
    return pick[ok]


def surely_exact(rays):
    """True for the rays that send their whole wave through the exact loop whatever the grid is (hit_world_device_grid's `!sane`): a
    squared length that is NaN or outside (1e-30, 1e30) -- here: outside [1e-31, 1e31], whatever the rounding -- or an origin that is not
    finite."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = rays.astype(np.float32)
        a = (r[:, 3:].astype(np.float64) ** 2).sum(axis=1)
        return ~(a >= 1e-31) | ~(a <= 1e31) | ~np.isfinite(r[:, :3]).all(axis=1)


def shuffled(rays, rng):
    """(rays under a random permutation, the permutation): shuffled[k] = rays[perm[k]], so out[perm] = out_of_shuffled un-permutes a result."""
    perm = rng.permutation(len(rays))
    return np.ascontiguousarray(rays[perm]), perm


def cells_crossed(rays, plan):
    """Plain geometry, no walk: the number of cell borders of the grid's rectangle a ray's line crosses ahead of its origin -- a lower
    estimate, within a cell or two, of the cells a walk that finds nothing reads."""
    x0, z0, cell, nx, nz = plan["x0"], plan["z0"], plan["cell"], plan["nx"], plan["nz"]
    out = np.zeros(len(rays), np.int64)
    t0, t1 = np.zeros(len(rays)), np.full(len(rays), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for o, d, lo, n in ((rays[:, 0], rays[:, 3], x0, nx), (rays[:, 2], rays[:, 5], z0, nz)):
            ta, tb = (lo - o) / d, (lo + n * cell - o) / d
            t0 = np.maximum(t0, np.where(d != 0, np.minimum(ta, tb), np.where((o >= lo) & (o <= lo + n * cell), 0.0, np.inf)))
            t1 = np.minimum(t1, np.where(d != 0, np.maximum(ta, tb), np.inf))
        ok = t0 < t1
        for o, d, lo in ((rays[:, 0], rays[:, 3], x0), (rays[:, 2], rays[:, 5], z0)):
            a, b = (o + t0 * d - lo) / cell, (o + np.where(np.isfinite(t1), t1, 0.0) * d - lo) / cell
            out += np.where(ok & (d != 0), np.abs(np.floor(b) - np.floor(a)), 0).astype(np.int64)
    return out


def dragged_along(rays, walked, perm):
    """A lower bound, from the kernel's text alone, on the rays that walk in family order and take the exact loop under `perm`: those
    whose wave of 64 in family order holds rays of `walked` (within_reach) only -- such a wave walks -- and whose wave under the
    permutation holds a surely_exact ray, which sends all 64 through the exact loop.  The probe hands lane k of wave w ray 64 w + k."""
    n = len(rays)
    waves = (n + 63) // 64
    clean = np.ones(waves * 64, bool); clean[:n] = False; clean[walked] = True
    walks_in_order = np.repeat(clean.reshape(waves, 64).all(axis=1), 64)[:n]
    exact = np.zeros(waves * 64, bool); exact[:n] = surely_exact(rays)[perm]
    exact_when_shuffled = np.zeros(n, bool)
    exact_when_shuffled[perm] = np.repeat(exact.reshape(waves, 64).any(axis=1), 64)[:n]
    return walks_in_order & exact_when_shuffled


def assert_floors(name, scene, plan, rays, where, index):
    """What keeps the ray-by-ray tests of the edge scenes from passing empty, of a reference's sphere index per ray (the oracle's on the
    CPU, the exact loop's on the GPU)."""
    hit = index >= 0
    assert hit.mean() >= 0.10 and (~hit).mean() >= 0.05, (name, float(hit.mean()))
    lists = index[where["lists"]]
    if name == "clusters":
        gridded = (lists >= 0) & ~np.isin(lists, plan["direct_list"])
        assert gridded.mean() >= 0.30, float(gridded.mean())
        low, high = (np.array(v) for v in zip(*large_scene.twins(scene)))
        assert len(low) >= 6
        assert np.isin(lists, low).sum() >= 100 and not np.isin(index, high).any(), (int(np.isin(lists, low).sum()), int(np.isin(index, high).sum()))
    if name == "equal_no_ground":
        assert len(plan["direct_list"]) == 0 and hit.any() and not hit.all()
    if name == "mixed_with_bad":
        # r = NaN and cx = inf make every discriminant NaN: never hit.  r = 0 and r = -0.3 are NOT never hit by the reference's arithmetic:
        # the radius enters as r^2, and with r = 0 the rounding of h^2 - a c leaves a discriminant >= 0 for a few far fp32 rays (5 of
        # 185 128 here, none in fp64; 35 and 38 rays return the sphere of r = -0.3).  For those two the bit comparison is the check.
        for bad in ("nan_radius", "inf_centre"):
            assert not (index == large_scene.MIXED_BAD[bad]).any(), bad
    if name == "sparse_wide":
        walk = where["long_walk"]
        crossed = cells_crossed(rays[walk].astype(np.float64), plan)
        assert crossed[~hit[walk]].max() >= 20, int(crossed.max())


def crossed_records(ray, plan, limit=12):
    """For an assertion's message: [(ix, iz, first, count, [sphere indices])] of the first `limit` cells the ray's line crosses inside the
    grid's rectangle, ahead of its origin, by plain fp64 geometry (a walk may read a neighbour more or less at a border)."""
    x0, z0, cell, nx, nz = plan["x0"], plan["z0"], plan["cell"], plan["nx"], plan["nz"]
    ray = np.asarray(ray, np.float64)
    if not np.isfinite(ray).all():
        return "not finite"
    o, d = ray[[0, 2]], ray[[3, 5]]
    lo, hi = np.array([x0, z0]), np.array([x0 + nx * cell, z0 + nz * cell])
    t0, t1 = 0.0, np.inf
    cuts = []
    for k in range(2):
        if d[k] == 0:
            if not lo[k] <= o[k] <= hi[k]:
                return "misses the rectangle"
            continue
        ta, tb = sorted(((lo[k] - o[k]) / d[k], (hi[k] - o[k]) / d[k]))
        t0, t1 = max(t0, ta), min(t1, tb)
        cuts += [(lo[k] + j * cell - o[k]) / d[k] for j in range(1, (nx, nz)[k])]
    if not t0 < t1:
        return "misses the rectangle"
    if not np.isfinite(t1):
        t1 = t0
    ts = [t0] + sorted(t for t in cuts if t0 < t < t1) + [t1]
    out = []
    for a, b in list(zip(ts[:-1], ts[1:]))[:limit] or [(t0, t1)]:
        p = o + 0.5 * (a + b) * d
        ix, iz = int(np.clip(np.floor((p[0] - x0) / cell), 0, nx - 1)), int(np.clip(np.floor((p[1] - z0) / cell), 0, nz - 1))
        first, count = (int(v) for v in plan["cells"][iz, ix])
        out.append((ix, iz, first, count, np.asarray(plan["indices"][first:first + count]).tolist()))
    return out


def describe(bad, rays, t, t_ref, index, index_ref, cells, plan):
    """The message of a failed bit comparison: the count, then the first five failing rays with both results, `cells` and the cell records
    they cross."""
    lines = ["%d rays differ" % len(bad)]
    for k in bad[:5]:
        lines.append("ray %d %s: walk (t %r, index %d, cells %d), reference (t %r, index %d); crosses %s"
                     % (k, rays[k].tolist(), t[k], index[k], cells[k], t_ref[k], index_ref[k], crossed_records(rays[k], plan)))
    return "\n".join(lines)
