"""Ray families for the volume grid's walk (rtiow_render_volume; device/hit_volume_grid.h): origins on the cell faces of all three axes
to the fp32 step, rays parallel to one and to two axes, rays through cell edges and corners where leaving parameters tie, diagonals
across the whole grid, rays entering through each of the six faces and the rim, origins inside the cloud and inside a sphere, verticals,
and the far and degenerate rays that must take the exact loop.  Plain numpy over a plan of api.debug_volume_grid_plan(..., tables=True);
every value is an fp32 number, so a handle of either precision traces the same rays.  tests/test_volume_grid_plan.py checks on the CPU,
against the oracle alone, that the families are what they say."""
import functools

import numpy as np

from tests import volume_scene
from tests.large_rays import _f32_steps, _unit, shuffled  # noqa: F401  (shuffled: re-exported for the GPU tests)

FAMILIES = ("faces", "parallel", "ties", "diagonals", "entering", "inside", "vertical", "far")
WALKED = FAMILIES[:-1]                                                  # every family but the far and degenerate rays
N_EACH = 20000
TINY = (0.0, -0.0, 1e-31, -1e-31, 1e-35, 1e-38, -1e-38)                 # components of an axis that never steps: exact zeros and |d| < 1e-30


def _frame(pl):
    lo = np.array([pl["x0"], pl["y0"], pl["z0"]])
    dims = np.array([pl["nx"], pl["ny"], pl["nz"]])
    return lo, dims, lo + dims * pl["cell"]


def _near_spheres(rng, cr, registered, n):
    """A point within 1.5 radii of the centre of a random gridded sphere, uniform in that ball: a line through it meets the sphere with
    probability 0.59.  The families aim a share of their rays at such points, so that they hit something in a scene that is thin
    inside its grid (the column fills a hundredth of its cells' cross-section) as they do in one that fills it."""
    k = registered[rng.integers(0, len(registered), n)]
    return cr[k, :3] + _unit(rng, n) * cr[k, 3:4] * 1.5 * rng.random((n, 1)) ** (1.0 / 3.0)


def _faces(rng, cr, pl, n, registered):
    lo, dims, hi = _frame(pl)
    o = rng.uniform(lo - 0.5 * pl["cell"], hi + 0.5 * pl["cell"], (n, 3))
    axis = np.arange(n) % 3
    for k in range(n):
        a = axis[k]
        j = rng.integers(0, dims[a] + 1)
        face = np.float32(lo[a]) + np.float32(j) * np.float32(pl["cell"])       # the face as fp32 arithmetic has it
        o[k, a] = _f32_steps(face, int(rng.integers(-2, 3)))
    d = _unit(rng, n)
    aimed = rng.random(n) < 0.6
    d[aimed] = (_near_spheres(rng, cr, registered, n) - o)[aimed]
    return np.hstack([o, d])


def _parallel(rng, cr, pl, n, registered):
    lo, dims, hi = _frame(pl)
    o = rng.uniform(lo, hi, (n, 3))
    d = _unit(rng, n)
    kind = np.arange(n) % 2                                                  # 0: one axis never steps; 1: two never step
    for k in range(n):
        still = rng.permutation(3)[: 1 + kind[k]]
        d[k, still] = rng.choice(TINY, len(still))
    # 0.6 of the rays from behind a point near a sphere, along their own direction
    aimed = rng.random(n) < 0.6
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    back = _near_spheres(rng, cr, registered, n) - u * rng.uniform(0.0, 1.0, (n, 1)) * (hi - lo).max()
    o[aimed] = np.clip(back, lo, hi)[aimed]
    return np.hstack([o, d])


def _ties(rng, pl, n):
    """Origins whose offsets from the grid's origin are equal on two or three axes, in fp32 as the kernel subtracts them, with equal
    direction components on those axes: the leaving parameters of those axes are equal at every step.  Candidates whose fp32
    offsets do not come out equal are kept last; tied() says which do."""
    lo, dims, hi = _frame(pl)
    lo32 = lo.astype(np.float32)
    m = 4 * n
    three = np.arange(m) % 3 == 0
    pair = np.array([(0, 1), (0, 2), (1, 2)])[rng.integers(0, 3, m)]
    f = (rng.uniform(0.0, float(dims.min()), m) * pl["cell"]).astype(np.float32)            # the common offset
    o = rng.uniform(lo, hi, (m, 3)).astype(np.float32)
    d = _unit(rng, m).astype(np.float32)
    s = rng.choice(np.array([-1.0, 1.0], np.float32), m) * rng.uniform(0.3, 1.0, m).astype(np.float32)
    for k in range(m):
        axes = (0, 1, 2) if three[k] else pair[k]
        for a in axes:
            o[k, a] = lo32[a] + f[k]
            d[k, a] = s[k]
    rays = np.hstack([o, d]).astype(np.float64)
    order = np.argsort(~tied(rays, pl), kind="stable")                       # the exact ties first
    keep = np.sort(order[:n])
    return rays[keep]


def tied(rays, pl):
    """True where two (or three) axes have equal direction components that step and equal fp32 offsets (float)O - origin: the kernel's
    b = (float)(c + 1 or c) * cell and t = (b - o) * inv_d are then equal on those axes at every step."""
    lo32 = np.array([pl["x0"], pl["y0"], pl["z0"]], np.float32)
    off = rays[:, :3].astype(np.float32) - lo32
    d = rays[:, 3:].astype(np.float32)
    out = np.zeros(len(rays), bool)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        out |= (off[:, a] == off[:, b]) & (d[:, a] == d[:, b]) & (np.abs(d[:, a]) >= 1e-30)
    return out


def _diagonals(rng, cr, pl, n, registered):
    lo, dims, hi = _frame(pl)
    corner = rng.integers(0, 2, (n, 3))
    a = np.where(corner == 0, lo, hi) + rng.uniform(-1.5, 1.5, (n, 3)) * pl["cell"]
    b = np.where(corner == 0, hi, lo) + rng.uniform(-1.5, 1.5, (n, 3)) * pl["cell"]
    # every other ray: a diagonal of one face of the box, within the outermost layer of cells
    face = np.arange(n) % 2 == 1
    axis = rng.integers(0, 3, n)
    level = np.where(corner[np.arange(n), axis] == 0, lo[axis], hi[axis]) + rng.uniform(-0.5, 0.5, n) * pl["cell"]
    a[face, axis[face]] = level[face]
    b[face, axis[face]] = level[face]
    # the space diagonals are moved sideways, without turning, so that they pass a point near a sphere
    u = (b - a) / np.linalg.norm(b - a, axis=1, keepdims=True)
    p = _near_spheres(rng, cr, registered, n)
    shift = (p - a) - ((p - a) * u).sum(axis=1, keepdims=True) * u
    a[~face] += shift[~face]
    b[~face] += shift[~face]
    d = (b - a) * np.exp(rng.uniform(-2, 2, (n, 1)))
    return np.hstack([a, d])


def _entering(rng, cr, pl, n, ctr, registered):
    lo, dims, hi = _frame(pl)
    far_corner = np.linalg.norm(np.maximum(np.abs(lo - ctr), np.abs(hi - ctr)))
    room = 0.9 * pl["rfar"] - far_corner                                     # how far outside the box 0.9 rfar still reaches
    assert room > pl["cell"]
    side = np.arange(n) % 6                                                  # x low, x high, y low, y high, z low, z high
    axis, high = side // 2, side % 2 == 1
    o = rng.uniform(lo, hi, (n, 3))
    depth = rng.uniform(0, 1, n) ** 2 * min(0.7 * room, 40.0 * pl["cell"])
    o[np.arange(n), axis] = np.where(high, hi[axis] + depth, lo[axis] - depth)
    tgt = rng.uniform(lo, hi, (n, 3))
    aimed = rng.random(n) < 0.8
    tgt[aimed] = _near_spheres(rng, cr, registered, n)[aimed]
    # the rim: every third ray is aimed at an edge of the face it enters through, within a tenth of a cell
    rim = np.arange(n) % 3 == 2
    other = (axis + 1 + rng.integers(0, 2, n)) % 3
    edge = np.where(rng.integers(0, 2, n) == 0, lo[other], hi[other]) + rng.uniform(-0.1, 0.1, n) * pl["cell"]
    tgt[rim, axis[rim]] = np.where(high, hi[axis], lo[axis])[rim]
    tgt[rim, other[rim]] = edge[rim]
    o[rim, other[rim]] = (edge + rng.uniform(-1, 1, n) * pl["cell"])[rim]
    assert (np.linalg.norm(o - ctr, axis=1) <= 0.9 * pl["rfar"]).all()
    return np.hstack([o, tgt - o])


def _inside(rng, cr, pl, n, registered):
    lo, dims, hi = _frame(pl)
    o = rng.uniform(lo, hi, (n, 3))
    k = registered[rng.integers(0, len(registered), n)]
    in_sphere = np.arange(n) % 3 == 0
    o[in_sphere] = (cr[k, :3] + _unit(rng, n) * cr[k, 3:4] * rng.uniform(0.0, 0.9, (n, 1)))[in_sphere]
    return np.hstack([o, _unit(rng, n) * np.exp(rng.uniform(-2, 2, (n, 1)))])


def _vertical(rng, cr, pl, n, registered):
    lo, dims, hi = _frame(pl)
    k = registered[rng.integers(0, len(registered), n)]
    ix, iz = rng.integers(0, dims[0] + 1, n), rng.integers(0, dims[2] + 1, n)
    kind = np.arange(n) % 3                                                  # through a sphere's centre, a cell's centre, a cell's corner
    x = np.where(kind == 0, cr[k, 0], lo[0] + (ix + np.where(kind == 1, 0.5, 0.0)) * pl["cell"])
    z = np.where(kind == 0, cr[k, 2], lo[2] + (iz + np.where(kind == 1, 0.5, 0.0)) * pl["cell"])
    y = rng.uniform(lo[1] - 3.0, hi[1] + 3.0, n)
    ends = np.arange(n) % 8 == 7                                             # from beyond either end, towards the grid: the whole height
    up = rng.random(n) < 0.5
    y[ends] = np.where(up, lo[1] - 2.0, hi[1] + 2.0)[ends]
    return np.column_stack([x, y, z, np.zeros(n), np.where(up, 1.0, -1.0), np.zeros(n)])


def _far(rng, pl, n, ctr):
    lo, dims, hi = _frame(pl)
    o = ctr + _unit(rng, n) * pl["rfar"] * rng.uniform(1.05, 3.0, (n, 1))
    d = rng.uniform(lo, hi, (n, 3)) - o                                       # beyond rfar, aimed at the cloud
    kind = np.arange(n) % 8
    o[kind == 4, rng.integers(0, 3)] = np.nan
    o[kind == 5, rng.integers(0, 3)] = np.inf
    o[kind == 6] *= 1e20                                                      # huge origins
    d[kind == 7] *= 1e25                                                      # huge directions: |D|^2 overflows the sane range
    d[kind == 3, rng.integers(0, 3)] = np.nan
    return np.hstack([o, d])


def families(cr, plan, prec, n_each, seed):
    """(rays [8 n_each, 6] in the type of a handle of `prec`, {family: slice}) around the volume grid of `plan` (with tables) for the
    spheres cr [n, 4]."""
    cr = np.asarray(cr, np.float64)
    rng = np.random.default_rng(seed)
    ctr = volume_scene.centre_of(cr)
    registered = np.nonzero(np.asarray(plan["halfwidth"]) > 0)[0]
    fam = [_faces(rng, cr, plan, n_each, registered), _parallel(rng, cr, plan, n_each, registered), _ties(rng, plan, n_each),
           _diagonals(rng, cr, plan, n_each, registered), _entering(rng, cr, plan, n_each, ctr, registered), _inside(rng, cr, plan, n_each, registered), _vertical(rng, cr, plan, n_each, registered),
           _far(rng, plan, n_each, ctr)]
    assert all(f.shape == (n_each, 6) for f in fam)
    with np.errstate(over="ignore", invalid="ignore"):
        rays = np.vstack(fam).astype(np.float32)                             # fp32 numbers in either precision
    return rays.astype(np.float32 if prec == 32 else np.float64), {name: slice(k * n_each, (k + 1) * n_each) for k, name in enumerate(FAMILIES)}


@functools.lru_cache(maxsize=4)
def case(rt, name, prec, n_each=N_EACH):
    """(scene, cr as fp64, plan with tables, rays, {family: slice}) of a scene of tests/volume_scene.py by name ("cube14", "with_bad",
    "column"): the very rays the GPU tests trace."""
    sc = {"cube14": lambda: volume_scene.cube(14, prec), "with_bad": lambda: volume_scene.with_bad(prec), "column": lambda: volume_scene.column(prec)}[name]()
    cr = np.asarray(sc["center_radius"], np.float64)
    pl = rt.debug_volume_grid_plan(cr, volume_scene.centre(sc), tables=True)
    rays, where = families(cr, pl, prec, n_each, 17 + prec)
    return sc, cr, pl, rays, where


def within_reach(rays, where, cr, plan):
    """Indices of the rays of the WALKED families whose origin lies within 0.99 rfar of the recentring point (the kernel walks for
    |O - ctr|^2 <= 0.999 rfar^2) and whose squared length is an ordinary number: every wave made of these alone must walk."""
    pick = np.concatenate([np.arange(where[name].start, where[name].stop) for name in WALKED])
    r = rays[pick].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        a = (r[:, 3:] ** 2).sum(axis=1)
        ok = (np.linalg.norm(r[:, :3] - volume_scene.centre_of(cr), axis=1) <= 0.99 * plan["rfar"]) & (a > 1e-29) & (a < 1e29)
    return pick[ok]
