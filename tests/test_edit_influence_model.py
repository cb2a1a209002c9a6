"""tests/edit_influence_model.py on the CPU: the edit list, omega, the sum's order, lambda and fade of INTEGRATION.md section 20 held to
scalar statements and to hand-computed values, and a small hand-built case pinned as literal bits."""
import types

import numpy as np
import pytest

from tests import edit_influence_model as E
from tests import scene_motion_model as M

DTYPES = [np.float32, np.float64]
INF = float("inf")


def tables(cr, af=None, dt=np.float32):
    cr = np.array(cr, dt).reshape(-1, 4)
    n = len(cr)
    return {"cr": cr, "af": np.array(af if af is not None else [[0.5, 0.5, 0.5, 0.0]] * n, dt).reshape(-1, 4), "ri": np.full(n, 1.5, dt),
            "ty": np.zeros(n, np.int32)}


def still_camera():
    """A camera whose pixel (i, j) looks along D = (i, j, 1) from the origin: P = t D."""
    return types.SimpleNamespace(center=[0.0, 0.0, 0.0], pixel00_loc=[0.0, 0.0, 1.0], pixel_delta_u=[1.0, 0.0, 0.0], pixel_delta_v=[0.0, 1.0, 0.0])


@pytest.mark.parametrize("dt", DTYPES)
def test_one_entry_at_twice_its_radius(dt):
    for r in (0.5, 1.0, 3.0):
        P = np.zeros((1, 1, 3), dt)
        s = E.solid_sum(P, np.full((1, 1), -1, np.int32), np.array([[2 * r, 0, 0, r]], dt), np.array([0], np.int32))
        want = dt(1) - np.sqrt(dt(0.75))                         # q = r^2 / (2r)^2 = 0.25 exactly
        assert s.dtype == dt and s[0, 0].tobytes() == dt(want).tobytes(), (r, s, want)


@pytest.mark.parametrize("dt", DTYPES)
def test_an_entry_that_contains_the_point_gives_one(dt):
    ids = np.full((1, 3), -1, np.int32)
    P = np.array([[[0.0, 0, 0], [0.9, 0, 0], [1.0, 0, 0]]], dt)   # the centre itself (q = inf), inside, on the surface (q = 1)
    s = E.solid_sum(P, ids, np.array([[0, 0, 0, 1]], dt), np.array([0], np.int32))
    assert (s == dt(1)).all()
    assert (E.solid_sum(P, ids, np.array([[0, 0, 0, 1]] * 3, dt), np.array([0, 1, 2], np.int32)) == dt(3)).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_the_own_sphere_is_skipped_and_the_order_is_the_lists(dt):
    entries = np.array([[3, 0, 0, 1], [0, 2.5, 0, 1.25], [0, 0, 7, 0.3], [1, 1, 1, 0.7]], dt)
    owners = np.array([0, 0, 1, 2], np.int32)
    P = np.zeros((1, 4, 3), dt)
    ids = np.array([[-1, 0, 1, 2]], np.int32)
    s = E.solid_sum(P, ids, entries, owners)

    def omega(e):                                                # the scalar statement
        v = e[:3] - P[0, 0]
        q = (e[3] * e[3]) / ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        return dt(1) if q >= 1 else dt(1) - np.sqrt(dt(1) - q)
    for x in range(4):
        want = dt(0)
        for e, o in zip(entries, owners):
            if o != ids[0, x]:
                want = want + omega(e)
        assert s[0, x].tobytes() == dt(want).tobytes(), x
    assert s[0, 1] < s[0, 0] and s[0, 2] < s[0, 0] and s[0, 3] < s[0, 0]
    # the order matters to the bits once the sum passes 1 (every omega is a multiple of half an ulp of 1, so smaller sums are exact):
    # some of these lists sum differently backwards
    rng = np.random.default_rng(3)
    found = False
    for _ in range(200):
        cr = np.concatenate([rng.uniform(-4, 4, (8, 3)), rng.uniform(0.2, 3.5, (8, 1))], axis=1).astype(dt)
        ow = np.arange(8, dtype=np.int32)
        a = E.solid_sum(P[:, :1], ids[:, :1], cr, ow)
        b = E.solid_sum(P[:, :1], ids[:, :1], cr[::-1], ow[::-1])
        fwd = dt(0)
        for e in cr:
            fwd = fwd + omega(e)
        assert a[0, 0].tobytes() == dt(fwd).tobytes()
        found = found or a[0, 0].tobytes() != b[0, 0].tobytes()
    assert found


@pytest.mark.parametrize("dt", DTYPES)
def test_lambda_and_fade(dt):
    cam = still_camera()
    depth = np.array([[2.0, 2.0, 0.0, 2.0]], dt)                 # pixel 2 is the sky
    carry = np.array([[1, 1, 1, 0]], np.int32)                   # pixel 3 shows a changed surface
    ids = np.array([[0, 1, -1, 2]], np.int32)
    entries = np.array([[0, 0, 4, 1]], dt)                       # owner 1: pixel 1's own sphere
    owners = np.array([1], np.int32)
    lam, fade, s = E.influence_np(cam, depth, carry, ids, entries, owners, 0.5)
    assert lam.dtype == fade.dtype == s.dtype == dt
    assert s[0, 0] > 0 and s[0, 1] == 0 and s[0, 2] == 0 and s[0, 3] == 0
    assert lam[0, 0].tobytes() == dt(dt(0.5) * s[0, 0]).tobytes() and fade[0, 0].tobytes() == dt(dt(1) - lam[0, 0]).tobytes()
    assert (lam[0, 1:] == 0).all() and fade[0, 1] == 1 and fade[0, 2] == 1 and fade[0, 3] == 0
    # kappa = inf: any influence at all drops the history; s == 0 gives 0, not NaN
    lam, fade, _ = E.influence_np(cam, depth, carry, ids, entries, owners, INF)
    assert np.array_equal(lam, np.array([[1, 0, 0, 0]], dt)) and np.array_equal(fade, np.array([[0, 1, 1, 0]], dt))
    # the cap at 1
    lam, _, _ = E.influence_np(cam, depth, carry, ids, entries, owners, 1e6)
    assert lam[0, 0] == 1
    # kappa == 0: fade is carry
    lam, fade, _ = E.influence_np(cam, depth, carry, ids, entries, owners, 0.0)
    assert (lam == 0).all() and np.array_equal(fade, carry.astype(dt))
    # an empty list
    lam, fade, s = E.influence_np(cam, depth, carry, ids, np.zeros((0, 4), dt), np.zeros(0, np.int32), INF)
    assert (lam == 0).all() and (s == 0).all() and np.array_equal(fade, carry.astype(dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_the_edit_list(dt):
    snap = tables([[0, 0, 0, 1], [2, 0, 0, 1], [4, 0, 0, 1], [6, 0, 0, 1], [8, 0, 0, 1]], dt=dt)
    cur = tables([[0, 0, 0, 1], [2, 0.5, 0, 1], [4, 0, 0, 1], [6, 0, 0, 1.5], [8, 0, 0, 1]], dt=dt)
    cur["af"][2, 0] = 0.25                                       # 2: changed only
    cur["ty"][3] = 1                                             # 3: moved and changed
    entries, owners = E.edit_list(cur, snap)
    assert entries.dtype == dt and owners.dtype == np.int32
    assert owners.tolist() == [1, 1, 2, 3, 3]
    assert np.array_equal(entries, np.array([[2, 0, 0, 1], [2, 0.5, 0, 1], [4, 0, 0, 1], [6, 0, 0, 1], [6, 0, 0, 1.5]], dt))
    entries, owners = E.edit_list(snap, snap)
    assert entries.shape == (0, 4) and owners.shape == (0,)
    neg = tables([[0.0, 0, 0, 1]], dt=dt)
    negz = tables([[-0.0, 0, 0, 1]], dt=dt)                      # bits against bits: -0 is a move
    assert E.edit_list(negz, neg)[1].tolist() == [0, 0]


def test_the_faded_gather_multiplies_after_the_cap():
    dt = np.float32
    cam = still_camera()
    cam.img_width, cam.img_height = 4, 1
    depth = np.full((1, 4), 2.0, dt)
    normal = np.tile(np.array([0, 0, -1], dt), (1, 4, 1))
    base = {"cam": cam, "H": np.full((1, 4, 3), 0.5, dt), "M": np.full((1, 4), 40.0, dt), "N": normal, "z": depth}
    Q = E.points(cam, depth)
    fade = np.array([[1.0, 0.75, 0.0, 0.25]], dt)
    params = (0.1, 0.9, 16.0)
    m, count = E.plan_np(cam, normal, depth, base, params, Q, fade)
    assert np.array_equal(m, np.array([[16.0, 12.0, 0.0, 4.0]], dt)) and count == 3          # the cap first, then the fade
    plain, _ = M.plan_np(cam, normal, depth, base, params, Q, np.ones((1, 4), np.int32))
    assert np.array_equal(plain, np.full((1, 4), 16.0, dt))
    cur = {"c": np.full((1, 4, 3), 0.25, dt), "n": np.full((1, 4), 4, np.int32), "N": normal, "t": depth}
    C, Mo, count = E.update_np(cam, cur, base, params, Q, fade)
    assert np.array_equal(Mo, m + dt(4)) and count == 3 and C[0, 2, 0] == dt(0.25)           # a fully faded pixel blends to its own colour


# 3 spheres (sphere 0 moved, sphere 1 changed, sphere 2 neither), 4 points: hits of spheres -1 (sky), 0, 2, 2.  s, lambda at kappa = 0.5
# and fade as the bits of T.
PINS = {
    np.float32: ([0, 1040789668, 1029927392, 1014647936], [0, 1032401060, 1021538784, 1006259328], [1065353216, 1064229356, 1064887409, 1065225063]),
    np.float64: ([0, 4593994963823283544, 4588163330925793312, 4579960198105721536], [0, 4589491364195913048, 4583659731298422816, 4575456598478351040],
                 [4607182418800017408, 4606579050858423893, 4606932340365954943, 4607113617422480938]),
}


@pytest.mark.parametrize("dt", DTYPES)
def test_a_hand_built_case_is_pinned(dt):
    snap = tables([[0, 0, 3, 1], [2, 0, 3, 0.5], [0, -100, 3, 99]], dt=dt)
    cur = tables([[0.25, 0.5, 3, 1], [2, 0, 3, 0.5], [0, -100, 3, 99]], af=[[0.5, 0.5, 0.5, 0], [0.1, 0.2, 0.3, 0], [0.5, 0.5, 0.5, 0]], dt=dt)
    entries, owners = E.edit_list(cur, snap)
    assert owners.tolist() == [0, 0, 1]
    cam = still_camera()
    depth = np.array([[0.0, 2.0, 2.5, 3.0]], dt)
    ids = np.array([[-1, 0, 2, 2]], np.int32)
    carry = np.ones((1, 4), np.int32)
    lam, fade, s = E.influence_np(cam, depth, carry, ids, entries, owners, 0.5)
    got = tuple(a.view(np.uint32 if dt == np.float32 else np.uint64).ravel().tolist() for a in (s, lam, fade))
    print(dt.__name__, got)
    assert got == PINS[dt]
    # against float64 arithmetic of the closed form, to the precision of T
    P = np.array([[i * t, 0.0, t] for i, t in enumerate(depth[0].astype(np.float64))])
    for x in range(1, 4):
        want = 0.0
        for e, o in zip(entries.astype(np.float64), owners):
            if o != ids[0, x]:
                q = e[3] ** 2 / ((e[:3] - P[x]) ** 2).sum()
                want += 1.0 if q >= 1 else 1 - np.sqrt(1 - q)
        assert abs(float(s[0, x]) - want) <= 16 * np.finfo(dt).eps * max(want, 1.0), (x, s[0, x], want)
    assert s[0, 0] == 0 and fade[0, 0] == 1
