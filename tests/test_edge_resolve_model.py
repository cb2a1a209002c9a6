"""tests/edge_resolve_model.py pinned on the CPU: the CRC-32 of its outputs on a small synthetic frame with hand-built layers and a random
filtered image, and on the coverage layers of a small real frame; the model against a scalar restatement written pixel by pixel; and the
properties INTEGRATION.md section 17 states -- pure pixels untouched, prior = +inf gives the rebuilt colour R, a mixed pixel without pure
neighbours untouched, a three-surface pixel keeps `rest` for its own value.  tests/test_edge_resolve.py compares the library with the
model bit for bit; this keeps the model itself from moving where there is no GPU."""
import zlib

import numpy as np
import pytest

from tests.edge_resolve_model import INF, NO_LAYER, SKY, coverage_np, layers_np, resolve_np, scene_of
from tests.preview_model import same_bits

W, H, S = 13, 9, 16
PINS = {
    32: {"r1": "2e10569a", "r3": "5357233c", "inf": "d13e9fdb", "ids": "5d7e1cc8", "counts": "648c44dc", "normal": "59748a21", "depth": "4894eb3b"},
    64: {"r1": "d83dd07b", "r3": "627bef8d", "inf": "aba2ab4e", "ids": "5d7e1cc8", "counts": "648c44dc", "normal": "5ee7bb86", "depth": "4e37460f"},
}


def _crc(a):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff)


def synthetic(T):
    """A 13 x 9 frame: sphere 5 on the left, sphere 7 on the right, a mixed column between them; sky above with a mixed row under it
    (sphere and sky); one three-surface pixel (counts 8 + 5 of 16); one mixed pixel whose layers (20, 21) no pure pixel has; mixed pixels
    in two corners.  Returns the layers, the first-hit guides, a random gamma-encoded image and sample counts with zeros."""
    rng = np.random.default_rng(17)
    ids = np.zeros((H, W, 2), np.int32); counts = np.zeros((H, W, 2), np.int32)
    ids[..., 0] = 5; ids[:, 7:, 0] = 7; ids[:2, :, 0] = SKY
    ids[..., 1] = NO_LAYER; counts[..., 0] = S
    mixed = lambda y, x, a, b, ca, cb: (ids.__setitem__((y, x), (a, b)), counts.__setitem__((y, x), (ca, cb)))
    for y in range(3, H):
        mixed(y, 6, 5, 7, 10, 6) if y % 2 else mixed(y, 6, 7, 5, 9, 7)
    for x in range(W):
        if x != 6:
            mixed(2, x, SKY, 5 if x < 6 else 7, 8, 8) if x % 3 else mixed(2, x, 5 if x < 6 else 7, SKY, 12, 4)
    mixed(2, 6, 5, 7, 8, 5)                                   # three surfaces: the sky's 3 sub-samples were dropped
    mixed(6, 10, 20, 21, 11, 5)                               # no pure pixel of either layer anywhere
    mixed(H - 1, 0, 5, 7, 15, 1); mixed(0, W - 1, SKY, 7, 13, 3)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    N = unit(rng.normal(size=(H, W, 3))).astype(T); Z = rng.uniform(1, 12, (H, W)).astype(T)
    sky = ids[..., 0] == SKY
    N[sky] = 0; Z[sky] = 0
    normal = unit(rng.normal(size=(H, W, 2, 3))).astype(T); depth = rng.uniform(1, 12, (H, W, 2)).astype(T)
    for l in range(2):
        none = ids[..., l] < 0
        normal[none, l] = 0; depth[none, l] = 0
    g = np.sqrt(rng.uniform(0, 1, (H, W, 3))).astype(T)
    n = rng.integers(0, 20, (H, W)).astype(np.int32)
    n[4, 6] = 0
    return ids, counts, normal, depth, N, Z, g, n


def scalar_resolve(T, g, ids, counts, normal, depth, N, Z, n_eff, radius, sn, sz, prior):
    """INTEGRATION.md section 17 pixel by pixel on scalars of T: the second statement the vectorised model is held to."""
    out = g.copy()
    i_n, i_z = T(1.0 / (sn * sn)), T(1.0 / (sz * sz))
    for y in range(H):
        for x in range(W):
            if ids[y, x, 1] == NO_LAYER:
                continue
            L = [g[y, x, c] * g[y, x, c] for c in range(3)]
            R, rest, any_found = [T(0)] * 3, T(1), False
            for l in range(2):
                Sx, Wt = [T(0)] * 3, T(0)
                for dy in range(-radius, radius + 1):
                    for dx in range(-radius, radius + 1):
                        qy, qx = y + dy, x + dx
                        if not (0 <= qy < H and 0 <= qx < W) or ids[qy, qx, 1] != NO_LAYER or ids[qy, qx, 0] != ids[y, x, l]:
                            continue
                        d = N[qy, qx] - normal[y, x, l]
                        en = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                        dz = Z[qy, qx] - depth[y, x, l]
                        w = T(1) / (T(1) + (en * i_n + (dz * dz) * i_z))
                        Sx = [Sx[c] + w * (g[qy, qx, c] * g[qy, qx, c]) for c in range(3)]
                        Wt = Wt + w
                if Wt > 0:
                    a = T(counts[y, x, l]) / T(S)
                    R = [R[c] + a * (Sx[c] / Wt) for c in range(3)]
                    rest = rest - a
                    any_found = True
            if not any_found:
                continue
            for c in range(3):
                r = R[c] + rest * L[c]
                o = r if prior == INF else L[c] + (T(prior) / (T(prior) + T(n_eff[y, x]))) * (r - L[c])
                out[y, x, c] = np.sqrt(o) if o > 0 else T(0)
    return out


@pytest.mark.parametrize("prec", [32, 64])
def test_the_model_keeps_its_bits(native, oracle, prec):
    T = np.float32 if prec == 32 else np.float64
    ids, counts, normal, depth, N, Z, g, n = synthetic(T)
    layers = (ids, counts, normal, depth)
    mixed = ids[..., 1] != NO_LAYER
    r1, w1 = resolve_np(g, *layers, N, Z, n, S, 1, 0.3, 0.5, 8.0)
    r3, w3 = resolve_np(g, *layers, N, Z, n.astype(T), S, 3, INF, 2.0, 2.5)
    rinf, winf = resolve_np(g, *layers, N, Z, n, S, 2, 0.3, 0.5, INF)
    for out, wrote in ((r1, w1), (r3, w3), (rinf, winf)):
        assert out.dtype == T and np.isfinite(out).all()
        # pure pixels keep their bits; so does the mixed pixel whose layers nobody has, and every other mixed pixel is rewritten
        assert same_bits(np.ascontiguousarray(out[~wrote]), np.ascontiguousarray(g[~wrote])) and not (wrote & ~mixed).any()
        assert not wrote[6, 10] and int(wrote.sum()) == int(mixed.sum()) - 1 == 21
    # the vectorised model is the scalar statement, bit for bit, on every pixel
    assert same_bits(r1, scalar_resolve(T, g, *layers, N, Z, n, 1, 0.3, 0.5, 8.0))
    assert same_bits(r3, scalar_resolve(T, g, *layers, N, Z, n, 3, INF, 2.0, 2.5))
    assert same_bits(rinf, scalar_resolve(T, g, *layers, N, Z, n, 2, 0.3, 0.5, INF))
    # n = 0: beta = 1, which is R up to the rounding of L + (R - L)
    np.testing.assert_allclose(resolve_np(g, *layers, N, Z, n, S, 2, 0.3, 0.5, 8.0)[0][4, 6], rinf[4, 6], rtol=1e-5)

    # the coverage layers of a small real frame: both lattices, a frame that is no multiple of the tile
    cam = native.camera(prec, 29, 19, 1, 5)
    cov4 = coverage_np(oracle, prec, scene_of(native, 3, prec), cam, np.arange(19), 4)
    cov2 = coverage_np(oracle, prec, scene_of(native, 3, prec), cam, np.arange(19), 2)
    assert ((cov4[1].sum(-1) <= 16) & (cov4[1][..., 0] >= cov4[1][..., 1])).all() and (cov2[1].sum(-1) <= 4).all()
    assert (cov4[4] >= 3).any() and ((cov4[0][..., 1] != NO_LAYER) == (cov4[4] >= 2)).all()
    assert ((cov4[0] == SKY).any(-1) & (cov4[0][..., 1] != NO_LAYER)).any()
    got = {"r1": r1, "r3": r3, "inf": rinf, "ids": np.concatenate([cov4[0].ravel(), cov2[0].ravel()]),
           "counts": np.concatenate([cov4[1].ravel(), cov2[1].ravel()]), "normal": np.concatenate([cov4[2].ravel(), cov2[2].ravel()]),
           "depth": np.concatenate([cov4[3].ravel(), cov2[3].ravel()])}
    assert {name: _crc(a) for name, a in got.items()} == PINS[prec]


@pytest.mark.parametrize("prec", [32, 64])
def test_layers_rank_by_count_then_by_the_smaller_id(prec):
    T = np.float32 if prec == 32 else np.float64
    # five pixels of 4 sub-samples: pure; 2 + 2 (the smaller id first, the sky smallest); 2 + 1 + 1 (the tie for second place goes to the
    # smaller id, the third is dropped); all sky; 3 + 1
    k = np.array([[4, 4, 4, 4], [9, 3, 3, 9], [SKY, 6, 6, SKY], [8, 2, 5, 8], [SKY] * 4, [1, 7, 7, 7]], np.int32).T
    t = (np.arange(24).reshape(4, 6) + 1).astype(T)
    t[k == SKY] = 0
    N = np.stack([t * T(0.25), -t, t * t], -1).astype(T)
    ids, counts, normal, depth = layers_np(k, N, t)
    assert ids.tolist() == [[4, NO_LAYER], [3, 9], [SKY, 6], [8, 2], [SKY, NO_LAYER], [7, 1]]
    assert counts.tolist() == [[4, 0], [2, 2], [2, 2], [2, 1], [4, 0], [3, 1]]
    third = T(1) / T(3)
    assert depth[5, 0] == ((T(0) + t[1, 5]) + t[2, 5] + t[3, 5]) * third and depth[5, 1] == t[0, 5] and depth[3, 1] == t[1, 3]
    assert (normal[2, 0] == 0).all() and depth[2, 0] == 0 and (normal[0, 1] == 0).all() and depth[4, 1] == 0
    assert normal[1, 1].tolist() == [((N[0, 1, c] + N[3, 1, c]) * T(0.5)) for c in range(3)]


@pytest.mark.parametrize("prec", [32, 64])
def test_a_three_surface_pixel_keeps_rest_for_its_own_value(prec):
    """Flat colours: every pure pixel of sphere 5 holds v5, of sphere 7 v7, so F_l is v_l^2 up to rounding, and with prior = +inf the
    three-surface pixel (8 + 5 of 16) must come out as 8/16 v5^2 + 5/16 v7^2 + 3/16 of its own L."""
    T = np.float32 if prec == 32 else np.float64
    ids, counts, normal, depth, N, Z, g, n = synthetic(T)
    g = g.copy()
    g[ids[..., 0] == 5] = (0.5, 0.25, 0.75); g[ids[..., 0] == 7] = (0.125, 1.0, 0.5)
    own = np.array((0.9, 0.8, 0.1), T)
    g[2, 6] = own
    out, wrote = resolve_np(g, ids, counts, normal, depth, N, Z, n, S, 2, 0.3, 0.5, INF)
    assert wrote[2, 6]
    want = 0.5 * np.array((0.5, 0.25, 0.75)) ** 2 + 0.3125 * np.array((0.125, 1.0, 0.5)) ** 2 + 0.1875 * own.astype(np.float64) ** 2
    np.testing.assert_allclose(out[2, 6].astype(np.float64) ** 2, want, rtol=2e-6 if prec == 32 else 1e-13)


@pytest.mark.parametrize("scene_id", [1, 3, "lattice"])
@pytest.mark.parametrize("prec", [32, 64])
def test_the_gpu_tests_big_frame_holds_every_class_of_pixel(native, oracle, prec, scene_id):
    """The 64 x 40 frames of tests/test_edge_resolve.py, on the CPU: their mixed pixels include a three-surface pixel and a mixed pixel
    with a sky layer, beside pure pixels of sphere and sky, at the 4 x 4 lattice; the 2 x 2 lattice finds mixed pixels too."""
    from tests.test_edge_resolve import BIG, view
    W, H = BIG
    cam = view(native, prec, scene_id, W, H)
    ids, counts, _, _, surfaces = coverage_np(oracle, prec, scene_of(native, scene_id, prec), cam, np.arange(H), 4)
    mixed = ids[..., 1] != NO_LAYER
    assert (surfaces >= 3).sum() >= 5 and (mixed & (ids == SKY).any(-1)).sum() >= 5
    assert (~mixed & (ids[..., 0] == SKY)).any() and (~mixed & (ids[..., 0] >= 0)).any()
    assert (coverage_np(oracle, prec, scene_of(native, scene_id, prec), cam, np.arange(H), 2)[0][..., 1] != NO_LAYER).sum() >= 20
