"""tests/preview_model.py pinned on the CPU: the CRC-32 of every restatement's output on one small input that reaches every case of the
history update -- carried, rejected, off the base's frame, sky, never sampled, empty -- with the clamp active on most pixels.  The GPU
tests compare the library with the model bit for bit; this keeps the model itself from moving where there is no GPU."""
import zlib

import numpy as np
import pytest

from tests.preview_drive import INF, history_defaults, moves
from tests.preview_model import (as_base, clipped_np, feedback_np, filter_np, gamma, guides_np, noise_np, plan_np, positive_part, same_bits,
                                 same_bits_nan, temporal_noise_np, update_np, variance_filter_np)

W, H = 48, 32
PINS = {
    32: {"C": "60c11327", "M": "0d1c0e8e", "cl": "95b6eee2", "V0": "250df2a7", "f": "68afd907", "fv": "d862ebe1", "fb": "88033a4b"},
    64: {"C": "952c0fc9", "M": "1812c367", "cl": "d50dfd50", "V0": "04469716", "f": "2c5fc402", "fv": "22b70fb5", "fb": "c5ab6a20"},
}


def _crc(a):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff)


@pytest.mark.parametrize("prec", [32, 64])
def test_the_model_keeps_its_bits(native, oracle, prec):
    T = np.float32 if prec == 32 else np.float64
    cams = moves(native, prec, W, H)
    params = history_defaults(native)
    g = {v: guides_np(native, oracle, prec, 3, cams[v], np.arange(H)) for v in ("home", "orbit")}
    y, x = np.mgrid[0:H, 0:W]
    colour = lambda shift: np.stack([((x * 7 + y * 13 + ch * 5 + shift) % 17) / 16.0 for ch in range(3)], axis=-1).astype(T)
    home = {"c": colour(0), "n": np.full((H, W), 3, np.int32), "N": g["home"][0], "t": g["home"][2]}
    c0, m0, _ = update_np(cams["home"], home, None, *params)
    base = as_base(cams["home"], home, c0, m0)
    n = ((x + 2 * y) % 4).astype(np.int32)
    c = np.where((n > 0)[..., None], colour(3), T(0)).astype(T)
    N, A, Z, _ = g["orbit"]
    cur = {"c": c, "n": n, "N": N, "t": Z}

    C, M, carried = update_np(cams["orbit"], cur, base, *params)
    cl = clipped_np(cams["orbit"], cur, base, params, 1, 0.75)
    V0 = temporal_noise_np(C, M, n, np.ones((H, W), T), 1)
    f = filter_np(C, N, A, Z, 3, 0.5, 0.3, 0.3, 1.0)
    fv = variance_filter_np(C, V0, N, A, Z, 3, 2.0, 0.3, 0.3, 1.0)
    fb, _ = feedback_np(C, M, N, A, Z, (0.5, 0.3, 0.3, 1.0), 0.5)
    out = {"C": C, "M": M, "cl": cl["C"], "V0": V0, "f": f, "fv": fv, "fb": fb}

    # the input reaches every case, so the pins cannot go hollow
    m_plan, planned = plan_np(cams["orbit"], N, Z, base, params)
    assert carried == 1480 and int((m_plan == 0).sum()) == 56
    assert int((Z == 0).sum()) == 239 and int((n == 0).sum()) == 384 and int((M == 0).sum()) == 15
    assert cl["clipped"] == 1112 and cl["reprojected"] == 1480
    for name, a in out.items():
        assert a.dtype == T and not np.isnan(a).any(), name

    assert {name: _crc(a) for name, a in out.items()} == PINS[prec]

    # the plan is the update with c = 0 and n = 0
    zero = dict(cur, c=np.zeros_like(c), n=np.zeros_like(n))
    h, m, count = update_np(cams["orbit"], zero, base, *params)
    assert same_bits(m_plan, m) and planned == count == carried and same_bits(cl["h"], h)
    # gamma = +inf clips nothing
    assert same_bits(clipped_np(cams["orbit"], cur, base, params, 1, INF)["C"], C)
    # feedback = 1 where every tap of the window that lies in the frame holds samples: level 0 of filter_np.  filter_np returns its image
    # through gamma, so the filtered commit is compared through gamma too.
    short = np.zeros((H, W), bool)
    pe = np.pad(M == 0, 2)
    for dy in range(5):
        for dx in range(5):
            short |= pe[dy:dy + H, dx:dx + W]
    assert (~short).sum() >= 0.5 * W * H
    full, _ = feedback_np(C, M, N, A, Z, (0.5, 0.3, 0.3, 1.0), 1.0)
    level0 = filter_np(C, N, A, Z, 1, 0.5, 0.3, 0.3, 1.0)
    assert same_bits(np.ascontiguousarray(gamma(full)[~short]), np.ascontiguousarray(level0[~short]))


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_nan_aware_comparison(T):
    """same_bits_nan tells apart what same_bits tells apart, except the bits of two NaNs."""
    bits = np.dtype("u%d" % np.dtype(T).itemsize)
    tiny = np.finfo(T).tiny
    a = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny / 4, 1.5], T)
    assert same_bits_nan(a, a.copy()) and not same_bits_nan(a, a[:-1]) and not same_bits_nan(a, a.astype(np.float16))

    def other(k, value):
        b = a.copy()
        b[k] = value
        return b

    assert not same_bits_nan(a, other(0, -0.0)) and not same_bits_nan(a, other(1, 0.0))          # +0 against -0
    assert not same_bits_nan(a, other(2, -np.inf)) and not same_bits_nan(a, other(3, np.inf))     # +inf against -inf
    assert not same_bits_nan(a, other(6, np.nan)) and not same_bits_nan(a, other(4, 1.0))         # a NaN on one side only
    assert not same_bits_nan(a, other(5, tiny / 2)) and not same_bits_nan(a, other(5, 0.0))       # subnormals count
    # two payloads and both signs of NaN: what x86 and gfx950 give inf - inf, and a propagated payload
    quiet = a.copy().view(bits)
    quiet[4] = (np.array([np.nan], T).view(bits)[0] | 1) ^ (bits.type(1) << bits.type(8 * bits.itemsize - 1))
    b = quiet.view(T)
    assert np.isnan(b[4]) and not same_bits(a, b) and same_bits_nan(a, b) and same_bits_nan(b, a)
    with np.errstate(invalid="ignore"):
        made = np.array([np.inf], T) - np.array([np.inf], T)
    assert same_bits_nan(made, np.array([np.nan], T))


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_max_zero_as_the_library_states_it(T):
    """positive_part is np.maximum(0, x) on everything but a NaN, which it turns into 0 (sections 8 and 10: a NaN variance estimate is
    no spread); noise_np, the restatement of err_p and V_p, through it."""
    tiny = np.finfo(T).tiny
    x = np.array([-np.inf, -1.0, -tiny / 4, -0.0, 0.0, tiny / 4, tiny, 1.0, np.finfo(T).max, np.inf], T)
    assert same_bits(positive_part(x), np.maximum(T(0), x) + T(0)) and positive_part(x).dtype == T
    assert same_bits(positive_part(np.array([np.nan, -np.nan], T)), np.zeros(2, T)) and np.isnan(np.maximum(T(0), T(np.nan)))
    # Y = Y(acc), s2, n -> (err, V): a finite pixel; s2 and the sum both overflowed (inf - inf); a NaN sum; s2 alone overflowed; n < 2
    err, V = noise_np(np.array([3.0, np.inf, np.nan, 3.0, 3.0]), np.array([5.0, np.inf, np.nan, np.inf, 5.0]), np.array([2, 2, 2, 2, 1]), T)
    assert err.dtype == np.float32 and V.dtype == T
    assert err[0] == np.float32(np.sqrt(0.25) / (1.5 + 1e-3)) and V[0] == T(0.25)
    assert err[1] == 0 and V[1] == 0 and np.isnan(err[2]) and V[2] == 0 and not np.signbit(V[1:3]).any()
    assert err[3] == np.inf and V[3] == np.inf and err[4] == np.inf and V[4] == 0
