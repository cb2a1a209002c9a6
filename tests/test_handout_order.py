"""The hand-out order of the sorted schedule itself: what decides WHEN and WHERE a pixel runs, which no image can show.

The test hook rtiow_debug_read_order (include/rtiow_debug.h) returns the order the render kernels take their pixels from -- the
ranking of a two-phase render (also after the renders that reuse it), the ranking of a progressive chunk, the active list of an adaptive
chunk -- with the parameters it was dealt by.  A plain numpy statement of the deal (forward_map: the comment at the top of
csrc/device/cost_sort.h) holds it to its invariants: a permutation with padding only in the deal's holes, the exact inverse in slot_of,
heavy bins first, one contiguous run of ranks per 64 x 64 super-tile and bin.  rtiow_debug_poison_staged makes a slot that a reused
order never hands out show in the image; rtiow_debug_timeline counts the pixels every wave took.  Nothing here is timed."""
import numpy as np
import pytest

from tests.conftest import compact
from tests.test_order_reuse import BASE, _check_image, _invalidation_cases, _reference, _setup

gpu = pytest.mark.gpu

POOL = 64            # pixels of a pool (device/render_kernels.h)
COST_BINS = 1024     # device/cost_sort.h


# ---- the reference: rank -> slot, and the sort key

def forward_map(n, solo_slots, pools_per_block, total_pools, deal_group):
    """Slot of every sorted rank 0..n-1.  The first solo_slots ranks keep their number.  The others are cut into blocks of
    pools_per_block pools (the last block has the pools that are left); inside a block, groups of deal_group consecutive ranks go
    round-robin over the block's pools, and a pool's groups fill its 64 lanes in turn."""
    r = np.arange(n, dtype=np.int64)
    q_all = np.maximum(r - solo_slots, 0)
    per_block = pools_per_block * POOL
    blk, q = q_all // per_block, q_all % per_block
    pools_here = np.minimum(pools_per_block, total_pools - blk * pools_per_block)
    g, j = q // deal_group, q % deal_group
    pool = blk * pools_per_block + g % pools_here
    lane = (g // pools_here) * deal_group + j
    return np.where(r < solo_slots, r, solo_slots + pool * POOL + lane)


def cost_bin(keys):
    return np.minimum(keys.astype(np.int64), COST_BINS - 1)


def smoothed_keys(own, strip, hw=6):
    """The sort key: the mean of the cost over the 13 x 13 window clipped to the image and to the pixel's own row strip, in quarter
    segments, rounded to nearest (the definition test_sort_key_is_the_neighbourhood_mean_of_the_prepass_cost holds cost_smooth_kernel to)."""
    rows, W = own.shape
    csum = np.zeros((rows + 1, W + 1), np.int64)
    csum[1:, 1:] = own.astype(np.int64).cumsum(0).cumsum(1)
    jl = np.arange(rows)[:, None]; i = np.arange(W)[None, :]
    s0 = (jl // strip) * strip
    j0 = np.maximum(jl - hw, s0); j1 = np.minimum(np.minimum(jl + hw, s0 + strip - 1), rows - 1)
    i0 = np.maximum(i - hw, 0); i1 = np.minimum(i + hw, W - 1)
    total = csum[j1 + 1, i1 + 1] - csum[j0, i1 + 1] - csum[j1 + 1, i0] + csum[j0, i0]
    cells = (j1 - j0 + 1) * (i1 - i0 + 1)
    return (4 * total + cells // 2) // cells


def _runs(ids):
    """Number of maximal runs of equal neighbours in a sequence."""
    return 0 if len(ids) == 0 else 1 + int(np.count_nonzero(np.diff(ids)))


def check_ranking(info, order, slot_of, keys, W, rows):
    """The invariants of a ranking (a render's: with slot_of; a progressive chunk's: without, and no solo slots).  Returns the local
    pixel index at every rank, heaviest first."""
    npix = W * rows
    assert (info["W"], info["local_rows"]) == (W, rows), info
    solo, pools, ppb, group = info["solo_slots"], info["total_pools"], info["pools_per_block"], info["deal_group"]
    assert pools == (npix + POOL - 1) // POOL and info["total_slots"] == solo + pools * POOL == len(order), info
    assert 1 <= ppb <= pools and group in (1, 64) and 0 <= solo <= npix // 2, info
    # permutation and padding
    fwd = forward_map(npix, solo, ppb, pools, group)
    taken = np.zeros(len(order), bool)
    taken[fwd] = True
    assert taken.sum() == npix                                              # the reference map itself hits npix distinct slots
    assert (order[taken] >= 0).all(), "a slot the deal hands a rank to holds no pixel"
    assert (order[~taken] == -1).all(), "a pixel (or rubbish) sits where the deal sends no rank"
    assert int((order == -1).sum()) == len(order) - npix
    packed = ((np.arange(rows, dtype=np.int64)[:, None] << 16) | np.arange(W, dtype=np.int64)[None, :]).ravel()
    assert np.array_equal(np.sort(order[taken].astype(np.int64)), packed), "the order is not every local pixel exactly once"   # packed is ascending
    # inverse
    if slot_of is not None:
        so = slot_of.ravel().astype(np.int64)
        assert so.min() >= 0 and so.max() < len(order)
        assert np.array_equal(order[so].astype(np.int64), packed), "slot_of is not the inverse of the order"
    else:
        assert solo == 0
    # heavy first
    at_rank = order[fwd].astype(np.int64)
    pix = (at_rank >> 16) * W + (at_rank & 0xffff)
    bins = cost_bin(keys.ravel())[pix]
    assert (np.diff(bins) <= 0).all(), "the bins do not run heavy-first along the ranks"
    if 0 < solo < npix:
        assert bins[:solo].min() >= bins[solo:].max()
    # locality: one contiguous run of ranks per (bin, 64 x 64 super-tile) -- a workgroup reserves its range of a bin with one atomic
    st = ((at_rank >> 16) >> 6) * ((W + 63) >> 6) + ((at_rank & 0xffff) >> 6)
    pair = bins * (int(st.max()) + 1) + st
    assert _runs(pair) == len(np.unique(pair)), "a super-tile's pixels of one bin are not adjacent in rank"
    return pix


def check_render_ranking(r, W, rows, strip, solo_expected=None):
    """check_ranking for what a render left, plus the parameters the stats and rtiow_debug_read_costs must agree with."""
    info, order, slot_of, keys = r.debug_read_order()
    st = r.stats()
    assert info["kind"] == 1 and slot_of is not None and keys is not None, info
    check_ranking(info, order, slot_of, keys, W, rows)
    assert info["solo_slots"] == st["solo_waves"] * st["solo_lanes"], (info, st)
    assert info["blocks"] == st["grid_blocks"] and info["lane_cap"] in (16, 32, 64), (info, st)
    if solo_expected is not None:
        assert (info["solo_slots"] > 0) == solo_expected, info
    own, smoothed = r.debug_read_costs()
    assert np.array_equal(keys, smoothed)
    assert np.array_equal(keys.astype(np.int64), smoothed_keys(own, strip)), "the keys are not the smoothing of this frame's prepass costs"
    return info, order, slot_of, keys


@pytest.fixture(scope="module")
def rt(native):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return native


def _strip(rows, shard):
    return shard[2] if shard else rows       # one rank: the window crosses its strips (plan_deal)


# ---- 3. the reference itself, on the CPU

def test_forward_map_is_a_bijection_into_the_slots():
    """So that a GPU failure points at the kernel and not at this file's arithmetic: for every parameter set the map sends the ranks
    [0, n) to n distinct slots inside [0, solo_slots + total_pools x 64), the solo ranks to themselves."""
    cases = []
    for total_pools in (1, 2, 5, 8, 68, 143):
        for ppb in sorted({1, 2, 3, 4, 8, 64, total_pools}):
            if ppb > total_pools:
                continue
            for group in (1, 8, 64):
                for solo in (0, 2, 256):
                    for n_ranked in {total_pools * POOL, total_pools * POOL - 1, total_pools * POOL - 63, (total_pools - 1) * POOL + 1, 1}:
                        if n_ranked >= 1:
                            cases.append((solo + n_ranked, solo, ppb, total_pools, group))
    # named: a last block with fewer pools (5 pools in blocks of 2 and 3; 143 in blocks of 64), n one below and one above a pool
    # boundary ((P - 1) x 64 + 1 and P x 64 - 1), pools_per_block == total_pools
    assert (5 * POOL, 0, 2, 5, 64) in cases and (143 * POOL - 1, 0, 64, 143, 1) in cases and (7 * POOL + 1 + 2, 2, 8, 8, 64) in cases
    assert any(c[2] == c[3] for c in cases) and any(c[3] % c[2] for c in cases)
    for n, solo, ppb, pools, group in cases:
        fwd = forward_map(n, solo, ppb, pools, group)
        assert fwd.min() >= 0 and fwd.max() < solo + pools * POOL, (n, solo, ppb, pools, group)
        assert len(np.unique(fwd)) == n, (n, solo, ppb, pools, group)
        assert np.array_equal(fwd[:solo], np.arange(solo)), (n, solo, ppb, pools, group)
        assert (fwd[solo:] >= solo).all()
    # one case by hand: 3 pools in blocks of 2, single ranks: ranks 0, 1, 2, 3 -> pools 0, 1, 0, 1 lanes 0, 0, 1, 1; the last block has one pool
    fwd = forward_map(3 * POOL, 0, 2, 3, 1)
    assert list(fwd[:4]) == [0, 64, 1, 65] and list(fwd[128:131]) == [128, 129, 130]
    # and whole pools: rank 64 starts pool 1
    assert list(forward_map(3 * POOL, 0, 2, 3, 64)[[0, 63, 64, 128]]) == [0, 63, 64, 128]


# ---- (a) a render's ranking

@gpu
@pytest.mark.parametrize("prec,scene_id,W,H,S,B,shard,solo", [
    (32, 1, 64, 64, 24, 40, None, True),            # the smallest frame that sorts: solo waves clamped to the grid, one super-tile
    (32, 3, 72, 60, 64, 20, None, False),           # 4320 pixels: a padded last pool, partial super-tiles
    (32, 3, 130, 70, 24, 8, None, False),           # neither dimension a multiple of 8; 3 x 2 super-tiles
    (32, 3, 128, 96, 24, 50, (1, 2, 4), True),      # strips plus solo waves
    (64, 3, 96, 48, 24, 8, None, False),
])
def test_ranking_of_a_render(rt, prec, scene_id, W, H, S, B, shard, solo):
    with rt.Renderer(0, prec, debug=True) as r:
        _setup(rt, r, prec, scene_id, rt.camera(prec, W, H, S, B), shard)
        r.render(0)
        assert r.stats()["phases"] == 2
        rows = r.local_rows
        info, _, _, _ = check_render_ranking(r, W, rows, _strip(rows, shard), solo)
        if (prec, W, H, S, B, shard) == (32, 64, 64, 24, 40, None):
            # the plan tests/native/launch_plan_main.cpp pins on the CPU is the plan the library made: these values hold on any device
            # with more than 64 resident workgroups, whatever its occupancy
            want = {"lane_cap": 16, "blocks": 64, "solo_slots": 128, "pools_per_block": 64, "deal_group": 1, "total_slots": 4224}
            assert {k: info[k] for k in want} == want, info
            assert r.stats()["prepass_samples"] == 2


# ---- (b) the coarse deal

# The size: plan_deal (csrc/library/launch_plan.h) deals whole pools (deal_group 64) from 2.5 pools per resident wave on.  A full fp32
# launch on the MI355X is 1280 workgroups (the hook's `blocks`: 256 CUs x 5, five dispatch-age classes of 1024 waves), 5120 resident waves,
# so the order needs 12800 pools = 819200 pixels; 1280 x 720 has 14400.  Of the 16:9 frames in steps of 16 columns, 1200 x 675 (12657 pools,
# 2.47 per wave) is the last with deal_group 1 and the frame below (12996 pools, 2.54 per wave) the first with 64: tests/native/launch_plan_main.cpp
# pins both plans on the CPU, and a scan with the hook on the device (960 x 540 ... 1408 x 792 at S 24, B 4) agreed; the render takes 1.4 ms.
COARSE_W, COARSE_H = 1216, 684


@gpu
def test_coarse_deal(rt):
    W, H = COARSE_W, COARSE_H
    with rt.Renderer(0, 32, debug=True) as r:
        _setup(rt, r, 32, 3, rt.camera(32, W, H, 24, 4))
        r.render(0)
        st = r.stats()
        assert st["phases"] == 2
        info, _, _, _ = r.debug_read_order()
        # the coverage this test exists for, asserted so that another part cannot lose it silently
        assert info["deal_group"] == 64 and info["blocks"] > st["num_cus"] and info["pools_per_block"] < info["blocks"] * 4, (info, st["num_cus"])
        check_render_ranking(r, W, H, H, False)


# ---- (c) a saturated ranking, from rtiow_accumulate

# The first chunk's length: the keys are quarter segments, so the clamp at 1023 sits at a neighbourhood mean of 256 segments per pixel.  From
# the CPU oracle's per-pixel segment counts of this very frame (scene 3, 96 x 72, 50 bounces: 2.50 segments per ray): 64 samples leave 5.9 %
# of the keys above 1023, 96 samples 31.4 % above and 68.5 % below, 128 samples 81.4 % / 18.5 %, 160 samples 87.2 % / 12.8 %.
SATURATED_CHUNK = 96


@gpu
def test_saturated_ranking_of_a_progressive_chunk(rt, oracle):
    W, H, B = 96, 72, 50
    cam = rt.camera(32, W, H, SATURATED_CHUNK, B)
    with rt.Renderer(0, 32, debug=True) as r:
        _setup(rt, r, 32, 3, cam, sched=rt.SCHED_SORTED)
        r.accumulate(SATURATED_CHUNK)
        costs = r.debug_read_chunk_costs()
        with pytest.raises(rt.RtiowError):          # the first chunk runs in tile order: no order yet on this handle
            r.debug_read_order()
        r.accumulate(2)
        info, order, slot_of, keys = r.debug_read_order()
    # the chunk's costs are the segments the oracle counts per pixel over the same samples
    _, _, seg = oracle.render(32, compact(oracle.build_scene(3, 32)), cam, 1227, segments=True)
    assert np.array_equal(costs, seg)
    assert info["kind"] == 2 and slot_of is None and info["solo_slots"] == 0, info
    want = smoothed_keys(costs, H)
    assert np.array_equal(keys.astype(np.int64), want)
    above, below = float((want > COST_BINS - 1).mean()), float((want < COST_BINS - 1).mean())
    print("keys above the clamp %.3f, below %.3f" % (above, below))
    assert above >= 0.1 and below >= 0.1, (above, below)
    check_ranking(info, order, None, keys, W, H)


# ---- (d) the carried order

@gpu
@pytest.mark.parametrize("prec,scene_id,W,H,S,B,shard", [
    (32, 1, 64, 64, 24, 40, None),
    (64, 3, 96, 48, 24, 8, None),
    (32, 3, 72, 60, 64, 20, None),
    (32, 3, 128, 96, 24, 50, (1, 2, 4)),
    (32, 2, 200, 100, 64, 50, None),
])
def test_reused_renders_leave_the_ranking_alone(rt, prec, scene_id, W, H, S, B, shard):
    with rt.Renderer(0, prec, debug=True) as r:
        _setup(rt, r, prec, scene_id, rt.camera(prec, W, H, S, B), shard)
        r.render(0)
        rows = r.local_rows
        first = check_render_ranking(r, W, rows, _strip(rows, shard))
        for _ in range(3):
            r.render(0)
            assert r.stats()["order_reused"] == 1
            info, order, slot_of, keys = r.debug_read_order()
            assert info == first[0]
            for got, want in zip((order, slot_of, keys), first[1:]):
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


@gpu
@pytest.mark.parametrize("name", ["camera_other_view", "camera_larger_then_smaller", "scene", "shard", "scene_source", "count_segments", "accumulate"])
def test_a_new_ranking_belongs_to_the_new_frame(rt, name):
    """Every case of test_what_drops_the_order that ranks again: the order read afterwards is a ranking of the frame rendered afterwards,
    by the smoothing of ITS prepass costs (check_render_ranking recomputes them from rtiow_debug_read_costs)."""
    change, after, keeps = _invalidation_cases(rt)[name]
    assert not keeps
    shard, cam_key = after.get("shard"), after.get("cam_key", BASE)
    W, H = (96, 64) if cam_key == "other_view" else cam_key[:2]
    with rt.Renderer(0, 32, debug=True) as r:
        _setup(rt, r, 32, 3, rt.camera(32, *BASE))
        r.render(0); r.render(0)
        assert r.stats()["order_reused"] == 1
        _, _, _, old_keys = r.debug_read_order()
        change(r)
        r.render(0)
        assert r.stats()["phases"] == 2 and r.stats()["order_reused"] == 0
        rows = r.local_rows
        _, _, _, keys = check_render_ranking(r, W, rows, _strip(rows, shard))
        if name in ("camera_other_view", "scene"):             # same geometry, other content: a leftover of the old frame would fit every shape
            assert not np.array_equal(keys, old_keys)


# ---- (e) a lost slot cannot hide

@gpu
@pytest.mark.parametrize("scene_id,W,H,S,B,solo", [
    (1, 64, 64, 24, 40, True),
    (3, 72, 60, 64, 20, False),                     # and a padded last pool
])
def test_a_reused_order_writes_every_slot(rt, oracle, scene_id, W, H, S, B, solo):
    """A reused render stores by slot and place_pixels_kernel gathers through slot_of: a slot that is never handed out would keep the
    bytes of the render before -- with the same seed the right ones.  NaN in the staging buffer first, then both the same and a new seed."""
    cam = rt.camera(32, W, H, S, B)
    with rt.Renderer(0, 32, debug=True) as r:
        with pytest.raises(rt.RtiowError):
            r.debug_poison_staged()                 # no staging buffer yet
        _setup(rt, r, 32, scene_id, cam)
        r.render(0)
        assert r.stats()["phases"] == 2 and (r.stats()["solo_waves"] > 0) == solo
        for seed in (1227, 7):
            r.debug_poison_staged()
            if seed != 1227:
                r.init_rng(seed)
            r.render(0)
            st = r.stats()
            assert st["order_reused"] == 1 and st["staged_stores"] == 1 and (st["solo_waves"] > 0) == solo, st
            got = r.read_framebuffer()
            assert not np.isnan(got).any(), seed
            _check_image(got, _reference(rt, oracle, 32, scene_id, cam, (W, H, S, B), seed=seed))


# ---- (f) the adaptive active list

def _check_active_list(r, before, after, returned, W, rows):
    info, order, slot_of, keys = r.debug_read_order()
    assert info["kind"] == 3 and slot_of is None and keys is None, info
    assert (info["W"], info["local_rows"]) == (W, rows)
    rose = (after > before).ravel()
    n = int(rose.sum())
    assert info["n_active"] == n == returned, (info, n, returned)
    if n == 0:
        assert info["total_slots"] == 0 and len(order) == 0
        return
    assert info["total_slots"] == (n + POOL - 1) // POOL * POOL == len(order)
    assert (order[n:] == -1).all()
    head = order[:n].astype(np.int64)
    assert head.min() >= 0
    jl, i = head >> 16, head & 0xffff
    assert jl.max() < rows and i.max() < W
    assert np.array_equal(np.sort(jl * W + i), np.flatnonzero(rose)), "the list is not the pixels whose count rose, each once"
    tile = (jl >> 3) * ((W + 7) >> 3) + (i >> 3)
    assert _runs(tile) == len(np.unique(tile)), "the active pixels of a tile are not adjacent in the list"


@gpu
@pytest.mark.parametrize("prec,W,H,shard", [(32, 64, 40, None), (32, 9, 9, None), (64, 64, 40, None), (32, 96, 72, (1, 3, 8))])
def test_adaptive_active_list(rt, prec, W, H, shard):
    with rt.Renderer(0, prec, debug=True) as r:
        _setup(rt, r, prec, 3, rt.camera(prec, W, H, 1, 25), shard)
        rows = r.local_rows
        c0, _ = r.adaptive_state()
        _, active = r.accumulate_adaptive(4, 0.0, min_samples=4)                     # everyone
        c1, e1 = r.adaptive_state()
        assert active == W * rows
        _check_active_list(r, c0, c1, active, W, rows)
        thr = float(np.median(e1))
        _, active = r.accumulate_adaptive(4, thr, min_samples=4)                     # a mix
        c2, _ = r.adaptive_state()
        assert 0 < active < W * rows
        assert np.array_equal(c2 > c1, e1.astype(np.float64) > thr)
        _check_active_list(r, c1, c2, active, W, rows)
        _, active = r.accumulate_adaptive(4, 0.0, max_samples=int(c2.min()) + 3)      # nobody may take four more
        c3, _ = r.adaptive_state()
        assert active == 0 and np.array_equal(c3, c2)
        _check_active_list(r, c2, c3, active, W, rows)


# ---- (g) exactly once, counted

# Counting runs use no solo waves (plan_sorted), so the solo kernel's hand-out is not counted here: that every one of ITS slots is
# written exactly where slot_of looks stays with test_a_reused_order_writes_every_slot above.
@gpu
@pytest.mark.parametrize("sched", [1, 2])          # RTIOW_SCHED_PERSISTENT, RTIOW_SCHED_SORTED
@pytest.mark.parametrize("prec,W,H,shard", [
    (32, 1, 1, None), (32, 1, 70, None), (32, 65, 3, None), (32, 33, 17, None), (32, 72, 60, None), (32, 64, 64, None),
    (32, 128, 96, (1, 2, 4)), (64, 72, 60, None),
])
def test_every_pixel_is_taken_exactly_once(rt, sched, prec, W, H, shard):
    with rt.Renderer(0, prec, debug=True) as r:
        _setup(rt, r, prec, 3, rt.camera(prec, W, H, 24, 8), shard, sched=sched)
        rows = r.local_rows
        r.render(0)
        st = r.stats()
        tl = r.debug_timeline(0)
        counted = r.stats()
        assert len(tl) == st["grid_blocks"] * 4, (len(tl), st["grid_blocks"])
        assert int(tl[:, 5].sum()) == W * rows, "the waves' pixel counts do not add up to the frame"
        assert (tl[:, 2] >= tl[:, 0]).all()
        assert counted["segments_prepass"] + counted["segments_main"] == r.count_segments(0)
        if sched == 2 and W * rows >= 4096:
            assert st["phases"] == 2 and counted["segments_prepass"] > 0
            info, order, slot_of, keys = r.debug_read_order()          # the counting run ranked too, without solo waves
            assert info["solo_slots"] == 0
            check_ranking(info, order, slot_of, keys, W, rows)
