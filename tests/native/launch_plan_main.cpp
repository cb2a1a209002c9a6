// Stand-alone check of the schedule's arithmetic (raytracingincuda_amd/csrc/library/launch_plan.h), built with
// -fsanitize=address,undefined by tests/test_launch_plan.py and run directly: plans pinned by hand, each rule one step either side of its
// edge, and the invariants of the plan over a sweep of frames and occupancies.  The device of the pinned plans: 256 CUs, five four-wave
// workgroups per CU (5120 resident waves), the solo kernel resident, the bounded twin keeping the occupancy.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "launch_plan.h"
#include "order_key.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// The three occupancy answers (workgroups per CU) and whether the launch has a bounded twin at all (fp32).
struct Device { int per_cu = 5, per_cu_twin = 5, per_cu_solo = 5; bool has_twin = true; };

static PlanFrame frame(int W, int rows, int S, int B) {
    PlanFrame f;
    f.W = W; f.local_rows = rows; f.S = S; f.B = B;
    f.rank = 0; f.nranks = 1; f.strip_rows = 8; f.precision = 32; f.schedule = PLAN_SCHED_SORTED; f.scene_source = 3;
    f.num_cus = 256; f.waves_per_simd = 0; f.counting = false; f.staged_stores = true;
    return f;
}

// The sequence of launch_render: every occupancy answer is given only where the launch asks for it.
static LaunchPlan render_plan(const PlanFrame& f, const Device& d = Device()) {
    LaunchPlan P{f};
    plan_size(P, plan_tile_slots(f.W, f.local_rows), d.per_cu);
    if (d.has_twin && P.want_twin) plan_twin(P, d.per_cu_twin);
    plan_sorted(P);
    if (P.ranked) {
        if (P.solo_waves > 0) plan_solo_resident(P, d.per_cu_solo);
        plan_sorted_finish(P);
    }
    return P;
}
// ... and of launch_accumulate.
static LaunchPlan chunk_plan(const PlanFrame& f, bool first, const Device& d = Device()) {
    LaunchPlan P{f};
    P.f.staged_stores = false;
    plan_size(P, plan_tile_slots(f.W, f.local_rows), d.per_cu);
    if (d.has_twin && P.want_twin) plan_twin(P, d.per_cu_twin);
    plan_chunk(P, first);
    return P;
}
static LaunchPlan sized(long long slots, int per_cu, int waves_per_simd = 0) {
    LaunchPlan P{frame(8, 8, 100, 50)};
    P.f.waves_per_simd = waves_per_simd;
    plan_size(P, slots, per_cu);
    return P;
}

struct Pinned { int W, H, S, B, lane_cap, blocks, twin, SA, total_pools, solo_waves, solo_lanes, pools_per_block, deal_group; unsigned counter_start; };

static void pinned_plans() {
    const Pinned rows[] = {
        {1920, 1080, 100, 50, 64, 1280, 1, 3, 32400, 0, 2, 1024, 64, 5120u * 64u},
        {1280, 720, 100, 50, 64, 1280, 0, 3, 14400, 256, 2, 1024, 64, 512u + 4864u * 64u},     // 14400 pools < 4 x 5120: no twin
        {1216, 684, 24, 4, 64, 1280, 0, 2, 12996, 0, 2, 1024, 64, 5120u * 64u},                // 2.538 pools per wave; B < 32: no solo waves
        {1200, 675, 24, 4, 64, 1280, 0, 2, 12657, 0, 2, 1024, 1, 5120u * 64u},                 // 2.472 pools per wave
        {64, 64, 24, 40, 16, 64, 0, 2, 64, 64, 2, 64, 1, 128u + 192u * 16u},                   // 128 solo waves clamped to the grid
    };
    for (const Pinned& r : rows) {
        const LaunchPlan P = render_plan(frame(r.W, r.H, r.S, r.B));
        CHECK(P.ranked && P.per_cu == 5);
        CHECK(P.lane_cap == r.lane_cap && P.blocks == r.blocks && (int)P.bounded_f32 == r.twin && P.want_twin == P.bounded_f32);
        CHECK(P.SA == r.SA && P.total_pools == r.total_pools && P.npix == r.W * r.H);
        CHECK(P.solo_waves == r.solo_waves && P.solo_lanes == r.solo_lanes && P.solo_slots == r.solo_waves * r.solo_lanes);
        CHECK(P.pools_per_block == r.pools_per_block && P.deal_group == r.deal_group && P.counter_start == r.counter_start);
        CHECK(P.total_slots == (long long)r.total_pools * PLAN_POOL + r.solo_waves * r.solo_lanes);
        CHECK(P.smooth_hw == 6 && P.window_strip == r.H && P.scatter_blocks == ((r.W + 63) / 64) * ((r.H + 63) / 64));
    }
    // the key of the headline launch is order_key_main.cpp's base key, word for word
    const LaunchPlan head = render_plan(frame(1920, 1080, 100, 50));
    const OrderKey base = {1920, 1080, 0, 1, 8, 100, 50, 32, 2, 3, 64, 1280, 32400, 0, 2, 1, 1};
    const OrderKey key = plan_order_key(head);
    CHECK(std::memcmp(&key, &base, sizeof base) == 0 && order_key_equal(key, base));
    // the records of the smallest frame that sorts: a render's, a chunk's, an adaptive list's (100 active pixels, none)
    const LaunchPlan small = render_plan(frame(64, 64, 24, 40));
    const OrderRecord rr = plan_ranking_record(small);
    const int want_rr[11] = {1, 4224, 128, 64, 64, 1, 16, 64, 0, 64, 64};
    static_assert(sizeof(OrderRecord) == sizeof want_rr, "OrderRecord: eleven ints");
    CHECK(std::memcmp(&rr, want_rr, sizeof want_rr) == 0);
    CHECK(!chunk_plan(frame(64, 64, 24, 40), true).ranked);
    const LaunchPlan chunk = chunk_plan(frame(64, 64, 24, 40), false);
    const OrderRecord cr = plan_ranking_record(chunk);
    const int want_cr[11] = {2, 4096, 0, 64, 64, 1, 16, 64, 0, 64, 64};
    CHECK(chunk.ranked && std::memcmp(&cr, want_cr, sizeof want_cr) == 0 && chunk.counter_start == 256u * 16u);
    LaunchPlan ad{frame(64, 64, 24, 40)};
    plan_adaptive(ad, 100);
    CHECK(ad.total_slots == 128 && ad.total_pools == 2);
    plan_size(ad, ad.total_slots, 5);
    const OrderRecord ar = plan_adaptive_record(ad);
    const int want_ar[11] = {3, 128, 0, 2, 0, 0, 16, 2, 100, 64, 64};
    CHECK(std::memcmp(&ar, want_ar, sizeof want_ar) == 0);
    LaunchPlan none{frame(64, 64, 24, 40)};
    plan_adaptive(none, 0);
    const OrderRecord nr = plan_adaptive_record(none);
    const int want_nr[11] = {3, 0, 0, 0, 0, 0, 0, 0, 0, 64, 64};
    CHECK(std::memcmp(&nr, want_nr, sizeof want_nr) == 0);
    // the stats: two phases, one launch in a carried order, no solo waves (their lanes read 0), nothing ranked
    auto stats_are = [](const PlanStats& s, int phases, int sa, int waves, int lanes, int staged) {
        return s.phases == phases && s.prepass_samples == sa && s.solo_waves == waves && s.solo_lanes == lanes && s.staged_stores == staged;
    };
    const LaunchPlan hd = render_plan(frame(1280, 720, 100, 50));
    CHECK(stats_are(plan_stats(hd), 2, 3, 256, 2, 1) && stats_are(plan_stats(hd, true), 1, 0, 256, 2, 1));
    CHECK(stats_are(plan_stats(head), 2, 3, 0, 0, 1) && stats_are(plan_stats(small), 2, 2, 64, 2, 1));
    CHECK(stats_are(plan_stats(chunk), 1, 0, 0, 0, 0) && stats_are(plan_stats(ad), 1, 0, 0, 0, 0));
    CHECK(stats_are(plan_stats(render_plan(frame(63, 65, 100, 50))), 1, 0, 0, 0, 0));
    PlanFrame direct = frame(1280, 720, 100, 50);
    direct.staged_stores = false;                                  // the direct-store A/B build
    CHECK(stats_are(plan_stats(render_plan(direct)), 2, 3, 256, 2, 0) && plan_ranking_record(render_plan(direct)).kind == 2);
}

static void edges() {
    // prepass length: S = 23 / 24 / 63 / 64
    CHECK(render_plan(frame(1280, 720, 23, 50)).SA == 0 && !render_plan(frame(1280, 720, 23, 50)).ranked);
    CHECK(render_plan(frame(1280, 720, 24, 50)).SA == 2 && render_plan(frame(1280, 720, 24, 50)).ranked);
    CHECK(render_plan(frame(1280, 720, 63, 50)).SA == 2 && render_plan(frame(1280, 720, 64, 50)).SA == 3);
    // bounce limit 31 / 32; a counting run
    CHECK(render_plan(frame(1280, 720, 100, 31)).solo_waves == 0 && render_plan(frame(1280, 720, 100, 32)).solo_waves == 256);
    PlanFrame counting = frame(1280, 720, 100, 50);
    counting.counting = true;
    CHECK(render_plan(counting).solo_waves == 0 && render_plan(counting).solo_slots == 0 && render_plan(counting).counter_start == 5120u * 64u);
    // fill level (pools per resident wave, 5120 of them) just under and at 1.2 and 4.0
    CHECK(render_plan(frame(6143, 64, 100, 50)).total_pools == 6143 && render_plan(frame(6143, 64, 100, 50)).solo_waves == 128);
    CHECK(render_plan(frame(6144, 64, 100, 50)).total_pools == 6144 && render_plan(frame(6144, 64, 100, 50)).solo_waves == 256);
    CHECK(render_plan(frame(20479, 64, 100, 50)).total_pools == 20479 && render_plan(frame(20479, 64, 100, 50)).solo_waves == 256);
    CHECK(render_plan(frame(20480, 64, 100, 50)).total_pools == 20480 && render_plan(frame(20480, 64, 100, 50)).solo_waves == 0);
    // deal group either side of 2.5 pools per wave: 12800 pools
    CHECK(render_plan(frame(12799, 64, 24, 4)).deal_group == 1 && render_plan(frame(12800, 64, 24, 4)).deal_group == 64);
    // the bounded twin: pools == 4 x waves and one fewer; a twin with lower occupancy is not taken; no twin (fp64)
    CHECK(sized(20480LL * 64, 5).want_twin && !sized(20479LL * 64, 5).want_twin && !sized(20480LL * 64 - 1, 5).want_twin);
    Device low; low.per_cu_twin = 4;
    CHECK(render_plan(frame(1920, 1080, 100, 50), low).want_twin && !render_plan(frame(1920, 1080, 100, 50), low).bounded_f32);
    Device fp64; fp64.has_twin = false;
    CHECK(!render_plan(frame(1920, 1080, 100, 50), fp64).bounded_f32);
    {   // ... compared with the occupancy AFTER the waves_per_simd cap: 2 workgroups per CU, a twin with 2 keeps it
        PlanFrame f = frame(1920, 1080, 100, 50);
        f.waves_per_simd = 2;
        Device d; d.per_cu_twin = 2;
        const LaunchPlan P = render_plan(f, d);
        CHECK(P.per_cu == 2 && P.blocks == 512 && P.bounded_f32);
        d.per_cu_twin = 1;
        CHECK(!render_plan(f, d).bounded_f32);
    }
    // waves_per_simd 0 (off) and 1..8: four-wave workgroups, so the cap is its value; an occupancy answer of 0 counts as 1
    CHECK(sized(32400LL * 64, 5, 0).per_cu == 5 && sized(32400LL * 64, 0).per_cu == 1 && sized(32400LL * 64, 0).blocks == 256);
    for (int w = 1; w <= 8; ++w) {
        const LaunchPlan P = sized(32400LL * 64, 5, w);
        CHECK(P.per_cu == (w < 5 ? w : 5) && P.blocks == 256LL * P.per_cu && P.lane_cap == 64);
    }
    // the lane cap halves while the shares do not reach every wave, and stops at 16
    CHECK(sized(5120LL * 64, 5).lane_cap == 64 && sized(5119LL * 64, 5).lane_cap == 32 && sized(2560LL * 64, 5).lane_cap == 32);
    CHECK(sized(2559LL * 64, 5).lane_cap == 16 && sized(64, 5).lane_cap == 16 && sized(64, 5).blocks == 1 && sized(65, 5).blocks == 2);
    // blocks: never more than lane_cap-pixel shares of the slots
    CHECK(sized(4096, 5).blocks == 64 && sized(1280LL * 64, 5).blocks == 1280 && sized(1279LL * 64, 5).blocks == 1279);
    // the sorted hand-out from 4096 pixels on, W below 65536, fewer than 32768 rows
    CHECK(!plan_sorted_handout(2, 4095, 1) && plan_sorted_handout(2, 4096, 1) && !plan_sorted_handout(2, 63, 65) && plan_sorted_handout(2, 64, 64));
    CHECK(!plan_sorted_handout(1, 64, 64) && !plan_sorted_handout(0, 1920, 1080));
    CHECK(plan_order_fits(65535, 32767) && !plan_order_fits(65536, 1) && !plan_order_fits(1, 32768));
    CHECK(render_plan(frame(65535, 1, 24, 4)).ranked && !render_plan(frame(65536, 1, 24, 4)).ranked);
    CHECK(render_plan(frame(1, 32767, 24, 4)).ranked && !render_plan(frame(1, 32768, 24, 4)).ranked);
    CHECK(chunk_plan(frame(65535, 1, 24, 4), false).ranked && !chunk_plan(frame(65536, 1, 24, 4), false).ranked);
    // the solo kernel not fully resident: no solo waves (4 x 256 < 1280 workgroups)
    Device tight; tight.per_cu_solo = 4;
    const LaunchPlan unres = render_plan(frame(1280, 720, 100, 50), tight);
    CHECK(unres.solo_waves == 0 && unres.solo_slots == 0 && unres.total_slots == 14400LL * 64 && unres.counter_start == 5120u * 64u);
    // the three clamps, on plans no built-in rule reaches: lanes to the lane cap, waves to the grid, slots to half the pixels
    {
        LaunchPlan P{frame(100, 1, 24, 40)};
        P.npix = 100; P.total_pools = 2; P.blocks = 1280; P.lane_cap = 64; P.solo_waves = 128; P.solo_lanes = 2;
        plan_sorted_finish(P);
        CHECK(P.solo_waves == 25 && P.solo_slots == 50 && P.total_slots == 178);
        P.npix = 101; P.solo_waves = 25; P.solo_lanes = 2;          // exactly half: kept
        plan_sorted_finish(P);
        CHECK(P.solo_waves == 25);
        P.npix = 1 << 20; P.blocks = 100; P.lane_cap = 16; P.solo_waves = 128; P.solo_lanes = 32;
        plan_sorted_finish(P);
        CHECK(P.solo_lanes == 16 && P.solo_waves == 100 && P.solo_slots == 1600);
    }
    // the smoothing window: one rank crosses its strips, a shard stays inside each
    PlanFrame shard = frame(1920, 540, 100, 50);
    CHECK(render_plan(shard).window_strip == 540);
    shard.nranks = 2; shard.rank = 1;
    CHECK(render_plan(shard).window_strip == 8 && render_plan(shard).smooth_hw == 6);
    CHECK(render_plan(shard).smooth_blocks == 30 * 34 && render_plan(shard).smooth_lds_bytes == (size_t)(64 + 12 + 64) * (16 + 12) * 4);
    // the workgroup shape
    int bx, by, wt;
    block_shape(0, true, bx, by, wt);  CHECK(bx == 16 && by == 16 && wt == 1);
    block_shape(8, true, bx, by, wt);  CHECK(bx == 8 && by == 8 && wt == 1);
    block_shape(24, true, bx, by, wt); CHECK(bx == 24 && by == 24 && wt == 0);
    block_shape(24, false, bx, by, wt); CHECK(bx == 16 && by == 16 && wt == 1);
    CHECK(plan_tiles(9, 9) == 4 && plan_tile_slots(1920, 1080) == 32400LL * 64 && plan_pools(4097) == 65 && plan_pools(0) == 0);
}

// The invariants of any plan the library can make.  The one intermediate that needs 64 bits is the tile-order slot count (65535 x 32767
// pixels: 2^31 slots; a frame of 2^31 - 1 pixels in one row: 2^34) and with it total_slots; everything per pixel fits an int.
static void check_invariants(const LaunchPlan& P, int per_cu) {
    const long long max_blocks = (long long)P.f.num_cus * per_cu;
    CHECK(P.lane_cap == 16 || P.lane_cap == 32 || P.lane_cap == 64);
    CHECK(P.blocks >= 1 && P.blocks <= max_blocks);
    if (!P.ranked) return;
    CHECK(P.pools_per_block >= 1 && P.pools_per_block <= P.total_pools);
    CHECK(P.solo_slots <= P.npix / 2 && P.solo_waves <= P.blocks && P.solo_lanes <= P.lane_cap);
    CHECK(P.total_slots == P.solo_slots + (long long)P.total_pools * PLAN_POOL);
    CHECK(P.deal_group == 1 || P.deal_group == 64);
    const long long first_pool_lanes = (P.blocks * PLAN_WAVES_PER_BLOCK - P.solo_waves) * P.lane_cap;
    if (first_pool_lanes <= (long long)P.total_pools * PLAN_POOL) CHECK((long long)P.counter_start <= P.total_slots);   // every resident wave can have a first pool
    CHECK((long long)P.counter_start == P.solo_slots + first_pool_lanes);
}

static void sweep() {
    const int Ws[] = {8, 9, 63, 64, 65, 100, 127, 128, 200, 320, 500, 640, 641, 1000, 1280, 1920, 2000, 3000, 3840, 4096};
    const int Hs[] = {8, 9, 63, 64, 65, 100, 192, 360, 500, 720, 1080, 1081, 2000, 2160, 2304};
    int ranked = 0;
    for (const int W : Ws) for (const int H : Hs) for (int per_cu = 1; per_cu <= 8; ++per_cu) {
        Device d; d.per_cu = d.per_cu_twin = d.per_cu_solo = per_cu;
        for (const int S : {24, 100}) {
            const LaunchPlan P = render_plan(frame(W, H, S, 50), d);
            check_invariants(P, per_cu);
            CHECK(P.ranked == ((long long)W * H >= 4096));
            ranked += P.ranked;
        }
        check_invariants(chunk_plan(frame(W, H, 24, 50), false, d), per_cu);
    }
    CHECK(ranked > 1000);
    // the largest frames: the largest whose order fits, and the API's limit of 2^31 - 1 pixels (not ranked: tile order)
    const LaunchPlan big = render_plan(frame(65535, 32767, 100, 50));
    check_invariants(big, 5);
    CHECK(big.ranked && big.npix == 2147385345 && big.total_pools == 33552897 && big.total_slots == 2147385408LL);
    CHECK(plan_tile_slots(65535, 32767) == (1LL << 31) && plan_ranking_record(big).total_slots == 2147385408);
    const LaunchPlan row = render_plan(frame(2147483647, 1, 100, 50));
    check_invariants(row, 5);
    CHECK(!row.ranked && row.blocks == 1280 && plan_tile_slots(2147483647, 1) == (1LL << 34));
    CHECK(chunk_plan(frame(2147483647, 1, 100, 50), false).total_pools == 33554432);
}

int main() {
    pinned_plans();
    edges();
    sweep();
    std::printf("%d launch-plan failure(s)\n", failures);
    return failures ? 1 : 0;
}
