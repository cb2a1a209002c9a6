// launch_plan.h -- the schedule's arithmetic: every host-side integer that decides how a frame is launched (workgroup shape, lane cap,
// workgroup count, fp32 bounded twin, prepass length, solo waves, pools, the deal, the smoothing window, the second hand-out counter's
// start), as pure functions of the frame, the shard, the device's CU count, three occupancy answers and the RTIOW_TUNE_* knobs.
// launch.h asks the plan, makes the occupancy queries the plan asks for, and enqueues; nothing here touches the device.
// Order of the calls for a sorted render: plan_size -> [plan_twin] -> plan_sorted -> [plan_solo_resident] -> plan_sorted_finish;
// for a ranked rtiow_accumulate chunk: plan_size -> [plan_twin] -> plan_chunk; for an adaptive chunk: plan_adaptive -> plan_size -> [plan_twin].
// Plain C++ (no HIP): also built on its own by tests/native/launch_plan_main.cpp.
#pragma once
#include <cstdint>
#include <cstdlib>

#include "order_key.h"

// The device's constants the plan counts in; launch.h asserts them equal to the device headers'.
constexpr int PLAN_POOL = 64;                            // pixels of a pool (device/render_kernels.h)
constexpr int PLAN_COST_BINS = 1024;                     // bins of the cost sort (device/cost_sort.h)
constexpr int PLAN_SMOOTH_TW = 64, PLAN_SMOOTH_TH = 16;  // cost_smooth_kernel's tile (device/cost_sort.h)
constexpr int PLAN_SCHED_SORTED = 2;                     // RTIOW_SCHED_SORTED (include/rtiow.h)
constexpr int PLAN_WAVES_PER_BLOCK = 4;                  // the persistent launches' 16 x 16 workgroup

// A schedule knob: its built-in value, or -- in the tuning build only (-DRTIOW_TUNING, scripts/tune_sweep.py,
// scripts/solo_sweep.py) -- the value of an environment variable.  The product build never reads the environment.
inline int tuned(const char* name, int builtin) {
#ifdef RTIOW_TUNING
    if (const char* e = std::getenv(name)) return std::atoi(e);
#endif
    (void)name;
    return builtin;
}

// T (the reference's --threads) shapes the workgroup of RTIOW_SCHED_STATIC, whose lanes ARE the
// pixels of a T x T block.  The dynamic schedules hand pixels to lanes themselves, so a workgroup
// there is just four waves whatever T says (measured with T as the workgroup size: 69 / 22.3 / 22.3 /
// 33 / 26 ms for T = 4 / 8 / 16 / 24 / 32 -- partly filled waves and uneven SIMD packing).
inline void block_shape(int T, bool static_schedule, int& bx, int& by, int& wave_tiles) {
    if (!static_schedule) T = 0;
    if (T == 0) { bx = 16; by = 16; wave_tiles = 1; }       // library tiling: 4 waves, each an 8x8 tile
    else if (T == 8) { bx = 8; by = 8; wave_tiles = 1; }    // == the reference's 8x8 block (one wave)
    else { bx = T; by = T; wave_tiles = 0; }                 // the reference's T x T row-major block
}

// 8 x 8 tiles of a local frame, and the hand-out slots of its tile order (a pool per tile).  64 bits: 65535 x 32767 pixels are 2^31 slots.
inline long long plan_tiles(int W, int rows) { return (((long long)W + 7) / 8) * (((long long)rows + 7) / 8); }
inline long long plan_tile_slots(int W, int rows) { return plan_tiles(W, rows) * PLAN_POOL; }
// Pools that hold n pixels of a ranked order or an active list.
inline int plan_pools(long long n) { return (int)((n + PLAN_POOL - 1) / PLAN_POOL); }
// Hand-out orders store a pixel as row << 16 | column.
inline bool plan_order_fits(int W, int rows) { return W < 65536 && rows < 32768; }
// The cost-sorted hand-out: the schedule asks for it, the frame is large enough to repay the ranking, and its order fits.
inline bool plan_sorted_handout(int schedule, int W, int rows) {
    return schedule == PLAN_SCHED_SORTED && (long long)W * rows >= 4096 && plan_order_fits(W, rows);
}

// What wrote h->order last, for the test hook rtiow_debug_read_order (include/rtiow_debug.h): a few ints on the host, in every build.
// kind: 0 nothing (or the buffers were reallocated since), 1 the ranking of a render (with slot_of), 2 the ranking of an rtiow_accumulate
// chunk, 3 the active list of an adaptive chunk.  The rest: the parameters the deal was made by and the launch it was made for; n_active and
// total_slots of an adaptive list.
struct OrderRecord {
    int kind = 0, total_slots = 0, solo_slots = 0, total_pools = 0, pools_per_block = 0, deal_group = 0, lane_cap = 0, blocks = 0, n_active = 0;
    int W = 0, local_rows = 0;                    // the local frame the order indexes
};

// What a launch is planned for.  At most 2^31 - 1 local pixels (the API's limit), so W * local_rows fits an int.
struct PlanFrame {
    int32_t W = 0, local_rows = 0;                // the local frame
    int32_t rank = 0, nranks = 1, strip_rows = 8; // the shard those rows belong to
    int32_t S = 0, B = 0;                         // samples and bounce limit
    int32_t precision = 32, schedule = 0, scene_source = 0;
    int num_cus = 1, waves_per_simd = 0;          // the device; the knob of rtiow_set_waves_per_simd (0: off)
    bool counting = false;                        // a counting run (rtiow_count_segments)
    bool staged_stores = false;                   // a sorted render stores finished pixels by slot and place_pixels_kernel writes the image
};

struct LaunchPlan {
    PlanFrame f;
    // plan_size, plan_twin
    int per_cu = 0;                               // resident workgroups per CU the launch is sized for
    int lane_cap = 64;                            // lanes of a wave that take pixels
    long long blocks = 0;                         // workgroups launched
    bool want_twin = false, bounded_f32 = false;  // fp32's bounded twin: asked for; taken
    // plan_sorted .. plan_sorted_finish, plan_chunk, plan_adaptive
    int SA = 0;                                   // prepass samples
    bool ranked = false;                          // the main launch takes its pixels from a ranking (the fields below)
    int npix = 0, total_pools = 0;
    int solo_waves = 0, solo_lanes = 0, solo_slots = 0;
    long long total_slots = 0;                    // solo_slots + total_pools x PLAN_POOL
    // plan_deal
    int pools_per_block = 0, deal_group = 0;
    int smooth_hw = 0, window_strip = 0;          // half-width of the cost smoothing (0: none) and the row strip its window stays inside
    int smooth_blocks = 0, hist_blocks = 0, scatter_blocks = 0;
    size_t smooth_lds_bytes = 0;
    unsigned counter_start = 0;                   // where the second hand-out counter starts
    int n_active = 0;                             // plan_adaptive
};

// Size a persistent launch over `slots` hand-out slots taken in tile order, given the kernel's occupancy (workgroups per CU): the lanes of
// a wave that take pixels, the workgroups to launch and whether fp32's bounded twin is asked for (then: its occupancy -> plan_twin).
inline void plan_size(LaunchPlan& P, long long slots, int per_cu) {
    const int waves_per_block = PLAN_WAVES_PER_BLOCK;
    if (per_cu < 1) per_cu = 1;
    if (P.f.waves_per_simd > 0) {                      // knob: fewer resident waves, more pixels per lane
        const int cap = (P.f.waves_per_simd * 4 + waves_per_block - 1) / waves_per_block;
        if (cap < per_cu) per_cu = cap;
    }
    // Underfilled launch (fewer 64-pixel pools than resident waves: small frames): let only the first
    // `lane_cap` lanes of every wave take pixels.  More waves are busy, each permanently in the
    // cooperative mode, where its idle lanes split the sphere loops of the live ones: a trip gets
    // shorter, and with so little work the frame is as long as its longest chain of trips.
    // Measured (profiles/archive/r01_lane_cap_sweep.txt): scene 1 320x192x10 2.27 -> 1.06 ms, 640x384x100
    // 19.4 -> 17.0 ms; frames with at least one pool per wave are unchanged (cap 64).
    int lane_cap = 64;
    const long long pools = slots / PLAN_POOL, waves = (long long)P.f.num_cus * per_cu * waves_per_block;
    while (lane_cap > 16 && pools * (64 / lane_cap) < waves) lane_cap >>= 1;  // the largest share that keeps every wave busy; not below 16 (with the grid walk 8-lane waves lose: scene 1 320x192x100 6.85 vs 5.96 ms, profiles/archive/r02_lane_cap_sweep.jsonl)
    lane_cap = tuned("RTIOW_TUNE_LANE_CAP", lane_cap);
    // fp32: the bounded rejection loop where throughput binds -- at least four pools per resident wave (1080p: 6.3; 1280 x 720, shards and small
    // frames end with one chain's latency and keep the blocking loop) -- if that kernel keeps the occupancy this launch was sized for
    P.want_twin = tuned("RTIOW_TUNE_RUV_BOUNDED", pools >= 4 * waves ? 1 : 0) != 0;
    P.bounded_f32 = false;
    P.blocks = (long long)P.f.num_cus * per_cu;
    const long long per_block = (long long)waves_per_block * lane_cap;
    const long long useful = (slots + per_block - 1) / per_block;
    if (P.blocks > useful) P.blocks = useful;               // never more waves than lane_cap-pixel shares of the pools
    P.per_cu = per_cu;
    P.lane_cap = lane_cap;
}
inline void plan_twin(LaunchPlan& P, int per_cu_twin) { P.bounded_f32 = per_cu_twin >= P.per_cu; }

// The deal of a ranking into P.total_pools pools behind P.solo_slots solo slots, for the P.blocks workgroups of plan_size: blocks of the
// order are one "age class" of resident waves wide (ColdParams::first_pools); the smoothing of the cost; the launches of cost_sort.h;
// and the second counter's start: the first solo_slots slots go to the solo waves, every other resident wave starts with a pool of its
// own, the counter hands out the rest.
inline void plan_deal(LaunchPlan& P) {
    const PlanFrame& f = P.f;
    P.total_slots = (long long)P.total_pools * PLAN_POOL + P.solo_slots;
    const int resident_waves = (int)P.blocks * PLAN_WAVES_PER_BLOCK;
    const int age_classes = (int)((P.blocks + f.num_cus - 1) / f.num_cus);
    P.pools_per_block = (resident_waves + age_classes - 1) / age_classes;
    if (P.pools_per_block > P.total_pools) P.pools_per_block = P.total_pools;
    // Deal granularity: `deal_group` consecutive ranks (= neighbouring pixels of equal cost) stay
    // in one pool, the groups go round-robin over the block's pools.  Coherent groups mean fewer
    // distinct spheres pass the screen per wave (8.9 exact blocks per wave-iteration with single
    // ranks vs 3.6 in tile order); mixed costs in a pool let a heavy pixel finish in the fast
    // cooperative mode, which is what small shards need.  Measured (profiles/archive/r01_deal_group_sweep.txt):
    // full frame 24.1 -> 22.5 ms with 16-32, half frame 14.7 -> 14.0 with 8, quarter and eighth
    // frames are fastest with 1.
    const double pools_per_wave = (double)P.total_pools / (double)resident_waves;
    // With the grid walk (a lane's cost follows ITS ray) coherence pays more: whole pools of 64 neighbouring
    // ranks, 15.3 -> 14.7 ms on the full frame (profiles/archive/r02_tune_sweep.jsonl) and, once the ranks come from
    // the smoothed cost, on every frame with at least 2.5 pools per wave (1280x720: 9.3 ms with groups of 1,
    // 11.4 with 8, 8.7 with 64; profiles/archive/r02_cost_smoothing_sweep.jsonl); smaller shards keep single ranks.
    P.deal_group = tuned("RTIOW_TUNE_DEAL", pools_per_wave >= 2.5 ? 64 : 1);
    P.smooth_hw = tuned("RTIOW_TUNE_SMOOTH", 6);     // 13 x 13 window: profiles/archive/r02_cost_smoothing_sweep.jsonl
    if (P.smooth_hw > 24) P.smooth_hw = 24;           // 2 x (tile + halo) words of LDS: 37 KB at 24
    if (P.smooth_hw < 0) P.smooth_hw = 0;
    const int whole_frame = f.local_rows > 0 ? f.local_rows : 1;
    // one rank: its strips are adjacent in the image, the window may cross them (it did not before: 13 x <= 8 rows)
    P.window_strip = f.nranks == 1 ? whole_frame : f.strip_rows;
    if (const int ws = tuned("RTIOW_TUNE_SMOOTH_STRIP", -1); ws >= 0) P.window_strip = ws > 0 ? ws : whole_frame;
    P.smooth_blocks = ((f.W + PLAN_SMOOTH_TW - 1) / PLAN_SMOOTH_TW) * ((f.local_rows + PLAN_SMOOTH_TH - 1) / PLAN_SMOOTH_TH);
    P.smooth_lds_bytes = ((size_t)(PLAN_SMOOTH_TW + 2 * P.smooth_hw) + PLAN_SMOOTH_TW) * (size_t)(PLAN_SMOOTH_TH + 2 * P.smooth_hw) * sizeof(uint32_t);
    const int sort_blocks = (P.npix + 255) / 256;
    P.hist_blocks = sort_blocks < 1024 ? sort_blocks : 1024;
    P.scatter_blocks = ((f.W + 63) / 64) * ((f.local_rows + 63) / 64);   // one per 64 x 64 super-tile
    P.counter_start = (unsigned)P.solo_slots + (unsigned)(resident_waves - P.solo_waves) * (unsigned)P.lane_cap;
}

// The sorted render's choices, after plan_size over the frame's tile slots: the prepass length, whether the frame is ranked at all, and
// the solo waves the rule asks for.  solo_waves > 0: the solo kernel's occupancy -> plan_solo_resident.  Then plan_sorted_finish.
inline void plan_sorted(LaunchPlan& P) {
    const PlanFrame& f = P.f;
    P.npix = f.W * f.local_rows;
    // prepass length: enough samples to rank the pixels, a small share of the frame
    P.SA = tuned("RTIOW_TUNE_SA", f.S >= 64 ? 3 : (f.S >= 24 ? 2 : 0));       // measured on the headline config: 1 -> 25.5 ms, 2 -> 22.5, 3 -> 22.1, 4 -> 22.4, 8 -> 23.1
    P.ranked = P.SA > 0 && plan_sorted_handout(f.schedule, f.W, f.local_rows);
    if (!P.ranked) return;
    P.total_pools = plan_pools(P.npix);
    // Solo waves (ColdParams::solo_*, render_solo_kernel).  A shard or small frame ends with its longest sample
    // chains (one pixel = one sequential chain), and a chain advances at the pace of its wave: 2452 segments at
    // ~3 us per trip among 63 other pixels.  Two heavy pixels alone in a wave share every sphere loop with the
    // idle lanes and skip the divergent work of wave-mates.  Which pixels: the top of the cost ranking.  How
    // many waves: more than ~5 % of the resident waves cost more throughput than the chains gain; measured per
    // fill level (profiles/archive/r02_handout_study/): 1/8 frame 6.96 -> 5.65 ms with 128 waves (5.78 with 256),
    // 1/4 frame 7.85 -> 6.61 with 256 (7.03 with 128), 1/2 frame 8.43 -> 8.21, 1280x720 8.82 -> 8.34; the full
    // frame (6.3 pools per wave) loses 1-2 % and keeps the plain kernel.  Outlier chains need a bounce limit
    // that lets rare long paths exist: at 10 bounces the solo waves cost 4-11 % on both scenes, at 25 scene 3
    // gains 9 % and scene 1 -- the reference's own benchmark grid -- loses 2-5 %, from 50 on both gain
    // (sweep6_bounce_limit.txt): the rule asks for more than 32.
    const double fill_level = (double)P.total_pools / (double)(P.blocks * PLAN_WAVES_PER_BLOCK);
    P.solo_waves = tuned("RTIOW_TUNE_SOLO_WAVES", (f.counting || f.B < 32) ? 0 : (fill_level < 1.2 ? 128 : (fill_level < 4.0 ? 256 : 0)));
    P.solo_lanes = tuned("RTIOW_TUNE_SOLO_LANES", 2);
    if (P.solo_lanes < 1) P.solo_lanes = 1;
}
// The solo kernel's workgroups must all be resident, as the first pools assume.
inline void plan_solo_resident(LaunchPlan& P, int per_cu_solo) { if ((long long)per_cu_solo * P.f.num_cus < P.blocks) P.solo_waves = 0; }
inline void plan_sorted_finish(LaunchPlan& P) {
    if (P.solo_lanes > P.lane_cap) P.solo_lanes = P.lane_cap;
    if (P.solo_waves > (int)P.blocks) P.solo_waves = (int)P.blocks;
    if ((long long)P.solo_waves * P.solo_lanes > P.npix / 2) P.solo_waves = P.npix / 2 / P.solo_lanes;
    P.solo_slots = P.solo_waves * P.solo_lanes;
    plan_deal(P);
}

// A chunk of rtiow_accumulate, after plan_size over the frame's tile slots: every chunk but the first ranks the pixels by the previous
// chunk's cost (same limits as the render).  No prepass, no solo waves, no staged stores.
inline void plan_chunk(LaunchPlan& P, bool first_chunk) {
    P.npix = P.f.W * P.f.local_rows;
    P.total_pools = plan_pools(P.npix);
    P.ranked = !first_chunk && plan_sorted_handout(P.f.schedule, P.f.W, P.f.local_rows);
    if (P.ranked) plan_deal(P);
}

// An adaptive chunk's active list of n_active pixels: whole pools of slots (the tail of the last pool holds no pixel).  n_active > 0:
// plan_size over total_slots follows.
inline void plan_adaptive(LaunchPlan& P, unsigned n_active) {
    P.n_active = (int)n_active;
    P.total_pools = plan_pools((long long)n_active);
    P.total_slots = (long long)P.total_pools * PLAN_POOL;
    P.lane_cap = 0;                                 // no render launch unless plan_size follows
}

// The structural key of the order a sorted render (plan_sorted_finish) leaves or reuses: order_key.h.
inline OrderKey plan_order_key(const LaunchPlan& P) {
    const PlanFrame& f = P.f;
    return {f.W, f.local_rows, f.rank, f.nranks, f.strip_rows, f.S, f.B, f.precision, f.schedule, f.scene_source,
            P.lane_cap, (int)P.blocks, P.total_pools, P.solo_waves, P.solo_lanes, P.bounded_f32 ? 1 : 0, f.staged_stores ? 1 : 0};
}
// OrderRecord of a ranking (plan_deal): a render's comes with slot_of (staged stores), a chunk's -- and a direct-store render's -- without.
inline OrderRecord plan_ranking_record(const LaunchPlan& P) {
    return {P.f.staged_stores ? 1 : 2, (int)P.total_slots, P.solo_slots, P.total_pools, P.pools_per_block, P.deal_group, P.lane_cap, (int)P.blocks, 0, P.f.W, P.f.local_rows};
}
// ... and of an adaptive list (plan_adaptive, then plan_size when any pixel is active).
inline OrderRecord plan_adaptive_record(const LaunchPlan& P) {
    return {3, (int)P.total_slots, 0, P.total_pools, 0, 0, P.lane_cap, (int)P.blocks, P.n_active, P.f.W, P.f.local_rows};
}

// The fields of rtiow_stats that describe the plan.  reused: the render ran in a carried order (one launch, no prepass).
struct PlanStats { int phases, prepass_samples, solo_waves, solo_lanes, staged_stores; };
inline PlanStats plan_stats(const LaunchPlan& P, bool reused = false) {
    const int phases = P.ranked && P.SA > 0 && !reused ? 2 : 1;
    return {phases, phases == 2 ? P.SA : 0, P.solo_waves, P.solo_waves > 0 ? P.solo_lanes : 0, P.ranked && P.f.staged_stores ? 1 : 0};
}
