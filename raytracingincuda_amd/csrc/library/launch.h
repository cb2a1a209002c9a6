// launch.h -- the render-family launches on one shared setup (layout_lds, persistent_setup, size_persistent, record_launch): launch_render
// (static / persistent / sorted with prepass + cost sort + solo waves, or in the order an earlier render left: order_key.h), launch_accumulate (one chunk of progressive rendering),
// launch_adaptive (one adaptive chunk); launch_guides / launch_linear / launch_denoise: the denoised previews; launch_variance_plane /
// launch_denoise_variance: the variance-guided filter; launch_history: the temporal reprojection
// Host side of librtiow_hip.so; part of the single translation unit rtiow_hip.hip (internal linkage).
#pragma once
#include "scene_tables.h"
#include "../device/render_kernels.h"
#include "../device/adaptive.h"
#include "../device/cost_sort.h"
#include "../device/denoise.h"
#include "../device/denoise_variance.h"
#include "../device/history.h"

namespace {

// A schedule knob: its built-in value, or -- in the tuning build only (-DRTIOW_TUNING, scripts/tune_sweep.py,
// scripts/solo_sweep.py) -- the value of an environment variable.  The product build never reads the environment.
inline int tuned(const char* name, int builtin) {
#ifdef RTIOW_TUNING
    if (const char* e = std::getenv(name)) return std::atoi(e);
#endif
    (void)name;
    return builtin;
}

template <class T> using RenderFn = void (*)(const RenderParams<T>);

// f(std::integral_constant<int, SRC>()) for the kernels' scene-source template argument: RTIOW_SCENE_LDS when the launch stages the
// scene in LDS (layout_lds), RTIOW_SCENE_SCALAR otherwise.
template <class F>
auto by_source(bool lds_source, F f) {
    if (lds_source) return f(std::integral_constant<int, RTIOW_SCENE_LDS>());
    return f(std::integral_constant<int, RTIOW_SCENE_SCALAR>());
}

// A kernel launched with more than 64 KB of dynamic LDS must be allowed it first (also before occupancy queries).
template <class K>
hipError_t allow_lds(K k, size_t lds) {
    return lds > 64 * 1024 ? hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}

// Hand-out orders store a pixel as row << 16 | column.
inline bool order_fits(const rtiow_handle_s* h) { return img_w(h) < 65536 && h->local_rows < 32768; }
// The cost-sorted hand-out: the schedule asks for it, the frame is large enough to repay the ranking, and its order fits.
inline bool sorted_handout(const rtiow_handle_s* h) { return h->schedule == RTIOW_SCHED_SORTED && local_pixels(h) >= 4096 && order_fits(h); }

// A render-family launch: parameters and LDS layout (layout_lds), kernel and sizing (persistent_setup, size_persistent).
template <class T>
struct Launch {
    RenderParams<T> p;
    size_t lds = 0;                    // dynamic LDS bytes per workgroup
    bool lds_source = false;           // the kernel reads the scene from LDS
    int effective_source = 0;          // rtiow_stats::scene_source
    RenderFn<T> k = nullptr;
    RenderFn<T> kb = nullptr;          // fp32: k with the bounded rejection loop (render_kernels.h, BOUND_F32); fp64 bounds it in every kernel
    hipFuncAttributes fa{};            // k's
    long long blocks = 0;              // workgroups launched
    bool bounded_f32 = false;          // k is kb
};

// LDS layout of a render launch (scene source, screening table and grid -- built at the first launch after rtiow_set_scene --, shade
// records, drain scratch) into L.p, L.lds, L.lds_source and L.effective_source.  record_stats: the grid_* fields of rtiow_stats describe it.
template <class T>
int layout_lds(rtiow_handle_s* h, Launch<T>& L, int threads, bool persistent, bool record_stats) {
    RenderParams<T>& p = L.p;
    size_t& lds = L.lds;
    bool& lds_source = L.lds_source;
    int& effective_source = L.effective_source;
    // A scene whose tables do not fit the CU's LDS next to the drain scratch (several thousand
    // spheres) is read through the scalar cache instead of failing: same image, exact loop.
    size_t coop_scratch = persistent ? (size_t)((threads + 63) / 64) * COOP_SLOTS * sizeof(CoopSlot<T>) : 0;
    lds_source = h->scene_source != RTIOW_SCENE_SCALAR;
    effective_source = h->scene_source;
    const bool screened = h->scene_source == RTIOW_SCENE_LDS || h->scene_source == RTIOW_SCENE_GRID;
    if (lds_source && (sizeof(T) + (screened ? sizeof(float) : 0)) * 4 * (size_t)h->n_padded + coop_scratch > 160 * 1024) {
        lds_source = false;
        effective_source = RTIOW_SCENE_SCALAR;
    }
    if (lds_source && screened && h->screen_dirty) {
        const auto t0 = std::chrono::steady_clock::now();
        int rc = build_screen_table<T>(h);
        if (rc) return rc;
        if ((rc = build_grid_tables<T>(h))) return rc;
        h->stats.scene_prepare_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    fill_screen_params<T>(p, h);
    if (!lds_source) p.use_screen = 0;
    lds = lds_source ? sizeof(T) * 4 * (size_t)h->n_padded : 0;
    p.screen_offset = (int)lds;
    if (p.use_screen) lds += sizeof(float) * 4 * (size_t)h->n_padded;
    // shade records ride along in LDS while a workgroup's share stays within 1/5 of the CU's LDS
    const size_t coop_bytes = coop_scratch;
    const size_t shade_bytes = (sizeof(T) * 12 * (size_t)h->n + 15) / 16 * 16;
    p.shade_offset = (int)lds;
    // ... and a wave's share stays under ~6.5 KB, so that LDS never caps occupancy below 6 waves/SIMD
    const size_t waves_in_block = (size_t)((threads + 63) / 64);
    p.shade_in_lds = (lds + shade_bytes + coop_bytes <= 32 * 1024 && (lds + shade_bytes + coop_bytes) / waves_in_block <= 6656) ? 1 : 0;
    if (p.shade_in_lds) lds += shade_bytes;
    p.coop_offset = (int)lds;                                // a multiple of 16
    lds += coop_bytes;
    // the grid blob (cells | fp32 AoS table | direct table | direct ids) goes last
    p.grid = GridParams{};
    p.use_grid = 0;
    if (record_stats) { h->stats.grid_nx = h->stats.grid_nz = h->stats.grid_registered = h->stats.grid_direct = 0; h->stats.grid_cell = 0; }
    if (lds_source && h->scene_source == RTIOW_SCENE_GRID && p.use_screen && h->grid.use_grid && lds + (size_t)h->grid.blob_bytes <= 160 * 1024) {
        p.grid = h->grid;
        p.grid.cells_offset = (int)lds;
        p.grid.aos_offset = p.grid.cells_offset + h->grid_cells_bytes;
        p.grid.direct_offset = p.grid.aos_offset + h->grid_aos_bytes;
        p.grid.direct_ids_offset = p.grid.direct_offset + h->grid_direct_bytes;
        lds += (size_t)h->grid.blob_bytes;
        p.use_grid = 1;
        if (record_stats) { h->stats.grid_nx = h->grid.nx; h->stats.grid_nz = h->grid.nz; h->stats.grid_registered = h->grid_registered; h->stats.grid_direct = h->grid_direct; h->stats.grid_cell = h->grid.cell; }
    } else if (effective_source == RTIOW_SCENE_GRID) effective_source = RTIOW_SCENE_LDS;   // no grid for this scene: the screened loop
    if (lds > 160 * 1024) return fail_arg(h, RTIOW_E_BADARG, "scene too large for LDS staging; use RTIOW_SCENE_SCALAR");
    return 0;
}

// The setup the persistent launches share (launch_render's dynamic schedules, launch_accumulate, launch_adaptive): four-wave 16 x 16
// workgroups, the main launch's clock stamps (stamp_clock), the LDS layout with drain scratch, the kernel pick(src, bounded) -- bounded:
// std::true_type for fp32's bounded twin only -- allowed its LDS, and the two hand-out counters.
template <class T, class Pick>
int persistent_setup(rtiow_handle_s* h, Launch<T>& L, bool stamp_clock, bool record_stats, Pick pick) {
    L.p.cold.bx = 16; L.p.cold.by = 16; L.p.cold.wave_tiles = 1;
    L.p.cold.clock_stamps = stamp_clock && h->clock_stamps_dev ? h->clock_stamps_dev + 4 : nullptr;
    if (int rc = layout_lds<T>(h, L, 256, true, record_stats)) return rc;
    L.k = by_source(L.lds_source, [&](auto src) { return pick(src, std::false_type()); });
    if constexpr (sizeof(T) == 4) L.kb = by_source(L.lds_source, [&](auto src) { return pick(src, std::true_type()); });
    HIP_TRY(h, allow_lds(L.k, L.lds));
    HIP_TRY(h, h->work_counter.ensure(2 * sizeof(unsigned int)));
    return 0;
}

// Size L's persistent launch over `slots` hand-out slots, taken from h->work_counter in tile order: the lanes of a wave that take pixels
// (p.lane_cap), the workgroups to launch (blocks) and whether the fp32 bounded twin kb replaces k (bounded_f32); then k's attributes.
template <class T>
int size_persistent(rtiow_handle_s* h, Launch<T>& L, long long slots) {
    const int threads = L.p.cold.bx * L.p.cold.by, waves_per_block = (threads + 63) / 64;
    int per_cu = 0;
    HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)L.k, threads, L.lds));
    if (per_cu < 1) per_cu = 1;
    if (h->waves_per_simd > 0) {                       // knob: fewer resident waves, more pixels per lane
        const int cap = (h->waves_per_simd * 4 + waves_per_block - 1) / waves_per_block;
        if (cap < per_cu) per_cu = cap;
    }
    // Underfilled launch (fewer 64-pixel pools than resident waves: small frames): let only the first
    // `lane_cap` lanes of every wave take pixels.  More waves are busy, each permanently in the
    // cooperative mode, where its idle lanes split the sphere loops of the live ones: a trip gets
    // shorter, and with so little work the frame is as long as its longest chain of trips.
    // Measured (profiles/archive/r01_lane_cap_sweep.txt): scene 1 320x192x10 2.27 -> 1.06 ms, 640x384x100
    // 19.4 -> 17.0 ms; frames with at least one pool per wave are unchanged (cap 64).
    int lane_cap = 64;
    const long long pools = slots / POOL, waves = (long long)h->num_cus * per_cu * waves_per_block;
    while (lane_cap > 16 && pools * (64 / lane_cap) < waves) lane_cap >>= 1;  // the largest share that keeps every wave busy; not below 16 (with the grid walk 8-lane waves lose: scene 1 320x192x100 6.85 vs 5.96 ms, profiles/archive/r02_lane_cap_sweep.jsonl)
    lane_cap = tuned("RTIOW_TUNE_LANE_CAP", lane_cap);
    // fp32: the bounded rejection loop where throughput binds -- at least four pools per resident wave (1080p: 6.3; 1280 x 720, shards and small
    // frames end with one chain's latency and keep the blocking loop) -- if that kernel keeps the occupancy this launch was sized for
    L.bounded_f32 = false;
    if (L.kb) {
#ifdef RTIOW_TUNING
        const bool want = tuned("RTIOW_TUNE_RUV_BOUNDED", pools >= 4 * waves ? 1 : 0) != 0;
#else
        const bool want = pools >= 4 * waves;
#endif
        if (want) {
            HIP_TRY(h, allow_lds(L.kb, L.lds));
            int per_cu_b = 0;
            HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_b, (const void*)L.kb, threads, L.lds));
            if (per_cu_b >= per_cu) { L.k = L.kb; L.bounded_f32 = true; }
        }
    }
    L.blocks = (long long)h->num_cus * per_cu;
    const long long per_block = (long long)waves_per_block * lane_cap;
    const long long useful = (slots + per_block - 1) / per_block;
    if (L.blocks > useful) L.blocks = useful;               // never more waves than lane_cap-pixel shares of the pools
    L.p.lane_cap = lane_cap;
    L.p.cold.total_slots = (int)slots;
    L.p.cold.work_counter = h->work_counter;
    HIP_TRY(h, hipFuncGetAttributes(&L.fa, (const void*)L.k));
    return 0;
}

// The hand-out order of a cost-sorted launch: the pixels ranked heavy-first by `cost` (segments per local pixel, smoothed over a window)
// and dealt into balanced pools, written to h->order (slot -> row << 16 | column, -1 for padding; the first solo_slots slots are the top
// ranks) and, when slot_of is given, its inverse.  Blocks of the order are one "age class" of resident waves wide (see first_pools).
// Needs h->order, h->cost_rank and h->sort_scratch sized for the frame.
inline int rank_pixels(rtiow_handle_s* h, const uint32_t* cost, long long blocks, int waves_per_block, int lane_cap, int total_pools, int solo_slots, int* slot_of) {
    const int W = img_w(h), npix = W * h->local_rows;
    unsigned* hist = h->sort_scratch; unsigned* start = hist + COST_BINS; unsigned* fill = start + COST_BINS;
    HIP_TRY(h, hipMemsetAsync(hist, 0, COST_BINS * sizeof(unsigned), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->order, 0xff, ((size_t)total_pools * POOL + (size_t)solo_slots) * sizeof(int), h->stream));
    const int sort_blocks = (npix + 255) / 256;
    const uint32_t* rank_by = cost;
    int smooth_hw = 6;                          // 13 x 13 window: profiles/archive/r02_cost_smoothing_sweep.jsonl
    smooth_hw = tuned("RTIOW_TUNE_SMOOTH", smooth_hw);
    if (smooth_hw > 0) {
        if (smooth_hw > 24) smooth_hw = 24;      // 2 x (tile + halo) words of LDS: 37 KB at 24
        const int smooth_blocks = ((W + SMOOTH_TW - 1) / SMOOTH_TW) * ((h->local_rows + SMOOTH_TH - 1) / SMOOTH_TH);
        const size_t smooth_lds_bytes = ((size_t)(SMOOTH_TW + 2 * smooth_hw) + SMOOTH_TW) * (size_t)(SMOOTH_TH + 2 * smooth_hw) * sizeof(uint32_t);
        // one rank: its strips are adjacent in the image, the window may cross them (it did not before: 13 x <= 8 rows)
        int window_strip = h->nranks == 1 ? (h->local_rows > 0 ? h->local_rows : 1) : h->strip_rows;
        if (const int ws = tuned("RTIOW_TUNE_SMOOTH_STRIP", -1); ws >= 0) window_strip = ws > 0 ? ws : (h->local_rows > 0 ? h->local_rows : 1);
        hipLaunchKernelGGL(cost_smooth_kernel, dim3(smooth_blocks), dim3(256), smooth_lds_bytes, h->stream, cost, h->cost_rank, W, h->local_rows, window_strip, smooth_hw, hist);
        rank_by = h->cost_rank;
    } else {
        hipLaunchKernelGGL(cost_hist_kernel, dim3(sort_blocks < 1024 ? sort_blocks : 1024), dim3(256), 0, h->stream, rank_by, npix, hist);
    }
    hipLaunchKernelGGL(cost_scan_kernel, dim3(1), dim3(COST_BINS), 0, h->stream, hist, start, fill);
    const int resident_waves = (int)blocks * waves_per_block;
    const int age_classes = (int)((blocks + h->num_cus - 1) / h->num_cus);
    int pools_per_block = (resident_waves + age_classes - 1) / age_classes;
    if (pools_per_block > total_pools) pools_per_block = total_pools;
    // Deal granularity: `deal_group` consecutive ranks (= neighbouring pixels of equal cost) stay
    // in one pool, the groups go round-robin over the block's pools.  Coherent groups mean fewer
    // distinct spheres pass the screen per wave (8.9 exact blocks per wave-iteration with single
    // ranks vs 3.6 in tile order); mixed costs in a pool let a heavy pixel finish in the fast
    // cooperative mode, which is what small shards need.  Measured (profiles/archive/r01_deal_group_sweep.txt):
    // full frame 24.1 -> 22.5 ms with 16-32, half frame 14.7 -> 14.0 with 8, quarter and eighth
    // frames are fastest with 1.
    const double pools_per_wave = (double)total_pools / (double)resident_waves;
    // With the grid walk (a lane's cost follows ITS ray) coherence pays more: whole pools of 64 neighbouring
    // ranks, 15.3 -> 14.7 ms on the full frame (profiles/archive/r02_tune_sweep.jsonl) and, once the ranks come from
    // the smoothed cost, on every frame with at least 2.5 pools per wave (1280x720: 9.3 ms with groups of 1,
    // 11.4 with 8, 8.7 with 64; profiles/archive/r02_cost_smoothing_sweep.jsonl); smaller shards keep single ranks.
    int deal_group = pools_per_wave >= 2.5 ? 64 : 1;
    deal_group = tuned("RTIOW_TUNE_DEAL", deal_group);
    const int scatter_blocks = ((W + 63) / 64) * ((h->local_rows + 63) / 64);   // one per 64 x 64 super-tile
    hipLaunchKernelGGL(cost_scatter_kernel, dim3(scatter_blocks), dim3(1024), 0, h->stream, rank_by, W, h->local_rows, start, fill, h->order,
                       pools_per_block, total_pools, deal_group, solo_slots, slot_of);
    HIP_TRY(h, hipGetLastError());
    h->order_rec = OrderRecord{slot_of ? 1 : 2, total_pools * POOL + solo_slots, solo_slots, total_pools, pools_per_block, deal_group, lane_cap, (int)blocks, 0, W, h->local_rows};
    return 0;
}

// The main launch of a ranked hand-out takes its slots from h->order (rank_pixels): the first solo_slots go to the solo waves, every other
// resident wave starts with a pool of its own (ColdParams::first_pools), and the second counter hands out the rest.
template <class T>
int hand_out_ranked(rtiow_handle_s* h, Launch<T>& L, int total_pools, int solo_slots, int solo_waves) {
    L.p.cold.order = h->order;
    L.p.cold.total_slots = solo_slots + total_pools * POOL;
    L.p.cold.work_counter = h->work_counter + 1;
    L.p.cold.first_pools = 1;
    const int resident_waves = (int)L.blocks * ((L.p.cold.bx * L.p.cold.by + 63) / 64);
    const unsigned counter_start = (unsigned)solo_slots + (unsigned)(resident_waves - solo_waves) * (unsigned)L.p.lane_cap;
    HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)(h->work_counter + 1), (int)counter_start, 1, h->stream));
    return 0;
}

// rtiow_stats of a render-family launch (not of a counting run).  A launch of no workgroups (an adaptive chunk without active pixels)
// reports no kernel resources.
template <class T>
void record_launch(rtiow_handle_s* h, const Launch<T>& L, int phases = 1, int solo_waves = 0, int solo_lanes = 0, int staged_stores = 0) {
    h->stats.vgprs = L.fa.numRegs;
    h->stats.sgprs = 0;
    h->stats.lds_bytes = L.blocks > 0 ? (int)(L.lds + L.fa.sharedSizeBytes) : 0;
    h->stats.block_x = L.p.cold.bx; h->stats.block_y = L.p.cold.by;
    h->stats.scene_source = L.effective_source;
    h->stats.schedule = h->schedule;
    h->stats.grid_blocks = (int)L.blocks;
    h->stats.phases = phases;
    if (phases == 1) h->stats.prepass_samples = 0;
    h->stats.solo_waves = solo_waves;
    h->stats.solo_lanes = solo_lanes;
    h->stats.staged_stores = staged_stores;
    h->stats.order_reused = 0;
}

template <class T>
int launch_render(rtiow_handle_s* h, int bx, int by, int wave_tiles, unsigned long long* seg_counter = nullptr, bool prepare_only = false) {
    const bool count = seg_counter != nullptr;
    Launch<T> L{make_params<T>(h)};
    RenderParams<T>& p = L.p;
    const dim3 block(bx * by);
    p.cold.seg_counter = seg_counter ? seg_counter + 1 : nullptr;     // [0] prepass launch, [1] main (or only) launch
    p.cold.pixel_times = seg_counter ? h->pixel_times : nullptr;
    int phases = 1;
    bool reused = false;                        // sorted schedule: the launch below runs in the order an earlier render ranked
    dim3 grid;
    if (h->schedule == RTIOW_SCHED_STATIC) {
        p.cold.bx = bx; p.cold.by = by; p.cold.wave_tiles = wave_tiles;
        p.lane_cap = 64;
        if (int rc = layout_lds<T>(h, L, bx * by, false, !count)) return rc;
        L.k = by_source(L.lds_source, [&](auto src) { return count ? render_kernel<T, src, true> : render_kernel<T, src, false>; });
        HIP_TRY(h, allow_lds(L.k, L.lds));
        HIP_TRY(h, hipFuncGetAttributes(&L.fa, (const void*)L.k));
        grid = dim3((p.cold.W + bx - 1) / bx, (h->local_rows + by - 1) / by);
        L.blocks = (long long)grid.x * grid.y;
    } else {
        int rc = persistent_setup(h, L, !count, !count, [&](auto src, auto bounded) {
            return count ? render_persistent_kernel<T, src, true, bounded> : render_persistent_kernel<T, src, false, bounded>;
        });
        if (rc) return rc;
        HIP_TRY(h, hipMemsetAsync(h->work_counter, 0, 2 * sizeof(unsigned int), h->stream));
        const int waves_per_block = 4;
        if ((rc = size_persistent<T>(h, L, (long long)((p.cold.W + 7) / 8) * ((h->local_rows + 7) / 8) * POOL))) return rc;
        const long long blocks = L.blocks;
        const int lane_cap = p.lane_cap;
        grid = dim3((unsigned)blocks);

        const int npix = p.cold.W * h->local_rows;
        const int S = p.cold.S;
        // prepass length: enough samples to rank the pixels, a small share of the frame
        int SA = S >= 64 ? 3 : (S >= 24 ? 2 : 0);
        SA = tuned("RTIOW_TUNE_SA", SA);       // measured on the headline config: 1 -> 25.5 ms, 2 -> 22.5, 3 -> 22.1, 4 -> 22.4, 8 -> 23.1
        if (SA > 0 && sorted_handout(h)) {
            const int total_pools = (npix + POOL - 1) / POOL;
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
            const double fill_level = (double)total_pools / (double)(blocks * waves_per_block);
            int solo_waves = (seg_counter || p.B < 32) ? 0 : (fill_level < 1.2 ? 128 : (fill_level < 4.0 ? 256 : 0)), solo_lanes = 2;
            solo_waves = tuned("RTIOW_TUNE_SOLO_WAVES", solo_waves);
            solo_lanes = tuned("RTIOW_TUNE_SOLO_LANES", solo_lanes);
            if (solo_lanes < 1) solo_lanes = 1;
            const RenderFn<T> k_solo = by_source(L.lds_source, [](auto src) { return render_solo_kernel<T, src>; });
            if (solo_waves > 0) {
                HIP_TRY(h, allow_lds(k_solo, L.lds));
                int per_cu_solo = 0;
                HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_solo, (const void*)k_solo, 256, L.lds));
                if ((long long)per_cu_solo * h->num_cus < blocks) solo_waves = 0;   // its workgroups must all be resident, as the first pools assume
            }
            if (solo_lanes > lane_cap) solo_lanes = lane_cap;
            if (solo_waves > (int)blocks) solo_waves = (int)blocks;
            if ((long long)solo_waves * solo_lanes > npix / 2) solo_waves = npix / 2 / solo_lanes;
            const int solo_slots = solo_waves * solo_lanes;
            // finished pixels go to their slot in a staging buffer and place_pixels_kernel writes the image (ColdParams::stage_by_slot)
#ifdef RTIOW_DIRECT_STORES
            const bool staged_stores = false;           // A/B build: every lane stores its pixel at its place in the image when it finishes
#else
            const bool staged_stores = true;
#endif
            // The carried order (order_key.h): the last two-phase render of this handle ranked this very frame for this very launch and
            // nothing has touched h->order / h->slot_of since.  Then the prepass and the ranking are skipped: one launch renders samples
            // [0, S) from the states of rtiow_init_rng in that order.  The order is a scheduling hint -- every pixel is its own
            // sequential chain -- so the image is the same bit for bit.  Counting runs always rank again.
            const OrderKey key = {p.cold.W, h->local_rows, h->rank, h->nranks, h->strip_rows, S, p.B, h->precision, h->schedule, h->scene_source,
                                  lane_cap, (int)blocks, total_pools, solo_waves, solo_lanes, L.bounded_f32 ? 1 : 0, staged_stores ? 1 : 0};
            reused = !count && staged_stores && h->order_reuse && h->carried.usable(key);
            if (!reused) {
                h->carried.clear();                      // the buffers below are about to be overwritten, perhaps reallocated
                h->order_rec = OrderRecord{};
                phases = 2;
                HIP_TRY(h, h->mid.ensure((size_t)npix * sizeof(MidState<T>)));
                HIP_TRY(h, h->cost.ensure((size_t)npix * sizeof(uint32_t)));
                HIP_TRY(h, h->cost_rank.ensure((size_t)npix * sizeof(uint32_t)));
            }
            const size_t total_slots = (size_t)total_pools * POOL + (size_t)solo_slots;
            HIP_TRY(h, h->order.ensure(total_slots * sizeof(int)));
            HIP_TRY(h, h->sort_scratch.ensure((size_t)3 * COST_BINS * sizeof(unsigned)));
            if (staged_stores) {
                HIP_TRY(h, h->slot_of.ensure((size_t)npix * sizeof(int)));
                HIP_TRY(h, h->staged.ensure(total_slots * 3 * sizeof(T)));
            }
            if (prepare_only) return 0;                  // every table and buffer of this configuration now exists
            if (!reused) {
                // ---- prepass: samples [0, SA) in tile order through the same persistent body (the static
                // kernel keeps only ~40 % of its lanes busy over a few samples: 2.6 ms vs 1.4 ms measured
                // for 4 samples); RNG state, colour sum and segment count are parked per pixel.
                RenderParams<T> pa = p;
                pa.s_end = SA; pa.cold.mid_out = h->mid; pa.cold.cost_out = h->cost;
                pa.cold.seg_counter = seg_counter;
                if (pa.cold.clock_stamps) pa.cold.clock_stamps = h->clock_stamps_dev;          // the prepass's four words
                const RenderFn<T> kp = by_source(L.lds_source, [&](auto src) -> RenderFn<T> {
                    if constexpr (sizeof(T) == 4)
                        if (L.bounded_f32) return count ? render_prepass_kernel<T, src, true, true> : render_prepass_kernel<T, src, false, true>;
                    return count ? render_prepass_kernel<T, src, true> : render_prepass_kernel<T, src, false>;
                });
                HIP_TRY(h, allow_lds(kp, L.lds));
                hipLaunchKernelGGL(kp, grid, block, L.lds, h->stream, pa);
                if (h->time_phases) HIP_TRY(h, hipEventRecord(h->ev_a, h->stream));
                h->stats.prepass_samples = SA;
                HIP_TRY(h, hipGetLastError());
                // ---- rank the pixels by measured cost, heavy first, dealt into balanced pools
                if ((rc = rank_pixels(h, h->cost, blocks, waves_per_block, lane_cap, total_pools, solo_slots, staged_stores ? h->slot_of.as<int>() : nullptr))) return rc;
                if (!count && staged_stores) h->carried.store(key);
                // ---- main launch: samples [SA, S) in that order
                p.cold.s_begin = SA; p.cold.mid_in = h->mid;
            }
            p.cold.solo_waves = solo_waves; p.cold.solo_lanes = solo_lanes;
            if (staged_stores) { p.cold.stage_by_slot = 1; p.cold.fb = h->staged.as<T>(); }
            if (solo_waves > 0) {
                L.k = k_solo;
                HIP_TRY(h, hipFuncGetAttributes(&L.fa, (const void*)L.k));
            }
            if ((rc = hand_out_ranked(h, L, total_pools, solo_slots, solo_waves))) return rc;
        }
    }
    if (prepare_only) return 0;
    if (seg_counter) {
        h->last_count_blocks = (int)L.blocks;
        h->last_count_waves_per_block = (int)((block.x + 63) / 64);
        // the kernel writes 8 words per wave: hand the buffer over only if it holds every wave of this launch
        if (h->timeline && (size_t)h->last_count_blocks * h->last_count_waves_per_block <= h->timeline_cap_waves) p.cold.timeline = h->timeline;
    }
    if (h->time_phases && phases == 2) HIP_TRY(h, hipEventRecord(h->ev_b, h->stream));
    hipLaunchKernelGGL(L.k, grid, block, L.lds, h->stream, p);
    HIP_TRY(h, hipGetLastError());
    if (p.cold.stage_by_slot) {                             // slot order -> image, in whole lines
        if (h->time_phases) HIP_TRY(h, hipEventRecord(h->ev_c, h->stream));
        const int npix = p.cold.W * h->local_rows;
        hipLaunchKernelGGL(place_pixels_kernel<T>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, h->stream, h->staged.as<const T>(), h->slot_of, (T*)h->fb, npix);
        HIP_TRY(h, hipGetLastError());
    }
    if (!count) {
        record_launch(h, L, phases, p.cold.solo_waves, p.cold.solo_waves > 0 ? p.cold.solo_lanes : 0, p.cold.stage_by_slot);
        h->stats.primary_rays = (uint64_t)h->local_rows * p.cold.W * (uint64_t)p.cold.S;
        h->stats.order_reused = reused ? 1 : 0;
    }
    return 0;
}

#ifdef RTIOW_DEBUG_API
// rtiow_debug_hit_world: hit_world on n caller rays {O, D} (device memory) with the scene laid out as the persistent launches lay it out.
template <class T>
int launch_probe(rtiow_handle_s* h, int n, const T* rays, T* t_out, int* index_out) {
    Launch<T> L{make_params<T>(h)};
    if (int rc = layout_lds<T>(h, L, 256, true, true)) return rc;
    if (!L.lds_source) return fail_arg(h, RTIOW_E_STATE, "rtiow_debug_hit_world needs an LDS scene source");
    HIP_TRY(h, allow_lds(hit_probe_kernel<T>, L.lds));
    const int blocks = std::min(2048, (n + 255) / 256);
    hipLaunchKernelGGL(hit_probe_kernel<T>, dim3(blocks), dim3(256), L.lds, h->stream, L.p, rays, n, t_out, index_out);
    HIP_TRY(h, hipGetLastError());
    h->stats.scene_source = L.effective_source;
    return 0;
}
#endif

// One chunk of progressive rendering (rtiow_accumulate): samples [h->acc_samples, h->acc_samples + samples) of every local pixel through
// render_accumulate_kernel, always with the persistent hand-out.  The first chunk after a reset starts from the RNG states of rtiow_init_rng
// in tile order; under RTIOW_SCHED_SORTED every later chunk ranks the pixels heavy-first by the segments each ran in the previous chunk
// (same limits as launch_render).  No solo waves, no staged stores: the preview is stored at its pixel.  timed: the start event goes
// behind the allocations and table builds, in front of the first enqueued work.
template <class T>
int launch_accumulate(rtiow_handle_s* h, int samples, bool timed) {
    Launch<T> L{make_params<T>(h)};
    RenderParams<T>& p = L.p;
    int rc = persistent_setup(h, L, timed, true, [](auto src, auto bounded) { return render_accumulate_kernel<T, src, bounded>; });
    if (rc) return rc;
    if ((rc = size_persistent<T>(h, L, (long long)((p.cold.W + 7) / 8) * ((h->local_rows + 7) / 8) * POOL))) return rc;

    // The state records ping-pong: the chunk reads acc_mid[acc_cur] and writes the other buffer.
    const int npix = p.cold.W * h->local_rows;
    const int n = h->acc_samples;
    for (auto& b : h->acc_mid) HIP_TRY(h, b.ensure((size_t)npix * sizeof(MidState<T>)));
    HIP_TRY(h, h->acc_cost.ensure((size_t)npix * sizeof(uint32_t)));
    const bool ranked = n > 0 && sorted_handout(h);
    const int total_pools = (npix + POOL - 1) / POOL;
    if (ranked) {
        h->carried.clear();                              // this chunk's ranking overwrites h->order: launch_render ranks again
        h->order_rec = OrderRecord{};
        HIP_TRY(h, h->cost_rank.ensure((size_t)npix * sizeof(uint32_t)));
        HIP_TRY(h, h->order.ensure((size_t)total_pools * POOL * sizeof(int)));
        HIP_TRY(h, h->sort_scratch.ensure((size_t)3 * COST_BINS * sizeof(unsigned)));
    }
    const int in = h->acc_cur, out = n > 0 ? 1 - in : 0;
    p.cold.s_begin = n; p.s_end = n + samples;
    p.cold.pixel_samples_scale = (T)1 / (T)(n + samples);   // rtiow_host_camera's 1 / samples_per_pixel at the running total
    if (n > 0) p.cold.mid_in = h->acc_mid[in];
    p.cold.mid_out = h->acc_mid[out];
    p.cold.cost_out = h->acc_cost;

    if (timed) HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->work_counter, 0, 2 * sizeof(unsigned int), h->stream));
    if (ranked) {
        // the previous chunk's segment counts rank this one (the launch below overwrites them: stream order)
        if ((rc = rank_pixels(h, h->acc_cost, L.blocks, 4, L.p.lane_cap, total_pools, 0, nullptr))) return rc;
        if ((rc = hand_out_ranked(h, L, total_pools, 0, 0))) return rc;
    }
    hipLaunchKernelGGL(L.k, dim3((unsigned)L.blocks), dim3(256), L.lds, h->stream, p);
    HIP_TRY(h, hipGetLastError());
    h->acc_cur = out;
    record_launch(h, L);
    h->stats.primary_rays = (uint64_t)npix * (uint64_t)samples;
    return 0;
}

// One adaptive chunk (rtiow_accumulate_adaptive): adaptive_select_kernel lists the active pixels in h->order and copies the records of the
// others, the host reads the active count back (the call blocks here once), render_adaptive_kernel renders `samples` more samples of the
// active pixels with a persistent grid sized from the active slots, and adaptive_finish_kernel writes every pixel's preview, count and
// error.  The records ping-pong between h->acc_mid[0/1] like launch_accumulate's.  No ranking by previous cost and no solo waves.
// timed: ev0 -> ev_a (select) plus ev_b -> ev1 (render and finish): the read-back between them is not counted.  The caller has checked
// order_fits.
template <class T>
int launch_adaptive(rtiow_handle_s* h, int samples, int min_samples, double rel_error, int max_samples, bool timed, int& active) {
    Launch<T> L{make_params<T>(h)};
    RenderParams<T>& p = L.p;
    int rc = persistent_setup(h, L, timed, true, [](auto src, auto bounded) { return render_adaptive_kernel<T, src, bounded>; });
    if (rc) return rc;

    const int W = p.cold.W, npix = W * h->local_rows;
    const int total_pools = (npix + POOL - 1) / POOL;
    for (auto& b : h->acc_mid) HIP_TRY(h, b.ensure((size_t)npix * sizeof(MidState<T>)));
    HIP_TRY(h, h->adapt_counts.ensure((size_t)npix * sizeof(int32_t)));
    HIP_TRY(h, h->adapt_err.ensure((size_t)npix * sizeof(float)));
    HIP_TRY(h, h->adapt_ctr.ensure(2 * sizeof(unsigned)));
    h->carried.clear();                                  // the active list overwrites h->order: launch_render ranks again
    h->order_rec = OrderRecord{};
    HIP_TRY(h, h->order.ensure((size_t)total_pools * POOL * sizeof(int)));
    const bool first = h->acc_mode != ACC_MODE_ADAPTIVE;  // first chunk after a reset: every pixel at n = 0 from rng_in
    const int in = h->acc_cur, out = first ? 0 : 1 - in;
    if (!first) p.cold.mid_in = h->acc_mid[in];
    p.cold.mid_out = h->acc_mid[out];

    if (timed) HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->adapt_ctr, 0, 2 * sizeof(unsigned), h->stream));
    const int tiles = ((W + 7) / 8) * ((h->local_rows + 7) / 8);
    hipLaunchKernelGGL(adaptive_select_kernel<T>, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, h->stream, FrameShape{W, h->local_rows},
                       samples, min_samples, max_samples, rel_error, h->adapt_counts, h->adapt_err, h->rng, p.cold.mid_in, p.cold.mid_out, h->order, h->adapt_ctr);
    HIP_TRY(h, hipGetLastError());
    if (timed) HIP_TRY(h, hipEventRecord(h->ev_a, h->stream));
    unsigned n_active = 0;
    HIP_TRY(h, hipMemcpyAsync(&n_active, h->adapt_ctr, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    active = (int)n_active;
    h->order_rec.kind = 3; h->order_rec.n_active = active; h->order_rec.total_slots = (int)(((long long)n_active + POOL - 1) / POOL * POOL);
    h->order_rec.total_pools = h->order_rec.total_slots / POOL; h->order_rec.W = W; h->order_rec.local_rows = h->local_rows;
    if (timed) HIP_TRY(h, hipEventRecord(h->ev_b, h->stream));

    if (n_active > 0) {
        const long long active_slots = ((long long)n_active + POOL - 1) / POOL * POOL;
        if ((rc = size_persistent<T>(h, L, active_slots))) return rc;
        p.s_end = samples;                                // the chunk's own sample numbering: adaptive_pixel adds it to the pixel's count
        p.cold.pixel_samples_scale = (T)0;                // not read: no preview in the render
        p.cold.order = h->order;
        if (active_slots > (long long)n_active)           // the tail of the last pool: -1, no pixel
            HIP_TRY(h, hipMemsetAsync(h->order + n_active, 0xff, (size_t)(active_slots - n_active) * sizeof(int), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->work_counter, 0, 2 * sizeof(unsigned int), h->stream));
        hipLaunchKernelGGL(L.k, dim3((unsigned)L.blocks), dim3(256), L.lds, h->stream, p);
        HIP_TRY(h, hipGetLastError());
        h->order_rec.lane_cap = p.lane_cap; h->order_rec.blocks = (int)L.blocks;
    }
    hipLaunchKernelGGL(adaptive_finish_kernel<T>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, h->stream, (size_t)npix, (const unsigned char*)p.cold.mid_out,
                       p.cold.fb, h->adapt_counts, h->adapt_err, h->adapt_ctr + 1);
    HIP_TRY(h, hipGetLastError());
    h->acc_cur = out;
    record_launch(h, L);
    h->stats.primary_rays = (uint64_t)n_active * (uint64_t)samples;
    return 0;
}

// First-hit guides of every local pixel (rtiow_render_guides) into h->guide_nd / h->guide_alb: guide_kernel with the scene staged as
// the render launches stage it (layout_lds of a non-persistent launch: no drain scratch), one 8x8 tile per wave, four waves a workgroup.
template <class T>
int launch_guides(rtiow_handle_s* h) {
    Launch<T> L{make_params<T>(h)};
    const int threads = 256;
    int rc = layout_lds<T>(h, L, threads, false, false);
    if (rc) return rc;
    const size_t npix = local_pixels(h);
    HIP_TRY(h, h->guide_nd.ensure(npix * 4 * sizeof(T)));
    HIP_TRY(h, h->guide_alb.ensure(npix * 4 * sizeof(T)));
    const auto k = by_source(L.lds_source, [](auto src) { return guide_kernel<T, src>; });
    HIP_TRY(h, allow_lds(k, L.lds));
    const int tiles = ((L.p.cold.W + 7) / 8) * ((h->local_rows + 7) / 8);
    hipLaunchKernelGGL(k, dim3((unsigned)((tiles + 3) / 4)), dim3(threads), L.lds, h->stream, L.p, h->guide_nd.as<T>(), h->guide_alb.as<T>());
    HIP_TRY(h, hipGetLastError());
    h->guides_ok = true;
    return 0;
}

// The accumulation's current records and counts: plain mode one count for all (counts = nullptr), adaptive mode the per-pixel array.
inline void accumulation_source(const rtiow_handle_s* h, const unsigned char*& mid, const int32_t*& counts, int& n_uniform) {
    mid = h->acc_mid[h->acc_cur];
    counts = h->acc_mode == ACC_MODE_ADAPTIVE ? h->adapt_counts : nullptr;
    n_uniform = h->acc_mode == ACC_MODE_ADAPTIVE ? 0 : h->acc_samples;
}

// The linear image of the accumulation into h->linear (rtiow_read_linear).  The caller has checked that a chunk has run.
template <class T>
int launch_linear(rtiow_handle_s* h) {
    const size_t npix = local_pixels(h);
    HIP_TRY(h, h->linear.ensure(npix * 3 * sizeof(T)));
    const unsigned char* mid; const int32_t* counts; int n_uniform;
    accumulation_source(h, mid, counts, n_uniform);
    hipLaunchKernelGGL(linear_kernel<T>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, h->stream, npix, mid, counts, n_uniform, h->linear.as<T>());
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// `levels` launches of denoise_level_kernel over the accumulation (rtiow_denoise): level 0 reads the records, the levels ping-pong through
// h->dn_tmp[0/1], the last writes the gamma-encoded image to h->denoised.  inv2[4] = 1 / sigma^2 of colour, normal, albedo, depth (double);
// the colour term of level k is scaled by 4^k and every weight is rounded to T here.  The caller has checked state and arguments and
// made the guides current.
// from_history: level 0 reads the temporal colour plane h->hist_rgb instead (rtiow_denoise_history).
template <class T>
int launch_denoise(rtiow_handle_s* h, int levels, const double inv2[4], bool from_history = false) {
    const int W = img_w(h), rows = h->local_rows;
    const size_t npix = (size_t)W * rows;
    HIP_TRY(h, h->denoised.ensure(npix * 3 * sizeof(T)));
    for (int b = 0; b < 2 && b < levels - 1; ++b) HIP_TRY(h, h->dn_tmp[b].ensure(npix * 3 * sizeof(T)));
    const unsigned char* mid; const int32_t* counts; int n_uniform;
    accumulation_source(h, mid, counts, n_uniform);
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((rows + 15) / 16));
    for (int k = 0; k < levels; ++k) {
        FilterWeights<T> fw;
        fw.ic = (T)(inv2[0] * std::ldexp(1.0, 2 * k));
        fw.in = (T)inv2[1]; fw.ia = (T)inv2[2]; fw.iz = (T)inv2[3];
        const bool last = k == levels - 1;
        const bool records = k == 0 && !from_history;
        const T* cin = k == 0 ? (from_history ? h->hist_rgb.as<const T>() : nullptr) : h->dn_tmp[(k - 1) & 1].as<const T>();
        T* cout = (last ? h->denoised : h->dn_tmp[k & 1]).as<T>();
        hipLaunchKernelGGL(denoise_level_kernel<T>, grid, dim3(256), 0, h->stream, FrameShape{W, rows}, 1 << k, fw, records ? mid : nullptr,
                           counts, n_uniform, cin, h->guide_nd.as<const T>(), h->guide_alb.as<const T>(), cout, last ? 1 : 0);
        HIP_TRY(h, hipGetLastError());
    }
    h->denoised_ok = true;
    return 0;
}

// The base camera's constants of history_reproject_kernel, in double from the stored camera fields and
// rounded once to T: a = pixel00' - O', w = du' x dv' turned so that f = a.w > 0, iu = 1 / |du'|^2, iv = 1 / |dv'|^2.  Returns whether
// the base can be reprojected into: f finite and not 0.
template <class T, class CAM>
bool history_constants(const CAM& b, HistoryParams<T>& hp) {
    const double O[3] = {(double)b.center[0], (double)b.center[1], (double)b.center[2]};
    const double du[3] = {(double)b.pixel_delta_u[0], (double)b.pixel_delta_u[1], (double)b.pixel_delta_u[2]};
    const double dv[3] = {(double)b.pixel_delta_v[0], (double)b.pixel_delta_v[1], (double)b.pixel_delta_v[2]};
    const double a[3] = {(double)b.pixel00_loc[0] - O[0], (double)b.pixel00_loc[1] - O[1], (double)b.pixel00_loc[2] - O[2]};
    double w[3] = {du[1] * dv[2] - du[2] * dv[1], du[2] * dv[0] - du[0] * dv[2], du[0] * dv[1] - du[1] * dv[0]};
    double f = (a[0] * w[0] + a[1] * w[1]) + a[2] * w[2];
    if (f < 0) { w[0] = -w[0]; w[1] = -w[1]; w[2] = -w[2]; f = -f; }
    const double iu = 1.0 / ((du[0] * du[0] + du[1] * du[1]) + du[2] * du[2]), iv = 1.0 / ((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]);
    hp.Ob = {(T)O[0], (T)O[1], (T)O[2]};
    hp.a = {(T)a[0], (T)a[1], (T)a[2]};
    hp.w = {(T)w[0], (T)w[1], (T)w[2]};
    hp.dub = {(T)du[0], (T)du[1], (T)du[2]};
    hp.dvb = {(T)dv[0], (T)dv[1], (T)dv[2]};
    hp.f = (T)f; hp.iu = (T)iu; hp.iv = (T)iv;
    return std::isfinite(hp.f) && hp.f != (T)0;
}

// history_reproject_kernel over the current accumulation and the base into h->hist_cm / h->hist_rgb (rtiow_history_update); the count of
// pixels that carried history goes to h->hist_ctr.  The caller has checked state and arguments and made the guides current.
template <class T>
int launch_history(rtiow_handle_s* h, double depth_tol, double normal_cos, double max_history) {
    const int W = img_w(h), rows = h->local_rows;
    const size_t npix = (size_t)W * rows;
    HIP_TRY(h, h->hist_cm.ensure(npix * 4 * sizeof(T)));
    HIP_TRY(h, h->hist_rgb.ensure(npix * 3 * sizeof(T)));
    HIP_TRY(h, h->hist_ctr.ensure(sizeof(unsigned)));
    const auto& c = camera<T>(h);
    HistoryParams<T> hp{};
    hp.O = {c.center[0], c.center[1], c.center[2]};
    hp.pixel00 = {c.pixel00_loc[0], c.pixel00_loc[1], c.pixel00_loc[2]};
    hp.du = {c.pixel_delta_u[0], c.pixel_delta_u[1], c.pixel_delta_u[2]};
    hp.dv = {c.pixel_delta_v[0], c.pixel_delta_v[1], c.pixel_delta_v[2]};
    hp.depth_tol = (T)depth_tol; hp.normal_cos = (T)normal_cos; hp.max_history = (T)max_history;
    const auto& b = [&]() -> const auto& { if constexpr (sizeof(T) == 4) return h->hist_cam32; else return h->hist_cam64; }();
    hp.have_base = h->hist_base_ok && b.img_width == W && b.img_height == rows && history_constants<T>(b, hp) ? 1 : 0;
    const unsigned char* mid; const int32_t* counts; int n_uniform;
    accumulation_source(h, mid, counts, n_uniform);
    HIP_TRY(h, hipMemsetAsync(h->hist_ctr, 0, sizeof(unsigned), h->stream));
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((rows + 15) / 16));
    hipLaunchKernelGGL(history_reproject_kernel<T>, grid, dim3(256), 0, h->stream, FrameShape{W, rows}, hp, mid, counts, n_uniform,
                       h->guide_nd.as<const Vec4<T>>(), h->hist_base_hm.as<const Vec4<T>>(), h->hist_base_nd.as<const Vec4<T>>(),
                       h->hist_cm.as<Vec4<T>>(), h->hist_rgb.as<T>(), (unsigned*)h->hist_ctr);
    HIP_TRY(h, hipGetLastError());
    h->hist_ok = true;
    return 0;
}

// The variance plane of an adaptive accumulation into h->variance (rtiow_read_variance, level 0 of rtiow_denoise_variance).  The caller
// has checked that the accumulation is adaptive.
template <class T>
int launch_variance_plane(rtiow_handle_s* h) {
    const size_t npix = local_pixels(h);
    HIP_TRY(h, h->variance.ensure(npix * sizeof(T)));
    hipLaunchKernelGGL(variance_plane_kernel<T>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, h->stream, npix,
                       (const unsigned char*)h->acc_mid[h->acc_cur], (const int32_t*)h->adapt_counts, h->variance.as<T>());
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// The levels of rtiow_denoise_variance that stage their taps in LDS (bit k = level k), by measurement at 1920 x 1080 (DESIGN.md section 4.9,
// profiles/denoise_variance/denoise_variance_probe.json): fp32 steps 1, 2 and 4 (5 levels about 1.8 -> 0.9 ms); fp64 steps 1 and 2 (about 2.1 -> 1.25 ms;
// step 4, 96 KB of LDS and one workgroup per CU, gains under 1 %).
constexpr int VARIANCE_TILE_LEVELS_F32 = 7, VARIANCE_TILE_LEVELS_F64 = 3;

// variance_plane_kernel, then `levels` launches of variance_tile_kernel (the levels above) or variance_filter_kernel over the adaptive accumulation (rtiow_denoise_variance): the
// colour ping-pongs through h->dn_tmp[0/1] into h->denoised as in launch_denoise, the variance from h->variance through h->dn_var[0/1]
// (the last level stores none).  sigma_variance in double, its square rounded to T here; +inf -- or a square that is not finite in T --
// turns the colour term off on the host.  inv2g[3] = 1 / sigma^2 of normal, albedo, depth.  The caller has checked state and arguments
// and made the guides current.
template <class T>
int launch_denoise_variance(rtiow_handle_s* h, int levels, double sigma_variance, const double inv2g[3]) {
    const int W = img_w(h), rows = h->local_rows;
    const size_t npix = (size_t)W * rows;
    if (int rc = launch_variance_plane<T>(h)) return rc;
    HIP_TRY(h, h->denoised.ensure(npix * 3 * sizeof(T)));
    for (int b = 0; b < 2 && b < levels - 1; ++b) {
        HIP_TRY(h, h->dn_tmp[b].ensure(npix * 3 * sizeof(T)));
        HIP_TRY(h, h->dn_var[b].ensure(npix * sizeof(T)));
    }
    VarianceWeights<T> fw;
    fw.sv2 = (T)(sigma_variance * sigma_variance);
    fw.colour_on = std::isfinite(fw.sv2) ? 1 : 0;
    if (!fw.colour_on) fw.sv2 = (T)0;
    fw.eps = (T)1e-8;
    fw.in = (T)inv2g[0]; fw.ia = (T)inv2g[1]; fw.iz = (T)inv2g[2];
    const unsigned char* mid = h->acc_mid[h->acc_cur];
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((rows + 15) / 16));
    // bit k: level k (step 1 << k, k < 3) stages its taps in LDS (variance_tile_kernel)
    const int tile_levels = tuned("RTIOW_TUNE_VARIANCE_TILE", sizeof(T) == 4 ? VARIANCE_TILE_LEVELS_F32 : VARIANCE_TILE_LEVELS_F64);
    for (int k = 0; k < levels; ++k) {
        fw.fk = (T)std::ldexp(1.0, 2 * k);
        const bool last = k == levels - 1;
        const T* cin = k == 0 ? nullptr : h->dn_tmp[(k - 1) & 1].as<const T>();
        const T* vin = k == 0 ? h->variance.as<const T>() : h->dn_var[(k - 1) & 1].as<const T>();
        T* cout = (last ? h->denoised : h->dn_tmp[k & 1]).as<T>();
        T* vout = last ? nullptr : h->dn_var[k & 1].as<T>();
        const bool tiled = k < 3 && ((tile_levels >> k) & 1);
        const size_t lds = tiled ? variance_tile_bytes<T>(1 << k) : 0;
        const auto kernel = tiled ? variance_tile_kernel<T> : variance_filter_kernel<T>;
        HIP_TRY(h, allow_lds(kernel, lds));
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, h->stream, FrameShape{W, rows}, 1 << k, fw, k == 0 ? mid : nullptr,
                           (const int32_t*)h->adapt_counts, cin, vin, h->guide_nd.as<const T>(), h->guide_alb.as<const T>(), cout, vout, last ? 1 : 0);
        HIP_TRY(h, hipGetLastError());
    }
    h->denoised_ok = true;
    return 0;
}

// T (the reference's --threads) shapes the workgroup of RTIOW_SCHED_STATIC, whose lanes ARE the
// pixels of a T x T block.  The dynamic schedules hand pixels to lanes themselves, so a workgroup
// there is just four waves whatever T says (measured with T as the workgroup size: 69 / 22.3 / 22.3 /
// 33 / 26 ms for T = 4 / 8 / 16 / 24 / 32 -- partly filled waves and uneven SIMD packing).
void block_shape(int T, bool static_schedule, int& bx, int& by, int& wave_tiles) {
    if (!static_schedule) T = 0;
    if (T == 0) { bx = 16; by = 16; wave_tiles = 1; }       // library tiling: 4 waves, each an 8x8 tile
    else if (T == 8) { bx = 8; by = 8; wave_tiles = 1; }    // == the reference's 8x8 block (one wave)
    else { bx = T; by = T; wave_tiles = 0; }                 // the reference's T x T row-major block
}

}  // namespace
