// launch.h -- the render-family launches on one shared setup (layout_lds, persistent_setup, size_persistent, record_launch): launch_render
// (static / persistent / sorted with prepass + cost sort + solo waves, or in the order an earlier render left: order_key.h), launch_accumulate (one chunk of progressive rendering),
// launch_adaptive (one adaptive chunk), each as: layout and kernel pick -> plan (launch_plan.h: every integer of the schedule; the occupancy
// queries it asks for are made here) -> buffers -> enqueue -> record; launch_guides / launch_linear / launch_denoise: the denoised previews; launch_variance_plane /
// launch_denoise_variance: the variance-guided filter (from_history: of the temporal image, by launch_temporal_noise's plane); launch_history: the temporal reprojection, plain or with the neighbourhood clamp; launch_history_plan: its history length alone; launch_coverage / launch_edge_resolve: the coverage layers and the resolve of the mixed pixels; prepare_upscale / finish_upscale: what the upscale launches share; launch_upscale: the preview at a multiple of the traced resolution (instantiated by rtiow_upscale.hip and, over the device grid, rtiow_large_upscale.hip); launch_upscale_wide: the same with 4 x 4 taps (instantiated by rtiow_upscale_wide.hip and rtiow_large_upscale.hip); upscale_call (pass.h): the body of the four entry points
// launch_accumulate, launch_adaptive, launch_guides, launch_coverage, prepare_upscale, launch_upscale and launch_upscale_wide take the scene
// binding of the call (StagedScene below for the calls that stage the scene by the handle's scene source; large_launch.h's DeviceGridScene
// for the device grid): each launch is stated once.
// Host side of librtiow_hip.so; part of the translation unit rtiow_hip.hip, of rtiow_upscale.hip for launch_upscale, of rtiow_upscale_wide.hip
// for launch_upscale_wide, of rtiow_large_preview.hip for the four launches over the device grid and of rtiow_large_upscale.hip for the
// two upscale launches over it (internal linkage).
#pragma once
#include "scene_tables.h"
#include "lds_placement.h"
#include "../device/render_kernels.h"
#include "../device/adaptive.h"
#include "../device/cost_sort.h"
#include "../device/denoise.h"
#include "../device/guide_chain.h"
#include "../device/guide_lens.h"
#include "../device/denoise_variance.h"
#include "../device/history.h"
#include "../device/history_clip.h"
#include "../device/history_budget.h"
#include "../device/temporal_noise.h"
#include "../device/edge_resolve.h"
#include "../device/upscale.h"
#include "../device/upscale_wide.h"

// The kernels of a chunk and of the guides that read no scene (the selects and the finish of an adaptive chunk, the edit influence) live in
// rtiow_hip.hip's code object alone: launch_adaptive and launch_guides enqueue them through these, whichever unit instantiates the launch.
// Defined in rtiow_hip.hip from the handle's own buffers, in its precision; not exported (librtiow_hip.map).
namespace rtiow_shared {
int enqueue_adaptive_select(rtiow_handle_s* h, int samples, int min_samples, int max_samples, bool budget, double rel_error, double target,
                            const unsigned char* mid_in, unsigned char* mid_out);
int enqueue_adaptive_finish(rtiow_handle_s* h, const unsigned char* mid_out);
int enqueue_edit_influence(rtiow_handle_s* h);
}  // namespace rtiow_shared

namespace {

static_assert(PLAN_POOL == POOL && PLAN_COST_BINS == COST_BINS && PLAN_SMOOTH_TW == SMOOTH_TW && PLAN_SMOOTH_TH == SMOOTH_TH && PLAN_SCHED_SORTED == RTIOW_SCHED_SORTED,
              "launch_plan.h counts in the device's constants");

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

// Finished pixels of a sorted render go to their slot in a staging buffer and place_pixels_kernel writes the image (ColdParams::stage_by_slot).
#ifdef RTIOW_DIRECT_STORES
constexpr bool STAGED_STORES = false;           // A/B build: every lane stores its pixel at its place in the image when it finishes
#else
constexpr bool STAGED_STORES = true;
#endif

// What the plan (launch_plan.h) is made for: the frame and shard of L's parameters, the device, the knobs.
template <class T>
LaunchPlan new_plan(const rtiow_handle_s* h, const RenderParams<T>& p, bool counting = false, bool staged_stores = false) {
    return LaunchPlan{PlanFrame{p.cold.W, h->local_rows, h->rank, h->preview.nranks, h->strip_rows, p.cold.S, p.B, h->precision, h->schedule, h->scene_source,
                                h->num_cus, h->waves_per_simd, counting, staged_stores}};
}

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
        place_grid_blob(p.grid, h->grid_at, lds);
        lds += (size_t)h->grid.blob_bytes;
        p.use_grid = 1;
        if (record_stats) { h->stats.grid_nx = h->grid.nx; h->stats.grid_nz = h->grid.nz; h->stats.grid_registered = h->grid_registered; h->stats.grid_direct = h->grid_direct; h->stats.grid_cell = h->grid.cell; }
    } else if (effective_source == RTIOW_SCENE_GRID) effective_source = RTIOW_SCENE_LDS;   // no grid for this scene: the screened loop
    if (lds > 160 * 1024) return fail_arg(h, RTIOW_E_BADARG, "scene too large for LDS staging; use RTIOW_SCENE_SCALAR");
    return 0;
}

// The scene binding of a launch: how the scene reaches its kernels.  prepare(h, call): what the entry point does for the scene
// before it changes any state (a refusal under the call's name); layout: the parameters and the LDS of the launch; by_source: the scene-source
// template argument of the kernels for that layout; accumulate_kernel / adaptive_kernel: the persistent kernels of a chunk.  This one is
// the binding of every call that stages the scene by the handle's scene source: layout_lds, RTIOW_SCENE_LDS or RTIOW_SCENE_SCALAR, the
// render_* kernels.  The device grid's is large_launch.h's DeviceGridScene (rtiow_large_preview.hip adds its persistent kernels).  render_guides /
// render_coverage: how a call that reads guides and layers makes stale ones current (pass.h: upscale_call).
struct StagedScene {
    int prepare(rtiow_handle_s*, const char*) const { return 0; }
    template <class T>
    int layout(rtiow_handle_s* h, Launch<T>& L, int threads, bool persistent, bool record_stats) const { return layout_lds<T>(h, L, threads, persistent, record_stats); }
    template <class T, class F>
    auto by_source(const Launch<T>& L, F f) const { return ::by_source(L.lds_source, f); }
    template <class T, class SRC, class BOUNDED>
    RenderFn<T> accumulate_kernel(SRC, BOUNDED) const { return render_accumulate_kernel<T, SRC::value, BOUNDED::value>; }
    template <class T, class SRC, class BOUNDED>
    RenderFn<T> adaptive_kernel(SRC, BOUNDED) const { return render_adaptive_kernel<T, SRC::value, BOUNDED::value>; }
    // stale guides and layers made current for a call that reads them (upscale_call): the library's own calls in their asynchronous form
    int render_guides(rtiow_handle_s* h) const { return rtiow_render_guides(h, nullptr); }
    int render_coverage(rtiow_handle_s* h, int subsamples_per_side) const { return rtiow_render_coverage(h, subsamples_per_side, nullptr); }
};

// The setup the persistent launches share (launch_render's dynamic schedules, launch_accumulate, launch_adaptive): four-wave 16 x 16
// workgroups, the main launch's clock stamps (stamp_clock), the scene's LDS layout with drain scratch, the kernel pick(src, bounded) --
// bounded: std::true_type for fp32's bounded twin only -- allowed its LDS, and the two hand-out counters.
template <class T, class Scene, class Pick>
int persistent_setup(rtiow_handle_s* h, Launch<T>& L, const Scene& scene, bool stamp_clock, bool record_stats, Pick pick) {
    block_shape(0, false, L.p.cold.bx, L.p.cold.by, L.p.cold.wave_tiles);
    L.p.cold.clock_stamps = stamp_clock && h->clock_stamps_dev ? h->clock_stamps_dev + 4 : nullptr;
    if (int rc = scene.template layout<T>(h, L, 256, true, record_stats)) return rc;
    L.k = scene.by_source(L, [&](auto src) { return pick(src, std::false_type()); });
    if constexpr (sizeof(T) == 4) L.kb = scene.by_source(L, [&](auto src) { return pick(src, std::true_type()); });
    HIP_TRY(h, allow_lds(L.k, L.lds));
    HIP_TRY(h, h->work_counter.ensure(2 * sizeof(unsigned int)));
    return 0;
}

// Size L's persistent launch over `slots` hand-out slots, taken from h->work_counter in tile order, as plan_size decides from k's
// occupancy: p.lane_cap, blocks, and -- when the plan asks for fp32's bounded twin and kb keeps the occupancy -- kb in place of k; then k's attributes.
template <class T>
int size_persistent(rtiow_handle_s* h, Launch<T>& L, LaunchPlan& P, long long slots) {
    const int threads = L.p.cold.bx * L.p.cold.by;
    int per_cu = 0;
    HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)L.k, threads, L.lds));
    plan_size(P, slots, per_cu);
    if (L.kb && P.want_twin) {
        HIP_TRY(h, allow_lds(L.kb, L.lds));
        int per_cu_twin = 0;
        HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_twin, (const void*)L.kb, threads, L.lds));
        plan_twin(P, per_cu_twin);
        if (P.bounded_f32) L.k = L.kb;
    }
    L.blocks = P.blocks;
    L.p.lane_cap = P.lane_cap;
    L.p.cold.total_slots = (int)slots;
    L.p.cold.work_counter = h->work_counter;
    HIP_TRY(h, hipFuncGetAttributes(&L.fa, (const void*)L.k));
    return 0;
}

// The hand-out order of a cost-sorted launch, as plan_deal dealt it: the pixels ranked heavy-first by `cost` (segments per local pixel,
// smoothed over a window) and dealt into balanced pools, written to h->order (slot -> row << 16 | column, -1 for padding; the first
// solo_slots slots are the top ranks) and, when slot_of is given, its inverse.  Needs h->order, h->cost_rank and h->sort_scratch sized for the frame.
inline int rank_pixels(rtiow_handle_s* h, const uint32_t* cost, const LaunchPlan& P, int* slot_of) {
    const int W = P.f.W, rows = P.f.local_rows;
    unsigned* hist = h->sort_scratch; unsigned* start = hist + COST_BINS; unsigned* fill = start + COST_BINS;
    HIP_TRY(h, hipMemsetAsync(hist, 0, COST_BINS * sizeof(unsigned), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->order, 0xff, (size_t)P.total_slots * sizeof(int), h->stream));
    const uint32_t* rank_by = cost;
    if (P.smooth_hw > 0) {
        hipLaunchKernelGGL(cost_smooth_kernel, dim3(P.smooth_blocks), dim3(256), P.smooth_lds_bytes, h->stream, cost, h->cost_rank, W, rows, P.window_strip, P.smooth_hw, hist);
        rank_by = h->cost_rank;
    } else {
        hipLaunchKernelGGL(cost_hist_kernel, dim3(P.hist_blocks), dim3(256), 0, h->stream, rank_by, P.npix, hist);
    }
    hipLaunchKernelGGL(cost_scan_kernel, dim3(1), dim3(COST_BINS), 0, h->stream, hist, start, fill);
    hipLaunchKernelGGL(cost_scatter_kernel, dim3(P.scatter_blocks), dim3(1024), 0, h->stream, rank_by, W, rows, start, fill, h->order,
                       P.pools_per_block, P.total_pools, P.deal_group, P.solo_slots, slot_of);
    HIP_TRY(h, hipGetLastError());
    h->order_rec = plan_ranking_record(P);
    return 0;
}

// The main launch of a ranked hand-out takes its slots from h->order (rank_pixels) through the second counter, which starts behind the solo
// waves' slots and every other resident wave's first pool (ColdParams::first_pools, plan_deal).
template <class T>
int hand_out_ranked(rtiow_handle_s* h, Launch<T>& L, const LaunchPlan& P) {
    L.p.cold.order = h->order;
    L.p.cold.total_slots = (int)P.total_slots;
    L.p.cold.work_counter = h->work_counter + 1;
    L.p.cold.first_pools = 1;
    HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)(h->work_counter + 1), (int)P.counter_start, 1, h->stream));
    return 0;
}

// rtiow_stats of a render-family launch (not of a counting run).  A launch of no workgroups (an adaptive chunk without active pixels)
// reports no kernel resources.
template <class T>
void record_launch(rtiow_handle_s* h, const Launch<T>& L, const PlanStats& st) {
    h->stats.vgprs = L.fa.numRegs;
    h->stats.sgprs = 0;
    h->stats.lds_bytes = L.blocks > 0 ? (int)(L.lds + L.fa.sharedSizeBytes) : 0;
    h->stats.block_x = L.p.cold.bx; h->stats.block_y = L.p.cold.by;
    h->stats.scene_source = L.effective_source;
    h->stats.schedule = h->schedule;
    h->stats.grid_blocks = (int)L.blocks;
    h->stats.phases = st.phases;
    h->stats.prepass_samples = st.prepass_samples;
    h->stats.solo_waves = st.solo_waves;
    h->stats.solo_lanes = st.solo_lanes;
    h->stats.staged_stores = st.staged_stores;
    h->stats.order_reused = 0;
}

template <class T>
int launch_render(rtiow_handle_s* h, int bx, int by, int wave_tiles, unsigned long long* seg_counter = nullptr, bool prepare_only = false) {
    const bool count = seg_counter != nullptr;
    Launch<T> L{make_params<T>(h)};
    RenderParams<T>& p = L.p;
    LaunchPlan P = new_plan(h, p, count, STAGED_STORES);
    const dim3 block(bx * by);
    p.cold.seg_counter = seg_counter ? seg_counter + 1 : nullptr;     // [0] prepass launch, [1] main (or only) launch
    p.cold.pixel_times = seg_counter ? h->pixel_times : nullptr;
    bool reused = false;                        // sorted schedule: the launch below runs in the order an earlier render ranked
    dim3 grid;
    if (h->schedule == RTIOW_SCHED_STATIC) {
        p.cold.bx = bx; p.cold.by = by; p.cold.wave_tiles = wave_tiles;
        p.lane_cap = P.lane_cap;
        if (int rc = layout_lds<T>(h, L, bx * by, false, !count)) return rc;
        L.k = by_source(L.lds_source, [&](auto src) { return count ? render_kernel<T, src, true> : render_kernel<T, src, false>; });
        HIP_TRY(h, allow_lds(L.k, L.lds));
        HIP_TRY(h, hipFuncGetAttributes(&L.fa, (const void*)L.k));
        grid = dim3((p.cold.W + bx - 1) / bx, (h->local_rows + by - 1) / by);
        L.blocks = (long long)grid.x * grid.y;
    } else {
        int rc = persistent_setup(h, L, StagedScene{}, !count, !count, [&](auto src, auto bounded) {
            return count ? render_persistent_kernel<T, src, true, bounded> : render_persistent_kernel<T, src, false, bounded>;
        });
        if (rc) return rc;
        HIP_TRY(h, hipMemsetAsync(h->work_counter, 0, 2 * sizeof(unsigned int), h->stream));
        if ((rc = size_persistent<T>(h, L, P, plan_tile_slots(p.cold.W, h->local_rows)))) return rc;
        grid = dim3((unsigned)P.blocks);
        plan_sorted(P);
        if (P.ranked) {
            const RenderFn<T> k_solo = by_source(L.lds_source, [](auto src) { return render_solo_kernel<T, src>; });
            if (P.solo_waves > 0) {
                HIP_TRY(h, allow_lds(k_solo, L.lds));
                int per_cu_solo = 0;
                HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_solo, (const void*)k_solo, 256, L.lds));
                plan_solo_resident(P, per_cu_solo);
            }
            plan_sorted_finish(P);
            // The carried order (order_key.h): the last two-phase render of this handle ranked this very frame for this very launch and
            // nothing has touched h->order / h->slot_of since.  Then the prepass and the ranking are skipped: one launch renders samples
            // [0, S) from the states of rtiow_init_rng in that order.  The order is a scheduling hint -- every pixel is its own
            // sequential chain -- so the image is the same bit for bit.  Counting runs always rank again.
            const OrderKey key = plan_order_key(P);
            reused = !count && P.f.staged_stores && h->order_reuse && h->carried.usable(key);
            if (!reused) {
                h->carried.clear();                      // the buffers below are about to be overwritten, perhaps reallocated
                h->order_rec = OrderRecord{};
                HIP_TRY(h, h->mid.ensure((size_t)P.npix * sizeof(MidState<T>)));
                HIP_TRY(h, h->cost.ensure((size_t)P.npix * sizeof(uint32_t)));
                HIP_TRY(h, h->cost_rank.ensure((size_t)P.npix * sizeof(uint32_t)));
            }
            HIP_TRY(h, h->order.ensure((size_t)P.total_slots * sizeof(int)));
            HIP_TRY(h, h->sort_scratch.ensure((size_t)3 * COST_BINS * sizeof(unsigned)));
            if (P.f.staged_stores) {
                HIP_TRY(h, h->slot_of.ensure((size_t)P.npix * sizeof(int)));
                HIP_TRY(h, h->staged.ensure((size_t)P.total_slots * 3 * sizeof(T)));
            }
            if (prepare_only) return 0;                  // every table and buffer of this configuration now exists
            if (!reused) {
                // ---- prepass: samples [0, SA) in tile order through the same persistent body (the static
                // kernel keeps only ~40 % of its lanes busy over a few samples: 2.6 ms vs 1.4 ms measured
                // for 4 samples); RNG state, colour sum and segment count are parked per pixel.
                RenderParams<T> pa = p;
                pa.s_end = P.SA; pa.cold.mid_out = h->mid; pa.cold.cost_out = h->cost;
                pa.cold.seg_counter = seg_counter;
                if (pa.cold.clock_stamps) pa.cold.clock_stamps = h->clock_stamps_dev;          // the prepass's four words
                const RenderFn<T> kp = by_source(L.lds_source, [&](auto src) -> RenderFn<T> {
                    if constexpr (sizeof(T) == 4)
                        if (P.bounded_f32) return count ? render_prepass_kernel<T, src, true, true> : render_prepass_kernel<T, src, false, true>;
                    return count ? render_prepass_kernel<T, src, true> : render_prepass_kernel<T, src, false>;
                });
                HIP_TRY(h, allow_lds(kp, L.lds));
                hipLaunchKernelGGL(kp, grid, block, L.lds, h->stream, pa);
                if (h->time_phases) HIP_TRY(h, hipEventRecord(h->ev_a, h->stream));
                h->stats.prepass_samples = P.SA;        // a counting run reports it too (record_launch does not run for it)
                HIP_TRY(h, hipGetLastError());
                // ---- rank the pixels by measured cost, heavy first, dealt into balanced pools
                if ((rc = rank_pixels(h, h->cost, P, P.f.staged_stores ? h->slot_of.as<int>() : nullptr))) return rc;
                if (!count && P.f.staged_stores) h->carried.store(key);
                // ---- main launch: samples [SA, S) in that order
                p.cold.s_begin = P.SA; p.cold.mid_in = h->mid;
            }
            p.cold.solo_waves = P.solo_waves; p.cold.solo_lanes = P.solo_lanes;
            if (P.f.staged_stores) { p.cold.stage_by_slot = 1; p.cold.fb = h->staged.as<T>(); }
            if (P.solo_waves > 0) {
                L.k = k_solo;
                HIP_TRY(h, hipFuncGetAttributes(&L.fa, (const void*)L.k));
            }
            if ((rc = hand_out_ranked(h, L, P))) return rc;
        }
    }
    if (prepare_only) return 0;
    const PlanStats st = plan_stats(P, reused);
    if (seg_counter) {
        h->last_count_blocks = (int)L.blocks;
        h->last_count_waves_per_block = (int)((block.x + 63) / 64);
        // the kernel writes 8 words per wave: hand the buffer over only if it holds every wave of this launch
        if (h->timeline && (size_t)h->last_count_blocks * h->last_count_waves_per_block <= h->timeline_cap_waves) p.cold.timeline = h->timeline;
    }
    if (h->time_phases && st.phases == 2) HIP_TRY(h, hipEventRecord(h->ev_b, h->stream));
    hipLaunchKernelGGL(L.k, grid, block, L.lds, h->stream, p);
    HIP_TRY(h, hipGetLastError());
    if (st.staged_stores) {                                 // slot order -> image, in whole lines
        if (h->time_phases) HIP_TRY(h, hipEventRecord(h->ev_c, h->stream));
        hipLaunchKernelGGL(place_pixels_kernel<T>, dim3((unsigned)((P.npix + 255) / 256)), dim3(256), 0, h->stream, h->staged.as<const T>(), h->slot_of, (T*)h->fb, P.npix);
        HIP_TRY(h, hipGetLastError());
    }
    if (!count) {
        record_launch(h, L, st);
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
// rtiow_debug_scatter: the scatter step on n caller records (device memory), one per lane, with the shade records where the persistent launches
// keep them (LDS or memory).  form 0 / 1 / 2: scatter_probe_kernel; 2 is fp64's rotated trip.
template <class T>
int launch_scatter_probe(rtiow_handle_s* h, int form, int n, const T* in_r, const int* in_i, const uint32_t* in_s, T* out_r, int* out_i, uint32_t* out_s) {
    Launch<T> L{make_params<T>(h)};
    if (int rc = layout_lds<T>(h, L, 256, true, false)) return rc;
    void (*k)(const RenderParams<T>, int, const T*, const int*, const uint32_t*, T*, int*, uint32_t*) = nullptr;
    if (form == 0) k = scatter_probe_kernel<T, 0>;
    else if (form == 1) k = scatter_probe_kernel<T, 1>;
    else if constexpr (sizeof(T) == 8) k = scatter_probe_kernel<T, 2>;
    if (!k) return fail_arg(h, RTIOW_E_BADARG, "rtiow_debug_scatter: form 2 (the rotated trip) exists in fp64 only");
    HIP_TRY(h, allow_lds(k, L.lds));
    hipLaunchKernelGGL(k, dim3((unsigned)((n + 255) / 256)), dim3(256), L.lds, h->stream, L.p, n, in_r, in_i, in_s, out_r, out_i, out_s);
    HIP_TRY(h, hipGetLastError());
    return 0;
}
#endif

// One chunk of progressive rendering (rtiow_accumulate): samples [acc_samples, acc_samples + samples) of every local pixel through
// render_accumulate_kernel, always with the persistent hand-out.  The first chunk after a reset starts from the RNG states of rtiow_init_rng
// in tile order; under RTIOW_SCHED_SORTED every later chunk ranks the pixels heavy-first by the segments each ran in the previous chunk
// (same limits as launch_render).  No solo waves, no staged stores: the preview is stored at its pixel.  timed: the start event goes
// behind the allocations and table builds, in front of the first enqueued work.  scene: the binding (StagedScene for rtiow_accumulate).
template <class T, class Scene>
int launch_accumulate(rtiow_handle_s* h, const Scene& scene, int samples, bool timed) {
    Launch<T> L{make_params<T>(h)};
    RenderParams<T>& p = L.p;
    LaunchPlan P = new_plan(h, p);
    int rc = persistent_setup(h, L, scene, timed, true, [&](auto src, auto bounded) { return scene.template accumulate_kernel<T>(src, bounded); });
    if (rc) return rc;
    if ((rc = size_persistent<T>(h, L, P, plan_tile_slots(p.cold.W, h->local_rows)))) return rc;
    const int n = h->preview.acc_samples;
    plan_chunk(P, n == 0);

    // The state records ping-pong: the chunk reads acc_mid[acc_cur] and writes the other buffer.
    for (auto& b : h->acc_mid) HIP_TRY(h, b.ensure((size_t)P.npix * sizeof(MidState<T>)));
    HIP_TRY(h, h->acc_cost.ensure((size_t)P.npix * sizeof(uint32_t)));
    if (P.ranked) {
        h->carried.clear();                              // this chunk's ranking overwrites h->order: launch_render ranks again
        h->order_rec = OrderRecord{};
        HIP_TRY(h, h->cost_rank.ensure((size_t)P.npix * sizeof(uint32_t)));
        HIP_TRY(h, h->order.ensure((size_t)P.total_slots * sizeof(int)));
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
    if (P.ranked) {
        // the previous chunk's segment counts rank this one (the launch below overwrites them: stream order)
        if ((rc = rank_pixels(h, h->acc_cost, P, nullptr))) return rc;
        if ((rc = hand_out_ranked(h, L, P))) return rc;
    }
    hipLaunchKernelGGL(L.k, dim3((unsigned)L.blocks), dim3(256), L.lds, h->stream, p);
    HIP_TRY(h, hipGetLastError());
    h->acc_cur = out;
    record_launch(h, L, plan_stats(P));
    h->stats.primary_rays = (uint64_t)P.npix * (uint64_t)samples;
    return 0;
}

// One adaptive chunk (rtiow_accumulate_adaptive, rtiow_accumulate_budget): the select kernel lists the active pixels in h->order and copies the records of the
// others, the host reads the active count back (the call blocks here once), render_adaptive_kernel renders `samples` more samples of the
// active pixels with a persistent grid sized from the active slots, and adaptive_finish_kernel writes every pixel's preview, count and
// error.  The records ping-pong between h->acc_mid[0/1] like launch_accumulate's.  No ranking by previous cost and no solo waves.
// timed: ev0 -> ev_a (select) plus ev_b -> ev1 (render and finish): the read-back between them is not counted.  The caller has checked
// plan_order_fits.  rule: which select decides (AdaptiveRule); the budget rule reads the plan h->plan_m, which the caller has found current.
struct AdaptiveRule {
    bool budget;                                         // false: adaptive_select_kernel by rel_error; true: budget_select_kernel by target
    double rel_error, target;
};
template <class T, class Scene>
int launch_adaptive(rtiow_handle_s* h, const Scene& scene, int samples, int min_samples, AdaptiveRule rule, int max_samples, bool timed, int& active) {
    Launch<T> L{make_params<T>(h)};
    RenderParams<T>& p = L.p;
    LaunchPlan P = new_plan(h, p);
    int rc = persistent_setup(h, L, scene, timed, true, [&](auto src, auto bounded) { return scene.template adaptive_kernel<T>(src, bounded); });
    if (rc) return rc;

    const int W = p.cold.W, npix = W * h->local_rows;
    for (auto& b : h->acc_mid) HIP_TRY(h, b.ensure((size_t)npix * sizeof(MidState<T>)));
    HIP_TRY(h, h->adapt_counts.ensure((size_t)npix * sizeof(int32_t)));
    HIP_TRY(h, h->adapt_err.ensure((size_t)npix * sizeof(float)));
    HIP_TRY(h, h->adapt_ctr.ensure(2 * sizeof(unsigned)));
    h->carried.clear();                                  // the active list overwrites h->order: launch_render ranks again
    h->order_rec = OrderRecord{};
    HIP_TRY(h, h->order.ensure((size_t)plan_pools(npix) * POOL * sizeof(int)));    // every pixel may be active
    const bool first = h->preview.acc_mode != ACC_MODE_ADAPTIVE;  // first chunk after a reset: every pixel at n = 0 from rng_in
    const int in = h->acc_cur, out = first ? 0 : 1 - in;
    if (!first) p.cold.mid_in = h->acc_mid[in];
    p.cold.mid_out = h->acc_mid[out];

    if (timed) HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->adapt_ctr, 0, 2 * sizeof(unsigned), h->stream));
    if ((rc = rtiow_shared::enqueue_adaptive_select(h, samples, min_samples, max_samples, rule.budget, rule.rel_error, rule.target, p.cold.mid_in, p.cold.mid_out))) return rc;
    if (timed) HIP_TRY(h, hipEventRecord(h->ev_a, h->stream));
    unsigned n_active = 0;
    HIP_TRY(h, hipMemcpyAsync(&n_active, h->adapt_ctr, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    active = (int)n_active;
    plan_adaptive(P, n_active);
    if (timed) HIP_TRY(h, hipEventRecord(h->ev_b, h->stream));

    if (n_active > 0) {
        const long long active_slots = P.total_slots;             // whole pools
        if ((rc = size_persistent<T>(h, L, P, active_slots))) return rc;
        p.s_end = samples;                                // the chunk's own sample numbering: adaptive_pixel adds it to the pixel's count
        p.cold.pixel_samples_scale = (T)0;                // not read: no preview in the render
        p.cold.order = h->order;
        if (active_slots > (long long)n_active)           // the tail of the last pool: -1, no pixel
            HIP_TRY(h, hipMemsetAsync(h->order + n_active, 0xff, (size_t)(active_slots - n_active) * sizeof(int), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->work_counter, 0, 2 * sizeof(unsigned int), h->stream));
        hipLaunchKernelGGL(L.k, dim3((unsigned)L.blocks), dim3(256), L.lds, h->stream, p);
        HIP_TRY(h, hipGetLastError());
    }
    h->order_rec = plan_adaptive_record(P);
    if ((rc = rtiow_shared::enqueue_adaptive_finish(h, p.cold.mid_out))) return rc;
    h->acc_cur = out;
    record_launch(h, L, plan_stats(P));
    h->stats.primary_rays = (uint64_t)n_active * (uint64_t)samples;
    return 0;
}

// First-hit guides of every local pixel (rtiow_render_guides) into h->guide_nd / h->guide_alb: guide_kernel with the scene staged as
// the render launches stage it (layout_lds of a non-persistent launch: no drain scratch), one 8x8 tile per wave, four waves a workgroup.
// RTIOW_GUIDES_SPECULAR: guide_chain_kernel follows on the same layout and grid and writes the filter guides to h->chain_nd / h->chain_alb.
// With the lens lattice in effect (rtiow_set_guide_lens, lens_in_effect) guide_lens_kernel writes them instead, in either guide mode.
// While motion is in effect (rtiow_edit_scene on a handle with a base) surface_motion_kernel follows on the same layout and grid and writes
// the motion plane to h->motion_qc / h->motion_ids, sized by the current frame; the table it reads is rtiow_edit_scene's.  With edit
// influence on (rtiow_set_edit_influence, kappa > 0) edit_influence_kernel follows it, one lane per pixel in 16 x 16 workgroups: it writes
// lambda to h->edit_lambda and the fade over the carry of h->motion_qc, from the guides, the ids and rtiow_edit_scene's edit list.
template <class T, class Scene>
int launch_guides(rtiow_handle_s* h, const Scene& scene) {
    Launch<T> L{make_params<T>(h)};
    const int threads = 256;
    int rc = scene.template layout<T>(h, L, threads, false, false);
    if (rc) return rc;
    const size_t npix = local_pixels(h);
    HIP_TRY(h, h->guide_nd.ensure(npix * 4 * sizeof(T)));
    HIP_TRY(h, h->guide_alb.ensure(npix * 4 * sizeof(T)));
    const auto k = scene.by_source(L, [](auto src) { return guide_kernel<T, src>; });
    HIP_TRY(h, allow_lds(k, L.lds));
    const int tiles = ((L.p.cold.W + 7) / 8) * ((h->local_rows + 7) / 8);
    hipLaunchKernelGGL(k, dim3((unsigned)((tiles + 3) / 4)), dim3(threads), L.lds, h->stream, L.p, h->guide_nd.as<T>(), h->guide_alb.as<T>());
    HIP_TRY(h, hipGetLastError());
    if (lens_in_effect(h)) {
        HIP_TRY(h, h->chain_nd.ensure(npix * 4 * sizeof(T)));
        HIP_TRY(h, h->chain_alb.ensure(npix * 4 * sizeof(T)));
        const auto kl = scene.by_source(L, [](auto src) { return guide_lens_kernel<T, src>; });
        HIP_TRY(h, allow_lds(kl, L.lds));
        const bool chain = h->guide_mode == RTIOW_GUIDES_SPECULAR;   // RTIOW_GUIDES_FIRST_HIT: every chain ends at its first hit
        hipLaunchKernelGGL(kl, dim3((unsigned)((tiles + 3) / 4)), dim3(threads), L.lds, h->stream, L.p, h->guide_lens, chain ? h->guide_max_bounces : 0,
                           chain ? h->guide_max_fuzz : 0.0, h->chain_nd.as<T>(), h->chain_alb.as<T>());
        HIP_TRY(h, hipGetLastError());
    } else if (h->guide_mode == RTIOW_GUIDES_SPECULAR) {
        HIP_TRY(h, h->chain_nd.ensure(npix * 4 * sizeof(T)));
        HIP_TRY(h, h->chain_alb.ensure(npix * 4 * sizeof(T)));
        const auto kc = scene.by_source(L, [](auto src) { return guide_chain_kernel<T, src>; });
        HIP_TRY(h, allow_lds(kc, L.lds));
        hipLaunchKernelGGL(kc, dim3((unsigned)((tiles + 3) / 4)), dim3(threads), L.lds, h->stream, L.p, h->guide_max_bounces, h->guide_max_fuzz,
                           h->chain_nd.as<T>(), h->chain_alb.as<T>());
        HIP_TRY(h, hipGetLastError());
    }
    if (motion_in_effect(h->preview)) {
        HIP_TRY(h, h->motion_qc.ensure(npix * sizeof(Vec4<T>)));
        HIP_TRY(h, h->motion_ids.ensure(npix * sizeof(int32_t)));
        const auto km = scene.by_source(L, [](auto src) { return surface_motion_kernel<T, src>; });
        HIP_TRY(h, allow_lds(km, L.lds));
        hipLaunchKernelGGL(km, dim3((unsigned)((tiles + 3) / 4)), dim3(threads), L.lds, h->stream, L.p, h->motion_snap.as<const Vec4<T>>(),
                           (const int32_t*)h->motion_flags, h->motion_qc.as<Vec4<T>>(), (int32_t*)h->motion_ids);
        HIP_TRY(h, hipGetLastError());
        if (influence_in_effect(h->preview)) {
            HIP_TRY(h, h->edit_lambda.ensure(npix * sizeof(T)));
            if ((rc = rtiow_shared::enqueue_edit_influence(h))) return rc;
        }
    }
    on_guides_rendered(h->preview);
    return 0;
}

// The coverage layers of every local pixel (rtiow_render_coverage) into h->cov_ic / h->cov_nz: coverage_kernel on the layout and grid of
// launch_guides, with `grid` sub-samples per side (2 or 4: the caller has checked).
template <class T, class Scene>
int launch_coverage(rtiow_handle_s* h, const Scene& scene, int grid) {
    Launch<T> L{make_params<T>(h)};
    const int threads = 256;
    int rc = scene.template layout<T>(h, L, threads, false, false);
    if (rc) return rc;
    const size_t npix = local_pixels(h);
    HIP_TRY(h, h->cov_ic.ensure(npix * sizeof(int4)));
    HIP_TRY(h, h->cov_nz.ensure(npix * 2 * sizeof(Vec4<T>)));
    const auto k = scene.by_source(L, [](auto src) { return coverage_kernel<T, src>; });
    HIP_TRY(h, allow_lds(k, L.lds));
    const int tiles = ((L.p.cold.W + 7) / 8) * ((h->local_rows + 7) / 8);
    hipLaunchKernelGGL(k, dim3((unsigned)((tiles + 3) / 4)), dim3(threads), L.lds, h->stream, L.p, grid, h->cov_ic.as<int4>(), h->cov_nz.as<Vec4<T>>());
    HIP_TRY(h, hipGetLastError());
    on_coverage_rendered(h->preview, grid);
    return 0;
}

// The grid of the kernels that give every 16 x 16 pixels of the local frame a workgroup (the filters, the history, the plan).
inline dim3 frame_grid(int W, int rows) { return dim3((unsigned)((W + 15) / 16), (unsigned)((rows + 15) / 16)); }

// The accumulation's current records and counts: plain mode one count for all (counts = nullptr), adaptive mode the per-pixel array.
inline void accumulation_source(const rtiow_handle_s* h, const unsigned char*& mid, const int32_t*& counts, int& n_uniform) {
    mid = h->acc_mid[h->acc_cur];
    counts = h->preview.acc_mode == ACC_MODE_ADAPTIVE ? h->adapt_counts : nullptr;
    n_uniform = h->preview.acc_mode == ACC_MODE_ADAPTIVE ? 0 : h->preview.acc_samples;
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
// made the guides current.  The guides are the handle's filter guides (filter_nd / filter_alb), here and in launch_denoise_variance.
// from_history: level 0 reads the temporal colour plane h->hist_rgb instead (rtiow_denoise_history).
template <class T>
int launch_denoise(rtiow_handle_s* h, int levels, const double inv2[4], bool from_history = false) {
    const int W = img_w(h), rows = h->local_rows;
    const size_t npix = (size_t)W * rows;
    HIP_TRY(h, h->denoised.ensure(npix * 3 * sizeof(T)));
    for (int b = 0; b < 2 && b < levels - 1; ++b) HIP_TRY(h, h->dn_tmp[b].ensure(npix * 3 * sizeof(T)));
    const unsigned char* mid; const int32_t* counts; int n_uniform;
    accumulation_source(h, mid, counts, n_uniform);
    const dim3 grid = frame_grid(W, rows);
    for (int k = 0; k < levels; ++k) {
        FilterWeights<T> fw;
        fw.ic = (T)(inv2[0] * std::ldexp(1.0, 2 * k));
        fw.in = (T)inv2[1]; fw.ia = (T)inv2[2]; fw.iz = (T)inv2[3];
        const bool last = k == levels - 1;
        const bool records = k == 0 && !from_history;
        const T* cin = k == 0 ? (from_history ? h->hist_rgb.as<const T>() : nullptr) : h->dn_tmp[(k - 1) & 1].as<const T>();
        T* cout = (last ? h->denoised : h->dn_tmp[k & 1]).as<T>();
        hipLaunchKernelGGL(denoise_level_kernel<T>, grid, dim3(256), 0, h->stream, FrameShape{W, rows}, 1 << k, fw, records ? mid : nullptr,
                           counts, n_uniform, cin, filter_nd(h).as<const T>(), filter_alb(h).as<const T>(), cout, last ? 1 : 0);
        HIP_TRY(h, hipGetLastError());
    }
    on_denoised(h->preview, from_history ? DENOISED_FROM_TEMPORAL : DENOISED_FROM_ACCUMULATION);
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

// The constants of a reprojection from the current camera into the base (history_reproject_kernel, history_length_kernel).
template <class T>
HistoryParams<T> history_params(const rtiow_handle_s* h, double depth_tol, double normal_cos, double max_history) {
    const int W = img_w(h), rows = h->local_rows;
    const auto& c = camera<T>(h);
    HistoryParams<T> hp{};
    hp.O = {c.center[0], c.center[1], c.center[2]};
    hp.pixel00 = {c.pixel00_loc[0], c.pixel00_loc[1], c.pixel00_loc[2]};
    hp.du = {c.pixel_delta_u[0], c.pixel_delta_u[1], c.pixel_delta_u[2]};
    hp.dv = {c.pixel_delta_v[0], c.pixel_delta_v[1], c.pixel_delta_v[2]};
    hp.depth_tol = (T)depth_tol; hp.normal_cos = (T)normal_cos; hp.max_history = (T)max_history;
    const auto& b = [&]() -> const auto& { if constexpr (sizeof(T) == 4) return h->hist_cam32; else return h->hist_cam64; }();
    hp.have_base = h->preview.hist_base_ok && b.img_width == W && b.img_height == rows && history_constants<T>(b, hp) ? 1 : 0;
    return hp;
}

// history_reproject_kernel over the current accumulation and the base into h->hist_cm / h->hist_rgb (rtiow_history_update), or --
// clip_radius > 0 -- history_clip_kernel, the same with the neighbourhood clamp (rtiow_history_update_clipped), which writes the same two
// images.  h->hist_ctr holds two words: the pixels that carried history and those of them the clamp changed (0 without a clamp).  The caller
// has checked state and arguments -- clip_radius in 1..CLIP_MAX_RADIUS, which the kernel's LDS tile is sized for -- and made the guides current.
// While motion is in effect the guides came with the motion plane, and motion_reproject_kernel / motion_clip_kernel gather through it.
template <class T>
int launch_history(rtiow_handle_s* h, double depth_tol, double normal_cos, double max_history, int clip_radius = 0, double clip_gamma = 0) {
    const int W = img_w(h), rows = h->local_rows;
    const size_t npix = (size_t)W * rows;
    HIP_TRY(h, h->hist_cm.ensure(npix * 4 * sizeof(T)));
    HIP_TRY(h, h->hist_rgb.ensure(npix * 3 * sizeof(T)));
    HIP_TRY(h, h->hist_ctr.ensure(2 * sizeof(unsigned)));
    const HistoryParams<T> hp = history_params<T>(h, depth_tol, normal_cos, max_history);
    const unsigned char* mid; const int32_t* counts; int n_uniform;
    accumulation_source(h, mid, counts, n_uniform);
    HIP_TRY(h, hipMemsetAsync(h->hist_ctr, 0, 2 * sizeof(unsigned), h->stream));
    const auto guide = h->guide_nd.as<const Vec4<T>>(), base_hm = h->hist_base_hm.as<const Vec4<T>>(), base_nd = h->hist_base_nd.as<const Vec4<T>>();
    const auto motion = h->motion_qc.as<const Vec4<T>>();
    if (motion_in_effect(h->preview) && clip_radius > 0)
        hipLaunchKernelGGL(motion_clip_kernel<T>, frame_grid(W, rows), dim3(256), 0, h->stream, FrameShape{W, rows}, hp, clip_radius, (T)clip_gamma, mid, counts,
                           n_uniform, guide, base_hm, base_nd, motion, h->hist_cm.as<Vec4<T>>(), h->hist_rgb.as<T>(), (unsigned*)h->hist_ctr);
    else if (motion_in_effect(h->preview))
        hipLaunchKernelGGL(motion_reproject_kernel<T>, frame_grid(W, rows), dim3(256), 0, h->stream, FrameShape{W, rows}, hp, mid, counts, n_uniform,
                           guide, base_hm, base_nd, motion, h->hist_cm.as<Vec4<T>>(), h->hist_rgb.as<T>(), (unsigned*)h->hist_ctr);
    else if (clip_radius > 0)
        hipLaunchKernelGGL(history_clip_kernel<T>, frame_grid(W, rows), dim3(256), 0, h->stream, FrameShape{W, rows}, hp, clip_radius, (T)clip_gamma, mid, counts,
                           n_uniform, guide, base_hm, base_nd, h->hist_cm.as<Vec4<T>>(), h->hist_rgb.as<T>(), (unsigned*)h->hist_ctr);
    else
        hipLaunchKernelGGL(history_reproject_kernel<T>, frame_grid(W, rows), dim3(256), 0, h->stream, FrameShape{W, rows}, hp, mid, counts, n_uniform,
                           guide, base_hm, base_nd, h->hist_cm.as<Vec4<T>>(), h->hist_rgb.as<T>(), (unsigned*)h->hist_ctr);
    HIP_TRY(h, hipGetLastError());
    on_history_updated(h->preview);
    return 0;
}

// feedback_filter_kernel over the temporal image and the filter guides (rtiow_history_commit_filtered): {H', M} goes straight into
// h->hist_base_hm, the buffer of the old base, which is dead at a commit (the first commit of a handle, or one at a larger frame, gets
// its storage here).  inv2[4] = 1 / sigma^2 of colour, normal, albedo, depth (double), rounded to T here as launch_denoise's level 0
// does.  feedback == 1 is decided here: the kernel then stores the filtered colour itself.  The caller has checked state and arguments,
// made the guides current and makes the result the base.
template <class T>
int launch_feedback(rtiow_handle_s* h, const double inv2[4], double feedback) {
    const int W = img_w(h), rows = h->local_rows;
    const size_t npix = (size_t)W * rows;
    HIP_TRY(h, h->hist_base_hm.ensure(npix * 4 * sizeof(T)));
    FilterWeights<T> fw;
    fw.ic = (T)inv2[0]; fw.in = (T)inv2[1]; fw.ia = (T)inv2[2]; fw.iz = (T)inv2[3];
    hipLaunchKernelGGL(feedback_filter_kernel<T>, frame_grid(W, rows), dim3(256), 0, h->stream, FrameShape{W, rows}, fw, feedback == 1.0 ? 0 : 1, (T)feedback,
                       h->hist_cm.as<const Vec4<T>>(), filter_nd(h).as<const Vec4<T>>(), filter_alb(h).as<const Vec4<T>>(),
                       h->hist_base_hm.as<Vec4<T>>());
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// edge_resolve_kernel over the denoised image, in place (rtiow_resolve_edges): the coverage layers, the FIRST-HIT guides whatever the guide
// mode, and the count behind the image -- the history length of the temporal image when the filter read that, else the accumulation's
// counts.  inv2[2] = 1 / sigma^2 of normal and depth (double), rounded to T here; prior = +inf is decided here: the kernel then stores the
// rebuilt colour itself.  h->edge_ctr holds the number of pixels rewritten.  The caller has checked state and arguments -- radius in
// 1..EDGE_MAX_RADIUS -- and made the guides and the layers current.
template <class T>
int launch_edge_resolve(rtiow_handle_s* h, int radius, const double inv2[2], double prior) {
    const int W = img_w(h), rows = h->local_rows;
    HIP_TRY(h, h->edge_ctr.ensure(sizeof(unsigned)));
    HIP_TRY(h, hipMemsetAsync(h->edge_ctr, 0, sizeof(unsigned), h->stream));
    const bool temporal = h->preview.denoised_from == DENOISED_FROM_TEMPORAL;
    const unsigned char* mid; const int32_t* counts; int n_uniform;
    accumulation_source(h, mid, counts, n_uniform);
    const int grid = h->preview.coverage_grid;
    hipLaunchKernelGGL(edge_resolve_kernel<T>, frame_grid(W, rows), dim3(256), 0, h->stream, FrameShape{W, rows}, radius, grid * grid, (T)inv2[0], (T)inv2[1],
                       (T)prior, std::isinf(prior) ? 1 : 0, h->cov_ic.as<const int4>(), h->cov_nz.as<const Vec4<T>>(), h->guide_nd.as<const Vec4<T>>(),
                       temporal ? nullptr : counts, n_uniform, temporal ? h->hist_cm.as<const Vec4<T>>() : nullptr, h->denoised.as<T>(), (unsigned*)h->edge_ctr);
    HIP_TRY(h, hipGetLastError());
    on_edges_resolved(h->preview);
    return 0;
}

// What launch_upscale and launch_upscale_wide share.  source picks the colour (RTIOW_UPSCALE_*: the denoised image, the accumulation's
// records and counts, the temporal image); the guides are the FIRST-HIT buffers whatever the guide mode; inv2[3] = 1 / sigma^2 of normal,
// albedo, depth (double), rounded to T here.  h->upscale_ctr holds the number of output pixels the share decided, in UPSCALE_COUNTERS
// words that upscale_call sums.  The caller has checked state and arguments -- out_bytes is check_upscale_extent's -- and made the guides
// and, with use_coverage, the layers current.
template <class T>
struct UpscaleLaunch {
    Launch<T> L;
    UpscaleParams<T> u;         // all but tally_offset, which follows from the kernel's own LDS layout
    size_t own_offset = 0;      // where the kernel's own_lds bytes begin, behind the staged scene
    size_t lds = 0;             // own_offset + own_lds
};

// Parameters, the layout of launch_guides by the call's scene binding with the kernel's own_lds bytes behind it (lds_placement.h:
// place_own_lds), h->upscaled, the zeroed counters and u.  A scene that
// does not fit is refused here, before h->upscaled is touched: growing it loses the image of an earlier call, which stays readable.
template <class T, class Scene>
int prepare_upscale(rtiow_handle_s* h, const Scene& scene, UpscaleLaunch<T>& U, size_t own_lds, int factor, int source, const double inv2[3], int use_coverage, size_t out_bytes) {
    U.L = Launch<T>{make_params<T>(h)};
    int rc = scene.template layout<T>(h, U.L, 64 * UPSCALE_WAVES, false, false);
    if (rc) return rc;
    const OwnLds own = place_own_lds(U.L.lds, own_lds);
    U.own_offset = own.offset;
    U.lds = own.end;
    if (!own.fits) return fail_arg(h, RTIOW_E_BADARG, "scene too large for LDS staging; use RTIOW_SCENE_SCALAR");
    HIP_TRY(h, h->upscaled.ensure(out_bytes));
    constexpr size_t ctr_bytes = (size_t)UPSCALE_COUNTERS * UPSCALE_COUNTER_STRIDE * sizeof(unsigned);
    HIP_TRY(h, h->upscale_ctr.ensure(ctr_bytes));
    HIP_TRY(h, hipMemsetAsync(h->upscale_ctr, 0, ctr_bytes, h->stream));
    UpscaleParams<T> u{};
    u.F = factor; u.source = source; u.use_coverage = use_coverage;
    u.S = h->preview.coverage_grid * h->preview.coverage_grid;
    u.i_n = (T)inv2[0]; u.i_a = (T)inv2[1]; u.i_z = (T)inv2[2];
    if (source == RTIOW_UPSCALE_LINEAR) accumulation_source(h, u.mid, u.counts, u.n_uniform);
    if (source == RTIOW_UPSCALE_DENOISED) u.g = h->denoised.as<const T>();
    if (source == RTIOW_UPSCALE_HISTORY) u.cm = h->hist_cm.as<const Vec4<T>>();
    u.nd = h->guide_nd.as<const Vec4<T>>(); u.alb = h->guide_alb.as<const Vec4<T>>();
    u.ic = use_coverage ? h->cov_ic.as<const int4>() : nullptr;
    U.u = u;
    return 0;
}

// Behind the enqueue: the image is there, at this factor.
inline int finish_upscale(rtiow_handle_s* h, int factor, size_t out_bytes) {
    HIP_TRY(h, hipGetLastError());
    h->upscaled_bytes = out_bytes;
    on_upscaled(h->preview, factor);
    return 0;
}

// upscale_kernel over the traced frame into h->upscaled (rtiow_upscale; rtiow_upscale_large with the device grid's binding): one word per wave behind the staged scene for the count, one 8x8
// tile of the factor x larger image per wave.
template <class T, class Scene>
int launch_upscale(rtiow_handle_s* h, const Scene& scene, int factor, int source, const double inv2[3], int use_coverage, size_t out_bytes) {
    UpscaleLaunch<T> U;
    if (int rc = prepare_upscale<T>(h, scene, U, UPSCALE_TALLY_BYTES, factor, source, inv2, use_coverage, out_bytes)) return rc;
    U.u.tally_offset = (int)U.own_offset;
    const auto k = scene.by_source(U.L, [](auto src) { return upscale_kernel<T, src>; });
    HIP_TRY(h, allow_lds(k, U.lds));
    const int tiles = ((U.L.p.cold.W * factor + 7) / 8) * ((h->local_rows * factor + 7) / 8);
    hipLaunchKernelGGL(k, dim3((unsigned)((tiles + UPSCALE_WAVES - 1) / UPSCALE_WAVES)), dim3(64 * UPSCALE_WAVES), U.lds, h->stream, U.L.p, U.u, h->upscaled.as<T>(),
                       (unsigned*)h->upscale_ctr);
    return finish_upscale(h, factor, out_bytes);
}

// upscale_wide_kernel over the traced frame into h->upscaled (rtiow_upscale_wide; rtiow_upscale_wide_large with the device grid's binding): one workgroup of 256 per 16 x 16 block of the factor x
// larger image.  Behind the staged scene the LDS holds the block's footprint of traced pixels (upscale_wide_stage_bytes) and, behind that,
// the word per wave of the count.  check_upscale_extent's limits on 8 x 8 tiles hold a fortiori for 16 x 16 blocks.
template <class T, class Scene>
int launch_upscale_wide(rtiow_handle_s* h, const Scene& scene, int factor, int source, const double inv2[3], int use_coverage, size_t out_bytes) {
    UpscaleLaunch<T> U;
    if (int rc = prepare_upscale<T>(h, scene, U, upscale_wide_stage_bytes<T>() + UPSCALE_TALLY_BYTES, factor, source, inv2, use_coverage, out_bytes)) return rc;
    const size_t stage_offset = U.own_offset;
    U.u.tally_offset = (int)(stage_offset + upscale_wide_stage_bytes<T>());
    const auto k = scene.by_source(U.L, [](auto src) { return upscale_wide_kernel<T, src>; });
    HIP_TRY(h, allow_lds(k, U.lds));
    const int blocks = ((U.L.p.cold.W * factor + UPSCALE_WIDE_BLOCK - 1) / UPSCALE_WIDE_BLOCK) * ((h->local_rows * factor + UPSCALE_WIDE_BLOCK - 1) / UPSCALE_WIDE_BLOCK);
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * UPSCALE_WAVES), U.lds, h->stream, U.L.p, U.u, (int)stage_offset, h->upscaled.as<T>(), (unsigned*)h->upscale_ctr);
    return finish_upscale(h, factor, out_bytes);
}

// history_length_kernel over the current guides and the base into h->plan_m (rtiow_history_plan): the m of launch_history for the same
// tolerances, before any sample of the frame; the count of pixels with m > 0 goes to h->plan_ctr.  The caller has checked state and
// arguments and made the guides current.  While motion is in effect: motion_length_kernel, through the motion plane.
template <class T>
int launch_history_plan(rtiow_handle_s* h, double depth_tol, double normal_cos, double max_history) {
    const int W = img_w(h), rows = h->local_rows;
    const size_t npix = (size_t)W * rows;
    HIP_TRY(h, h->plan_m.ensure(npix * sizeof(T)));
    HIP_TRY(h, h->plan_ctr.ensure(sizeof(unsigned)));
    const HistoryParams<T> hp = history_params<T>(h, depth_tol, normal_cos, max_history);
    HIP_TRY(h, hipMemsetAsync(h->plan_ctr, 0, sizeof(unsigned), h->stream));
    if (motion_in_effect(h->preview))
        hipLaunchKernelGGL(motion_length_kernel<T>, frame_grid(W, rows), dim3(256), 0, h->stream, FrameShape{W, rows}, hp, h->guide_nd.as<const Vec4<T>>(),
                           h->hist_base_hm.as<const T>(), h->hist_base_nd.as<const Vec4<T>>(), h->motion_qc.as<const Vec4<T>>(), h->plan_m.as<T>(),
                           (unsigned*)h->plan_ctr);
    else
        hipLaunchKernelGGL(history_length_kernel<T>, frame_grid(W, rows), dim3(256), 0, h->stream, FrameShape{W, rows}, hp, h->guide_nd.as<const Vec4<T>>(),
                           h->hist_base_hm.as<const T>(), h->hist_base_nd.as<const Vec4<T>>(), h->plan_m.as<T>(), (unsigned*)h->plan_ctr);
    HIP_TRY(h, hipGetLastError());
    on_plan_written(h->preview);
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

// temporal_noise_kernel over the temporal image and the current accumulation into h->hist_var (level 0 of rtiow_denoise_history_variance,
// rtiow_read_history_variance).  The caller has checked that the temporal image is current and the accumulation the one its update read,
// and variance_radius in 1..NOISE_MAX_RADIUS, which the kernel's LDS tile is sized for.  Plain chunks keep no second moment: no counts.
template <class T>
int launch_temporal_noise(rtiow_handle_s* h, int variance_radius) {
    const int W = img_w(h), rows = h->local_rows;
    HIP_TRY(h, h->hist_var.ensure((size_t)W * rows * sizeof(T)));
    const int32_t* counts = h->preview.acc_mode == ACC_MODE_ADAPTIVE ? (const int32_t*)h->adapt_counts : nullptr;
    hipLaunchKernelGGL(temporal_noise_kernel<T>, frame_grid(W, rows), dim3(256), 0, h->stream, FrameShape{W, rows}, variance_radius, h->hist_cm.as<const Vec4<T>>(),
                       (const unsigned char*)h->acc_mid[h->acc_cur], counts, h->hist_var.as<T>());
    HIP_TRY(h, hipGetLastError());
    on_temporal_variance_written(h->preview);
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
// from_history (rtiow_denoise_history_variance): level 0 reads the temporal colour plane h->hist_rgb and the plane h->hist_var that
// launch_temporal_noise writes first, at variance_radius; the later levels are the same launches.
template <class T>
int launch_denoise_variance(rtiow_handle_s* h, int levels, double sigma_variance, const double inv2g[3], bool from_history = false, int variance_radius = 0) {
    const int W = img_w(h), rows = h->local_rows;
    const size_t npix = (size_t)W * rows;
    if (int rc = from_history ? launch_temporal_noise<T>(h, variance_radius) : launch_variance_plane<T>(h)) return rc;
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
    const dim3 grid = frame_grid(W, rows);
    // bit k: level k (step 1 << k, k < 3) stages its taps in LDS (variance_tile_kernel)
    const int tile_levels = tuned("RTIOW_TUNE_VARIANCE_TILE", sizeof(T) == 4 ? VARIANCE_TILE_LEVELS_F32 : VARIANCE_TILE_LEVELS_F64);
    for (int k = 0; k < levels; ++k) {
        fw.fk = (T)std::ldexp(1.0, 2 * k);
        const bool last = k == levels - 1;
        const T* cin = k == 0 ? (from_history ? h->hist_rgb.as<const T>() : nullptr) : h->dn_tmp[(k - 1) & 1].as<const T>();
        const T* vin = k == 0 ? (from_history ? h->hist_var : h->variance).as<const T>() : h->dn_var[(k - 1) & 1].as<const T>();
        T* cout = (last ? h->denoised : h->dn_tmp[k & 1]).as<T>();
        T* vout = last ? nullptr : h->dn_var[k & 1].as<T>();
        const bool tiled = k < 3 && ((tile_levels >> k) & 1);
        const size_t lds = tiled ? variance_tile_bytes<T>(1 << k) : 0;
        const auto kernel = tiled ? variance_tile_kernel<T> : variance_filter_kernel<T>;
        HIP_TRY(h, allow_lds(kernel, lds));
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, h->stream, FrameShape{W, rows}, 1 << k, fw, k == 0 && !from_history ? mid : nullptr,
                           (const int32_t*)h->adapt_counts, cin, vin, filter_nd(h).as<const T>(), filter_alb(h).as<const T>(), cout, vout, last ? 1 : 0);
        HIP_TRY(h, hipGetLastError());
    }
    on_denoised(h->preview, from_history ? DENOISED_FROM_TEMPORAL : DENOISED_FROM_ACCUMULATION);
    return 0;
}

}  // namespace
