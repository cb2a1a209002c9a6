// rtiow_large.hip -- large scenes: the fifth translation unit compiled for gfx950, linked
// into librtiow_hip.so beside the others.  It holds large_scene_kernel and its debug probe (device/hit_device_grid.h), the device grid's
// tables (library/device_grid.h: plan and blob), the launch and the entry points, and nothing else: the other code objects keep exactly
// the kernels they had.  The headers are library/unit.h's, as in every unit, with this unit's two behind them (internal linkage; templates
// this unit does not call are not instantiated here).
//
// Floating-point contract: rtiow_hip.hip's, the same flags.

#include "library/unit.h"
#include "device/hit_device_grid.h"
#include "library/device_grid.h"

namespace {

// The recentring point of the device grid: build_screen_table's (grid_plan.h's recentring_point, rounded to T) over the finite spheres.
// (The handle's own ctr is built only when an LDS source renders the scene.)
template <class T>
void large_centre(const rtiow_handle_s* h, double* ctr) {
    recentring_point(h->n, h->host_cr, true, ctr);
    for (int k = 0; k < 3; ++k) ctr[k] = (double)(T)ctr[k];
}

// Plan, blob and description of the device grid for the current scene, once per upload.  h->large_info.usable says whether the scene has one.
template <class T>
int ensure_large_grid(rtiow_handle_s* h) {
    if (!h->large_dirty) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    GridParams& g = h->large_grid;
    g = GridParams{};
    h->large_info = rtiow_large_grid_info{};
    HIP_TRY(h, hipStreamSynchronize(h->stream));          // a launch on the old blob may still be running
    HIP_TRY(h, h->large_blob.reset());
    const int m = h->n;
    large_centre<T>(h, h->large_ctr);
    const DeviceGridPlan pl = plan_device_grid(m, h->host_cr, h->large_ctr);
    if (pl.usable) {
        const DeviceGridBlob b = build_device_grid_blob<T>(pl, m, h->host_cr);
        if (b.bytes.size() >= 0x7fffffffull) return fail_arg(h, RTIOW_E_BADARG, "rtiow_render_large: the device grid of this scene exceeds 2 GiB; use rtiow_render");
        HIP_TRY(h, h->large_blob.ensure(b.bytes.size()));
        HIP_TRY(h, hipMemcpy(h->large_blob, b.bytes.data(), b.bytes.size(), hipMemcpyHostToDevice));
        fill_grid_params(g, pl);
        place_grid_blob(g, b, 0);
        g.blob = h->large_blob;
        g.blob_bytes = (int)b.bytes.size();
        rtiow_large_grid_info& o = h->large_info;
        o.usable = 1; o.nx = pl.nx; o.nz = pl.nz; o.cell = pl.cellf; o.rfar = pl.rfar; o.registered = pl.registered; o.direct = (int)pl.direct.size();
        o.index_entries = pl.indices.size(); o.longest_list = pl.longest; o.blob_bytes = b.bytes.size();
    }
    h->large_dirty = false;
    h->stats.scene_prepare_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

// The parameters and LDS layout of a launch over the device grid: the direct table and its ids at the start of LDS (stage_device_grid),
// the shade records behind them while they fit by layout_lds's rule, the drain scratch last.  The caller has found the grid usable.
template <class T>
void layout_large(const rtiow_handle_s* h, Launch<T>& L, int threads, bool persistent) {
    RenderParams<T>& p = L.p;
    const GridParams& g = h->large_grid;
    size_t lds = (size_t)g.n_direct_padded * 4 * sizeof(T) + (size_t)g.n_direct_padded * sizeof(int);       // a multiple of 16
    p.use_screen = 0; p.screen_offset = (int)lds;
    p.screen.geom_s = nullptr;
    p.screen.ctr_x = (T)h->large_ctr[0]; p.screen.ctr_y = (T)h->large_ctr[1]; p.screen.ctr_z = (T)h->large_ctr[2]; p.screen.omax2 = (T)0;
    const size_t waves_in_block = (size_t)((threads + 63) / 64);
    const size_t coop_bytes = persistent ? waves_in_block * COOP_SLOTS * sizeof(CoopSlot<T>) : 0;
    const size_t shade_bytes = (sizeof(T) * 12 * (size_t)h->n + 15) / 16 * 16;
    p.shade_offset = (int)lds;
    p.shade_in_lds = (lds + shade_bytes + coop_bytes <= 32 * 1024 && (lds + shade_bytes + coop_bytes) / waves_in_block <= 6656) ? 1 : 0;
    if (p.shade_in_lds) lds += shade_bytes;
    p.coop_offset = (int)lds;
    lds += coop_bytes;
    p.grid = g;
    p.use_grid = 1;            // persistent_body: the drain shares a sphere loop among idle lanes only while a ray's share of it is short
    L.lds = lds;
    L.lds_source = false;
    L.effective_source = RTIOW_SCENE_DEVICE_GRID;
}

// rtiow_render through the device grid: one persistent launch over the frame's tiles, samples [0, S) from the states of rtiow_init_rng.
template <class T>
int launch_render_large(rtiow_handle_s* h, bool timed, bool prepare_only) {
    Launch<T> L{make_params<T>(h)};
    RenderParams<T>& p = L.p;
    LaunchPlan P = new_plan(h, p);
    block_shape(0, false, p.cold.bx, p.cold.by, p.cold.wave_tiles);
    p.cold.clock_stamps = timed && h->clock_stamps_dev ? h->clock_stamps_dev + 4 : nullptr;
    layout_large<T>(h, L, 256, true);
    L.k = large_scene_kernel<T, false>;
    if constexpr (sizeof(T) == 4) L.kb = large_scene_kernel<T, true>;
    HIP_TRY(h, allow_lds(L.k, L.lds));
    HIP_TRY(h, h->work_counter.ensure(2 * sizeof(unsigned int)));
    if (int rc = size_persistent<T>(h, L, P, plan_tile_slots(p.cold.W, h->local_rows))) return rc;
    if (prepare_only) return 0;
    HIP_TRY(h, hipMemsetAsync(h->work_counter, 0, 2 * sizeof(unsigned int), h->stream));
    hipLaunchKernelGGL(L.k, dim3((unsigned)L.blocks), dim3(256), L.lds, h->stream, p);
    HIP_TRY(h, hipGetLastError());
    record_launch(h, L, plan_stats(P));
    h->stats.schedule = RTIOW_SCHED_PERSISTENT;
    h->stats.primary_rays = (uint64_t)h->local_rows * p.cold.W * (uint64_t)p.cold.S;
    h->stats.grid_nx = h->large_grid.nx; h->stats.grid_nz = h->large_grid.nz; h->stats.grid_cell = h->large_grid.cell;
    h->stats.grid_registered = h->large_info.registered; h->stats.grid_direct = h->large_info.direct;
    return 0;
}

#ifdef RTIOW_DEBUG_API
template <class T>
int launch_probe_large(rtiow_handle_s* h, int n, const T* rays, T* t_out, int* index_out, int* cells_out) {
    Launch<T> L{make_params<T>(h)};
    layout_large<T>(h, L, 256, true);
    HIP_TRY(h, allow_lds(large_hit_probe_kernel<T>, L.lds));
    const int blocks = std::min(2048, (n + 255) / 256);
    hipLaunchKernelGGL(large_hit_probe_kernel<T>, dim3(blocks), dim3(256), L.lds, h->stream, L.p, rays, n, t_out, index_out, cells_out);
    HIP_TRY(h, hipGetLastError());
    return 0;
}
#endif

const char* const LARGE_UNSUITED = ": the device grid does not suit this scene (too few spheres, or too many too big for a cell); use rtiow_render";

}  // namespace

extern "C" {

// ---- Large scenes
int rtiow_render_large(rtiow_handle h, float* kernel_ms) {
    if (!h) return RTIOW_E_BADARG;
    if (kernel_ms) *kernel_ms = 0;
    if (!h->preview.scene || !h->preview.have_camera) return fail_arg(h, RTIOW_E_BADARG, "rtiow_render_large before rtiow_set_scene/rtiow_set_camera");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = by_precision(h, [&](auto t) { return ensure_large_grid<decltype(t)>(h); })) return rc;
    if (!h->large_info.usable) { h->err = std::string("rtiow_render_large") + LARGE_UNSUITED; return RTIOW_E_BADARG; }
    PREVIEW_TRY(h, need_rng(h->preview, "rtiow_render_large"));
    int rc = ensure_framebuffer(h);
    if (rc) return rc;
    h->render_pending = false;
    if (h->local_rows == 0) { h->stats.render_ms = 0; h->stats.prepass_ms = 0; h->stats.main_ms = 0; return 0; }
    const bool timed = kernel_ms != nullptr;
    // allocations and occupancy queries before the start event, as in rtiow_render
    auto render = [&](bool prepare_only) { return by_precision(h, [&](auto t) { return launch_render_large<decltype(t)>(h, timed, prepare_only); }); };
    if ((rc = render(true))) return rc;
    if (h->clock_stamps) std::memset(h->clock_stamps, 0, 8 * sizeof(unsigned long long));
    if ((rc = timed_begin(h, kernel_ms))) return rc;
    if ((rc = render(false))) return rc;
    if ((rc = timed_end(h, kernel_ms))) return rc;
    if (timed) { h->stats.render_ms = *kernel_ms; h->stats.prepass_ms = 0; h->stats.main_ms = *kernel_ms; h->stats.place_ms = 0; }
    return 0;
}

int rtiow_read_large_grid(rtiow_handle h, rtiow_large_grid_info* out) {
    if (!h || !out) return RTIOW_E_BADARG;
    if (!h->preview.scene) return fail_arg(h, RTIOW_E_BADARG, "rtiow_read_large_grid before rtiow_set_scene");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = by_precision(h, [&](auto t) { return ensure_large_grid<decltype(t)>(h); })) return rc;
    *out = h->large_info;
    return 0;
}

#ifdef RTIOW_DEBUG_API
int rtiow_debug_large_grid_plan(int n, const double* center_radius, const double* centre3, int32_t* dims6, double* params8,
                                uint32_t* cells, size_t cells_cap, uint32_t* indices, size_t indices_cap, int32_t* direct, size_t direct_cap, double* halfwidth) {
    if (n <= 0 || !center_radius || !centre3 || !dims6 || !params8) return RTIOW_E_BADARG;
    const std::vector<double> cr(center_radius, center_radius + 4 * (size_t)n);
    const DeviceGridPlan pl = plan_device_grid(n, cr, centre3);                      // host only, no GPU needed
    dims6[0] = pl.nx; dims6[1] = pl.nz; dims6[2] = pl.registered; dims6[3] = (int)pl.direct.size(); dims6[4] = (int)pl.indices.size(); dims6[5] = pl.longest;
    params8[0] = pl.x0f; params8[1] = pl.z0f; params8[2] = pl.cellf; params8[3] = pl.ylo; params8[4] = pl.yhi; params8[5] = pl.rfar; params8[6] = pl.eps; params8[7] = pl.cmax_g;
    if (cells) { if (cells_cap < pl.cells.size()) return RTIOW_E_BADARG; std::copy(pl.cells.begin(), pl.cells.end(), cells); }
    if (indices) { if (indices_cap < pl.indices.size()) return RTIOW_E_BADARG; std::copy(pl.indices.begin(), pl.indices.end(), indices); }
    if (direct) { if (direct_cap < pl.direct.size()) return RTIOW_E_BADARG; std::copy(pl.direct.begin(), pl.direct.end(), direct); }
    if (halfwidth && !pl.halfwidth.empty()) std::copy(pl.halfwidth.begin(), pl.halfwidth.end(), halfwidth);
    return pl.usable ? 1 : 0;
}

int rtiow_debug_hit_world_large(rtiow_handle h, int n, const void* rays, void* t_out, int32_t* index_out, int32_t* cells_out) {
    if (!h || n <= 0 || !rays || !t_out || !index_out || !cells_out) return RTIOW_E_BADARG;
    PREVIEW_TRY(h, need_scene(h->preview, "rtiow_debug_hit_world_large"));
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = by_precision(h, [&](auto t) { return ensure_large_grid<decltype(t)>(h); })) return rc;
    if (!h->large_info.usable) { h->err = std::string("rtiow_debug_hit_world_large") + LARGE_UNSUITED; return RTIOW_E_BADARG; }
    const size_t es = elem_size(h);
    DeviceBuffer<> dr, dt;
    DeviceBuffer<int> di, dc;
    HIP_TRY(h, dr.ensure((size_t)n * 6 * es)); HIP_TRY(h, dt.ensure((size_t)n * es)); HIP_TRY(h, di.ensure((size_t)n * sizeof(int))); HIP_TRY(h, dc.ensure((size_t)n * sizeof(int)));
    HIP_TRY(h, hipMemcpy(dr, rays, (size_t)n * 6 * es, hipMemcpyHostToDevice));
    if (int rc = by_precision(h, [&](auto t) { using T = decltype(t); return launch_probe_large<T>(h, n, dr.as<const T>(), dt.as<T>(), di, dc); })) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(t_out, dt, (size_t)n * es, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(index_out, di, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(cells_out, dc, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}
#endif

}  // extern "C"
