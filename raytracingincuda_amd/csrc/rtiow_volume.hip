// rtiow_volume.hip -- volume scenes: the eighth translation unit compiled for gfx950,
// linked into librtiow_hip.so beside the others.  It holds volume_scene_kernel and its debug probe (device/hit_volume_grid.h), the
// volume grid's tables (library/volume_grid.h: plan and blob; library/volume_launch.h: their upload and the layout of a launch), the
// launch and the entry points, and nothing else: the other code objects keep exactly the kernels they had.  The headers are
// library/unit.h's, as in every unit, with this unit's three behind them (internal linkage; templates this unit does not call are not
// instantiated here).
//
// Floating-point contract: rtiow_hip.hip's, the same flags.

#include "library/unit.h"
#include "device/hit_volume_grid.h"
#include "library/volume_grid.h"
#include "library/volume_launch.h"

namespace {

// rtiow_render through the volume grid: one persistent launch over the frame's tiles, samples [0, S) from the states of rtiow_init_rng.
template <class T>
int launch_render_volume(rtiow_handle_s* h, bool timed, bool prepare_only) {
    Launch<T> L{make_params<T>(h)};
    RenderParams<T>& p = L.p;
    LaunchPlan P = new_plan(h, p);
    block_shape(0, false, p.cold.bx, p.cold.by, p.cold.wave_tiles);
    p.cold.clock_stamps = timed && h->clock_stamps_dev ? h->clock_stamps_dev + 4 : nullptr;
    layout_volume<T>(h, L, 256, true);
    L.k = volume_scene_kernel<T, false>;
    if constexpr (sizeof(T) == 4) L.kb = volume_scene_kernel<T, true>;
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
    record_volume_grid(h);
    return 0;
}

#ifdef RTIOW_DEBUG_API
template <class T>
int launch_probe_volume(rtiow_handle_s* h, int n, const T* rays, T* t_out, int* index_out, int* cells_out) {
    Launch<T> L{make_params<T>(h)};
    layout_volume<T>(h, L, 256, true);
    HIP_TRY(h, allow_lds(volume_hit_probe_kernel<T>, L.lds));
    const int blocks = std::min(2048, (n + 255) / 256);
    hipLaunchKernelGGL(volume_hit_probe_kernel<T>, dim3(blocks), dim3(256), L.lds, h->stream, L.p, rays, n, t_out, index_out, cells_out);
    HIP_TRY(h, hipGetLastError());
    return 0;
}
#endif

}  // namespace

extern "C" {

// ---- Volume scenes
int rtiow_render_volume(rtiow_handle h, float* kernel_ms) {
    if (!h) return RTIOW_E_BADARG;
    if (kernel_ms) *kernel_ms = 0;
    if (!h->preview.scene || !h->preview.have_camera) return fail_arg(h, RTIOW_E_BADARG, "rtiow_render_volume before rtiow_set_scene/rtiow_set_camera");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = by_precision(h, [&](auto t) { return ensure_volume_grid<decltype(t)>(h); })) return rc;
    if (!h->volume_info.usable) return refuse_unsuited_volume(h, "rtiow_render_volume", "rtiow_render");
    PREVIEW_TRY(h, need_rng(h->preview, "rtiow_render_volume"));
    int rc = ensure_framebuffer(h);
    if (rc) return rc;
    h->render_pending = false;
    if (h->local_rows == 0) { h->stats.render_ms = 0; h->stats.prepass_ms = 0; h->stats.main_ms = 0; return 0; }
    const bool timed = kernel_ms != nullptr;
    // allocations and occupancy queries before the start event, as in rtiow_render
    auto render = [&](bool prepare_only) { return by_precision(h, [&](auto t) { return launch_render_volume<decltype(t)>(h, timed, prepare_only); }); };
    if ((rc = render(true))) return rc;
    if (h->clock_stamps) std::memset(h->clock_stamps, 0, 8 * sizeof(unsigned long long));
    if ((rc = timed_begin(h, kernel_ms))) return rc;
    if ((rc = render(false))) return rc;
    if ((rc = timed_end(h, kernel_ms))) return rc;
    if (timed) { h->stats.render_ms = *kernel_ms; h->stats.prepass_ms = 0; h->stats.main_ms = *kernel_ms; h->stats.place_ms = 0; }
    return 0;
}

int rtiow_read_volume_grid(rtiow_handle h, rtiow_volume_grid_info* out) {
    if (!h || !out) return RTIOW_E_BADARG;
    if (!h->preview.scene) return fail_arg(h, RTIOW_E_BADARG, "rtiow_read_volume_grid before rtiow_set_scene");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = by_precision(h, [&](auto t) { return ensure_volume_grid<decltype(t)>(h); })) return rc;
    *out = h->volume_info;
    return 0;
}

#ifdef RTIOW_DEBUG_API
int rtiow_debug_volume_grid_plan(int n, const double* center_radius, const double* centre3, int64_t max_cells, int32_t* dims8, double* params8,
                                 uint32_t* cells, size_t cells_cap, uint32_t* indices, size_t indices_cap, int32_t* direct, size_t direct_cap, double* halfwidth) {
    if (n <= 0 || !center_radius || !centre3 || !dims8 || !params8 || max_cells > VOLUME_GRID_MAX_CELLS) return RTIOW_E_BADARG;   // a cap above the library's is none
    const std::vector<double> cr(center_radius, center_radius + 4 * (size_t)n);
    const VolumeGridPlan pl = plan_volume_grid(n, cr, centre3, max_cells > 0 ? (long long)max_cells : VOLUME_GRID_MAX_CELLS);      // host only, no GPU needed
    dims8[0] = pl.nx; dims8[1] = pl.ny; dims8[2] = pl.nz; dims8[3] = pl.registered; dims8[4] = (int)pl.direct.size(); dims8[5] = (int)pl.indices.size();
    dims8[6] = pl.longest; dims8[7] = (int)pl.occupied;
    params8[0] = pl.x0f; params8[1] = pl.y0f; params8[2] = pl.z0f; params8[3] = pl.cellf; params8[4] = pl.rfar; params8[5] = pl.eps; params8[6] = pl.cmax_g; params8[7] = 0;
    if (cells) { if (cells_cap < pl.cells.size()) return RTIOW_E_BADARG; std::copy(pl.cells.begin(), pl.cells.end(), cells); }
    if (indices) { if (indices_cap < pl.indices.size()) return RTIOW_E_BADARG; std::copy(pl.indices.begin(), pl.indices.end(), indices); }
    if (direct) { if (direct_cap < pl.direct.size()) return RTIOW_E_BADARG; std::copy(pl.direct.begin(), pl.direct.end(), direct); }
    if (halfwidth && !pl.halfwidth.empty()) std::copy(pl.halfwidth.begin(), pl.halfwidth.end(), halfwidth);
    return pl.usable ? 1 : 0;
}

int rtiow_debug_hit_world_volume(rtiow_handle h, int n, const void* rays, void* t_out, int32_t* index_out, int32_t* cells_out) {
    if (!h || n <= 0 || !rays || !t_out || !index_out || !cells_out) return RTIOW_E_BADARG;
    PREVIEW_TRY(h, need_scene(h->preview, "rtiow_debug_hit_world_volume"));
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = by_precision(h, [&](auto t) { return ensure_volume_grid<decltype(t)>(h); })) return rc;
    if (!h->volume_info.usable) return refuse_unsuited_volume(h, "rtiow_debug_hit_world_volume", "rtiow_render");
    const size_t es = elem_size(h);
    DeviceBuffer<> dr, dt;
    DeviceBuffer<int> di, dc;
    HIP_TRY(h, dr.ensure((size_t)n * 6 * es)); HIP_TRY(h, dt.ensure((size_t)n * es)); HIP_TRY(h, di.ensure((size_t)n * sizeof(int))); HIP_TRY(h, dc.ensure((size_t)n * sizeof(int)));
    HIP_TRY(h, hipMemcpy(dr, rays, (size_t)n * 6 * es, hipMemcpyHostToDevice));
    if (int rc = by_precision(h, [&](auto t) { using T = decltype(t); return launch_probe_volume<T>(h, n, dr.as<const T>(), dt.as<T>(), di, dc); })) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(t_out, dt, (size_t)n * es, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(index_out, di, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(cells_out, dc, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}
#endif

}  // extern "C"
