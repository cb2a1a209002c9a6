// large_launch.h -- what the launches over the device grid share (INTEGRATION.md sections 24 and 25): the grid of the current scene built
// once per upload (ensure_large_grid), the parameters and LDS layout of a launch over it (layout_large), the refusal of a scene it does
// not suit, the grid_* fields of rtiow_stats and the scene binding that hands all of it to the launches of launch.h (DeviceGridScene).
// Host side of librtiow_hip.so; part of rtiow_large.hip, rtiow_large_preview.hip and rtiow_large_upscale.hip,
// behind library/unit.h, device/hit_device_grid.h and library/device_grid.h (internal linkage).
#pragma once
#include "handle.h"
#include "launch.h"
#include "device_grid.h"

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

// The parameters and LDS layout of a launch over the device grid (lds_placement.h: place_large_lds): the direct table and its ids at the
// start of LDS (stage_device_grid), the shade records behind them while they fit by layout_lds's rule, the drain scratch last (persistent
// launches only: the tile kernels of the guides, the coverage layers and the upscalers have none, as layout_lds(..., persistent = false)
// has none).  The caller has found the grid usable.
template <class T>
void layout_large(const rtiow_handle_s* h, Launch<T>& L, int threads, bool persistent) {
    RenderParams<T>& p = L.p;
    const GridParams& g = h->large_grid;
    const size_t waves_in_block = (size_t)((threads + 63) / 64);
    const LargeLds at = place_large_lds(g.n_direct_padded, sizeof(T), h->n, threads, persistent ? waves_in_block * COOP_SLOTS * sizeof(CoopSlot<T>) : 0);
    p.use_screen = 0; p.screen_offset = (int)at.direct_bytes;
    p.screen.geom_s = nullptr;
    p.screen.ctr_x = (T)h->large_ctr[0]; p.screen.ctr_y = (T)h->large_ctr[1]; p.screen.ctr_z = (T)h->large_ctr[2]; p.screen.omax2 = (T)0;
    p.shade_offset = (int)at.shade_offset;
    p.shade_in_lds = at.shade_in_lds ? 1 : 0;
    p.coop_offset = (int)at.coop_offset;
    p.grid = g;
    p.use_grid = 1;            // persistent_body: the drain shares a sphere loop among idle lanes only while a ray's share of it is short
    L.lds = at.lds;
    L.lds_source = false;
    L.effective_source = RTIOW_SCENE_DEVICE_GRID;
}

// The grid_* fields of rtiow_stats after a launch over the device grid.
inline void record_large_grid(rtiow_handle_s* h) {
    h->stats.grid_nx = h->large_grid.nx; h->stats.grid_nz = h->large_grid.nz; h->stats.grid_cell = h->large_grid.cell;
    h->stats.grid_registered = h->large_info.registered; h->stats.grid_direct = h->large_info.direct;
}

// A scene the device grid does not suit is refused under the call's name, with the call that renders it: never rendered another way.
const char* const LARGE_UNSUITED = ": the device grid does not suit this scene (too few spheres, or too many too big for a cell); use ";
inline int refuse_unsuited(rtiow_handle_s* h, const char* call, const char* twin) {
    h->err = std::string(call) + LARGE_UNSUITED + twin;
    return RTIOW_E_BADARG;
}

// The scene binding of the _large calls (launch.h: StagedScene is the twins'): the device grid of the current scene, built at first use
// after an upload; a scene it does not suit is refused under the call's name with the twin's; layout_large; the tile kernels over
// RTIOW_SCENE_DEVICE_GRID; stale guides and layers made current through the grid as well.  rtiow_stats reports the source and the grid
// as rtiow_render_large does.  The persistent kernels of a chunk are added where they live (rtiow_large_preview.hip).
struct DeviceGridScene {
    const char* twin;
    int prepare(rtiow_handle_s* h, const char* call) const {
        if (int rc = by_precision(h, [&](auto t) { return ensure_large_grid<decltype(t)>(h); })) return rc;
        if (!h->large_info.usable) return refuse_unsuited(h, call, twin);
        return 0;
    }
    template <class T>
    int layout(rtiow_handle_s* h, Launch<T>& L, int threads, bool persistent, bool) const {
        layout_large<T>(h, L, threads, persistent);
        h->stats.scene_source = L.effective_source;
        record_large_grid(h);
        return 0;
    }
    template <class T, class F>
    auto by_source(const Launch<T>&, F f) const { return f(std::integral_constant<int, RTIOW_SCENE_DEVICE_GRID>()); }
    int render_guides(rtiow_handle_s* h) const { return rtiow_render_guides_large(h, nullptr); }
    int render_coverage(rtiow_handle_s* h, int subsamples_per_side) const { return rtiow_render_coverage_large(h, subsamples_per_side, nullptr); }
};

}  // namespace
