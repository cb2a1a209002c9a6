// volume_launch.h -- what the launches over the volume grid share: the three-axis grid of the current scene
// built once per upload (ensure_volume_grid), the parameters and LDS layout of a launch over it (layout_volume), the refusal of a scene
// it does not suit, the grid_* fields of rtiow_stats and the scene binding that hands all of it to the launches of launch.h, shaped like
// large_launch.h's DeviceGridScene (VolumeGridScene).  Host side of librtiow_hip.so; part of rtiow_volume.hip,
// rtiow_volume_preview.hip and rtiow_volume_upscale.hip, behind library/unit.h, device/hit_volume_grid.h and library/volume_grid.h
// (internal linkage).
#pragma once
#include "handle.h"
#include "launch.h"
#include "volume_grid.h"

namespace {

// Plan, blob and description of the volume grid for the current scene, once per upload.  h->volume_info.usable says whether the scene
// has one.  The recentring point is the device grid's: grid_plan.h's recentring_point over the finite spheres, rounded to T.
template <class T>
int ensure_volume_grid(rtiow_handle_s* h) {
    if (!h->volume_dirty) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    GridParams& g = h->volume_grid;
    g = GridParams{};
    h->volume_info = rtiow_volume_grid_info{};
    HIP_TRY(h, hipStreamSynchronize(h->stream));          // a launch on the old blob may still be running
    HIP_TRY(h, h->volume_blob.reset());
    const int m = h->n;
    recentring_point(m, h->host_cr, true, h->volume_ctr);
    for (int k = 0; k < 3; ++k) h->volume_ctr[k] = (double)(T)h->volume_ctr[k];
    const VolumeGridPlan pl = plan_volume_grid(m, h->host_cr, h->volume_ctr);
    if (pl.usable) {
        const VolumeGridBlob b = build_volume_grid_blob<T>(pl, m, h->host_cr);
        if (b.bytes.size() >= 0x7fffffffull) return fail_arg(h, RTIOW_E_BADARG, "rtiow_render_volume: the volume grid of this scene exceeds 2 GiB; use rtiow_render");
        HIP_TRY(h, h->volume_blob.ensure(b.bytes.size()));
        HIP_TRY(h, hipMemcpy(h->volume_blob, b.bytes.data(), b.bytes.size(), hipMemcpyHostToDevice));
        fill_volume_grid_params(g, pl);
        place_grid_blob(g, b, 0);
        g.blob = h->volume_blob;
        g.blob_bytes = (int)b.bytes.size();
        rtiow_volume_grid_info& o = h->volume_info;
        o.usable = 1; o.nx = pl.nx; o.ny = pl.ny; o.nz = pl.nz; o.cell = pl.cellf; o.rfar = pl.rfar; o.registered = pl.registered; o.direct = (int)pl.direct.size();
        o.index_entries = pl.indices.size(); o.occupied_cells = pl.occupied; o.longest_list = pl.longest; o.blob_bytes = b.bytes.size();
    }
    h->volume_dirty = false;
    h->stats.scene_prepare_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

// The parameters and LDS layout of a launch over the volume grid: layout_large's, by place_large_lds as it is -- the direct table and its
// ids at the start of LDS (stage_device_grid), the shade records behind them while they fit, the drain scratch last (persistent launches
// only).  The caller has found the grid usable.
template <class T>
void layout_volume(const rtiow_handle_s* h, Launch<T>& L, int threads, bool persistent) {
    RenderParams<T>& p = L.p;
    const GridParams& g = h->volume_grid;
    const size_t waves_in_block = (size_t)((threads + 63) / 64);
    const LargeLds at = place_large_lds(g.n_direct_padded, sizeof(T), h->n, threads, persistent ? waves_in_block * COOP_SLOTS * sizeof(CoopSlot<T>) : 0);
    p.use_screen = 0; p.screen_offset = (int)at.direct_bytes;
    p.screen.geom_s = nullptr;
    p.screen.ctr_x = (T)h->volume_ctr[0]; p.screen.ctr_y = (T)h->volume_ctr[1]; p.screen.ctr_z = (T)h->volume_ctr[2]; p.screen.omax2 = (T)0;
    p.shade_offset = (int)at.shade_offset;
    p.shade_in_lds = at.shade_in_lds ? 1 : 0;
    p.coop_offset = (int)at.coop_offset;
    p.grid = g;
    p.use_grid = 1;            // persistent_body: the drain shares a sphere loop among idle lanes only while a ray's share of it is short
    L.lds = at.lds;
    L.lds_source = false;
    L.effective_source = RTIOW_SCENE_VOLUME_GRID;
}

// The grid_* fields of rtiow_stats after a launch over the volume grid (ny: rtiow_read_volume_grid).
inline void record_volume_grid(rtiow_handle_s* h) {
    h->stats.grid_nx = h->volume_grid.nx; h->stats.grid_nz = h->volume_grid.nz; h->stats.grid_cell = h->volume_grid.cell;
    h->stats.grid_registered = h->volume_info.registered; h->stats.grid_direct = h->volume_info.direct;
}

// A scene the volume grid does not suit is refused under the call's name, with the call that renders it: never rendered another way.
const char* const VOLUME_UNSUITED = ": the volume grid does not suit this scene (too few spheres, or too many too big for a cell); use ";
inline int refuse_unsuited_volume(rtiow_handle_s* h, const char* call, const char* twin) {
    h->err = std::string(call) + VOLUME_UNSUITED + twin;
    return RTIOW_E_BADARG;
}

// The scene binding of the _volume calls (launch.h: StagedScene is the twins', large_launch.h: DeviceGridScene the _large calls'): the
// volume grid of the current scene, built at first use after an upload; a scene it does not suit is refused under the call's name with
// the twin's; layout_volume; the tile kernels over RTIOW_SCENE_VOLUME_GRID; stale guides and layers made current through the volume
// grid as well.  rtiow_stats reports the source and the grid as rtiow_render_volume does.  device/upscale_wide.h skips its own barrier
// for this source by name, as for RTIOW_SCENE_DEVICE_GRID: stage_device_grid, which stages both, ends in one.  The persistent kernels
// of a chunk are added where they live (rtiow_volume_preview.hip); rtiow_render_volume stays a persistent launch of its own.
struct VolumeGridScene {
    const char* twin;
    int prepare(rtiow_handle_s* h, const char* call) const {
        if (int rc = by_precision(h, [&](auto t) { return ensure_volume_grid<decltype(t)>(h); })) return rc;
        if (!h->volume_info.usable) return refuse_unsuited_volume(h, call, twin);
        return 0;
    }
    template <class T>
    int layout(rtiow_handle_s* h, Launch<T>& L, int threads, bool persistent, bool) const {
        layout_volume<T>(h, L, threads, persistent);
        h->stats.scene_source = L.effective_source;
        record_volume_grid(h);
        return 0;
    }
    template <class T, class F>
    auto by_source(const Launch<T>&, F f) const { return f(std::integral_constant<int, RTIOW_SCENE_VOLUME_GRID>()); }
    int render_guides(rtiow_handle_s* h) const { return rtiow_render_guides_volume(h, nullptr); }
    int render_coverage(rtiow_handle_s* h, int subsamples_per_side) const { return rtiow_render_coverage_volume(h, subsamples_per_side, nullptr); }
};

}  // namespace
