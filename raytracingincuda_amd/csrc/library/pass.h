// pass.h -- what the entry points of the gfx950 translation units share around a timed pass: the events of kernel_ms and the copy of a
// result to the host; and upscale_call, the body of rtiow_upscale, rtiow_upscale_wide and their _large twins.
// Host side of librtiow_hip.so (internal linkage).
#pragma once
#include "handle.h"
#include "launch.h"             // UPSCALE_* (device/upscale.h)

namespace {

// kernel_ms: events around the work enqueued between timed_begin (or a launch that records ev0 itself) and timed_end (NULL: asynchronous,
// nothing recorded).
int timed_begin(rtiow_handle_s* h, float* kernel_ms) {
    h->render_pending = false;                           // the call reuses the start / stop events of rtiow_render_async
    if (kernel_ms) { *kernel_ms = 0; HIP_TRY(h, hipEventRecord(h->ev0, h->stream)); }
    return 0;
}
int timed_end(rtiow_handle_s* h, float* kernel_ms) {
    if (!kernel_ms) return 0;
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    HIP_TRY(h, hipEventElapsedTime(kernel_ms, h->ev0, h->ev1));
    return 0;
}

// D2H copy of `bytes` from a device buffer on the handle's stream, then wait.  A NULL host wanted the call's checks only.
int copy_out(rtiow_handle_s* h, void* host, const void* dev, size_t bytes) {
    if (!bytes || !host) return 0;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

// rtiow_upscale, rtiow_upscale_wide and their _large twins under the call's name (INTEGRATION.md sections 22, 23 and 26): the checks in their
// order, what the scene binding asks last of them (launch.h: StagedScene nothing; the device grid's a scene it suits), stale guides and
// -- with the share -- stale layers made current through the same binding inside kernel_ms, launch(inv2, out_bytes), and the count summed
// over its words.
template <class Scene, class LaunchFn>
int upscale_call(const char* call, const Scene& scene, rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth, int use_coverage,
                 float* kernel_ms, uint64_t* covered_pixels, LaunchFn launch) {
    if (!h) return RTIOW_E_BADARG;
    if (kernel_ms) *kernel_ms = 0;
    if (covered_pixels) *covered_pixels = 0;
    double inv2[3];
    PREVIEW_TRY(h, check_upscale(call, factor, UPSCALE_MIN_FACTOR, UPSCALE_MAX_FACTOR, source, RTIOW_UPSCALE_HISTORY + 1,
                                 {sigma_normal, sigma_albedo, sigma_depth}, use_coverage, inv2));
    PREVIEW_TRY(h, need_scene(h->preview, call));
    PREVIEW_TRY(h, need_unsharded(h->preview, call, true));
    if (source == RTIOW_UPSCALE_DENOISED) PREVIEW_TRY(h, need_denoised(h->preview, call));
    if (source == RTIOW_UPSCALE_LINEAR) PREVIEW_TRY(h, need_chunk(h->preview, call, ASKS_SCENE));
    if (source == RTIOW_UPSCALE_HISTORY) PREVIEW_TRY(h, need_temporal_image(h->preview, call, ASKS_SCENE));
    uint64_t out_bytes = 0;
    PREVIEW_TRY(h, check_upscale_extent(call, factor, img_w(h), h->local_rows, (int64_t)elem_size(h), &out_bytes));
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = scene.prepare(h, call);                     // the binding's refusal: behind the call's own, before anything changes
    if (rc) return rc;
    if ((rc = timed_begin(h, kernel_ms))) return rc;
    // stale guides and, with the share, stale layers first, inside kernel_ms: the library's own calls in their asynchronous form (their
    // kernels live in another unit's code object)
    if (!h->preview.guides_ok && (rc = scene.render_guides(h))) return rc;
    if (use_coverage && !h->preview.coverage_ok && (rc = scene.render_coverage(h, coverage_grid_or_default(h->preview)))) return rc;
    if ((rc = launch(inv2, (size_t)out_bytes))) return rc;
    if ((rc = timed_end(h, kernel_ms))) return rc;
    if (!covered_pixels) return 0;
    std::vector<unsigned> words((size_t)UPSCALE_COUNTERS * UPSCALE_COUNTER_STRIDE);     // the count is spread over UPSCALE_COUNTERS words (device/upscale.h)
    if ((rc = copy_out(h, words.data(), h->upscale_ctr, words.size() * sizeof(unsigned)))) return rc;
    for (int k = 0; k < UPSCALE_COUNTERS; ++k) *covered_pixels += words[(size_t)k * UPSCALE_COUNTER_STRIDE];
    return 0;
}

}  // namespace
