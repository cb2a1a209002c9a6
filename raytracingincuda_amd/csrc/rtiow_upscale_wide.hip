// rtiow_upscale_wide.hip -- wide-support guided upscaling: the third translation unit
// compiled for gfx950, linked into librtiow_hip.so beside rtiow_hip.hip and rtiow_upscale.hip.  It holds upscale_wide_kernel
// (device/upscale_wide.h), its launch (library/launch.h: launch_upscale_wide) and the one entry point, and nothing else: the code objects
// of the other two units keep exactly the kernels they had.  The headers are rtiow_upscale.hip's, in its order, with the kernel's own
// behind them (internal linkage; templates it does not call are not instantiated here); stale guides and coverage layers are rendered
// through the C-ABI, by the kernels of rtiow_hip.hip, and the image is read by rtiow_upscale.hip's two readers.
//
// Floating-point contract: rtiow_hip.hip's, the same flags.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <array>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <mutex>
#include <vector>

#include "rtiow.h"
#ifdef RTIOW_DEBUG_API
#include "rtiow_debug.h"
#endif

#include "device/xorwow.h"
#include "device/params.h"
#include "device/probes.h"
#include "device/vecmath.h"
#include "device/sampling.h"
#include "device/roots.h"
#include "device/hit_loop.h"
#include "device/hit_grid.h"
#include "device/shade.h"
#include "device/hit_coop.h"
#include "device/pixel_io.h"
#include "device/render_kernels.h"
#include "device/cost_sort.h"
#include "device/denoise.h"
#include "device/denoise_variance.h"
#include "device/history.h"
#include "device/history_clip.h"
#include "device/history_feedback.h"
#include "device/history_budget.h"
#include "device/temporal_noise.h"
#include "device/guide_chain.h"
#include "device/edge_resolve.h"
#include "device/scene_motion.h"
#include "device/edit_influence.h"
#include "device/upscale.h"
#include "device/upscale_wide.h"
#include "library/xorwow_jump.h"
#include "library/handle.h"
#include "library/scene_tables.h"
#include "library/launch.h"
#include "library/pass.h"

extern "C" {

// ---- Wide-support guided upscaling: rtiow_upscale's checks, in its order, under this call's name
int rtiow_upscale_wide(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth, int use_coverage,
                       float* kernel_ms, uint64_t* covered_pixels) {
    if (!h) return RTIOW_E_BADARG;
    if (kernel_ms) *kernel_ms = 0;
    if (covered_pixels) *covered_pixels = 0;
    double inv2[3];
    PREVIEW_TRY(h, check_upscale("rtiow_upscale_wide", factor, UPSCALE_MIN_FACTOR, UPSCALE_MAX_FACTOR, source, RTIOW_UPSCALE_HISTORY + 1,
                                 {sigma_normal, sigma_albedo, sigma_depth}, use_coverage, inv2));
    PREVIEW_TRY(h, need_scene(h->preview, "rtiow_upscale_wide"));
    PREVIEW_TRY(h, need_unsharded(h->preview, "rtiow_upscale_wide", true));
    if (source == RTIOW_UPSCALE_DENOISED) PREVIEW_TRY(h, need_denoised(h->preview, "rtiow_upscale_wide"));
    if (source == RTIOW_UPSCALE_LINEAR) PREVIEW_TRY(h, need_chunk(h->preview, "rtiow_upscale_wide", ASKS_SCENE));
    if (source == RTIOW_UPSCALE_HISTORY) PREVIEW_TRY(h, need_temporal_image(h->preview, "rtiow_upscale_wide", ASKS_SCENE));
    uint64_t out_bytes = 0;
    PREVIEW_TRY(h, check_upscale_extent("rtiow_upscale_wide", factor, img_w(h), h->local_rows, (int64_t)elem_size(h), &out_bytes));
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = timed_begin(h, kernel_ms);
    if (rc) return rc;
    // stale guides and, with the share, stale layers first, inside kernel_ms: the library's own calls in their asynchronous form (their
    // kernels live in rtiow_hip.hip's code object)
    if (!h->preview.guides_ok && (rc = rtiow_render_guides(h, nullptr))) return rc;
    if (use_coverage && !h->preview.coverage_ok && (rc = rtiow_render_coverage(h, coverage_grid_or_default(h->preview), nullptr))) return rc;
    if ((rc = by_precision(h, [&](auto t) { return launch_upscale_wide<decltype(t)>(h, factor, source, inv2, use_coverage, (size_t)out_bytes); }))) return rc;
    if ((rc = timed_end(h, kernel_ms))) return rc;
    if (!covered_pixels) return 0;
    std::vector<unsigned> words((size_t)UPSCALE_COUNTERS * UPSCALE_COUNTER_STRIDE);     // the count is spread over UPSCALE_COUNTERS words (device/upscale.h)
    if (int rc = copy_out(h, words.data(), h->upscale_ctr, words.size() * sizeof(unsigned))) return rc;
    for (int k = 0; k < UPSCALE_COUNTERS; ++k) *covered_pixels += words[(size_t)k * UPSCALE_COUNTER_STRIDE];
    return 0;
}

}  // extern "C"
