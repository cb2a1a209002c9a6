// scene_calls.h -- the bodies of the entry points that trace the scene into the preview chain's buffers, each stated once for every scene
// binding (launch.h: StagedScene; rtiow_large_preview.hip: the device grid's): a plain chunk (rtiow_accumulate, rtiow_accumulate_large),
// an adaptive or budget chunk (rtiow_accumulate_adaptive, rtiow_accumulate_budget and their _large twins), the guides (rtiow_render_guides,
// rtiow_render_guides_large) and the coverage layers (rtiow_render_coverage, rtiow_render_coverage_large): the checks in their order under
// the call's name, the answers of a rank without rows, the transitions of preview_state.h and the times.
// Host side of librtiow_hip.so; part of rtiow_hip.hip and rtiow_large_preview.hip (internal linkage).
#pragma once
#include "handle.h"
#include "launch.h"
#include "pass.h"

namespace {

// The times a render call on a shard without rows reports.
void zero_times(rtiow_handle_s* h) { h->stats.render_ms = 0; h->stats.prepass_ms = 0; h->stats.main_ms = 0; }

// One plain chunk under the name `call`.
template <class Scene>
int accumulate_call(rtiow_handle_s* h, const char* call, const Scene& scene, int samples, float* kernel_ms) {
    PREVIEW_TRY(h, need_scene(h->preview, call));
    PREVIEW_TRY(h, need_rng(h->preview, call));
    if (samples <= 0 || samples > 0x7fffffff - h->preview.acc_samples)
        return fail_arg(h, RTIOW_E_BADARG, (std::string(call) + ": samples must be > 0 and keep the total below 2^31").c_str());
    PREVIEW_TRY(h, need_no_chunk_of(h->preview, call, ACC_MODE_ADAPTIVE));
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = scene.prepare(h, call);
    if (rc) return rc;
    if ((rc = ensure_framebuffer(h))) return rc;
    h->render_pending = false;                           // the chunk reuses the start / stop events of rtiow_render_async
    if (kernel_ms) *kernel_ms = 0;
    on_chunk_begin(h->preview);
    if (h->local_rows == 0) { zero_times(h); on_plain_chunk(h->preview, samples); return 0; }
    const bool timed = kernel_ms != nullptr;
    if (h->clock_stamps) std::memset(h->clock_stamps, 0, 8 * sizeof(unsigned long long));
    if ((rc = by_precision(h, [&](auto t) { return launch_accumulate<decltype(t)>(h, scene, samples, timed); }))) return rc;
    on_plain_chunk(h->preview, samples);
    h->stats.prepass_ms = 0; h->stats.place_ms = 0;
    if (timed) {                                         // the start event: launch_accumulate, behind its allocations
        if ((rc = timed_end(h, kernel_ms))) return rc;
        h->stats.render_ms = *kernel_ms; h->stats.main_ms = *kernel_ms;
    }
    return 0;
}

// What the adaptive and the budget chunk (`call`) share: the checks (rule_ok, rule_text: the rule's own argument), the chunk and its times.
template <class Scene>
int adaptive_chunk(rtiow_handle_s* h, const char* call, const Scene& scene, int samples, int min_samples, AdaptiveRule rule, bool rule_ok, const char* rule_text,
                   int max_samples, float* kernel_ms, int* active_pixels) {
    if (active_pixels) *active_pixels = 0;
    if (kernel_ms) *kernel_ms = 0;
    PREVIEW_TRY(h, need_scene(h->preview, call));
    PREVIEW_TRY(h, need_rng(h->preview, call));
    if (samples <= 0 || min_samples < 0 || max_samples < min_samples || !rule_ok)
        return fail_arg(h, RTIOW_E_BADARG, (std::string(call) + ": need samples > 0, 0 <= min_samples <= max_samples, " + rule_text).c_str());
    if (!plan_order_fits(img_w(h), h->local_rows))
        return fail_arg(h, RTIOW_E_BADARG, (std::string(call) + ": frames wider than 65535 or with more than 32767 local rows are not supported").c_str());
    PREVIEW_TRY(h, need_no_chunk_of(h->preview, call, ACC_MODE_PLAIN));
    if (rule.budget) PREVIEW_TRY(h, need_plan(h->preview, call));
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = scene.prepare(h, call);
    if (rc) return rc;
    if ((rc = ensure_framebuffer(h))) return rc;
    h->render_pending = false;                           // the chunk reuses the events of rtiow_render_async
    on_chunk_begin(h->preview);
    if (h->local_rows == 0) { zero_times(h); h->stats.primary_rays = 0; on_adaptive_chunk(h->preview); return 0; }
    const bool timed = kernel_ms != nullptr;
    if (h->clock_stamps) std::memset(h->clock_stamps, 0, 8 * sizeof(unsigned long long));
    int active = 0;
    rc = by_precision(h, [&](auto t) { return launch_adaptive<decltype(t)>(h, scene, samples, min_samples, rule, max_samples, timed, active); });
    if (rc) return rc;
    on_adaptive_chunk(h->preview);
    if (active_pixels) *active_pixels = active;
    h->stats.prepass_ms = 0; h->stats.place_ms = 0;
    if (timed) {
        HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
        HIP_TRY(h, hipEventSynchronize(h->ev1));
        float a = 0, b = 0;
        HIP_TRY(h, hipEventElapsedTime(&a, h->ev0, h->ev_a));
        HIP_TRY(h, hipEventElapsedTime(&b, h->ev_b, h->ev1));
        *kernel_ms = a + b;
        h->stats.render_ms = a + b; h->stats.main_ms = a + b;
    }
    return 0;
}
template <class Scene>
int adaptive_call(rtiow_handle_s* h, const char* call, const Scene& scene, int samples, int min_samples, double rel_error, int max_samples, float* kernel_ms, int* active_pixels) {
    return adaptive_chunk(h, call, scene, samples, min_samples, AdaptiveRule{false, rel_error, 0.0}, rel_error >= 0, "rel_error >= 0", max_samples, kernel_ms, active_pixels);
}
template <class Scene>
int budget_call(rtiow_handle_s* h, const char* call, const Scene& scene, int samples, int min_samples, double target, int max_samples, float* kernel_ms, int* active_pixels) {
    return adaptive_chunk(h, call, scene, samples, min_samples, AdaptiveRule{true, 0.0, target}, target > 0, "target > 0 (+inf: everybody)", max_samples, kernel_ms, active_pixels);
}

// The guides of every local pixel, and what launch_guides renders with them, under the name `call`.
template <class Scene>
int guides_call(rtiow_handle_s* h, const char* call, const Scene& scene, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0;
    PREVIEW_TRY(h, need_scene(h->preview, call));
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = scene.prepare(h, call);
    if (rc) return rc;
    if (h->local_rows == 0) { on_guides_rendered(h->preview); return 0; }
    if ((rc = timed_begin(h, kernel_ms))) return rc;
    if ((rc = by_precision(h, [&](auto t) { return launch_guides<decltype(t)>(h, scene); }))) return rc;
    return timed_end(h, kernel_ms);
}

// The coverage layers of every local pixel under the name `call`.
template <class Scene>
int coverage_call(rtiow_handle_s* h, const char* call, const Scene& scene, int subsamples_per_side, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0;
    PREVIEW_TRY(h, check_coverage_grid(call, subsamples_per_side));
    PREVIEW_TRY(h, need_scene(h->preview, call));
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = scene.prepare(h, call);
    if (rc) return rc;
    if (h->local_rows == 0) { on_coverage_rendered(h->preview, subsamples_per_side); return 0; }
    if ((rc = timed_begin(h, kernel_ms))) return rc;
    if ((rc = by_precision(h, [&](auto t) { return launch_coverage<decltype(t)>(h, scene, subsamples_per_side); }))) return rc;
    return timed_end(h, kernel_ms);
}

}  // namespace
