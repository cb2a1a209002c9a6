// rtiow_large_preview.hip -- the preview chain on large scenes: the sixth translation
// unit compiled for gfx950, linked into librtiow_hip.so beside the others.  It holds the chunk, guide and coverage kernels over the device
// grid of rtiow_render_large (device/hit_device_grid.h) -- the persistent ones as thin wrappers of persistent_body in the manner of
// large_scene_kernel, the tile kernels as the existing templates instantiated with RTIOW_SCENE_DEVICE_GRID --, the scene binding that
// hands them to the launches of library/launch.h, and the five entry points, whose bodies are library/scene_calls.h's: the twins', stated
// once.  The other code objects keep exactly the kernels they had; the kernels of a chunk and of the guides that read no scene stay in
// rtiow_hip.hip's (launch.h: rtiow_shared).
//
// Floating-point contract: rtiow_hip.hip's, the same flags.

#include "library/unit.h"
#include "device/hit_device_grid.h"
#include "library/device_grid.h"
#include "library/large_launch.h"
#include "library/scene_calls.h"

namespace {

// One chunk of progressive rendering and one adaptive chunk through the device grid: render_accumulate_kernel's and
// render_adaptive_kernel's body over RTIOW_SCENE_DEVICE_GRID.  No solo waves, as in large_scene_kernel.
template <class T, bool BOUND_F32>
__global__ void __launch_bounds__(1024) RT_MAIN_OCCUPANCY large_accumulate_kernel(const RenderParams<T> p) { persistent_body<T, RTIOW_SCENE_DEVICE_GRID, false, false, BOUND_F32, true>(p); }
template <class T, bool BOUND_F32>
__global__ void __launch_bounds__(1024) RT_MAIN_OCCUPANCY large_adaptive_kernel(const RenderParams<T> p) { persistent_body<T, RTIOW_SCENE_DEVICE_GRID, false, false, BOUND_F32, false, true>(p); }

// The scene binding of the _large calls (launch.h: StagedScene is the twins'): the device grid of the current scene, built at first use
// after an upload; a scene it does not suit is refused under the call's name with the twin's; layout_large; the kernels above and the
// tile kernels over RTIOW_SCENE_DEVICE_GRID.  rtiow_stats reports the source and the grid as rtiow_render_large does.
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
    template <class T, class SRC, class BOUNDED>
    RenderFn<T> accumulate_kernel(SRC, BOUNDED) const { return large_accumulate_kernel<T, BOUNDED::value>; }
    template <class T, class SRC, class BOUNDED>
    RenderFn<T> adaptive_kernel(SRC, BOUNDED) const { return large_adaptive_kernel<T, BOUNDED::value>; }
};

}  // namespace

extern "C" {

// ---- The preview chain on large scenes
int rtiow_accumulate_large(rtiow_handle h, int samples, float* kernel_ms) {
    if (!h) return RTIOW_E_BADARG;
    return accumulate_call(h, "rtiow_accumulate_large", DeviceGridScene{"rtiow_accumulate"}, samples, kernel_ms);
}

int rtiow_accumulate_adaptive_large(rtiow_handle h, int samples, int min_samples, double rel_error, int max_samples, float* kernel_ms, int* active_pixels) {
    if (!h) return RTIOW_E_BADARG;
    return adaptive_call(h, "rtiow_accumulate_adaptive_large", DeviceGridScene{"rtiow_accumulate_adaptive"}, samples, min_samples, rel_error, max_samples, kernel_ms, active_pixels);
}

int rtiow_accumulate_budget_large(rtiow_handle h, int samples, int min_samples, double target, int max_samples, float* kernel_ms, int* active_pixels) {
    if (!h) return RTIOW_E_BADARG;
    return budget_call(h, "rtiow_accumulate_budget_large", DeviceGridScene{"rtiow_accumulate_budget"}, samples, min_samples, target, max_samples, kernel_ms, active_pixels);
}

int rtiow_render_guides_large(rtiow_handle h, float* kernel_ms) {
    if (!h) return RTIOW_E_BADARG;
    return guides_call(h, "rtiow_render_guides_large", DeviceGridScene{"rtiow_render_guides"}, kernel_ms);
}

int rtiow_render_coverage_large(rtiow_handle h, int subsamples_per_side, float* kernel_ms) {
    if (!h) return RTIOW_E_BADARG;
    return coverage_call(h, "rtiow_render_coverage_large", DeviceGridScene{"rtiow_render_coverage"}, subsamples_per_side, kernel_ms);
}

}  // extern "C"
