// rtiow_volume_preview.hip -- the preview chain on volume scenes: the ninth translation
// unit compiled for gfx950, linked into librtiow_hip.so beside the others.  It holds the chunk, guide and coverage kernels over the
// volume grid of rtiow_render_volume (device/hit_volume_grid.h) -- the persistent ones as thin wrappers of persistent_body in the manner
// of large_accumulate_kernel, the tile kernels as the existing templates instantiated with RTIOW_SCENE_VOLUME_GRID --, the scene binding
// that hands them to the launches of library/launch.h, and the five entry points, whose bodies are library/scene_calls.h's: the twins',
// stated once.  There is no hit_world of its own here: the walk, the staging and the exact-loop fallback are rtiow_render_volume's.  The
// other code objects keep exactly the kernels they had; the kernels of a chunk and of the guides that read no scene stay in
// rtiow_hip.hip's (launch.h: rtiow_shared).
//
// Floating-point contract: rtiow_hip.hip's, the same flags.

#include "library/unit.h"
#include "device/hit_volume_grid.h"
#include "library/volume_grid.h"
#include "library/volume_launch.h"
#include "library/scene_calls.h"

namespace {

// One chunk of progressive rendering and one adaptive chunk through the volume grid: render_accumulate_kernel's and
// render_adaptive_kernel's body over RTIOW_SCENE_VOLUME_GRID.  No solo waves, as in volume_scene_kernel.
template <class T, bool BOUND_F32>
__global__ void __launch_bounds__(1024) RT_MAIN_OCCUPANCY volume_accumulate_kernel(const RenderParams<T> p) { persistent_body<T, RTIOW_SCENE_VOLUME_GRID, false, false, BOUND_F32, true>(p); }
template <class T, bool BOUND_F32>
__global__ void __launch_bounds__(1024) RT_MAIN_OCCUPANCY volume_adaptive_kernel(const RenderParams<T> p) { persistent_body<T, RTIOW_SCENE_VOLUME_GRID, false, false, BOUND_F32, false, true>(p); }

// The scene binding of the chunks, guides and layers over the volume grid: library/volume_launch.h's VolumeGridScene with the persistent
// kernels above.
struct VolumeGridChunks : VolumeGridScene {
    template <class T, class SRC, class BOUNDED>
    RenderFn<T> accumulate_kernel(SRC, BOUNDED) const { return volume_accumulate_kernel<T, BOUNDED::value>; }
    template <class T, class SRC, class BOUNDED>
    RenderFn<T> adaptive_kernel(SRC, BOUNDED) const { return volume_adaptive_kernel<T, BOUNDED::value>; }
};

}  // namespace

extern "C" {

// ---- The preview chain on volume scenes
int rtiow_accumulate_volume(rtiow_handle h, int samples, float* kernel_ms) {
    if (!h) return RTIOW_E_BADARG;
    return accumulate_call(h, "rtiow_accumulate_volume", VolumeGridChunks{{"rtiow_accumulate"}}, samples, kernel_ms);
}

int rtiow_accumulate_adaptive_volume(rtiow_handle h, int samples, int min_samples, double rel_error, int max_samples, float* kernel_ms, int* active_pixels) {
    if (!h) return RTIOW_E_BADARG;
    return adaptive_call(h, "rtiow_accumulate_adaptive_volume", VolumeGridChunks{{"rtiow_accumulate_adaptive"}}, samples, min_samples, rel_error, max_samples, kernel_ms, active_pixels);
}

int rtiow_accumulate_budget_volume(rtiow_handle h, int samples, int min_samples, double target, int max_samples, float* kernel_ms, int* active_pixels) {
    if (!h) return RTIOW_E_BADARG;
    return budget_call(h, "rtiow_accumulate_budget_volume", VolumeGridChunks{{"rtiow_accumulate_budget"}}, samples, min_samples, target, max_samples, kernel_ms, active_pixels);
}

int rtiow_render_guides_volume(rtiow_handle h, float* kernel_ms) {
    if (!h) return RTIOW_E_BADARG;
    return guides_call(h, "rtiow_render_guides_volume", VolumeGridChunks{{"rtiow_render_guides"}}, kernel_ms);
}

int rtiow_render_coverage_volume(rtiow_handle h, int subsamples_per_side, float* kernel_ms) {
    if (!h) return RTIOW_E_BADARG;
    return coverage_call(h, "rtiow_render_coverage_volume", VolumeGridChunks{{"rtiow_render_coverage"}}, subsamples_per_side, kernel_ms);
}

}  // extern "C"
