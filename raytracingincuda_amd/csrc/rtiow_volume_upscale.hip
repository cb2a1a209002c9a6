// rtiow_volume_upscale.hip -- guided upscaling on volume scenes: the tenth translation
// unit compiled for gfx950, linked into librtiow_hip.so beside the others.  It holds upscale_kernel and upscale_wide_kernel
// (device/upscale.h, device/upscale_wide.h) instantiated over the volume grid of rtiow_render_volume (device/hit_volume_grid.h:
// RTIOW_SCENE_VOLUME_GRID), and the two entry points, and nothing else: the other code objects keep exactly the kernels they had.  The
// launches are library/launch.h's launch_upscale and launch_upscale_wide, the checks library/pass.h's upscale_call, both with the volume
// grid's scene binding (library/volume_launch.h: VolumeGridScene) where the twins pass StagedScene: each is stated once.  Stale guides
// and coverage layers are rendered through the C-ABI by the kernels of rtiow_volume_preview.hip, and the image is read by
// rtiow_upscale.hip's two readers.
//
// Floating-point contract: rtiow_hip.hip's, the same flags.

#include "library/unit.h"
#include "device/hit_volume_grid.h"
#include "library/volume_grid.h"
#include "library/volume_launch.h"

extern "C" {

// ---- Guided upscaling on volume scenes: upscale_call under these calls' names, through the volume grid
int rtiow_upscale_volume(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth, int use_coverage,
                         float* kernel_ms, uint64_t* covered_pixels) {
    const VolumeGridScene scene{"rtiow_upscale"};
    return upscale_call("rtiow_upscale_volume", scene, h, factor, source, sigma_normal, sigma_albedo, sigma_depth, use_coverage, kernel_ms, covered_pixels, [&](const double* inv2, size_t out_bytes) {
        return by_precision(h, [&](auto t) { return launch_upscale<decltype(t)>(h, scene, factor, source, inv2, use_coverage, out_bytes); });
    });
}

int rtiow_upscale_wide_volume(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth, int use_coverage,
                              float* kernel_ms, uint64_t* covered_pixels) {
    const VolumeGridScene scene{"rtiow_upscale_wide"};
    return upscale_call("rtiow_upscale_wide_volume", scene, h, factor, source, sigma_normal, sigma_albedo, sigma_depth, use_coverage, kernel_ms, covered_pixels, [&](const double* inv2, size_t out_bytes) {
        return by_precision(h, [&](auto t) { return launch_upscale_wide<decltype(t)>(h, scene, factor, source, inv2, use_coverage, out_bytes); });
    });
}

}  // extern "C"
