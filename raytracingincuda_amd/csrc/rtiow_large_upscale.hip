// rtiow_large_upscale.hip -- guided upscaling on large scenes: the seventh translation
// unit compiled for gfx950, linked into librtiow_hip.so beside the others.  It holds upscale_kernel and upscale_wide_kernel
// (device/upscale.h, device/upscale_wide.h) instantiated over the device grid of rtiow_render_large (device/hit_device_grid.h:
// RTIOW_SCENE_DEVICE_GRID), and the two entry points, and nothing else: the other code objects keep exactly the kernels they had.  The
// launches are library/launch.h's launch_upscale and launch_upscale_wide, the checks library/pass.h's upscale_call, both with the device
// grid's scene binding (library/large_launch.h: DeviceGridScene) where the twins pass StagedScene: each is stated once.  Stale guides and
// coverage layers are rendered through the C-ABI by the kernels of rtiow_large_preview.hip, and the image is read by rtiow_upscale.hip's
// two readers.
//
// Floating-point contract: rtiow_hip.hip's, the same flags.

#include "library/unit.h"
#include "device/hit_device_grid.h"
#include "library/device_grid.h"
#include "library/large_launch.h"

extern "C" {

// ---- Guided upscaling on large scenes: upscale_call under these calls' names, through the device grid
int rtiow_upscale_large(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth, int use_coverage,
                        float* kernel_ms, uint64_t* covered_pixels) {
    const DeviceGridScene scene{"rtiow_upscale"};
    return upscale_call("rtiow_upscale_large", scene, h, factor, source, sigma_normal, sigma_albedo, sigma_depth, use_coverage, kernel_ms, covered_pixels, [&](const double* inv2, size_t out_bytes) {
        return by_precision(h, [&](auto t) { return launch_upscale<decltype(t)>(h, scene, factor, source, inv2, use_coverage, out_bytes); });
    });
}

int rtiow_upscale_wide_large(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth, int use_coverage,
                             float* kernel_ms, uint64_t* covered_pixels) {
    const DeviceGridScene scene{"rtiow_upscale_wide"};
    return upscale_call("rtiow_upscale_wide_large", scene, h, factor, source, sigma_normal, sigma_albedo, sigma_depth, use_coverage, kernel_ms, covered_pixels, [&](const double* inv2, size_t out_bytes) {
        return by_precision(h, [&](auto t) { return launch_upscale_wide<decltype(t)>(h, scene, factor, source, inv2, use_coverage, out_bytes); });
    });
}

}  // extern "C"
