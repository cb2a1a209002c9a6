// rtiow_upscale_wide.hip -- wide-support guided upscaling: the third translation unit
// compiled for gfx950, linked into librtiow_hip.so beside rtiow_hip.hip and rtiow_upscale.hip.  It holds upscale_wide_kernel
// (device/upscale_wide.h), its launch (library/launch.h: launch_upscale_wide) and the one entry point, and nothing else: the code objects
// of the other two units keep exactly the kernels they had.  The headers are library/unit.h's, as in every unit (internal linkage;
// templates it does not call are not instantiated here); the pixel, the tap, the resolve and the count are device/upscale.h's, shared
// with upscale_kernel, and the checks library/pass.h's upscale_call; stale guides and coverage layers are rendered through the C-ABI, by
// the kernels of rtiow_hip.hip, and the image is read by rtiow_upscale.hip's two readers.
//
// Floating-point contract: rtiow_hip.hip's, the same flags.

#include "library/unit.h"

extern "C" {

// ---- Wide-support guided upscaling: upscale_call under this call's name
int rtiow_upscale_wide(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth, int use_coverage,
                       float* kernel_ms, uint64_t* covered_pixels) {
    return upscale_call("rtiow_upscale_wide", StagedScene{}, h, factor, source, sigma_normal, sigma_albedo, sigma_depth, use_coverage, kernel_ms, covered_pixels, [&](const double* inv2, size_t out_bytes) {
        return by_precision(h, [&](auto t) { return launch_upscale_wide<decltype(t)>(h, StagedScene{}, factor, source, inv2, use_coverage, out_bytes); });
    });
}

}  // extern "C"
