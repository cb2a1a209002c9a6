// rtiow_upscale.hip -- guided upscaling: the second translation unit compiled for gfx950,
// linked into librtiow_hip.so beside rtiow_hip.hip.  It holds upscale_kernel (device/upscale.h), its launch (library/launch.h:
// launch_upscale) and the three entry points, and nothing else: rtiow_hip.hip's code object keeps exactly the kernels it had.  The
// headers are library/unit.h's, as in every unit (internal linkage; templates it does not call are not instantiated here); the checks of
// rtiow_upscale are library/pass.h's upscale_call; stale guides and coverage layers are rendered through the C-ABI, by the kernels of the
// other unit.
//
// Floating-point contract: rtiow_hip.hip's, the same flags.

#include "library/unit.h"

extern "C" {

// ---- Guided upscaling
int rtiow_upscale(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth, int use_coverage,
                  float* kernel_ms, uint64_t* covered_pixels) {
    return upscale_call("rtiow_upscale", StagedScene{}, h, factor, source, sigma_normal, sigma_albedo, sigma_depth, use_coverage, kernel_ms, covered_pixels, [&](const double* inv2, size_t out_bytes) {
        return by_precision(h, [&](auto t) { return launch_upscale<decltype(t)>(h, StagedScene{}, factor, source, inv2, use_coverage, out_bytes); });
    });
}

int rtiow_read_upscaled(rtiow_handle h, void* host_rgb, size_t bytes) {
    if (!h) return RTIOW_E_BADARG;
    PREVIEW_TRY(h, need_upscaled(h->preview, "rtiow_read_upscaled"));
    if (bytes != h->upscaled_bytes || !host_rgb)
        return fail_arg(h, RTIOW_E_BADARG, "rtiow_read_upscaled: bytes must be (factor x height) x (factor x width) x 3 x sizeof(T)");
    return copy_out(h, host_rgb, h->upscaled, bytes);
}

int rtiow_upscaled_device_ptr(rtiow_handle h, void** device_ptr, size_t* bytes) {
    if (!h || !device_ptr || !bytes) return RTIOW_E_BADARG;
    PREVIEW_TRY(h, need_upscaled(h->preview, "rtiow_upscaled_device_ptr"));
    *device_ptr = h->upscaled;
    *bytes = h->upscaled_bytes;
    return 0;
}

}  // extern "C"
