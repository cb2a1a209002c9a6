// pass.h -- what the entry points of both gfx950 translation units (rtiow_hip.hip, rtiow_upscale.hip) share around a timed pass: the events
// of kernel_ms and the copy of a result to the host.
// Host side of librtiow_hip.so (internal linkage).
#pragma once
#include "handle.h"

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

}  // namespace
