// temporal_noise.h -- V^0, the variance plane rtiow_denoise_history_variance filters the temporal image by:
// where the current accumulation measured a pixel's noise (an adaptive record with n >= 2), the variance of the blend
// Cout = h + alpha (c - h) under the assumption that the history's samples are as noisy as the frame's, alpha V_p; everywhere else the
// spatial variance of the temporal image's luminance over the (2r + 1)^2 window, SVGF's fallback for short histories (Schied et al.
// 2017).  Nothing is carried from frame to frame: alpha = n / Mout is recomputed from the stored Mout.
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, after history_clip.h and denoise_variance.h; internal linkage).
//
// Every value is defined operation by operation and evaluated in T with plain * + - /, unfused
// (-ffp-contract=off), so a numpy restatement gives the same bits; V_p alone passes through double (mean_variance).
#pragma once
#include "history_clip.h"       // Vec4, FrameShape
#include "denoise_variance.h"   // mean_variance

namespace {

constexpr int NOISE_MAX_RADIUS = 3;
constexpr int NOISE_TILE_SIDE = 16 + 2 * NOISE_MAX_RADIUS;      // 22 rows of the tile, whatever r
// A tile row is NOISE_TILE_PITCH entries {Y, counts} of 2 T apart.  fp32: an entry is 8 bytes, read by ds_read_b64, whose 32 lanes a
// cycle are two pixel rows of the workgroup; 48 entries = 384 bytes put the second row in the other half of the 256-byte bank row.
// fp64: an entry is a 16-byte slot, read by ds_read_b128, whose 16 lanes a cycle are 8 of one row and 8 of the next at complementary
// columns; 32 slots = two bank rows keep them on 16 different slots (as denoise_variance.h's TILE_PITCH).  8.3 KB and 11 KB.
template <class T> constexpr int NOISE_TILE_PITCH = sizeof(T) == 4 ? 48 : 32;

template <class T> struct alignas(2 * sizeof(T)) NoiseEntry { T y, k; };

// One lane per pixel, 16 x 16 pixels per workgroup.  The workgroup stages {Y_q, Mout_q > 0 ? 1 : 0} of its (16 + 2r)^2 window from the
// temporal image hist_cm ({C.rgb, M}: one 16-byte load per pixel in fp32); lanes outside the frame help fill and meet the barrier.
// An entry that does not count (outside the frame, or Mout = 0) holds {+0, 0}: a sum started at +0 keeps its bits under + (+0)
// (history_clip.h), so the window loop needs no branch, and k <= 49 is exact in T.  counts == nullptr: the accumulation is not adaptive,
// every pixel takes the spatial estimate.  r in 1..NOISE_MAX_RADIUS (the host checks it) is wave-uniform.  No atomics, no counters.
template <class T>
__global__ void __launch_bounds__(256) temporal_noise_kernel(FrameShape fr, int r, const Vec4<T>* __restrict__ hist_cm, const unsigned char* __restrict__ mid,
                                                             const int32_t* __restrict__ counts, T* __restrict__ out) {
    constexpr int PITCH = NOISE_TILE_PITCH<T>;
    __shared__ NoiseEntry<T> tile[NOISE_TILE_SIDE * PITCH];
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
    const int x0w = (int)blockIdx.x * 16, y0w = (int)blockIdx.y * 16;
    const int side = 16 + 2 * r;
    for (int i = (int)threadIdx.x; i < side * side; i += 256) {
        const int ty = i / side, tx = i - ty * side;
        const int qx = x0w - r + tx, qy = y0w - r + ty;
        NoiseEntry<T> e = {(T)0, (T)0};
        if (qx >= 0 && qx < fr.W && qy >= 0 && qy < fr.local_rows) {
            const Vec4<T> cm = hist_cm[(size_t)qy * fr.W + qx];
            if (cm.w > (T)0) e = {luminance<T>({cm.x, cm.y, cm.z}), (T)1};
        }
        tile[ty * PITCH + tx] = e;
    }
    __syncthreads();
    const int x = x0w + lx, y = y0w + ly;
    if (x >= fr.W || y >= fr.local_rows) return;             // after the barrier
    const size_t lp = (size_t)y * fr.W + x;
    const int n = counts ? counts[lp] : 0;
    T v0;
    if (n >= 2) {
        // measured: the update's alpha (history.h: nT / mout) times rtiow_read_variance's V_p
        const MidState<T> rec = load_record<T>(mid, lp);
        const T vp = mean_variance<T>({rec.acc[0], rec.acc[1], rec.acc[2]}, adapt_s2<T>(rec), n);
        const T alpha = (T)n / hist_cm[lp].w;
        v0 = alpha * vp;
    } else {
        // spatial: dy then dx in -r..r
        T a = 0, q = 0, kT = 0;
        for (int ty = ly; ty <= ly + 2 * r; ++ty)
            for (int tx = lx; tx <= lx + 2 * r; ++tx) {
                const NoiseEntry<T> e = tile[ty * PITCH + tx];
                a = a + e.y;
                q = q + e.y * e.y;
                kT = kT + e.k;
            }
        const T mu = a / kT;
        T s = q / kT - mu * mu;
        s = s > (T)0 ? s : (T)0;
        v0 = kT >= (T)2 ? s : (T)0;
    }
    out[lp] = v0;
}

}  // namespace
