// adaptive.h -- adaptive progressive rendering (rtiow_accumulate_adaptive): the select and finish kernels around render_adaptive_kernel
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, in this order; internal linkage).
#pragma once
#include "render_kernels.h"

namespace {

struct FrameShape { int W, local_rows; };       // what tile_slot_pixel reads

// One pass over the local pixels, one 8x8 tile per wave in the render's tile order (bottom-up).  A pixel is active iff
// (n < min_samples or (double)err > rel_error) and n + samples <= max_samples, with n and err the state the previous chunk's
// adaptive_finish_kernel left (first chunk after a reset: mid_in == nullptr, n = 0, err = +inf).  Active pixels are appended to `order`
// as (row << 16 | column): one atomic per wave, ranks by ballot, so the active pixels of a tile stay together; their count becomes
// n + samples here.  The host pads the tail pool with -1.  An inactive pixel's record is copied into mid_out (the first chunk builds it
// from rng_in with zero sums and sets n = 0), so that mid_out holds every pixel's state after the render.  n_active[0] counts the active
// pixels.
template <class T>
__global__ void __launch_bounds__(256) adaptive_select_kernel(FrameShape f, int samples, int min_samples, int max_samples, double rel_error,
                                                              int32_t* __restrict__ counts, const float* __restrict__ err,
                                                              const uint32_t* __restrict__ rng_in, const unsigned char* __restrict__ mid_in,
                                                              unsigned char* __restrict__ mid_out, int* __restrict__ order, unsigned* __restrict__ n_active) {
    const int tiles = ((f.W + 7) >> 3) * ((f.local_rows + 7) >> 3);
    const int tile = (int)blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    if (tile >= tiles) return;                                   // wave-uniform
    int i = 0, jl = 0;
    const bool valid = tile_slot_pixel(f, tile * 64 + (int)(threadIdx.x & 63u), i, jl);
    const size_t lp = (size_t)jl * f.W + i;
    bool active = false;
    if (valid) {
        const int n = mid_in ? counts[lp] : 0;
        const double e = mid_in ? (double)err[lp] : (double)__builtin_huge_valf();
        active = (n < min_samples || e > rel_error) && (long long)n + samples <= (long long)max_samples;
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(active);
    if (m != 0) {
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        int base = 0;
        if ((threadIdx.x & 63u) == 0) base = (int)atomicAdd(n_active, (unsigned)__builtin_popcountll(m));
        base = __builtin_amdgcn_readfirstlane(base);
        if (active) order[base + rank] = (jl << 16) | i;
    }
    if (active) counts[lp] = (mid_in ? counts[lp] : 0) + samples;
    else if (valid && !mid_in) counts[lp] = 0;
    if (valid && !active) {
        if (mid_in) store_record<T>(mid_out, lp, load_record<T>(mid_in, lp));
        else {
            const size_t npix = (size_t)f.W * f.local_rows;
            MidState<T> r;
            r.v[0] = rng_in[0 * npix + lp]; r.v[1] = rng_in[1 * npix + lp]; r.v[2] = rng_in[2 * npix + lp];
            r.v[3] = rng_in[3 * npix + lp]; r.v[4] = rng_in[4 * npix + lp]; r.d = rng_in[5 * npix + lp];
            r.acc[0] = 0; r.acc[1] = 0; r.acc[2] = 0;
            set_s2<T>(r, (T)0, 0u);
            store_record<T>(mid_out, lp, r);
        }
    }
}

// Relative standard error of a pixel's mean luminance, in double, from its record:
// m = Y(acc) / n, var = max(0, (s2 - n m^2) / (n - 1)), err = sqrt(var / n) / (m + 1e-3); +inf below two samples.
template <class T>
__device__ __forceinline__ float relative_error(V3<T> acc, T s2, uint32_t n) {
    if (n < 2) return __builtin_huge_valf();
    const double dn = (double)n;
    const double mean = (double)luminance<T>(acc) / dn;
    double var = ((double)s2 - dn * mean * mean) / (dn - 1.0);
    if (!(var > 0.0)) var = 0.0;
    return (float)(sqrt(var / dn) / (mean + 1e-3));
}

// One pass in image order after the render: every local pixel's preview from its record, scaled by (T)1 / (T)n (correctly rounded:
// the scale rtiow_host_camera computes for samples_per_pixel = n), through store_pixel -- the bits rtiow_render stores at n samples.
// Also err, which rtiow_read_adaptive_state returns with the counts and the next select reads, and the largest count (max_count, zeroed
// by the host).
template <class T>
__global__ void __launch_bounds__(256) adaptive_finish_kernel(size_t npix, const unsigned char* __restrict__ mid, T* __restrict__ fb,
                                                              const int32_t* __restrict__ counts, float* __restrict__ err, unsigned* __restrict__ max_count) {
    const size_t lp = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned n = 0;
    if (lp < npix) {
        const MidState<T> r = load_record<T>(mid, lp);
        n = (unsigned)counts[lp];
        const V3<T> acc = {r.acc[0], r.acc[1], r.acc[2]};
        struct { T pixel_samples_scale; T* fb; } out = {(T)1 / (T)n, fb};
        store_pixel<T>(out, lp, acc);
        err[lp] = relative_error<T>(acc, adapt_s2<T>(r), n);
    }
    for (int off = 32; off > 0; off >>= 1) { const unsigned o = (unsigned)__shfl_xor((int)n, off, 64); n = o > n ? o : n; }
    if ((threadIdx.x & 63u) == 0 && n) atomicMax(max_count, n);
}

}  // namespace
