// history_budget.h -- history-guided sample budgets (rtiow_history_plan, rtiow_accumulate_budget): the history length every pixel of the
// current camera will carry, computed before the first sample of the frame is traced, and the select of an adaptive chunk that samples
// a pixel while its count plus that length is below a target.
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, in this order; internal linkage).
//
// history_length_kernel is the `m` of history_reproject_kernel and nothing else of it: both call
// gather_history (history.h), the one statement of that arithmetic, this kernel with COLOUR == false, so that m + (T)n is the Mout
// rtiow_history_update gives later, bit for bit.  tests/test_frame_edges.py holds the two to each other on every class of pixel.
#pragma once
#include "history.h"            // HistoryParams, Vec4, gather_history
#include "adaptive.h"           // FrameShape, tile_slot_pixel, MidState records

namespace {

// One lane per pixel, 16 x 16 pixels per workgroup (history_reproject_kernel's launch shape).  Per tap: the base's {normal', depth'} as one
// vector load and M alone, the last of the four T of {H.rgb, M}.  out_m receives m, one T per pixel.  *reprojected counts the pixels
// with m > 0: one ballot and one atomic per wave.
template <class T>
__global__ void __launch_bounds__(256) history_length_kernel(FrameShape fr, const HistoryParams<T> hp, const Vec4<T>* __restrict__ cur_nd,
                                                             const T* __restrict__ base_hm, const Vec4<T>* __restrict__ base_nd,
                                                             T* __restrict__ out_m, unsigned* __restrict__ reprojected) {
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15u), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    const bool inside = x < fr.W && y < fr.local_rows;
    bool carried = false;
    if (inside) {
        const size_t lp = (size_t)y * fr.W + x;
        const T m = gather_history<T, false>(fr, hp, x, y, lp, cur_nd, reinterpret_cast<const Vec4<T>*>(base_hm), base_nd).m;
        carried = m > (T)0;
        out_m[lp] = m;
    }
    const unsigned long long votes = __ballot(carried);
    if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(reprojected, (unsigned)__popcll(votes));
}

// adaptive_select_kernel with another rule: a pixel is active iff (n < min_samples or (T)n + m < target) and n + samples <= max_samples,
// with n the count the previous chunk's adaptive_finish_kernel left (first chunk after a reset: mid_in == nullptr, n = 0) and m the
// plan's history length (history_length_kernel).  The sum and the comparison are in T.  Everything else is that kernel's: one 8x8 tile
// per wave in the render's tile order, active pixels appended to `order` as (row << 16 | column) by ballot ranks and one atomic per wave,
// their count becoming n + samples here, an inactive pixel's record copied into mid_out (the first chunk builds it from rng_in with zero
// sums and n = 0), n_active[0] the active pixels.
template <class T>
__global__ void __launch_bounds__(256) budget_select_kernel(FrameShape f, int samples, int min_samples, int max_samples, T target,
                                                            int32_t* __restrict__ counts, const T* __restrict__ length,
                                                            const uint32_t* __restrict__ rng_in, const unsigned char* __restrict__ mid_in,
                                                            unsigned char* __restrict__ mid_out, int* __restrict__ order, unsigned* __restrict__ n_active) {
    const int tiles = ((f.W + 7) >> 3) * ((f.local_rows + 7) >> 3);
    const int tile = (int)blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    if (tile >= tiles) return;                                   // wave-uniform
    int i = 0, jl = 0;
    const bool valid = tile_slot_pixel(f, tile * 64 + (int)(threadIdx.x & 63u), i, jl);
    const size_t lp = (size_t)jl * f.W + i;
    bool active = false;
    int n = 0;
    if (valid) {
        n = mid_in ? counts[lp] : 0;
        const T have = (T)n + length[lp];
        active = (n < min_samples || have < target) && (long long)n + samples <= (long long)max_samples;
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(active);
    if (m != 0) {
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        int base = 0;
        if ((threadIdx.x & 63u) == 0) base = (int)atomicAdd(n_active, (unsigned)__builtin_popcountll(m));
        base = __builtin_amdgcn_readfirstlane(base);
        if (active) order[base + rank] = (jl << 16) | i;
    }
    if (active) counts[lp] = n + samples;
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

}  // namespace
