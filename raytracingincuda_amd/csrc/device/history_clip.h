// history_clip.h -- the temporal reprojection with a neighbourhood clamp (rtiow_history_update_clipped): history.h's update with one
// step between the cap of the history length and the blend -- the gathered history colour is clamped, per channel, to
// mean +- gamma * sigma of the current accumulation's (2r + 1)^2 window around the pixel, so a history the current frame contradicts
// (a reflection reprojected as if painted on the first surface) is pulled to what the frame sees.  The length m is not touched.
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, in this order; internal linkage).
//
// Every value is defined operation by operation (INTEGRATION.md sections 11 and 14) and evaluated in T with plain * + - /, floor,
// fabs and a correctly rounded sqrt: no RT_FMA, madd3 or dot3.  -ffp-contract=off keeps the plain operations unfused, so a numpy
// restatement gives the same bits.
#pragma once
#include "history.h"            // HistoryParams, Vec4, gather_history, blend_history, linear_colour, FrameShape

namespace {

constexpr int CLIP_MAX_RADIUS = 3;
constexpr int CLIP_TILE_SIDE = 16 + 2 * CLIP_MAX_RADIUS;     // 22: 484 entries of 4 T -- 7.7 KB in fp32, 15.5 KB in fp64

// One lane per pixel, 16 x 16 pixels per workgroup, as history_reproject_kernel, whose arguments these are but for r, gamma and the
// second counter.  The workgroup first decodes the (16 + 2r)^2 records of its pixels and their halo once each into LDS as
// {c.rgb, counts ? 1 : 0}; lanes outside the frame help fill and meet the barrier.  A lane then sums its window from LDS, gathers
// the history with gather_history (history.h), clamps it and blends with blend_history.  ctr[0] counts the pixels with m > 0, ctr[1] those of them whose
// history the clamp changed: two ballots and at most two LDS atomics per wave, then one global atomic per counter and workgroup.
// Every wave of the grid adding to the same word of device memory is what history_reproject_kernel's time is made of (DESIGN.md
// section 4.13), so the workgroup adds its four waves up first.
//
// An entry that does not count (outside the frame, or never sampled: linear_colour gives 0) holds {+0, +0, +0, 0}.  The sums start
// at +0 and x + (+0) has the bits of x for every x but -0, which a sum that started at +0 never is, so adding every entry of the
// window gives the bits of adding the counting ones alone, and the window loop needs no branch.  k <= 49 is exact in T.
template <class T>
__global__ void __launch_bounds__(256) history_clip_kernel(FrameShape fr, const HistoryParams<T> hp, int r, T gamma, const unsigned char* __restrict__ mid,
                                                           const int32_t* __restrict__ counts, int n_uniform, const Vec4<T>* __restrict__ cur_nd,
                                                           const Vec4<T>* __restrict__ base_hm, const Vec4<T>* __restrict__ base_nd,
                                                           Vec4<T>* __restrict__ out_cm, T* __restrict__ out_rgb, unsigned* __restrict__ ctr) {
    __shared__ Vec4<T> tile[CLIP_TILE_SIDE * CLIP_TILE_SIDE];
    __shared__ unsigned tally[2];
    if (threadIdx.x < 2u) tally[threadIdx.x] = 0;
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
    const int x0w = (int)blockIdx.x * 16, y0w = (int)blockIdx.y * 16;
    const int side = 16 + 2 * r;
    for (int i = (int)threadIdx.x; i < side * side; i += 256) {
        const int ty = i / side, tx = i - ty * side;
        const int qx = x0w - r + tx, qy = y0w - r + ty;
        Vec4<T> e = {(T)0, (T)0, (T)0, (T)0};
        if (qx >= 0 && qx < fr.W && qy >= 0 && qy < fr.local_rows) {
            const size_t q = (size_t)qy * fr.W + qx;
            const V3<T> cq = linear_colour<T>(mid, counts, n_uniform, q);
            const int nq = counts ? counts[q] : n_uniform;
            e = {cq.x, cq.y, cq.z, nq > 0 ? (T)1 : (T)0};
        }
        tile[i] = e;
    }
    __syncthreads();
    const int x = x0w + lx, y = y0w + ly;
    const bool inside = x < fr.W && y < fr.local_rows;
    bool carried = false, clipped = false;
    if (inside) {
        const size_t lp = (size_t)y * fr.W + x;
        const Vec4<T> own = tile[(ly + r) * side + lx + r];
        const V3<T> c = {own.x, own.y, own.z};
        const int n = counts ? counts[lp] : n_uniform;
        // the window: dy then dx in -r..r
        T ax = 0, ay = 0, az = 0, qx2 = 0, qy2 = 0, qz2 = 0, kT = 0;
        for (int ty = ly; ty <= ly + 2 * r; ++ty)
            for (int tx = lx; tx <= lx + 2 * r; ++tx) {
                const Vec4<T> e = tile[ty * side + tx];
                ax = ax + e.x; ay = ay + e.y; az = az + e.z;
                qx2 = qx2 + e.x * e.x; qy2 = qy2 + e.y * e.y; qz2 = qz2 + e.z * e.z;
                kT = kT + e.w;
            }
        Gathered<T> h = gather_history<T, true>(fr, hp, x, y, lp, cur_nd, base_hm, base_nd);       // section 11, history.h's one statement
        carried = h.m > (T)0;
        // the clamp: lo = mu - gamma sd, hi = mu + gamma sd; a comparison with NaN is false and leaves h alone
        if (carried && kT >= (T)2) {
            const T mux = ax / kT, muy = ay / kT, muz = az / kT;
            T vx = qx2 / kT - mux * mux, vy = qy2 / kT - muy * muy, vz = qz2 / kT - muz * muz;
            vx = vx > (T)0 ? vx : (T)0; vy = vy > (T)0 ? vy : (T)0; vz = vz > (T)0 ? vz : (T)0;
            const T ex = gamma * Real<T>::sqrt(vx), ey = gamma * Real<T>::sqrt(vy), ez = gamma * Real<T>::sqrt(vz);
            const T lox = mux - ex, hix = mux + ex, loy = muy - ey, hiy = muy + ey, loz = muz - ez, hiz = muz + ez;
            clipped = h.hx < lox || h.hx > hix || h.hy < loy || h.hy > hiy || h.hz < loz || h.hz > hiz;
            h.hx = h.hx < lox ? lox : (h.hx > hix ? hix : h.hx);
            h.hy = h.hy < loy ? loy : (h.hy > hiy ? hiy : h.hy);
            h.hz = h.hz < loz ? loz : (h.hz > hiz ? hiz : h.hz);
        }
        blend_history<T>(h, c, n, lp, out_cm, out_rgb);
    }
    const unsigned long long votes = __ballot(carried), cuts = __ballot(clipped);
    if ((threadIdx.x & 63u) == 0) {
        if (votes) atomicAdd(&tally[0], (unsigned)__popcll(votes));
        if (cuts) atomicAdd(&tally[1], (unsigned)__popcll(cuts));
    }
    __syncthreads();
    if (threadIdx.x < 2u && tally[threadIdx.x]) atomicAdd(ctr + threadIdx.x, tally[threadIdx.x]);
}

}  // namespace
