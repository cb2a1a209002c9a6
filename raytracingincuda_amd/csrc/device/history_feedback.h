// history_feedback.h -- the filtered commit of the temporal history (rtiow_history_commit_filtered): one level of the edge-avoiding
// a-trous filter at step 1 over the temporal image {C.rgb, M}, steered by the filter guides, whose result becomes the base of later
// updates in place of the raw temporal image -- the recurrent half of the SVGF recipe (Schied et al. 2017).  The length M is copied.
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, in this order; internal linkage).
//
// Every value is defined operation by operation and evaluated in T with plain * + - /: no RT_FMA, madd3 or
// dot3.  -ffp-contract=off keeps the plain operations unfused, so a numpy restatement gives the same bits.
#pragma once
#include "history.h"            // Vec4, FrameShape, FilterWeights (through denoise.h)

namespace {

constexpr int FEEDBACK_RADIUS = 2;
constexpr int FEEDBACK_TILE_SIDE = 16 + 2 * FEEDBACK_RADIUS;     // 20: 400 entries of 3 x 4 T -- 19.2 KB in fp32, 38.4 KB in fp64

// One lane per pixel, 16 x 16 pixels per workgroup, as history_clip_kernel.  The workgroup first copies the 20 x 20 entries of its pixels
// and their halo of 2 once each into LDS: {C.rgb, M} of the temporal image, {N, Z} and {A, .} of the filter guides, one 4-T vector each
// (three vector loads and three vector LDS stores per entry; neighbouring lanes fill neighbouring entries).  Lanes outside the frame
// help fill and meet the barrier.  An entry outside the frame holds M = 0, which is what "does not count" looks like inside the frame
// too (M_q > 0 is false), so the tap loop has one test.  A lane then runs its 25 taps from LDS, dy then dx in -2..2:
//   kern = K[dx+2] K[dy+2], e = ((ec ic + en in) + ea ia) + ez iz, w = kern / (1 + e)          (level 0 of denoise_level_kernel)
//   S = S + w C_q, Wt = Wt + w over the taps with M_q > 0; F = S / Wt
//   out = blend ? C_p + fb (F - C_p) : F                                                         (blend == 0: feedback is 1)
// and writes {out, M_p} as one vector.  A pixel whose own M_p > 0 is false keeps its entry bit for bit.  The pixel itself is a tap with
// e = 0, so Wt >= 9/64 wherever the loop runs.  out must not alias cm: the halo of one workgroup is the interior of another.
template <class T>
__global__ void __launch_bounds__(256) feedback_filter_kernel(FrameShape fr, FilterWeights<T> fw, int blend, T fb, const Vec4<T>* __restrict__ cm,
                                                              const Vec4<T>* __restrict__ nd, const Vec4<T>* __restrict__ alb, Vec4<T>* __restrict__ out) {
    constexpr int SIDE = FEEDBACK_TILE_SIDE, R = FEEDBACK_RADIUS;
    __shared__ Vec4<T> tile_c[SIDE * SIDE];
    __shared__ Vec4<T> tile_g[SIDE * SIDE];
    __shared__ Vec4<T> tile_a[SIDE * SIDE];
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
    const int x0w = (int)blockIdx.x * 16, y0w = (int)blockIdx.y * 16;
    for (int i = (int)threadIdx.x; i < SIDE * SIDE; i += 256) {
        const int ty = i / SIDE, tx = i - ty * SIDE;
        const int qx = x0w - R + tx, qy = y0w - R + ty;
        Vec4<T> c = {(T)0, (T)0, (T)0, (T)0}, g = c, a = c;
        if (qx >= 0 && qx < fr.W && qy >= 0 && qy < fr.local_rows) {
            const size_t q = (size_t)qy * fr.W + qx;
            c = cm[q]; g = nd[q]; a = alb[q];
        }
        tile_c[i] = c; tile_g[i] = g; tile_a[i] = a;
    }
    __syncthreads();
    const int x = x0w + lx, y = y0w + ly;
    if (x >= fr.W || y >= fr.local_rows) return;                 // after the barrier
    const int own = (ly + R) * SIDE + lx + R;
    const Vec4<T> cp = tile_c[own];
    Vec4<T> o = cp;
    if (cp.w > (T)0) {                                           // false for NaN
        const Vec4<T> gp = tile_g[own], ap = tile_a[own];
        const T K[5] = {(T)0.0625, (T)0.25, (T)0.375, (T)0.25, (T)0.0625};
        T sx = 0, sy = 0, sz = 0, sw = 0;
#pragma unroll
        for (int dy = 0; dy <= 2 * R; ++dy) {
#pragma unroll
            for (int dx = 0; dx <= 2 * R; ++dx) {
                const int i = (ly + dy) * SIDE + lx + dx;
                const Vec4<T> cq = tile_c[i], gq = tile_g[i], aq = tile_a[i];
                const bool counts = cq.w > (T)0;
                const T kern = K[dx] * K[dy];
                const T dcx = cq.x - cp.x, dcy = cq.y - cp.y, dcz = cq.z - cp.z;
                const T dnx = gq.x - gp.x, dny = gq.y - gp.y, dnz = gq.z - gp.z, dz = gq.w - gp.w;
                const T dax = aq.x - ap.x, day = aq.y - ap.y, daz = aq.z - ap.z;
                const T ec = (dcx * dcx + dcy * dcy) + dcz * dcz;
                const T en = (dnx * dnx + dny * dny) + dnz * dnz;
                const T ea = (dax * dax + day * day) + daz * daz;
                const T ez = dz * dz;
                const T e = ((ec * fw.ic + en * fw.in) + ea * fw.ia) + ez * fw.iz;
                const T w = kern / ((T)1 + e);
                sx = counts ? sx + w * cq.x : sx; sy = counts ? sy + w * cq.y : sy; sz = counts ? sz + w * cq.z : sz;
                sw = counts ? sw + w : sw;
            }
        }
        const T fx = sx / sw, fy = sy / sw, fz = sz / sw;
        if (blend) { o.x = cp.x + fb * (fx - cp.x); o.y = cp.y + fb * (fy - cp.y); o.z = cp.z + fb * (fz - cp.z); }
        else { o.x = fx; o.y = fy; o.z = fz; }
    }
    out[(size_t)y * fr.W + x] = o;
}

}  // namespace
