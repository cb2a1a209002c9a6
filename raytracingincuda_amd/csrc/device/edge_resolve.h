// edge_resolve.h -- silhouette pixels rebuilt from sub-pixel coverage layers (rtiow_render_coverage, rtiow_resolve_edges): which first-hit
// spheres share a pixel and in what proportion, from a small lattice of primary rays, and the mixed pixels of the denoised image rebuilt
// as the coverage-weighted sum of what the filter produced on the pure pixels of each layer nearby.
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, in this order; internal linkage).
//
// Every value is defined operation by operation and evaluated in T with plain * + - / and sqrt, as in
// denoise.h: no RT_FMA, madd3 or dot3 for a stored value.  -ffp-contract=off keeps the plain operations unfused, so a numpy restatement
// gives the same bits.
#pragma once
#include "history.h"            // Vec4, FrameShape (through denoise.h: guide_kernel, whose ray and normal these are)

namespace {

constexpr int COVERAGE_MAX_SIDE = 4, COVERAGE_MAX_SUBSAMPLES = COVERAGE_MAX_SIDE * COVERAGE_MAX_SIDE;
constexpr int COVERAGE_NO_LAYER = -2;                           // the id of a pure pixel's second layer (the sky is hit_world's -1)
constexpr int EDGE_MAX_RADIUS = 3;

// The direction of sub-sample s = a + G b of pixel (i, j): o_a = ((T)a + 0.5) / G - 0.5 (exact for G = 2, 4), fx = (T)i + o_a, fy likewise,
// D = ((pixel00 + fx du) + fy dv) - O.  No lens sample.
template <class T>
__device__ __forceinline__ V3<T> coverage_direction(const CameraParams<T>& cam, int i, int j, int s, int G) {
    const int a = s & (G - 1), b = s / G;
    const T fG = (T)G;
    const T fx = (T)i + (((T)a + (T)0.5) / fG - (T)0.5), fy = (T)j + (((T)b + (T)0.5) / fG - (T)0.5);
    const V3<T> ps = {(cam.pixel00.x + fx * cam.du.x) + fy * cam.dv.x, (cam.pixel00.y + fx * cam.du.y) + fy * cam.dv.y,
                      (cam.pixel00.z + fx * cam.du.z) + fy * cam.dv.z};
    return {ps.x - cam.center.x, ps.y - cam.center.y, ps.z - cam.center.z};
}

// ---- Coverage layers: one lane per local pixel, one 8x8 tile per wave, the scene staged as in guide_kernel.  G in {2, 4} sub-samples per
// side (a runtime argument), S = G G.  First the lane traces its S rays in one loop around a single hit_world and keeps (k, t) of each
// in registers (the slot is chosen by compare-and-select: no indexed private array, no scratch); a miss keeps k = -1, t = 0.  Then, on
// registers alone: c(k) = how many sub-samples hit k; layer 0 = the k of the largest c, the smaller k on a tie (the sky, -1, is the
// smallest); layer 1 = the same among the rest (none: the pixel is pure, {-2, 0, 0, 0}); further surfaces are dropped.  Last, in
// sub-sample order from 0, the normal of every sub-sample of the two layers is rebuilt from (t, k) as guide_kernel builds it -- P = O + t D,
// outward = (P - C_k) * inv_r_k, facing the ray; 0 for the sky -- and summed with t; n_l = sum * ((T)1 / (T)c_l) per component, z_l likewise.
// Per pixel: ic = {id_0, id_1, c_0, c_1} and nz[2 lp + l] = {n_l, z_l}.
template <class T, int SRC>
__global__ void __launch_bounds__(256) coverage_kernel(const RenderParams<T> p, int G, int4* __restrict__ ic, Vec4<T>* __restrict__ nz) {
    const T* lds_geom = stage_scene<T, SRC>(p);
    const int W = p.cold.W, rows = p.cold.local_rows;
    const int tiles_x = (W + 7) >> 3, tiles = tiles_x * ((rows + 7) >> 3);
    const int tile = (int)blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63u);
    const int i = (tile % tiles_x) * 8 + (lane & 7), jl = (tile / tiles_x) * 8 + (lane >> 3);
    if (tile >= tiles || i >= W || jl >= rows) return;           // after the staging barrier
    const int j = global_row(jl, p.cold.strip_rows, p.cold.nranks, p.cold.rank);
    const CameraParams<T>& cam = p.cam;
    const V3<T> O = cam.center;
    const int S = G * G;
    constexpr int M = COVERAGE_MAX_SUBSAMPLES;
    int ks[M];
    T ts[M];
#pragma unroll
    for (int q = 0; q < M; ++q) { ks[q] = COVERAGE_NO_LAYER; ts[q] = (T)0; }
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
        const V3<T> D = coverage_direction<T>(cam, i, j, s, G);
        T t = __builtin_huge_val();
        int k = -1;
        hit_world<T, SRC>(p, lds_geom, O, D, dot3(D, D), t, k);      // dot3: the |D|^2 every caller of hit_world passes (not part of a stored value)
        if (k < 0) t = (T)0;
#pragma unroll
        for (int q = 0; q < M; ++q) { ks[q] = q == s ? k : ks[q]; ts[q] = q == s ? t : ts[q]; }
    }
    // the two layers: unused slots hold COVERAGE_NO_LAYER, which no sub-sample has
    int id0 = COVERAGE_NO_LAYER, c0 = 0, id1 = COVERAGE_NO_LAYER, c1 = 0;
#pragma unroll
    for (int q = 0; q < M; ++q) {
        int c = 0;
#pragma unroll
        for (int r = 0; r < M; ++r) c += ks[r] == ks[q] ? 1 : 0;
        const bool used = q < S;
        if (used && (c > c0 || (c == c0 && ks[q] < id0))) { id0 = ks[q]; c0 = c; }
    }
#pragma unroll
    for (int q = 0; q < M; ++q) {
        int c = 0;
#pragma unroll
        for (int r = 0; r < M; ++r) c += ks[r] == ks[q] ? 1 : 0;
        const bool used = q < S && ks[q] != id0;
        if (used && (c > c1 || (c == c1 && ks[q] < id1))) { id1 = ks[q]; c1 = c; }
    }
    T sum[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
    for (int q = 0; q < M; ++q) {
        const int k = ks[q];
        const bool in0 = q < S && k == id0, in1 = q < S && k == id1; // an unused slot, like id1 == COVERAGE_NO_LAYER, matches nobody
        T v[4] = {0, 0, 0, ts[q]};
        if (k >= 0 && (in0 || in1)) {
            const V3<T> D = coverage_direction<T>(cam, i, j, q, G);
            const T t = ts[q];
            const T* rec = p.screen.shade_tbl + 12 * (size_t)k;       // {cx,cy,cz,1/r | ...}
            const V3<T> P = {O.x + t * D.x, O.y + t * D.y, O.z + t * D.z};
            const T inv_r = rec[3];
            V3<T> n = {(P.x - rec[0]) * inv_r, (P.y - rec[1]) * inv_r, (P.z - rec[2]) * inv_r};
            const T dn = (D.x * n.x + D.y * n.y) + D.z * n.z;
            if (!(dn < (T)0)) n = {-n.x, -n.y, -n.z};
            v[0] = n.x; v[1] = n.y; v[2] = n.z;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            sum[0][c] = in0 ? sum[0][c] + v[c] : sum[0][c];
            sum[1][c] = in1 ? sum[1][c] + v[c] : sum[1][c];
        }
    }
    const size_t lp = (size_t)jl * W + i;
    const T s0 = (T)1 / (T)c0;
    Vec4<T> l0 = {sum[0][0] * s0, sum[0][1] * s0, sum[0][2] * s0, sum[0][3] * s0}, l1 = {(T)0, (T)0, (T)0, (T)0};
    if (c1 > 0) {
        const T s1 = (T)1 / (T)c1;
        l1 = {sum[1][0] * s1, sum[1][1] * s1, sum[1][2] * s1, sum[1][3] * s1};
    }
    ic[lp] = make_int4(id0, id1, c0, c1);
    nz[2 * lp] = l0; nz[2 * lp + 1] = l1;
}

// ---- The resolve: one lane per pixel, 16 x 16 pixels per workgroup.  Only a mixed pixel (id_1 != -2) works: its window of (2 r + 1)^2
// taps, dy then dx in -r..r, served by L1/L2.  A tap counts when it lies in the frame and is pure; it belongs to layer l when its id is
// id_l (the two ids differ, so to one layer at most), with the weight of its FIRST-HIT guides against the layer's mean normal and depth:
//   d = N_q - n_l, en = (d.x d.x + d.y d.y) + d.z d.z, dz = Z_q - z_l, e = en i_n + (dz dz) i_z, w = 1 / (1 + e)
//   Sx = Sx + w (g_q g_q) per channel, Wt = Wt + w
// A layer with Wt > 0 is found: F_l = Sx / Wt, a_l = (T)c_l / (T)S.  R = 0, rest = 1; per found layer in order R = R + a_l F_l,
// rest = rest - a_l; then R = R + rest L_p, L_p = g_p g_p.  beta_one (prior = +inf, decided on the host): out = R; otherwise
// beta = prior / (prior + n_eff) and out = L_p + beta (R - L_p); stored out > 0 ? sqrt(out) : 0.  n_eff: the pixel's history length (cm,
// when the filter read the temporal image), else its sample count (counts, or n_uniform for all).  Pure pixels and mixed pixels without
// a found layer are not written, so the kernel reads only pure pixels and its own and writes only mixed ones: in place is race-free.
template <class T>
__global__ void __launch_bounds__(256) edge_resolve_kernel(FrameShape f, int r, int S, T i_n, T i_z, T prior, int beta_one, const int4* __restrict__ ic,
                                                           const Vec4<T>* __restrict__ nz, const Vec4<T>* __restrict__ nd, const int32_t* __restrict__ counts,
                                                           int n_uniform, const Vec4<T>* __restrict__ cm, T* g, unsigned* __restrict__ resolved) {
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15u), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    if (x >= f.W || y >= f.local_rows) return;
    const size_t lp = (size_t)y * f.W + x;
    const int4 own = ic[lp];
    if (own.y == COVERAGE_NO_LAYER) return;                      // pure
    const Vec4<T> l0 = nz[2 * lp], l1 = nz[2 * lp + 1];
    T sx[2][3] = {{0, 0, 0}, {0, 0, 0}}, wt[2] = {0, 0};
    for (int dy = -r; dy <= r; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= f.local_rows) continue;
        for (int dx = -r; dx <= r; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= f.W) continue;
            const size_t q = (size_t)qy * f.W + qx;
            const int4 tap = ic[q];
            const bool in0 = tap.x == own.x, in1 = tap.x == own.y;
            if (tap.y != COVERAGE_NO_LAYER || !(in0 || in1)) continue;
            const Vec4<T> gq = nd[q], l = in0 ? l0 : l1;
            const T ddx = gq.x - l.x, ddy = gq.y - l.y, ddz = gq.z - l.z;
            const T en = (ddx * ddx + ddy * ddy) + ddz * ddz;
            const T dz = gq.w - l.w;
            const T e = en * i_n + (dz * dz) * i_z;
            const T w = (T)1 / ((T)1 + e);
            const T cx = g[3 * q], cy = g[3 * q + 1], cz = g[3 * q + 2];
            const T lx = cx * cx, ly = cy * cy, lz = cz * cz;
            sx[0][0] = in0 ? sx[0][0] + w * lx : sx[0][0]; sx[0][1] = in0 ? sx[0][1] + w * ly : sx[0][1]; sx[0][2] = in0 ? sx[0][2] + w * lz : sx[0][2];
            sx[1][0] = in1 ? sx[1][0] + w * lx : sx[1][0]; sx[1][1] = in1 ? sx[1][1] + w * ly : sx[1][1]; sx[1][2] = in1 ? sx[1][2] + w * lz : sx[1][2];
            wt[0] = in0 ? wt[0] + w : wt[0];
            wt[1] = in1 ? wt[1] + w : wt[1];
        }
    }
    const bool found0 = wt[0] > (T)0, found1 = wt[1] > (T)0;
    if (!found0 && !found1) return;
    const T gp[3] = {g[3 * lp], g[3 * lp + 1], g[3 * lp + 2]};
    const T cnt[2] = {(T)own.z / (T)S, (T)own.w / (T)S};
    T beta = (T)1;
    if (!beta_one) {
        const T n_eff = cm ? cm[lp].w : (T)(counts ? counts[lp] : n_uniform);
        beta = prior / (prior + n_eff);
    }
    T rest = (T)1;
    if (found0) rest = rest - cnt[0];
    if (found1) rest = rest - cnt[1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const T L = gp[c] * gp[c];
        T R = (T)0;
        if (found0) R = R + cnt[0] * (sx[0][c] / wt[0]);
        if (found1) R = R + cnt[1] * (sx[1][c] / wt[1]);
        R = R + rest * L;
        const T out = beta_one ? R : L + beta * (R - L);
        g[3 * lp + c] = out > (T)0 ? Real<T>::sqrt(out) : (T)0;
    }
    atomicAdd(resolved, 1u);
}

}  // namespace
