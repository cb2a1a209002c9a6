// denoise.h -- denoised previews of progressive rendering: first-hit guide buffers (rtiow_render_guides), the linear read of the
// accumulation (rtiow_read_linear) and the edge-avoiding a-trous filter (rtiow_denoise, after Dammertz et al. 2010)
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, in this order; internal linkage).
//
// Every value here is defined operation by operation and evaluated in T with plain * + - / and sqrt:
// no RT_FMA, madd3 or dot3, which emit true FMAs.  -ffp-contract=off keeps the plain operations unfused, so a numpy restatement
// gives the same bits.
#pragma once
#include "adaptive.h"           // FrameShape, and through it the render kernels

namespace {

// ---- Linear colour of a pixel of the accumulation: c = n > 0 ? acc * ((T)1 / (T)n) : 0, n = the uniform count of a plain accumulation
// (counts == nullptr) or the pixel's own count (adaptive).  store_pixel applies the same product before its sqrt.
template <class T>
__device__ __forceinline__ V3<T> linear_colour(const unsigned char* __restrict__ mid, const int32_t* __restrict__ counts, int n_uniform, size_t lp) {
    const MidState<T> r = load_record<T>(mid, lp);
    const int n = counts ? counts[lp] : n_uniform;
    if (n <= 0) return {(T)0, (T)0, (T)0};
    const T s = (T)1 / (T)n;
    return {r.acc[0] * s, r.acc[1] * s, r.acc[2] * s};
}

// The linear image of the accumulation, local_rows x W x 3 T, for rtiow_read_linear.
template <class T>
__global__ void __launch_bounds__(256) linear_kernel(size_t npix, const unsigned char* __restrict__ mid, const int32_t* __restrict__ counts, int n_uniform,
                                                     T* __restrict__ out) {
    const size_t lp = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= npix) return;
    const V3<T> c = linear_colour<T>(mid, counts, n_uniform, lp);
    out[3 * lp] = c.x; out[3 * lp + 1] = c.y; out[3 * lp + 2] = c.z;
}

// ---- First-hit guides: one lane per local pixel, one 8x8 tile per wave (coherent rays for the grid walk), the scene staged by
// stage_scene as in the render kernels (p is the kernel's first argument: hit_world reads its grid and screen through the kernarg
// segment).  The ray of pixel (i, j) has no jitter and no defocus: O = centre, D = ((pixel00 + i du) + j dv) - O.  On a hit at sphere
// k: P = O + t D, outward = (P - C_k) * inv_r_k, the normal faces the ray; albedo {r,g,b} (lambertian, metal) or {1,1,1} (dielectric);
// depth t.  A miss stores zeros.  Two 4-T vectors per pixel: nd = {normal, depth}, alb = {albedo, 0}.
template <class T, int SRC>
__global__ void __launch_bounds__(256) guide_kernel(const RenderParams<T> p, T* __restrict__ nd, T* __restrict__ alb) {
    const T* lds_geom = stage_scene<T, SRC>(p);
    const int W = p.cold.W, rows = p.cold.local_rows;
    const int tiles_x = (W + 7) >> 3, tiles = tiles_x * ((rows + 7) >> 3);
    const int tile = (int)blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63u);
    const int i = (tile % tiles_x) * 8 + (lane & 7), jl = (tile / tiles_x) * 8 + (lane >> 3);
    if (tile >= tiles || i >= W || jl >= rows) return;           // after the staging barrier
    const int j = global_row(jl, p.cold.strip_rows, p.cold.nranks, p.cold.rank);
    const CameraParams<T>& cam = p.cam;
    const T fi = (T)i, fj = (T)j;
    const V3<T> O = cam.center;
    const V3<T> ps = {(cam.pixel00.x + fi * cam.du.x) + fj * cam.dv.x, (cam.pixel00.y + fi * cam.du.y) + fj * cam.dv.y,
                      (cam.pixel00.z + fi * cam.du.z) + fj * cam.dv.z};
    const V3<T> D = {ps.x - O.x, ps.y - O.y, ps.z - O.z};
    T t = __builtin_huge_val();
    int k = -1;
    hit_world<T, SRC>(p, lds_geom, O, D, dot3(D, D), t, k);      // dot3: the |D|^2 every caller of hit_world passes (not part of a guide value)
    const size_t lp = (size_t)jl * W + i;
    T g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (k >= 0) {
        const T* rec = p.screen.shade_tbl + 12 * (size_t)k;       // {cx,cy,cz,1/r | albedo r,g,b,fuzz | eta,1/eta,type,0}
        const V3<T> P = {O.x + t * D.x, O.y + t * D.y, O.z + t * D.z};
        const T inv_r = rec[3];
        V3<T> n = {(P.x - rec[0]) * inv_r, (P.y - rec[1]) * inv_r, (P.z - rec[2]) * inv_r};
        const T dn = (D.x * n.x + D.y * n.y) + D.z * n.z;
        if (!(dn < (T)0)) n = {-n.x, -n.y, -n.z};
        const bool glass = (int)rec[10] == RTIOW_DIELECTRIC;
        g[0] = n.x; g[1] = n.y; g[2] = n.z; g[3] = t;
        g[4] = glass ? (T)1 : rec[4]; g[5] = glass ? (T)1 : rec[5]; g[6] = glass ? (T)1 : rec[6];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { nd[4 * lp + q] = g[q]; alb[4 * lp + q] = g[4 + q]; }
}

// ---- One level of the edge-avoiding a-trous filter: taps (dx, dy) in -2..2 at step s, in row order (dy outer), those outside the
// frame skipped; kern = K[dx+2] K[dy+2] with K = {1/16, 1/4, 3/8, 1/4, 1/16}; e = ((ec ic + en in) + ea ia) + ez iz from the squared
// distances of colour, normal, albedo and depth; w = kern / (1 + e); out = (sum w c_q) / (sum w).  Level 0 reads the linear colour
// straight from the accumulation records (mid != nullptr), later levels the previous level's T buffer.  The last level writes
// x > 0 ? sqrt(x) : 0 like store_pixel (gamma != 0).  16 x 16 pixels per workgroup; the taps are served by L1/L2.
template <class T> struct FilterWeights { T ic, in, ia, iz; };

template <class T>
__global__ void __launch_bounds__(256) denoise_level_kernel(FrameShape f, int step, FilterWeights<T> fw, const unsigned char* __restrict__ mid,
                                                            const int32_t* __restrict__ counts, int n_uniform, const T* __restrict__ cin,
                                                            const T* __restrict__ nd, const T* __restrict__ alb, T* __restrict__ cout, int gamma) {
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15u), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    if (x >= f.W || y >= f.local_rows) return;
    auto colour = [&](size_t q) __attribute__((always_inline)) -> V3<T> {
        if (mid) return linear_colour<T>(mid, counts, n_uniform, q);
        return {cin[3 * q], cin[3 * q + 1], cin[3 * q + 2]};
    };
    const size_t lp = (size_t)y * f.W + x;
    const V3<T> cp = colour(lp);
    const T npx = nd[4 * lp], npy = nd[4 * lp + 1], npz = nd[4 * lp + 2], zp = nd[4 * lp + 3];
    const T apx = alb[4 * lp], apy = alb[4 * lp + 1], apz = alb[4 * lp + 2];
    const T K[5] = {(T)0.0625, (T)0.25, (T)0.375, (T)0.25, (T)0.0625};
    T sx = 0, sy = 0, sz = 0, sw = 0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * step;
        if (qy < 0 || qy >= f.local_rows) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * step;
            if (qx < 0 || qx >= f.W) continue;
            const size_t q = (size_t)qy * f.W + qx;
            const T kern = K[dx + 2] * K[dy + 2];
            const V3<T> cq = colour(q);
            const T dcx = cq.x - cp.x, dcy = cq.y - cp.y, dcz = cq.z - cp.z;
            const T dnx = nd[4 * q] - npx, dny = nd[4 * q + 1] - npy, dnz = nd[4 * q + 2] - npz, dz = nd[4 * q + 3] - zp;
            const T dax = alb[4 * q] - apx, day = alb[4 * q + 1] - apy, daz = alb[4 * q + 2] - apz;
            const T ec = (dcx * dcx + dcy * dcy) + dcz * dcz;
            const T en = (dnx * dnx + dny * dny) + dnz * dnz;
            const T ea = (dax * dax + day * day) + daz * daz;
            const T ez = dz * dz;
            const T e = ((ec * fw.ic + en * fw.in) + ea * fw.ia) + ez * fw.iz;
            const T w = kern / ((T)1 + e);
            sx = sx + w * cq.x; sy = sy + w * cq.y; sz = sz + w * cq.z;
            sw = sw + w;
        }
    }
    T o[3] = {sx / sw, sy / sw, sz / sw};
    if (gamma) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = o[c] > (T)0 ? Real<T>::sqrt(o[c]) : (T)0;
    }
    cout[3 * lp] = o[0]; cout[3 * lp + 1] = o[1]; cout[3 * lp + 2] = o[2];
}

}  // namespace
