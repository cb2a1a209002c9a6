// denoise_variance.h -- variance-guided denoising of adaptive accumulations: the per-pixel variance of the mean luminance
// (rtiow_read_variance) and the a-trous filter whose colour edge-stop follows it (rtiow_denoise_variance; the spatial half of SVGF,
// Schied et al. 2017, in the rational-weight form of rtiow_denoise)
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, after denoise.h; internal linkage).
//
// As in denoise.h every value is defined operation by operation and evaluated in T with plain * + - /,
// unfused (-ffp-contract=off), so a numpy restatement gives the same bits.  The variance plane alone passes through double, with the
// expressions and order of relative_error (adaptive.h).
#pragma once
#include "denoise.h"

namespace {

// ---- V_p, the estimated variance of pixel p's MEAN luminance, from its adaptive record and count: in double m = Y(acc) / n,
// var = max(0, (s2 - n m^2) / (n - 1)), V_p = (T)(var / n); 0 below two samples (no estimate).  sqrt(var / n) / (m + 1e-3) is the
// err_p adaptive_finish_kernel stores.
template <class T>
__device__ __forceinline__ T mean_variance(V3<T> acc, T s2, int32_t n) {
    if (n < 2) return (T)0;
    const double dn = (double)n;
    const double mean = (double)luminance<T>(acc) / dn;
    double var = ((double)s2 - dn * mean * mean) / (dn - 1.0);
    if (!(var > 0.0)) var = 0.0;
    return (T)(var / dn);
}

// The variance plane of the accumulation, local_rows x W T: one lane per pixel, like linear_kernel.
template <class T>
__global__ void __launch_bounds__(256) variance_plane_kernel(size_t npix, const unsigned char* __restrict__ mid, const int32_t* __restrict__ counts,
                                                             T* __restrict__ out) {
    const size_t lp = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= npix) return;
    const MidState<T> r = load_record<T>(mid, lp);
    out[lp] = mean_variance<T>({r.acc[0], r.acc[1], r.acc[2]}, adapt_s2<T>(r), counts[lp]);
}

// ---- One level of the variance-guided filter.  Frame, taps, tap order, kern, the guide terms en, ea, ez and the gamma of the last
// level are denoise_level_kernel's; the colour term's weight is the pixel's own:
//   g_p = (sum b V_q) / (sum b) over the 3 x 3 neighbours at step 1 (dy then dx in -1..1, b = B[dx+1] B[dy+1], B = {1/4, 1/2, 1/4},
//         those outside the frame skipped, sums from 0),
//   i_p = f_k / (sv2 g_p + eps), f_k = (T)(4^k), sv2 = (T)(sigma_variance^2), eps = (T)1e-8; 0 when the host turned the term off,
//   e = ((ec i_p + en i_n) + ea i_a) + ez i_z,  w = kern / (1 + e),
//   C'_p = (sum w C_q) / (sum w),  V'_p = (sum (w w) V_q) / ((sum w) (sum w)).
// Level 0 reads the linear colour from the accumulation records (mid != nullptr), later levels the previous level's buffer; V comes
// from a plane at every level (variance_plane_kernel wrote level 0's).  The last level stores no variance (vout == nullptr).
// 16 x 16 pixels per workgroup.
template <class T> struct VarianceWeights { T sv2, fk, eps, in, ia, iz; int colour_on; };

// What a tap reads of a pixel: {colour, V | normal, depth | albedo, 0}, and the sums of a pixel's taps.
template <class T> struct TapPixel { T c[3], v, nd[4], a[3]; };
template <class T> struct TapSums { T sx = 0, sy = 0, sz = 0, sw = 0, su = 0; };

template <class T>
__device__ __forceinline__ void variance_tap(TapSums<T>& s, T kern, T ip, const VarianceWeights<T>& fw, const TapPixel<T>& p, const TapPixel<T>& q) {
    const T dcx = q.c[0] - p.c[0], dcy = q.c[1] - p.c[1], dcz = q.c[2] - p.c[2];
    const T dnx = q.nd[0] - p.nd[0], dny = q.nd[1] - p.nd[1], dnz = q.nd[2] - p.nd[2], dz = q.nd[3] - p.nd[3];
    const T dax = q.a[0] - p.a[0], day = q.a[1] - p.a[1], daz = q.a[2] - p.a[2];
    const T ec = (dcx * dcx + dcy * dcy) + dcz * dcz;
    const T en = (dnx * dnx + dny * dny) + dnz * dnz;
    const T ea = (dax * dax + day * day) + daz * daz;
    const T ez = dz * dz;
    const T e = ((ec * ip + en * fw.in) + ea * fw.ia) + ez * fw.iz;
    const T w = kern / ((T)1 + e);
    s.sx = s.sx + w * q.c[0]; s.sy = s.sy + w * q.c[1]; s.sz = s.sz + w * q.c[2];
    s.sw = s.sw + w;
    s.su = s.su + (w * w) * q.v;
}

// The end of a pixel: C' (gamma-encoded on the last level) and V'.
template <class T>
__device__ __forceinline__ void variance_store(const TapSums<T>& s, size_t lp, T* __restrict__ cout, T* __restrict__ vout, int gamma) {
    T o[3] = {s.sx / s.sw, s.sy / s.sw, s.sz / s.sw};
    if (gamma) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = o[c] > (T)0 ? Real<T>::sqrt(o[c]) : (T)0;
    }
    cout[3 * lp] = o[0]; cout[3 * lp + 1] = o[1]; cout[3 * lp + 2] = o[2];
    if (vout) vout[lp] = s.su / (s.sw * s.sw);
}

// A pixel's tap values from global memory.
template <class T>
__device__ __forceinline__ TapPixel<T> load_tap_pixel(size_t q, const unsigned char* __restrict__ mid, const int32_t* __restrict__ counts, const T* __restrict__ cin,
                                                      const T* __restrict__ vin, const T* __restrict__ nd, const T* __restrict__ alb) {
    TapPixel<T> t;
    if (mid) { const V3<T> c = linear_colour<T>(mid, counts, 0, q); t.c[0] = c.x; t.c[1] = c.y; t.c[2] = c.z; }
    else { t.c[0] = cin[3 * q]; t.c[1] = cin[3 * q + 1]; t.c[2] = cin[3 * q + 2]; }
    t.v = vin[q];
#pragma unroll
    for (int k = 0; k < 4; ++k) t.nd[k] = nd[4 * q + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t.a[k] = alb[4 * q + k];
    return t;
}

// The form whose taps are served by L1/L2, every step.
template <class T>
__global__ void __launch_bounds__(256) variance_filter_kernel(FrameShape f, int step, VarianceWeights<T> fw, const unsigned char* __restrict__ mid,
                                                              const int32_t* __restrict__ counts, const T* __restrict__ cin,
                                                              const T* __restrict__ vin, const T* __restrict__ nd, const T* __restrict__ alb,
                                                              T* __restrict__ cout, T* __restrict__ vout, int gamma) {
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15u), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    if (x >= f.W || y >= f.local_rows) return;
    const size_t lp = (size_t)y * f.W + x;
    T ip = (T)0;
    if (fw.colour_on) {
        const T B[3] = {(T)0.25, (T)0.5, (T)0.25};
        T gv = 0, gw = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= f.local_rows) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= f.W) continue;
                const T b = B[dx + 1] * B[dy + 1];
                gv = gv + b * vin[(size_t)qy * f.W + qx];
                gw = gw + b;
            }
        }
        const T g = gv / gw;
        ip = fw.fk / (fw.sv2 * g + fw.eps);
    }
    const TapPixel<T> p = load_tap_pixel<T>(lp, mid, counts, cin, vin, nd, alb);
    const T K[5] = {(T)0.0625, (T)0.25, (T)0.375, (T)0.25, (T)0.0625};
    TapSums<T> s;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * step;
        if (qy < 0 || qy >= f.local_rows) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * step;
            if (qx < 0 || qx >= f.W) continue;
            variance_tap<T>(s, K[dx + 2] * K[dy + 2], ip, fw, p, load_tap_pixel<T>((size_t)qy * f.W + qx, mid, counts, cin, vin, nd, alb));
        }
    }
    variance_store<T>(s, lp, cout, vout, gamma);
}

// The same level with the workgroup's taps staged in LDS, for the small steps: the (16 + 4 step)^2 pixels around its 16 x 16 lie in
// TILE_PLANES planes of 16-byte slots -- the 12 T {colour, V | normal, depth | albedo, 0} of a pixel cut into float4s (3 planes) or
// double2s (6) --, a tile row TILE_PITCH = 32 slots apart, so that the 16 lanes ds_read_b128 serves per cycle -- 8 of one row and 8
// of the next, at complementary columns -- fall on 16 different slots of the 256-byte bank row.  Pixels outside the frame are
// neither written nor read.  Dynamic LDS: variance_tile_bytes.  Same operations in the same order as variance_filter_kernel.
constexpr int TILE_PITCH = 32;
template <class T> constexpr int TILE_PLANES = 3 * (int)sizeof(T) / 4;
template <class T> inline size_t variance_tile_bytes(int step) { return (size_t)(16 + 4 * step) * TILE_PITCH * 16 * TILE_PLANES<T>; }

template <class T>
__global__ void __launch_bounds__(256) variance_tile_kernel(FrameShape f, int step, VarianceWeights<T> fw, const unsigned char* __restrict__ mid,
                                                            const int32_t* __restrict__ counts, const T* __restrict__ cin,
                                                            const T* __restrict__ vin, const T* __restrict__ nd, const T* __restrict__ alb,
                                                            T* __restrict__ cout, T* __restrict__ vout, int gamma) {
    constexpr int E = 16 / (int)sizeof(T);                   // T per slot
    typedef T slot_t __attribute__((ext_vector_type(E)));
    extern __shared__ __attribute__((aligned(16))) unsigned char variance_tile_lds[];
    slot_t* tile = reinterpret_cast<slot_t*>(variance_tile_lds);
    const int side = 16 + 4 * step, halo = 2 * step;
    const int plane = side * TILE_PITCH;                      // slots per plane
    const int x0 = (int)blockIdx.x * 16 - halo, y0 = (int)blockIdx.y * 16 - halo;
    for (int t = (int)threadIdx.x; t < side * side; t += 256) {
        const int ty = t / side, tx = t - ty * side;
        const int gx = x0 + tx, gy = y0 + ty;
        if (gx < 0 || gx >= f.W || gy < 0 || gy >= f.local_rows) continue;
        const TapPixel<T> q = load_tap_pixel<T>((size_t)gy * f.W + gx, mid, counts, cin, vin, nd, alb);
        const T flat[12] = {q.c[0], q.c[1], q.c[2], q.v, q.nd[0], q.nd[1], q.nd[2], q.nd[3], q.a[0], q.a[1], q.a[2], (T)0};
#pragma unroll
        for (int j = 0; j < TILE_PLANES<T>; ++j) {
            slot_t v;
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = flat[j * E + e];
            tile[j * plane + ty * TILE_PITCH + tx] = v;
        }
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & 15u) + halo, ly = (int)(threadIdx.x >> 4) + halo;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= f.W || y >= f.local_rows) return;               // after the barrier
    auto staged = [&](int tx, int ty) __attribute__((always_inline)) -> TapPixel<T> {
        T flat[12];
#pragma unroll
        for (int j = 0; j < TILE_PLANES<T>; ++j) {
            const slot_t v = tile[j * plane + ty * TILE_PITCH + tx];
#pragma unroll
            for (int e = 0; e < E; ++e) flat[j * E + e] = v[e];
        }
        return {{flat[0], flat[1], flat[2]}, flat[3], {flat[4], flat[5], flat[6], flat[7]}, {flat[8], flat[9], flat[10]}};
    };
    constexpr int VP = 3 / E, VE = 3 % E;                     // V's plane and element: flat[3]
    T ip = (T)0;
    if (fw.colour_on) {
        const T B[3] = {(T)0.25, (T)0.5, (T)0.25};
        T gv = 0, gw = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= f.local_rows) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= f.W) continue;
                const T b = B[dx + 1] * B[dy + 1];
                gv = gv + b * tile[VP * plane + (ly + dy) * TILE_PITCH + (lx + dx)][VE];
                gw = gw + b;
            }
        }
        const T g = gv / gw;
        ip = fw.fk / (fw.sv2 * g + fw.eps);
    }
    const TapPixel<T> p = staged(lx, ly);
    const T K[5] = {(T)0.0625, (T)0.25, (T)0.375, (T)0.25, (T)0.0625};
    TapSums<T> s;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * step;
        if (qy < 0 || qy >= f.local_rows) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * step;
            if (qx < 0 || qx >= f.W) continue;
            variance_tap<T>(s, K[dx + 2] * K[dy + 2], ip, fw, p, staged(lx + dx * step, ly + dy * step));
        }
    }
    variance_store<T>(s, (size_t)y * f.W + x, cout, vout, gamma);
}

}  // namespace
