// upscale.h -- guided upscaling (rtiow_upscale): a preview at F times the traced resolution.  Every output pixel traces its own primary
// ray -- a sub-pixel of the traced pixel it lies in, the lattice rtiow_render_coverage traces -- and gathers the colour of the four traced
// pixels around it, each weighed bilinearly, by how well its first-hit guides match what the output pixel's ray hit, and (use_coverage) by
// the share of it that is the surface the output pixel sees.
// Part of the gfx950 translation units rtiow_upscale.hip and, over the device grid, rtiow_large_upscale.hip: the only ones that
// instantiate the kernel (internal linkage).
//
// Every value is defined operation by operation and evaluated in T with plain * + - / and sqrt, as in
// denoise.h: no RT_FMA, madd3 or dot3 for a stored value.  -ffp-contract=off keeps the plain operations unfused, so a numpy restatement
// gives the same bits.
#pragma once
#include "edge_resolve.h"       // COVERAGE_NO_LAYER, Vec4, and through it guide_kernel, whose normal, albedo and depth these are

namespace {

constexpr int UPSCALE_MIN_FACTOR = 2, UPSCALE_MAX_FACTOR = 4;
constexpr int UPSCALE_WAVES = 4;                                // both kernels run as workgroups of four waves, an 8 x 8 output tile each
constexpr int UPSCALE_TALLY_BYTES = UPSCALE_WAVES * (int)sizeof(unsigned);     // one word per wave of the workgroup, behind the staged scene
// The count is kept in UPSCALE_COUNTERS words, UPSCALE_COUNTER_STRIDE words apart, which the host sums: a 3840 x 2160 output has 32400
// workgroups, and their atomics on ONE word ran one after the other, about 12 ns each -- a floor of 0.4 ms under a 0.2 to 0.4 ms kernel
// (DESIGN.md section 4.22).
constexpr int UPSCALE_COUNTERS = 64, UPSCALE_COUNTER_STRIDE = 64;

// What the launch hands over beside the render parameters.  source: RTIOW_UPSCALE_*, which of g (DENOISED: 3 T per pixel, gamma-encoded),
// mid / counts / n_uniform (LINEAR: linear_colour's arguments) and cm (HISTORY: {C.rgb, M}) is read.  S = G G of the coverage layers ic.
template <class T>
struct UpscaleParams {
    int F, source, use_coverage, S;
    T i_n, i_a, i_z;
    int n_uniform, tally_offset;
    const unsigned char* mid;
    const int32_t* counts;
    const T* g;
    const Vec4<T>* cm;
    const Vec4<T>* nd;
    const Vec4<T>* alb;
    const int4* ic;
};

// ---- What upscale_kernel and upscale_wide_kernel (upscale_wide.h) share, each stated once: the output pixel and its ray, the colour of a
// traced pixel, one tap, the resolve with its store, and the count.  Every value of INTEGRATION.md sections 22 and 23 that does not depend
// on the taps' layout is defined here, operation by operation; the kernels add where the taps lie and what b each one carries.

// Output pixel (I, J) of the F W x F rows image.  i = I / F, a = I - F i (j, b likewise): the ray is sub-sample (a, b) of traced pixel (i, j)
// on the F x F lattice -- oa = ((T)a + 0.5) / F - 0.5, fx = (T)i + oa, D = ((pixel00 + fx du) + fy dv) - O -- with N, A, Z of its hit as
// guide_kernel builds them (a miss: k = -1, zeros).  x0 = oa < 0 ? i - 1 : i, gx = oa < 0 ? 1 + oa : oa (y0, gy likewise): the traced pixel at
// or before the ray on each axis and the ray's place between it and the next, in [0, 1).
template <class T>
struct UpscalePixel {
    int x0, y0, k;
    T gx, gy;
    V3<T> N, A;
    T Z;
};

template <class T, int SRC>
__device__ __forceinline__ UpscalePixel<T> upscale_pixel(const RenderParams<T>& p, const T* lds_geom, const int I, const int J, const int F) {
    UpscalePixel<T> px;
    const int i = I / F, j = J / F, a = I - F * i, b = J - F * j;
    const T fF = (T)F;
    const T oa = ((T)a + (T)0.5) / fF - (T)0.5, ob = ((T)b + (T)0.5) / fF - (T)0.5;
    const T fx = (T)i + oa, fy = (T)j + ob;
    const CameraParams<T>& cam = p.cam;
    const V3<T> O = cam.center;
    const V3<T> ps = {(cam.pixel00.x + fx * cam.du.x) + fy * cam.dv.x, (cam.pixel00.y + fx * cam.du.y) + fy * cam.dv.y,
                      (cam.pixel00.z + fx * cam.du.z) + fy * cam.dv.z};
    const V3<T> D = {ps.x - O.x, ps.y - O.y, ps.z - O.z};
    T t = __builtin_huge_val();
    int k = -1;
    hit_world<T, SRC>(p, lds_geom, O, D, dot3(D, D), t, k);      // dot3: the |D|^2 every caller of hit_world passes (not part of a stored value)
    V3<T> N = {(T)0, (T)0, (T)0}, A = {(T)0, (T)0, (T)0};
    T Z = (T)0;
    if (k >= 0) {
        const T* rec = p.screen.shade_tbl + 12 * (size_t)k;       // {cx,cy,cz,1/r | albedo r,g,b,fuzz | eta,1/eta,type,0}
        const V3<T> P = {O.x + t * D.x, O.y + t * D.y, O.z + t * D.z};
        const T inv_r = rec[3];
        N = {(P.x - rec[0]) * inv_r, (P.y - rec[1]) * inv_r, (P.z - rec[2]) * inv_r};
        const T dn = (D.x * N.x + D.y * N.y) + D.z * N.z;
        if (!(dn < (T)0)) N = {-N.x, -N.y, -N.z};
        const bool glass = (int)rec[10] == RTIOW_DIELECTRIC;
        A = {glass ? (T)1 : rec[4], glass ? (T)1 : rec[5], glass ? (T)1 : rec[6]};
        Z = t;
    }
    px.k = k;
    px.x0 = oa < (T)0 ? i - 1 : i; px.y0 = ob < (T)0 ? j - 1 : j;
    px.gx = oa < (T)0 ? (T)1 + oa : oa; px.gy = ob < (T)0 ? (T)1 + ob : ob;
    px.N = N; px.A = A; px.Z = Z;
    return px;
}

// The colour of traced pixel q from u.source into c.x, c.y, c.z (C: V3<T>, or the Vec4<T> a kernel stages), and whether q holds colour at
// all -- DENOISED: always, the stored value squared; LINEAR: n_q > 0, linear_colour's; HISTORY: M_q > 0, C.rgb.  c is not to be read on false.
template <class T, class C>
__device__ __forceinline__ bool upscale_source_colour(const UpscaleParams<T>& u, const size_t q, C& c) {
    if (u.source == RTIOW_UPSCALE_DENOISED) {
        const T g0 = u.g[3 * q], g1 = u.g[3 * q + 1], g2 = u.g[3 * q + 2];
        c.x = g0 * g0; c.y = g1 * g1; c.z = g2 * g2;
        return true;
    }
    if (u.source == RTIOW_UPSCALE_LINEAR) {
        if ((u.counts ? u.counts[q] : u.n_uniform) <= 0) return false;
        const V3<T> l = linear_colour<T>(u.mid, u.counts, u.n_uniform, q);
        c.x = l.x; c.y = l.y; c.z = l.z;
        return true;
    }
    const Vec4<T> cm = u.cm[q];
    c.x = cm.x; c.y = cm.y; c.z = cm.z;
    return cm.w > (T)0;
}

// One tap that counts: b = bw, its colour c, {N, Z} = nq, albedo = aq.xyz, and its coverage layers *layers (global memory or LDS), read
// only under use_coverage.  S1, W1: the taps by b and the guides; Sp, Wp: those of them that hold the surface the output pixel sees, by their
// share of it -- four separate locals of the kernel: as members of one struct the compiler pairs S1.z with W1 and Sp.z with Wp into packed
// additions (the same sums, another instruction mix than the kernels had).  d = N_q - N, en = (d.x d.x + d.y d.y) + d.z d.z, ea the same of the albedo, ez = (Z_q - Z)^2,
// e = (en i_n + ea i_a) + ez i_z, w = b / (1 + e); S1 = S1 + w c_q, W1 = W1 + w.  use_coverage: m = the count of q's layer whose id is k (0:
// none); m > 0: wp = w ((T)m / (T)S), Sp = Sp + wp c_q, Wp = Wp + wp.
template <class T, class C>
__device__ __forceinline__ void upscale_tap(const UpscaleParams<T>& u, const UpscalePixel<T>& px, const T bw, const C& c, const Vec4<T>& nq, const Vec4<T>& aq,
                                            const int4* layers, T (&s1)[3], T& w1, T (&sp)[3], T& wp_sum) {
    const V3<T>& N = px.N;
    const V3<T>& A = px.A;
    const T dnx = nq.x - N.x, dny = nq.y - N.y, dnz = nq.z - N.z, dz = nq.w - px.Z;
    const T dax = aq.x - A.x, day = aq.y - A.y, daz = aq.z - A.z;
    const T en = (dnx * dnx + dny * dny) + dnz * dnz;
    const T ea = (dax * dax + day * day) + daz * daz;
    const T ez = dz * dz;
    const T e = (en * u.i_n + ea * u.i_a) + ez * u.i_z;
    const T w = bw / ((T)1 + e);
    s1[0] = s1[0] + w * c.x; s1[1] = s1[1] + w * c.y; s1[2] = s1[2] + w * c.z;
    w1 = w1 + w;
    if (u.use_coverage) {
        const int4 l = *layers;
        const int m = l.x == px.k ? l.z : (l.y == px.k ? l.w : 0);
        if (m > 0) {
            const T wp = w * ((T)m / (T)u.S);
            sp[0] = sp[0] + wp * c.x; sp[1] = sp[1] + wp * c.y; sp[2] = sp[2] + wp * c.z;
            wp_sum = wp_sum + wp;
        }
    }
}

// out = Wp > 0 ? Sp / Wp : W1 > 0 ? S1 / W1 : 0, stored out > 0 ? sqrt(out) : 0 at output pixel op.  Returns Wp > 0: the share decided it.
template <class T>
__device__ __forceinline__ bool upscale_resolve(const T (&s1)[3], const T w1, const T (&sp)[3], const T wp_sum, T* __restrict__ out, const size_t op) {
    const bool shared_tap = wp_sum > (T)0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const T v = shared_tap ? sp[ch] / wp_sum : (w1 > (T)0 ? s1[ch] / w1 : (T)0);
        out[3 * op + ch] = v > (T)0 ? Real<T>::sqrt(v) : (T)0;
    }
    return shared_tap;
}

// covered counts the pixels with Wp > 0: one ballot per wave into its word of LDS, one global atomic per workgroup of UPSCALE_WAVES waves, on the
// word of covered[] that the workgroup's number picks (UPSCALE_COUNTERS).  Every lane of the workgroup comes here: it holds a barrier.
// wave and lane are the kernel's own values: recomputed from threadIdx.x here they cost upscale_wide_kernel two VGPRs, and with them
// upscale_wide_kernel<double, 0> a wave per SIMD (82 VGPRs: 5 waves instead of 6).
__device__ __forceinline__ void upscale_count(const bool shared_tap, const int wave, const int lane, unsigned* tally, unsigned* __restrict__ covered) {
    const unsigned long long votes = __ballot(shared_tap);
    if (lane == 0) tally[wave] = (unsigned)__popcll(votes);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned sum = 0;
#pragma unroll
        for (int wv = 0; wv < UPSCALE_WAVES; ++wv) sum += tally[wv];
        if (sum) atomicAdd(covered + (size_t)(blockIdx.x % (unsigned)UPSCALE_COUNTERS) * UPSCALE_COUNTER_STRIDE, sum);
    }
}

// ---- One lane per output pixel (I, J) of the F W x F rows image, one 8x8 output tile per wave, the scene staged as in guide_kernel.
// Taps: q = (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) with b = (1 - gx)(1 - gy), gx (1 - gy), (1 - gx) gy, gx gy.  A tap counts
// when q is in the frame -- tested before any load --, b > 0 and q holds colour.  The taps are served by L1/L2: a wave's 64 pixels read at
// most a 5 x 5 block of traced pixels.  Lanes outside the frame do nothing behind the staging barrier but wait for the count.
template <class T, int SRC>
__global__ void __launch_bounds__(64 * UPSCALE_WAVES) upscale_kernel(const RenderParams<T> p, const UpscaleParams<T> u, T* __restrict__ out, unsigned* __restrict__ covered) {
    const T* lds_geom = stage_scene<T, SRC>(p);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned* tally = reinterpret_cast<unsigned*>(smem_raw + u.tally_offset);
    const int W = p.cold.W, rows = p.cold.local_rows, F = u.F;
    const int OW = W * F, OH = rows * F;
    const int tiles_x = (OW + 7) >> 3, tiles = tiles_x * ((OH + 7) >> 3);
    const int tile = (int)blockIdx.x * UPSCALE_WAVES + (int)(threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63u);
    const int I = (tile % tiles_x) * 8 + (lane & 7), J = (tile / tiles_x) * 8 + (lane >> 3);
    bool shared_tap = false;
    if (tile < tiles && I < OW && J < OH) {                      // after the staging barrier
        const UpscalePixel<T> px = upscale_pixel<T, SRC>(p, lds_geom, I, J, F);
        const T gx = px.gx, gy = px.gy;
        const T bw[4] = {((T)1 - gx) * ((T)1 - gy), gx * ((T)1 - gy), ((T)1 - gx) * gy, gx * gy};
        T s1[3] = {0, 0, 0}, w1 = 0, sp[3] = {0, 0, 0}, wp_sum = 0;
#pragma unroll
        for (int tap = 0; tap < 4; ++tap) {
            const int qx = px.x0 + (tap & 1), qy = px.y0 + (tap >> 1);
            if (qx < 0 || qx >= W || qy < 0 || qy >= rows || !(bw[tap] > (T)0)) continue;
            const size_t q = (size_t)qy * W + qx;
            V3<T> c;
            if (!upscale_source_colour(u, q, c)) continue;
            upscale_tap(u, px, bw[tap], c, u.nd[q], u.alb[q], u.use_coverage ? u.ic + q : nullptr, s1, w1, sp, wp_sum);
        }
        shared_tap = upscale_resolve(s1, w1, sp, wp_sum, out, (size_t)J * OW + I);
    }
    upscale_count(shared_tap, (int)(threadIdx.x >> 6), lane, tally, covered);
}

}  // namespace
