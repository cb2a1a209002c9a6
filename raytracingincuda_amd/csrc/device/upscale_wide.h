// upscale_wide.h -- wide-support guided upscaling (rtiow_upscale_wide): rtiow_upscale's preview with sixteen taps under the cubic B-spline
// where that call has four under the bilinear hat.  Every output pixel traces the same primary ray of its own and gathers the 4 x 4 traced
// pixels around it, each weighed by the B-spline, by how well its first-hit guides match what the output pixel's ray hit, and
// (use_coverage) by the share of it that is the surface the output pixel sees.
// Part of the gfx950 translation unit rtiow_upscale_wide.hip, the only one that instantiates the kernel (internal linkage).
//
// Every value is defined operation by operation and evaluated in T with plain * + - / and sqrt, as in
// upscale.h: no RT_FMA, madd3 or dot3 for a stored value.  -ffp-contract=off keeps the plain operations unfused, so a numpy restatement
// gives the same bits.
#pragma once
#include "upscale.h"            // UpscaleParams, UPSCALE_COUNTERS, UPSCALE_TALLY_BYTES and the headers that kernel needs

namespace {

constexpr int UPSCALE_WIDE_BLOCK = 16;                          // a workgroup's output block is 16 x 16: four 8 x 8 wave tiles, 2 x 2
// The traced pixels a block's taps land on: ceil(16 / F) pixels hold its output pixels, and a pixel's taps reach two further to each side.
__host__ __device__ constexpr int upscale_wide_side(int F) { return (UPSCALE_WIDE_BLOCK + F - 1) / F + 4; }
constexpr int UPSCALE_WIDE_MAX_SIDE = upscale_wide_side(UPSCALE_MIN_FACTOR);        // 12: at most 144 staged pixels, one per lane
static_assert(UPSCALE_WIDE_MAX_SIDE * UPSCALE_WIDE_MAX_SIDE <= 256, "one staged pixel per lane of the workgroup");
// The footprint in LDS, behind the staged scene: four arrays of UPSCALE_WIDE_MAX_SIDE^2 entries -- {N, Z}, {A, counts}, {c, 0} as Vec4<T>
// and the layers as int4 --, 64 B (fp32) or 112 B (fp64) a staged pixel.
template <class T>
constexpr size_t upscale_wide_stage_bytes() { return (size_t)UPSCALE_WIDE_MAX_SIDE * UPSCALE_WIDE_MAX_SIDE * (3 * sizeof(Vec4<T>) + sizeof(int4)); }

// ---- One lane per output pixel (I, J) of the F W x F rows image, one workgroup of 256 per 16 x 16 output block, its waves' 8 x 8 tiles
// arranged 2 x 2.  The ray, N, A, Z and k of the output pixel, x0, gx, y0, gy: upscale_kernel's, to the letter.  Taps: the 16 traced pixels
// q = (x0 - 1 + u, y0 - 1 + v), v outer, u inner, with b = cy[v] cx[u], c[] the cubic B-spline of g (h = 1 - g): c0 = ((h h) h) / 6,
// c1 = (((3 g - 6) g) g + 4) / 6, c2 = (((3 h - 6) h) h + 4) / 6, c3 = ((g g) g) / 6.  A tap counts when q is in the frame, b > 0 and q
// holds colour; e, w, S1, W1, the share, the result and the count are upscale_kernel's.
// The block's taps land on a footprint of side x side traced pixels, side = ceil(16 / F) + 4 <= 12, from (i0 - 2, j0 - 2) with i0, j0 the
// traced pixel of the block's first output pixel.  Lane t < side^2 stages footprint pixel t once -- the guides, the decoded colour (the same
// operations on the same inputs as a load per tap: the same bits), whether it counts at all (inside the frame -- tested before any load
// -- and holding colour) and, with the share, the layers -- before the scene's staging barrier, which then serves both; the 16 taps of
// a lane are 16-byte LDS reads.  4096 tap reads of a block land on at most 144 pixels.  Lanes outside the output skip the taps and reach
// every barrier.
template <class T, int SRC>
__global__ void __launch_bounds__(256) upscale_wide_kernel(const RenderParams<T> p, const UpscaleParams<T> u, const int stage_offset, T* __restrict__ out,
                                                           unsigned* __restrict__ covered) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int CAP = UPSCALE_WIDE_MAX_SIDE * UPSCALE_WIDE_MAX_SIDE;
    Vec4<T>* s_nd = reinterpret_cast<Vec4<T>*>(smem_raw + stage_offset);
    Vec4<T>* s_ah = s_nd + CAP;
    Vec4<T>* s_c = s_ah + CAP;
    int4* s_ic = reinterpret_cast<int4*>(s_c + CAP);
    unsigned* tally = reinterpret_cast<unsigned*>(smem_raw + u.tally_offset);
    const int W = p.cold.W, rows = p.cold.local_rows, F = u.F;
    const int OW = W * F, OH = rows * F;
    const int blocks_x = (OW + UPSCALE_WIDE_BLOCK - 1) / UPSCALE_WIDE_BLOCK;
    const int I0 = ((int)blockIdx.x % blocks_x) * UPSCALE_WIDE_BLOCK, J0 = ((int)blockIdx.x / blocks_x) * UPSCALE_WIDE_BLOCK;
    const int side = upscale_wide_side(F);
    const int fx0 = I0 / F - 2, fy0 = J0 / F - 2;                // the footprint's first traced pixel (may lie outside the frame)
    {
        const int t = (int)threadIdx.x;
        if (t < side * side) {
            const int qx = fx0 + t % side, qy = fy0 + t / side;
            Vec4<T> nd = {(T)0, (T)0, (T)0, (T)0}, ah = nd, c = nd;
            int4 ic = {COVERAGE_NO_LAYER, COVERAGE_NO_LAYER, 0, 0};
            if (qx >= 0 && qx < W && qy >= 0 && qy < rows) {
                const size_t q = (size_t)qy * W + qx;
                bool has = true;
                if (u.source == RTIOW_UPSCALE_DENOISED) {
                    const T g0 = u.g[3 * q], g1 = u.g[3 * q + 1], g2 = u.g[3 * q + 2];
                    c = {g0 * g0, g1 * g1, g2 * g2, (T)0};
                } else if (u.source == RTIOW_UPSCALE_LINEAR) {
                    has = (u.counts ? u.counts[q] : u.n_uniform) > 0;
                    if (has) { const V3<T> l = linear_colour<T>(u.mid, u.counts, u.n_uniform, q); c = {l.x, l.y, l.z, (T)0}; }
                } else {
                    const Vec4<T> cm = u.cm[q];
                    has = cm.w > (T)0;
                    c = {cm.x, cm.y, cm.z, (T)0};
                }
                if (has) {
                    nd = u.nd[q];
                    ah = u.alb[q];
                    ah.w = (T)1;
                    if (u.use_coverage) ic = u.ic[q];
                }
            }
            s_nd[t] = nd; s_ah[t] = ah; s_c[t] = c;
            if (u.use_coverage) s_ic[t] = ic;
        }
    }
    const T* lds_geom = stage_scene<T, SRC>(p);
    if (!(SRC == RTIOW_SCENE_LDS || p.shade_in_lds)) __syncthreads();     // stage_scene's own barrier otherwise (uniform: a kernel argument)
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int I = I0 + (wave & 1) * 8 + (lane & 7), J = J0 + (wave >> 1) * 8 + (lane >> 3);
    bool shared_tap = false;
    if (I < OW && J < OH) {
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
        hit_world<T, SRC>(p, lds_geom, O, D, dot3(D, D), t, k);  // dot3: the |D|^2 every caller of hit_world passes (not part of a stored value)
        V3<T> N = {(T)0, (T)0, (T)0}, A = {(T)0, (T)0, (T)0};
        T Z = (T)0;
        if (k >= 0) {
            const T* rec = p.screen.shade_tbl + 12 * (size_t)k;   // {cx,cy,cz,1/r | albedo r,g,b,fuzz | eta,1/eta,type,0}
            const V3<T> P = {O.x + t * D.x, O.y + t * D.y, O.z + t * D.z};
            const T inv_r = rec[3];
            N = {(P.x - rec[0]) * inv_r, (P.y - rec[1]) * inv_r, (P.z - rec[2]) * inv_r};
            const T dn = (D.x * N.x + D.y * N.y) + D.z * N.z;
            if (!(dn < (T)0)) N = {-N.x, -N.y, -N.z};
            const bool glass = (int)rec[10] == RTIOW_DIELECTRIC;
            A = {glass ? (T)1 : rec[4], glass ? (T)1 : rec[5], glass ? (T)1 : rec[6]};
            Z = t;
        }
        const int x0 = oa < (T)0 ? i - 1 : i, y0 = ob < (T)0 ? j - 1 : j;
        const T gx = oa < (T)0 ? (T)1 + oa : oa, gy = ob < (T)0 ? (T)1 + ob : ob;
        const T hx = (T)1 - gx, hy = (T)1 - gy;
        const T cx[4] = {((hx * hx) * hx) / (T)6, ((((T)3 * gx - (T)6) * gx) * gx + (T)4) / (T)6, ((((T)3 * hx - (T)6) * hx) * hx + (T)4) / (T)6,
                         ((gx * gx) * gx) / (T)6};
        const T cy[4] = {((hy * hy) * hy) / (T)6, ((((T)3 * gy - (T)6) * gy) * gy + (T)4) / (T)6, ((((T)3 * hy - (T)6) * hy) * hy + (T)4) / (T)6,
                         ((gy * gy) * gy) / (T)6};
        const int first = (y0 - 1 - fy0) * side + (x0 - 1 - fx0);   // the lane's first tap in the footprint: both terms are >= 0
        T s1[3] = {0, 0, 0}, w1 = 0, sp[3] = {0, 0, 0}, wp_sum = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
#pragma unroll
            for (int uu = 0; uu < 4; ++uu) {
                const int s = first + v * side + uu;
                const Vec4<T> aq = s_ah[s];
                const T bw = cy[v] * cx[uu];
                if (!(aq.w > (T)0) || !(bw > (T)0)) continue;
                const Vec4<T> nq = s_nd[s], c = s_c[s];
                const T dnx = nq.x - N.x, dny = nq.y - N.y, dnz = nq.z - N.z, dz = nq.w - Z;
                const T dax = aq.x - A.x, day = aq.y - A.y, daz = aq.z - A.z;
                const T en = (dnx * dnx + dny * dny) + dnz * dnz;
                const T ea = (dax * dax + day * day) + daz * daz;
                const T ez = dz * dz;
                const T e = (en * u.i_n + ea * u.i_a) + ez * u.i_z;
                const T w = bw / ((T)1 + e);
                s1[0] = s1[0] + w * c.x; s1[1] = s1[1] + w * c.y; s1[2] = s1[2] + w * c.z;
                w1 = w1 + w;
                if (u.use_coverage) {
                    const int4 l = s_ic[s];
                    const int m = l.x == k ? l.z : (l.y == k ? l.w : 0);
                    if (m > 0) {
                        const T wp = w * ((T)m / (T)u.S);
                        sp[0] = sp[0] + wp * c.x; sp[1] = sp[1] + wp * c.y; sp[2] = sp[2] + wp * c.z;
                        wp_sum = wp_sum + wp;
                    }
                }
            }
        }
        shared_tap = wp_sum > (T)0;
        const size_t op = (size_t)J * OW + I;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const T v = shared_tap ? sp[ch] / wp_sum : (w1 > (T)0 ? s1[ch] / w1 : (T)0);
            out[3 * op + ch] = v > (T)0 ? Real<T>::sqrt(v) : (T)0;
        }
    }
    const unsigned long long votes = __ballot(shared_tap);
    if (lane == 0) tally[wave] = (unsigned)__popcll(votes);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned sum = (tally[0] + tally[1]) + (tally[2] + tally[3]);
        if (sum) atomicAdd(covered + (size_t)(blockIdx.x % (unsigned)UPSCALE_COUNTERS) * UPSCALE_COUNTER_STRIDE, sum);
    }
}

}  // namespace
