// upscale_wide.h -- wide-support guided upscaling (rtiow_upscale_wide): rtiow_upscale's preview with sixteen taps under the cubic B-spline
// where that call has four under the bilinear hat.  Every output pixel traces the same primary ray of its own and gathers the 4 x 4 traced
// pixels around it, each weighed by the B-spline, by how well its first-hit guides match what the output pixel's ray hit, and
// (use_coverage) by the share of it that is the surface the output pixel sees.
// Part of the gfx950 translation units rtiow_upscale_wide.hip and, over the device grid, rtiow_large_upscale.hip: the only ones that
// instantiate the kernel (internal linkage).
//
// Every value is defined operation by operation and evaluated in T with plain * + - / and sqrt, as in
// upscale.h: no RT_FMA, madd3 or dot3 for a stored value.  -ffp-contract=off keeps the plain operations unfused, so a numpy restatement
// gives the same bits.
#pragma once
#include "upscale.h"            // UpscaleParams, the shared statements of pixel, colour, tap, resolve and count, and the headers they need

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

static_assert(UPSCALE_WIDE_BLOCK * UPSCALE_WIDE_BLOCK == 64 * UPSCALE_WAVES, "one lane per output pixel of the block");

// ---- One lane per output pixel (I, J) of the F W x F rows image, one workgroup of 256 per 16 x 16 output block, its waves' 8 x 8 tiles
// arranged 2 x 2.  The pixel is upscale_pixel's, the tap upscale_tap's, the result and the count upscale_resolve's and upscale_count's
// (upscale.h).  Taps: the 16 traced pixels q = (x0 - 1 + u, y0 - 1 + v), v outer, u inner, with b = cy[v] cx[u], c[] the cubic B-spline of
// g (h = 1 - g): c0 = ((h h) h) / 6, c1 = (((3 g - 6) g) g + 4) / 6, c2 = (((3 h - 6) h) h + 4) / 6, c3 = ((g g) g) / 6.  A tap counts when
// q is in the frame, b > 0 and q holds colour.
// The block's taps land on a footprint of side x side traced pixels, side = ceil(16 / F) + 4 <= 12, from (i0 - 2, j0 - 2) with i0, j0 the
// traced pixel of the block's first output pixel.  Lane t < side^2 stages footprint pixel t once -- the guides, the decoded colour (the same
// operations on the same inputs as a load per tap: the same bits), whether it counts at all (inside the frame -- tested before any load
// -- and holding colour: the albedo's fourth word is 1, else 0) and, with the share, the layers -- before the scene's staging barrier,
// which then serves both; the 16 taps of a lane are 16-byte LDS reads.  4096 tap reads of a block land on at most 144 pixels.  Lanes
// outside the output skip the taps and reach every barrier.
template <class T, int SRC>
__global__ void __launch_bounds__(64 * UPSCALE_WAVES) upscale_wide_kernel(const RenderParams<T> p, const UpscaleParams<T> u, const int stage_offset, T* __restrict__ out,
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
                if (upscale_source_colour(u, q, c)) {
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
    // stage_scene's own barrier otherwise (uniform: a kernel argument); stage_device_grid, which stages both grids in device memory, always ends in one
    if (!(SRC == RTIOW_SCENE_LDS || SRC == RTIOW_SCENE_DEVICE_GRID || SRC == RTIOW_SCENE_VOLUME_GRID || p.shade_in_lds)) __syncthreads();
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int I = I0 + (wave & 1) * 8 + (lane & 7), J = J0 + (wave >> 1) * 8 + (lane >> 3);
    bool shared_tap = false;
    if (I < OW && J < OH) {
        const UpscalePixel<T> px = upscale_pixel<T, SRC>(p, lds_geom, I, J, F);
        const T gx = px.gx, gy = px.gy, hx = (T)1 - gx, hy = (T)1 - gy;
        const T cx[4] = {((hx * hx) * hx) / (T)6, ((((T)3 * gx - (T)6) * gx) * gx + (T)4) / (T)6, ((((T)3 * hx - (T)6) * hx) * hx + (T)4) / (T)6,
                         ((gx * gx) * gx) / (T)6};
        const T cy[4] = {((hy * hy) * hy) / (T)6, ((((T)3 * gy - (T)6) * gy) * gy + (T)4) / (T)6, ((((T)3 * hy - (T)6) * hy) * hy + (T)4) / (T)6,
                         ((gy * gy) * gy) / (T)6};
        const int first = (px.y0 - 1 - fy0) * side + (px.x0 - 1 - fx0);   // the lane's first tap in the footprint: both terms are >= 0
        T s1[3] = {0, 0, 0}, w1 = 0, sp[3] = {0, 0, 0}, wp_sum = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
#pragma unroll
            for (int uu = 0; uu < 4; ++uu) {
                const int at = first + v * side + uu;
                const Vec4<T> aq = s_ah[at];
                const T bw = cy[v] * cx[uu];
                if (!(aq.w > (T)0) || !(bw > (T)0)) continue;
                const Vec4<T> nq = s_nd[at], c = s_c[at];            // read here, ahead of the tap's division, not where upscale_tap first uses them
                upscale_tap(u, px, bw, c, nq, aq, s_ic + at, s1, w1, sp, wp_sum);
            }
        }
        shared_tap = upscale_resolve(s1, w1, sp, wp_sum, out, (size_t)J * OW + I);
    }
    upscale_count(shared_tap, wave, lane, tally, covered);
}

}  // namespace
