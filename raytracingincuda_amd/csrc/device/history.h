// history.h -- temporal history for progressive previews (rtiow_history_update): every pixel of the current camera is reprojected into
// the frame of an earlier camera (the base), gathers that frame's history colour bilinearly from the taps whose surface matches, and
// blends it with the current accumulation by sample count.
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, in this order; internal linkage).
//
// Every value is defined operation by operation and evaluated in T with plain * + - /, floor and fabs:
// no RT_FMA, madd3 or dot3.  -ffp-contract=off keeps the plain operations unfused, so a numpy restatement gives the same bits.
#pragma once
#include "denoise.h"            // linear_colour, FrameShape

namespace {

// The kernel's constants (kernarg segment: wave-uniform, read into SGPRs).  The current camera's are the guide kernel's; the base
// camera's (primed in section 11) are derived on the host in double and rounded once to T (history_constants, library/launch.h):
// a = pixel00' - O', w = du' x dv' turned so that f = a.w > 0, iu = 1 / |du'|^2, iv = 1 / |dv'|^2.  have_base == 0 (no base, a base
// of another frame size, a degenerate base camera): every pixel has m = 0.
template <class T> struct HistoryParams {
    V3<T> O, pixel00, du, dv;
    V3<T> Ob, a, w, dub, dvb;
    T f, iu, iv;
    T depth_tol, normal_cos, max_history;
    int have_base;
};

template <class T> using Vec4 = T __attribute__((ext_vector_type(4)));

// The gather of section 11, stated once for the three kernels that need it: the pixel (x, y) of the current camera (lp its index) is
// reprojected into the base's frame, the four bilinear taps whose surface matches are summed by weight, and the length is capped at
// max_history.  cur_nd: the current guides {normal, depth}; base_hm / base_nd: the base's {H.rgb, M} and {normal', depth'}, one 4-T
// vector per pixel each, so a tap is two vector loads (neighbouring pixels gather neighbouring taps: L2 serves them).  COLOUR == false
// gathers the length alone: a tap then loads M, the last of the four T of {H.rgb, M}, and the colour sums and quotients are not formed;
// what is left is operation for operation the `m` of COLOUR == true.  fr and hp by value: they stay the kernel's wave-uniform constants.
// MOTION == true (device/scene_motion.h) is the gather through an edited scene, with exactly two changes at a
// hit pixel: d = Q_p - O' with {Q_p, carry_p} = motion[lp], the motion plane's point of the old surface, instead of (O + t_p D) - O'; and
// carry_p == 0 (a surface that changed colour or kind) takes no taps, m = 0.  Everything after d is shared.  Where the first hit is the
// sky or a sphere that neither moved nor changed, Q_p has the bits of O + t_p D and carry_p is 1: the bits of MOTION == false.  A pixel
// that now sees what a moved sphere used to hide fails the depth test against the base as any disocclusion does.  The normal test needs no
// change: translation and scaling about the centre keep the normal of corresponding points.  After the cap, m = m * w with w the plane's
// fourth T: carry_p, or with edit influence on (section 20, device/edit_influence.h) fade_p = 1 - lambda_p in [0, 1], which shortens the
// history where the edit can have changed the pixel's light; w = 1 leaves the bits of m.  MOTION == false never reads `motion`, and
// its instantiations compile to the code they had before the parameter existed.
template <class T> struct Gathered { T hx = 0, hy = 0, hz = 0, m = 0; };

template <class T, bool COLOUR, bool MOTION = false>
__device__ __forceinline__ Gathered<T> gather_history(FrameShape fr, HistoryParams<T> hp, int x, int y, size_t lp, const Vec4<T>* cur_nd,
                                                      const Vec4<T>* base_hm, const Vec4<T>* base_nd, const Vec4<T>* motion = nullptr) {
    Gathered<T> h;
    if (!hp.have_base) return h;
    const Vec4<T> g = cur_nd[lp];
    Vec4<T> mq = {(T)0, (T)0, (T)0, (T)1};
    if constexpr (MOTION) mq = motion[lp];
    const T fi = (T)x, fj = (T)y;
    const V3<T> D = {((hp.pixel00.x + fi * hp.du.x) + fj * hp.dv.x) - hp.O.x, ((hp.pixel00.y + fi * hp.du.y) + fj * hp.dv.y) - hp.O.y,
                     ((hp.pixel00.z + fi * hp.du.z) + fj * hp.dv.z) - hp.O.z};
    const bool hit = g.w > (T)0;
    V3<T> d = D;
    if (hit) {
        if constexpr (MOTION) d = {mq.x - hp.Ob.x, mq.y - hp.Ob.y, mq.z - hp.Ob.z};
        else d = {(hp.O.x + g.w * D.x) - hp.Ob.x, (hp.O.y + g.w * D.y) - hp.Ob.y, (hp.O.z + g.w * D.z) - hp.Ob.z};
    }
    const T den = (d.x * hp.w.x + d.y * hp.w.y) + d.z * hp.w.z;
    bool taps = den > (T)0;
    if constexpr (MOTION) taps = taps && !(hit && mq.w == (T)0);
    if (taps) {
        const T s = hp.f / den;
        const T ex = s * d.x - hp.a.x, ey = s * d.y - hp.a.y, ez = s * d.z - hp.a.z;
        const T u = ((ex * hp.dub.x + ey * hp.dub.y) + ez * hp.dub.z) * hp.iu;
        const T v = ((ex * hp.dvb.x + ey * hp.dvb.y) + ez * hp.dvb.z) * hp.iv;
        const T te = den / hp.f;
        if (u > (T)-1 && u < (T)fr.W && v > (T)-1 && v < (T)fr.local_rows) {      // false for NaN
            const T xf = __builtin_elementwise_floor(u), yf = __builtin_elementwise_floor(v);
            const int x0 = (int)xf, y0 = (int)yf;
            const T fx = u - xf, fy = v - yf;
            const T gx = (T)1 - fx, gy = (T)1 - fy;
            const T b[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
            const T tol = hp.depth_tol * te;
            T sx = 0, sy = 0, sz = 0, sl = 0, sb = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                if (qx < 0 || qx >= fr.W || qy < 0 || qy >= fr.local_rows) continue;
                const size_t q = (size_t)qy * fr.W + qx;
                Vec4<T> hq = {(T)0, (T)0, (T)0, (T)0};
                if constexpr (COLOUR) hq = base_hm[q];
                else hq.w = reinterpret_cast<const T*>(base_hm)[4 * q + 3];
                const Vec4<T> gq = base_nd[q];
                bool ok = hq.w > (T)0;
                if (hit) {
                    const T dd = gq.w - te;
                    const T nn = (g.x * gq.x + g.y * gq.y) + g.z * gq.z;
                    ok = ok && gq.w > (T)0 && __builtin_elementwise_abs(dd) <= tol && nn >= hp.normal_cos;
                } else ok = ok && gq.w == (T)0;
                if (!ok) continue;
                if constexpr (COLOUR) { sx = sx + b[k] * hq.x; sy = sy + b[k] * hq.y; sz = sz + b[k] * hq.z; }
                sl = sl + b[k] * hq.w;
                sb = sb + b[k];
            }
            if (sb > (T)0) {
                if constexpr (COLOUR) { h.hx = sx / sb; h.hy = sy / sb; h.hz = sz / sb; }
                h.m = sl / sb;
            }
        }
    }
    h.m = h.m < hp.max_history ? h.m : hp.max_history;
    if constexpr (MOTION) h.m = h.m * mq.w;                      // section 20: the fade; with w = 1 the product has the bits of m
    return h;
}

// The blend by sample count: Mout = m + n, alpha = n / Mout, o = h + alpha (c - h); nobody sampled and nothing carried gives 0.  out_cm
// receives {C.rgb, Mout}, out_rgb the colour alone as the 3-T plane the a-trous filter reads (denoise_level_kernel's cin).
template <class T>
__device__ __forceinline__ void blend_history(Gathered<T> h, V3<T> c, int n, size_t lp, Vec4<T>* out_cm, T* out_rgb) {
    const T nT = (T)n, mout = h.m + nT;
    Vec4<T> o = {(T)0, (T)0, (T)0, mout};
    if (mout > (T)0) {
        const T alpha = nT / mout;
        o.x = h.hx + alpha * (c.x - h.hx); o.y = h.hy + alpha * (c.y - h.hy); o.z = h.hz + alpha * (c.z - h.hz);
    }
    out_cm[lp] = o;
    out_rgb[3 * lp] = o.x; out_rgb[3 * lp + 1] = o.y; out_rgb[3 * lp + 2] = o.z;
}

// One lane per pixel, 16 x 16 pixels per workgroup: gather, blend.  *reprojected counts the pixels with m > 0: one atomic per wave.
template <class T>
__global__ void __launch_bounds__(256) history_reproject_kernel(FrameShape fr, const HistoryParams<T> hp, const unsigned char* __restrict__ mid,
                                                                const int32_t* __restrict__ counts, int n_uniform, const Vec4<T>* __restrict__ cur_nd,
                                                                const Vec4<T>* __restrict__ base_hm, const Vec4<T>* __restrict__ base_nd,
                                                                Vec4<T>* __restrict__ out_cm, T* __restrict__ out_rgb, unsigned* __restrict__ reprojected) {
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15u), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    const bool inside = x < fr.W && y < fr.local_rows;
    bool carried = false;
    if (inside) {
        const size_t lp = (size_t)y * fr.W + x;
        const V3<T> c = linear_colour<T>(mid, counts, n_uniform, lp);
        const int n = counts ? counts[lp] : n_uniform;
        const Gathered<T> h = gather_history<T, true>(fr, hp, x, y, lp, cur_nd, base_hm, base_nd);
        carried = h.m > (T)0;
        blend_history<T>(h, c, n, lp, out_cm, out_rgb);
    }
    const unsigned long long votes = __ballot(carried);
    if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(reprojected, (unsigned)__popcll(votes));
}

}  // namespace
