// scene_motion.h -- scene edits that keep the history (rtiow_edit_scene): the motion plane, which tells every pixel of the current frame
// which point of the scene the base was committed under its first hit came from, and the three history kernels that gather through it.
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, in this order; internal linkage).
//
// Every value is defined operation by operation and evaluated in T with plain * + - /: no RT_FMA, madd3 or
// dot3 for a stored value.  -ffp-contract=off keeps the plain operations unfused, so a numpy restatement gives the same bits.
#pragma once
#include "history_clip.h"       // CLIP_TILE_SIDE, and through history.h: Vec4, HistoryParams, gather_history, blend_history
#include "history_budget.h"     // history_length_kernel, whose shell motion_length_kernel restates

namespace {

// Flags of a kept sphere k against the snapshot the commit took (compared on the host, bit for bit): MOVED: any of the 4 T of
// {C_k, r_k} differs; CHANGED: the material record (type, the 4 T of albedo_fuzz, refraction_index) differs.
constexpr int MOTION_MOVED = 1, MOTION_CHANGED = 2;

// ---- The motion plane: one lane per local pixel, one 8x8 tile per wave, the scene staged as in guide_kernel, whose ray this is:
// O = centre, D = ((pixel00 + i du) + j dv) - O, (t, k) = hit_world(O, D) -- the (t, k) behind the guides' depth.  Per pixel
// qc = {Q.xyz, (T)carry} and ids = k:
//   a miss              k = -1, Q = 0, carry = 1 (the sky is matched by the base's depth 0, as ever)
//   hit, CHANGED        Q = 0, carry = 0: a surface that changed colour or kind carries nothing
//   hit, not MOVED      Q = O + t D per component: the expression gather_history forms from the guides' depth, with the same operands
//   hit, MOVED          P = O + t D, o = (P - C_k) * ((T)1 / r_k) per component (the guides' outward, 1 / r_k from the shade table),
//                       Q = C'_k + r'_k o per component: the point of the sphere's old surface this one came from, under translation
//                       and scaling about the centre.  {C'_k, r'_k} = snap[k].
// snap and flags are indexed by k, the numbering of the kept spheres, and read with ordinary vector loads.
template <class T, int SRC>
__global__ void __launch_bounds__(256) surface_motion_kernel(const RenderParams<T> p, const Vec4<T>* __restrict__ snap, const int32_t* __restrict__ flags,
                                                             Vec4<T>* __restrict__ qc, int32_t* __restrict__ ids) {
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
    hit_world<T, SRC>(p, lds_geom, O, D, dot3(D, D), t, k);      // dot3: the |D|^2 every caller of hit_world passes (not part of a stored value)
    const size_t lp = (size_t)jl * W + i;
    Vec4<T> out = {(T)0, (T)0, (T)0, (T)1};
    if (k >= 0) {
        const int f = flags[k];
        const V3<T> P = {O.x + t * D.x, O.y + t * D.y, O.z + t * D.z};
        if (f & MOTION_CHANGED) out.w = (T)0;
        else if (!(f & MOTION_MOVED)) { out.x = P.x; out.y = P.y; out.z = P.z; }
        else {
            const T* rec = p.screen.shade_tbl + 12 * (size_t)k;   // {cx,cy,cz,1/r | ...}
            const T inv_r = rec[3];
            const V3<T> o = {(P.x - rec[0]) * inv_r, (P.y - rec[1]) * inv_r, (P.z - rec[2]) * inv_r};
            const Vec4<T> s = snap[k];
            out.x = s.x + s.w * o.x; out.y = s.y + s.w * o.y; out.z = s.z + s.w * o.z;
        }
    }
    qc[lp] = out;
    ids[lp] = k;
}

// ---- The history kernels through the motion plane: history_reproject_kernel, history_length_kernel and history_clip_kernel with the
// plane as one more operand and gather_history's MOTION == true in place of its MOTION == false, launched in their place while motion is in
// effect.  The arithmetic -- the gather, the blend, the linear colour -- is stated once, in history.h and denoise.h, for both families.
// The shells around it (pixel of a lane, window, clamp, counters) are restated here, line for line: routing the existing kernels through a
// shared body template, by value or by reference, changed their scalar loads and schedules (the kernel's constants pass through one more
// copy), and their code objects are to stay what they were.  tests/test_scene_motion.py holds each pair to each other bit for bit with an
// edit that changes nothing.
template <class T>
__global__ void __launch_bounds__(256) motion_reproject_kernel(FrameShape fr, const HistoryParams<T> hp, const unsigned char* __restrict__ mid,
                                                               const int32_t* __restrict__ counts, int n_uniform, const Vec4<T>* __restrict__ cur_nd,
                                                               const Vec4<T>* __restrict__ base_hm, const Vec4<T>* __restrict__ base_nd,
                                                               const Vec4<T>* __restrict__ motion, Vec4<T>* __restrict__ out_cm, T* __restrict__ out_rgb,
                                                               unsigned* __restrict__ reprojected) {
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15u), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    const bool inside = x < fr.W && y < fr.local_rows;
    bool carried = false;
    if (inside) {
        const size_t lp = (size_t)y * fr.W + x;
        const V3<T> c = linear_colour<T>(mid, counts, n_uniform, lp);
        const int n = counts ? counts[lp] : n_uniform;
        const Gathered<T> h = gather_history<T, true, true>(fr, hp, x, y, lp, cur_nd, base_hm, base_nd, motion);
        carried = h.m > (T)0;
        blend_history<T>(h, c, n, lp, out_cm, out_rgb);
    }
    const unsigned long long votes = __ballot(carried);
    if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(reprojected, (unsigned)__popcll(votes));
}

template <class T>
__global__ void __launch_bounds__(256) motion_length_kernel(FrameShape fr, const HistoryParams<T> hp, const Vec4<T>* __restrict__ cur_nd,
                                                            const T* __restrict__ base_hm, const Vec4<T>* __restrict__ base_nd,
                                                            const Vec4<T>* __restrict__ motion, T* __restrict__ out_m, unsigned* __restrict__ reprojected) {
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15u), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    const bool inside = x < fr.W && y < fr.local_rows;
    bool carried = false;
    if (inside) {
        const size_t lp = (size_t)y * fr.W + x;
        const T m = gather_history<T, false, true>(fr, hp, x, y, lp, cur_nd, reinterpret_cast<const Vec4<T>*>(base_hm), base_nd, motion).m;
        carried = m > (T)0;
        out_m[lp] = m;
    }
    const unsigned long long votes = __ballot(carried);
    if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(reprojected, (unsigned)__popcll(votes));
}

template <class T>
__global__ void __launch_bounds__(256) motion_clip_kernel(FrameShape fr, const HistoryParams<T> hp, int r, T gamma, const unsigned char* __restrict__ mid,
                                                          const int32_t* __restrict__ counts, int n_uniform, const Vec4<T>* __restrict__ cur_nd,
                                                          const Vec4<T>* __restrict__ base_hm, const Vec4<T>* __restrict__ base_nd,
                                                          const Vec4<T>* __restrict__ motion, Vec4<T>* __restrict__ out_cm, T* __restrict__ out_rgb,
                                                          unsigned* __restrict__ ctr) {
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
        Gathered<T> h = gather_history<T, true, true>(fr, hp, x, y, lp, cur_nd, base_hm, base_nd, motion);   // section 19: through the plane
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
