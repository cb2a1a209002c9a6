// edit_influence.h -- edit influence (rtiow_set_edit_influence): how much of a pixel's incoming light a scene
// edit can have changed, as a plane lambda in [0, 1], and the fade 1 - lambda that the three motion gathers multiply the history length by.
// The sky is the only light, so the irradiance at a point changes by at most the share of its surroundings that the edited spheres occupy,
// before and after the edit: the entries of the edit list (library/edit_list.h).
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, in this order; internal linkage).
//
// Every value is defined operation by operation and evaluated in T with plain * + - / and sqrt: no RT_FMA,
// madd3 or dot3.  -ffp-contract=off keeps the plain operations unfused, so a numpy restatement gives the same bits.
#pragma once
#include "scene_motion.h"               // the motion plane {Q, carry} and the ids, written just before this kernel runs
#include "../library/edit_list.h"       // EDIT_LIST_CHUNK

namespace {

// The kernel's constants (kernarg segment: wave-uniform).  The camera's are the guide kernel's; kappa is rounded once to T on the host;
// the shard's fields turn a local row into the global row the ray was formed with.
template <class T> struct InfluenceParams {
    V3<T> O, pixel00, du, dv;
    T kappa;
    int W, local_rows, strip_rows, nranks, rank;
    int entries;
};

// An image-space pass: one lane per local pixel, 16 x 16 pixels per workgroup, no hit_world and no scene staging.  Per pixel p, from the
// first-hit guides {normal, depth}, the motion plane {Q, carry}, the id k_p and the edit list:
//   a miss (depth == 0) or carry_p == 0:   lambda_p = 0
//   otherwise   P = O + t_p D per component (the operands and order of gather_history<MOTION == false> at a hit pixel), s = 0, and
//               for every entry e in list order with owner_e != k_p:
//                   v = C_e - P, d2 = (v.x v.x + v.y v.y) + v.z v.z, q = (r_e r_e) / d2,
//                   omega = q >= 1 ? 1 : 1 - sqrt(1 - q)      (NaN compares false), s = s + omega
//               lambda_p = s > 0 ? min(1, kappa s) : 0
//   fade_p = carry_p == 0 ? 0 : 1 - lambda_p
// lambda goes to a plane of its own; fade replaces the fourth T of the motion plane's {Q, carry}, in place.  The list is wave-uniform: it is
// staged in LDS EDIT_LIST_CHUNK entries at a time and every lane reads the same address (a broadcast).  Every lane reaches both barriers of
// every chunk; a lane outside the frame, on the sky or on a changed surface only skips the arithmetic.  entries == 0 (list may be null):
// no chunk, lambda = 0 everywhere.
template <class T>
__global__ void __launch_bounds__(256) edit_influence_kernel(const InfluenceParams<T> ip, const Vec4<T>* __restrict__ cur_nd, const int32_t* __restrict__ ids,
                                                             const Vec4<T>* __restrict__ list, const int32_t* __restrict__ owner,
                                                             Vec4<T>* __restrict__ qc, T* __restrict__ lambda) {
    __shared__ Vec4<T> ent[EDIT_LIST_CHUNK];
    __shared__ int32_t own[EDIT_LIST_CHUNK];
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15u), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    const bool inside = x < ip.W && y < ip.local_rows;
    const size_t lp = inside ? (size_t)y * ip.W + x : 0;
    T depth = 0, carry = 0;
    int k = -1;
    if (inside) { depth = cur_nd[lp].w; carry = qc[lp].w; k = ids[lp]; }
    const bool lit = inside && depth != (T)0 && carry != (T)0;
    const int j = global_row(inside ? y : 0, ip.strip_rows, ip.nranks, ip.rank);
    const T fi = (T)x, fj = (T)j;
    const V3<T> D = {((ip.pixel00.x + fi * ip.du.x) + fj * ip.dv.x) - ip.O.x, ((ip.pixel00.y + fi * ip.du.y) + fj * ip.dv.y) - ip.O.y,
                     ((ip.pixel00.z + fi * ip.du.z) + fj * ip.dv.z) - ip.O.z};
    const V3<T> P = {ip.O.x + depth * D.x, ip.O.y + depth * D.y, ip.O.z + depth * D.z};
    T s = 0;
    for (int e0 = 0; e0 < ip.entries; e0 += EDIT_LIST_CHUNK) {
        const int count = ip.entries - e0 < EDIT_LIST_CHUNK ? ip.entries - e0 : EDIT_LIST_CHUNK;
        __syncthreads();                                         // the chunk before this one has been read
        if ((int)threadIdx.x < count) { ent[threadIdx.x] = list[e0 + (int)threadIdx.x]; own[threadIdx.x] = owner[e0 + (int)threadIdx.x]; }
        __syncthreads();
        if (lit)
            for (int e = 0; e < count; ++e) {
                if (own[e] == k) continue;                       // a pixel's own sphere: its history is the motion plane's business
                const Vec4<T> c = ent[e];
                const T vx = c.x - P.x, vy = c.y - P.y, vz = c.z - P.z;
                const T d2 = (vx * vx + vy * vy) + vz * vz;
                const T q = (c.w * c.w) / d2;
                const T omega = q >= (T)1 ? (T)1 : (T)1 - Real<T>::sqrt((T)1 - q);
                s = s + omega;
            }
    }
    if (!inside) return;
    T lam = 0;
    if (s > (T)0) { const T ks = ip.kappa * s; lam = ks < (T)1 ? ks : (T)1; }
    lambda[lp] = lam;
    reinterpret_cast<T*>(qc)[4 * lp + 3] = carry == (T)0 ? (T)0 : (T)1 - lam;
}

}  // namespace
