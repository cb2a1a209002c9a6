// guide_chain.h -- filter guides that follow mirrors and glass to the first diffuse surface (rtiow_set_guide_mode, RTIOW_GUIDES_SPECULAR):
// the deterministic specular chain of each pixel's centre ray, for the a-trous filters to steer by what is SEEN in a specular sphere
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, in this order; internal linkage).
//
// Every value here is defined operation by operation and evaluated in T with plain * + - / and sqrt, as in
// denoise.h: no RT_FMA, madd3, dot3, unit3 or reflect3 for a guide value.
#pragma once
#include "denoise.h"

namespace {

// ---- The chain of local pixel (i, jl): the ray of guide_kernel, then (t, k) = hit_world(O, D) once per bounce level b = 0, 1, ... with
// A = {1,1,1} (the product of the albedos passed), Z = 0 (the sum of the hit distances passed).  A miss ends the chain: everything 0 at
// b = 0, else normal 0, albedo A, depth Z.  A hit has P, outward, front and N as in guide_kernel and the albedo a_k = {r,g,b} ({1,1,1}
// for a dielectric); it is SPECULAR when it is a dielectric, or a metal with (double)fuzz <= max_fuzz.  A hit that is not specular, or
// b == max_bounces, ends the chain: normal N, albedo A a_k, depth Z + t.  Otherwise A = A a_k (not multiplied for a dielectric), Z = Z + t,
// O = P, b = b + 1 and D follows the material: the mirror direction for a metal; for a dielectric the refracted direction where there is
// one (Schlick's reflectance is not consulted), else the total internal reflection, both of the unit direction and scaled back by |D|, so
// that every t of the chain is in the units of the primary ray.  Two 4-T vectors per pixel: nd = {normal', depth'}, alb = {albedo', (T)b}.
// One lane per local pixel, one 8x8 tile per wave, the scene staged as in guide_kernel; the bounce loop runs while any lane of the wave
// still has a chain (ballot), a finished lane sits out.  At most max_bounces + 1 trips: every trip ends the lane's chain or raises its b.
template <class T, int SRC>
__global__ void __launch_bounds__(256) guide_chain_kernel(const RenderParams<T> p, int max_bounces, double max_fuzz, T* __restrict__ nd, T* __restrict__ alb) {
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
    V3<T> O = cam.center;
    const V3<T> ps = {(cam.pixel00.x + fi * cam.du.x) + fj * cam.dv.x, (cam.pixel00.y + fi * cam.du.y) + fj * cam.dv.y,
                      (cam.pixel00.z + fi * cam.du.z) + fj * cam.dv.z};
    V3<T> D = {ps.x - O.x, ps.y - O.y, ps.z - O.z};
    V3<T> A = {(T)1, (T)1, (T)1};
    T Z = 0;
    int b = 0;
    T gnx = 0, gny = 0, gnz = 0, gz = 0, gax = 0, gay = 0, gaz = 0;
    bool alive = true;
    while (__builtin_amdgcn_ballot_w64(alive) != 0) {
        if (alive) {
            T t = __builtin_huge_val();
            int k = -1;
            hit_world<T, SRC>(p, lds_geom, O, D, dot3(D, D), t, k);   // dot3: the |D|^2 every caller of hit_world passes (not part of a guide value)
            if (k < 0) {
                if (b > 0) { gax = A.x; gay = A.y; gaz = A.z; gz = Z; }
                alive = false;
            } else {
                const T* rec = p.screen.shade_tbl + 12 * (size_t)k;   // {cx,cy,cz,1/r | albedo r,g,b,fuzz | eta,1/eta,type,0}
                const V3<T> P = {O.x + t * D.x, O.y + t * D.y, O.z + t * D.z};
                const T inv_r = rec[3];
                const V3<T> out = {(P.x - rec[0]) * inv_r, (P.y - rec[1]) * inv_r, (P.z - rec[2]) * inv_r};
                const T dn = (D.x * out.x + D.y * out.y) + D.z * out.z;
                const bool front = dn < (T)0;
                const V3<T> N = front ? out : V3<T>{-out.x, -out.y, -out.z};
                const int mtype = (int)rec[10];
                const bool glass = mtype == RTIOW_DIELECTRIC;
                const bool specular = glass || (mtype == RTIOW_METAL && (double)rec[7] <= max_fuzz);
                const V3<T> An = glass ? A : V3<T>{A.x * rec[4], A.y * rec[5], A.z * rec[6]};
                const T Zn = Z + t;
                if (!specular || b == max_bounces) {
                    gnx = N.x; gny = N.y; gnz = N.z; gz = Zn;
                    gax = An.x; gay = An.y; gaz = An.z;
                    alive = false;
                } else {
                    A = An; Z = Zn; O = P; ++b;
                    if (!glass) {                                  // metal: the mirror direction, as long as D
                        const T dN = (D.x * N.x + D.y * N.y) + D.z * N.z;
                        const T c2 = (T)2 * dN;
                        D = {D.x - c2 * N.x, D.y - c2 * N.y, D.z - c2 * N.z};
                    } else {
                        const T dd = (D.x * D.x + D.y * D.y) + D.z * D.z;
                        const T len = Real<T>::sqrt(dd);
                        const T il = (T)1 / len;
                        const V3<T> u = {D.x * il, D.y * il, D.z * il};
                        const T m = -((u.x * N.x + u.y * N.y) + u.z * N.z);
                        const T ct = m < (T)1 ? m : (T)1;          // min(m, 1); 1 for a NaN
                        const T st = Real<T>::sqrt((T)1 - ct * ct);
                        const T ri = front ? rec[9] : rec[8];
                        V3<T> r;
                        if (ri * st > (T)1) {                      // total internal reflection
                            const T c2 = (T)2 * -ct;
                            r = {u.x - c2 * N.x, u.y - c2 * N.y, u.z - c2 * N.z};
                        } else {
                            const V3<T> perp = {ri * (u.x + ct * N.x), ri * (u.y + ct * N.y), ri * (u.z + ct * N.z)};
                            const T kk = -Real<T>::sqrt(Real<T>::fabs((T)1 - ((perp.x * perp.x + perp.y * perp.y) + perp.z * perp.z)));
                            r = {perp.x + kk * N.x, perp.y + kk * N.y, perp.z + kk * N.z};
                        }
                        D = {r.x * len, r.y * len, r.z * len};
                    }
                }
            }
        }
    }
    const size_t lp = (size_t)jl * W + i;
    nd[4 * lp] = gnx; nd[4 * lp + 1] = gny; nd[4 * lp + 2] = gnz; nd[4 * lp + 3] = gz;
    alb[4 * lp] = gax; alb[4 * lp + 1] = gay; alb[4 * lp + 2] = gaz; alb[4 * lp + 3] = (T)b;
}

}  // namespace
