// guide_lens.h -- lens-sampled filter guides (rtiow_set_guide_lens): the mean of the guide values over a fixed G x G lattice of points on
// the camera's defocus disk, for the a-trous filters to steer by what the APERTURE sees of a pixel, as the image they filter is rendered
// Part of the single gfx950 translation unit rtiow_hip.hip (included there, in this order; internal linkage).
//
// Every value here is defined operation by operation and evaluated in T with plain * + - / and sqrt, as in
// denoise.h: no RT_FMA, madd3, dot3, unit3 or reflect3 for a guide value.
#pragma once
#include "guide_chain.h"

namespace {

// ---- The lens guides of local pixel (i, jl) with global row j: G in {2, 4} lens points per side (a runtime argument), S = G G.  Lens
// sample s = a + G b (b outer) leaves from the lattice point o_a = (T)(2 a + 1) / (T)G - 1 (o_b likewise; -+0.5, or -+0.75 and -+0.25:
// exact) scaled by kappa = 1 (G = 2) or (T)sqrt(0.8) (G = 4), which gives the lattice the second moment of the uniform unit disk and keeps
// every point inside it: lx = kappa o_a, ly = kappa o_b, O_s = (O + lx U) + ly V per component with U, V the camera's defocus_disk_u / _v,
// and goes through the pixel centre on the focus plane, ps = (pixel00 + (T)i du) + (T)j dv of guide_kernel: D_s = ps - O_s.  These are
// the rays the render kernels draw, without their randomness.  From (O_s, D_s) the chain of guide_chain.h runs to the letter -- its bounce
// step is restated here, so that guide_chain_kernel's code stays what it was -- and ends in (normal'_s, albedo'_s, depth'_s, b_s).
// max_bounces = 0 ends every chain at its first hit: guide_kernel's values (1 a_k = a_k and 0 + t = t are exact).  The pixel's guides:
// the sums from 0 in s order, per component, times q = (T)1 / (T)S (0.25 or 0.0625, exact), not renormalised -- a blurred normal is shorter,
// and that is the information -- and bounces = the largest b_s.  A ray that misses adds zeros.  Two 4-T vectors per pixel, as the chain's:
// nd = {normal, depth}, alb = {albedo, (T)bounces}.
// One lane per local pixel, one 8x8 tile per wave, the scene staged as in guide_kernel.  The S rays run in one loop that is not unrolled,
// around a single inlined hit_world inside the chain's ballot-driven bounce loop; all rays of a trip leave from the same lens point, so a
// wave's rays are as coherent as guide_kernel's.  Seven running sums and a maximum per lane; no indexed private array.
template <class T, int SRC>
__global__ void __launch_bounds__(256) guide_lens_kernel(const RenderParams<T> p, int G, int max_bounces, double max_fuzz, T* __restrict__ nd, T* __restrict__ alb) {
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
    const V3<T> ps = {(cam.pixel00.x + fi * cam.du.x) + fj * cam.dv.x, (cam.pixel00.y + fi * cam.du.y) + fj * cam.dv.y,
                      (cam.pixel00.z + fi * cam.du.z) + fj * cam.dv.z};
    const int S = G * G;
    const T fG = (T)G, kappa = G == 2 ? (T)1 : (T)0.8944271909999159;
    T snx = 0, sny = 0, snz = 0, sz = 0, sax = 0, say = 0, saz = 0;
    int bmax = 0;
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
        const int la = s & (G - 1), lb = s >> (G >> 1);          // s % G and s / G for G = 2, 4
        const T lx = kappa * ((T)(2 * la + 1) / fG - (T)1), ly = kappa * ((T)(2 * lb + 1) / fG - (T)1);
        V3<T> O = {(cam.center.x + lx * cam.ddu.x) + ly * cam.ddv.x, (cam.center.y + lx * cam.ddu.y) + ly * cam.ddv.y,
                   (cam.center.z + lx * cam.ddu.z) + ly * cam.ddv.z};
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
        snx = snx + gnx; sny = sny + gny; snz = snz + gnz; sz = sz + gz;
        sax = sax + gax; say = say + gay; saz = saz + gaz;
        bmax = b > bmax ? b : bmax;
    }
    const T q = (T)1 / (T)S;
    const size_t lp = (size_t)jl * W + i;
    nd[4 * lp] = snx * q; nd[4 * lp + 1] = sny * q; nd[4 * lp + 2] = snz * q; nd[4 * lp + 3] = sz * q;
    alb[4 * lp] = sax * q; alb[4 * lp + 1] = say * q; alb[4 * lp + 2] = saz * q; alb[4 * lp + 3] = (T)bmax;
}

}  // namespace
