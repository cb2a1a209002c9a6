// hit_device_grid.h -- hit_world over a uniform grid that stays in device memory (RTIOW_SCENE_DEVICE_GRID, rtiow_render_large), and the
// scene staging that goes with it.  Included by rtiow_large.hip, rtiow_large_preview.hip and rtiow_large_upscale.hip alone, behind the
// headers every unit shares: the other code objects do not see it and keep their kernels.
#pragma once
#include "hit_grid.h"
#include "pixel_io.h"

namespace {

// =====================================================================================
// The LDS grid (hit_grid.h) ends where a scene's tables outgrow a compute unit's LDS.  Here only the DIRECT list -- the few spheres too
// big for a cell -- is staged in LDS; the cell table, the index array and the spheres stay in the device blob (library/device_grid.h):
//     cells {first, count} x nx nz | indices (32 bit) | AoS spheres {cx, cy, cz, r^2} x (n + 1) | direct table | direct ids
// and a lane reads the record of each cell its ray crosses, the cell's slice of the index array and the listed spheres from there.
//
// Why the result is unchanged: hit_world_grid's argument, word for word.  The registration (half-width, eps, Rfar) is library/grid_plan.h's, the
// setup below is hit_world_grid's (near / sane / crosses, clip_axis), every listed sphere is tested with the reference's arithmetic and
// the ANYORDER tie rule, so the result is the lexicographic minimum of (root, index) over a superset of the spheres the reference
// could accept.  Far, NaN and huge rays send the wave through the exact loop over the device table.
//
// The walk's boundaries.  The LDS grid advances the leaving parameters incrementally, which is exact enough only because its walks
// take at most nx + nz <= 128 steps.  This grid has up to about 190 cells an axis (library/device_grid.h), so the parameters are computed in CLOSED FORM at every step:
//     b = (float)(c + 1 or c) * cell          one rounding: <= 2^-24 |b|
//     t = (b - o) * inv_d                     the difference rounds once (<= 2^-24 max(|b|, |o|)), the raw reciprocal is within 1 ulp
//                                             (2^-23 relative) and the product rounds once (2^-24 relative): <= 2^-22 relative of t
// As a position along the ray that is at most 2^-23 L for b and b - o (|b|, |o| <= L, the largest coordinate in play, of which
// eps = 2^-16 L) plus 2^-22 of the distance walked (<= 2 L): under 2^-20 L = eps / 16 at every step, however long the walk -- nothing
// accumulates.  The bound the exactness argument asks for is eps / 2.
// =====================================================================================

// LDS of a large-scene launch: the direct table (n_direct_padded x 4 T, laid out like geom_a) at offset 0, its ids behind it, then
// what RenderParams places (shade records, drain scratch).  The table is what the kernels pass on as `lds_geom`.
template <class T>
__device__ __forceinline__ T* stage_device_grid(const RenderParams<T>& p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* lds_direct = reinterpret_cast<T*>(smem_raw);
    const int ndp = p.grid.n_direct_padded;
    const unsigned char* blob = p.grid.blob;
    {
        const T* src = reinterpret_cast<const T*>(blob + p.grid.direct_offset);
        for (int k = threadIdx.x; k < ndp * 4; k += blockDim.x) lds_direct[k] = src[k];
        int* ids = reinterpret_cast<int*>(lds_direct + 4 * ndp);
        const int* src_ids = reinterpret_cast<const int*>(blob + p.grid.direct_ids_offset);
        for (int k = threadIdx.x; k < ndp; k += blockDim.x) ids[k] = src_ids[k];
    }
    if (p.shade_in_lds) {
        T* lds_shade = reinterpret_cast<T*>(smem_raw + p.shade_offset);
        const T* tbl = p.screen.shade_tbl;
        for (int k = threadIdx.x; k < p.n * 12; k += blockDim.x) lds_shade[k] = tbl[k];
    }
    __syncthreads();
    return lds_direct;
}
template <>
__device__ __forceinline__ float* stage_scene<float, RTIOW_SCENE_DEVICE_GRID>(const RenderParams<float>& p) { return stage_device_grid<float>(p); }
template <>
__device__ __forceinline__ double* stage_scene<double, RTIOW_SCENE_DEVICE_GRID>(const RenderParams<double>& p) { return stage_device_grid<double>(p); }

// One sphere of a cell's list for this lane's ray: hittable.h:42-47 on a 16-byte gather (fp64: two).
template <class T>
__device__ __forceinline__ void list_slot(const unsigned char* __restrict__ blob, unsigned aos_at, int i, V3<T> O, V3<T> D, T a, T& h, T& disc) {
    T cx, cy, cz, r2;
    load_sphere(reinterpret_cast<const T*>(blob + (aos_at + (unsigned)i * (unsigned)(4 * sizeof(T)))), 0, cx, cy, cz, r2);
    const T ocx = cx - O.x, ocy = cy - O.y, ocz = cz - O.z;                         // :42
    h = RT_FMA(D.z, ocz, RT_FMA(D.y, ocy, D.x * ocx));                              // :44
    const T c = RT_FMA(ocz, ocz, RT_FMA(ocy, ocy, ocx * ocx)) - r2;                 // :45
    disc = RT_FMA(h, h, -(a * c));                                                  // :47
}

// The spheres of one cell, in pairs: a pair's two discriminants share one candidate branch (as in cell_tests), and the
// next pair runs behind ONE wave-level branch -- only while some lane of this step still has entries.  A lane whose list is shorter
// tests the never-hit entry `pad` (index n of the sphere table) instead: no load outside its slice of the index array.  list_at: the
// byte offset of the cell's slice from the blob's start.
template <class T>
__device__ __forceinline__ void cell_list_tests(const unsigned char* __restrict__ blob, unsigned aos_at, unsigned list_at, unsigned count, int pad,
                                                V3<T> O, V3<T> D, T a, T& closest, int& hit, FastDiv<T> fd) {
    for (unsigned k = 0; __builtin_amdgcn_ballot_w64(k < count) != 0; k += 2) {
        int i0 = pad, i1 = pad;
        if (k < count) i0 = *reinterpret_cast<const int*>(blob + (list_at + k * 4u));
        if (k + 1 < count) i1 = *reinterpret_cast<const int*>(blob + (list_at + k * 4u + 4u));
        T h0, d0, h1, d1;
        list_slot<T>(blob, aos_at, i0, O, D, a, h0, d0);
        list_slot<T>(blob, aos_at, i1, O, D, a, h1, d1);
        if (Real<T>::fmax(d0, d1) >= (T)0) {                                            // :48 for either of the two
            if (d0 >= (T)0) finish_sphere_test<T, true>(i0, h0, d0, a, closest, hit, fd);
            if (d1 >= (T)0) finish_sphere_test<T, true>(i1, h1, d1, a, closest, hit, fd);
        }
    }
}

// visited (COUNT only): the cells this lane's walk read, or -1 when its wave took the exact loop.
template <class T, bool COUNT>
__device__ __forceinline__ void hit_world_device_grid(const RenderParams<T>& p, const T* lds_direct, V3<T> O, V3<T> D, T a, T& closest, int& hit, int& visited) {
    const auto& g = grid_of(p);
    // ---- which rays the registration margins cover: hit_world_grid's setup
    const auto& sc = screen_of(p);
    const float fx = (float)(O.x - (T)sc.ctr_x), fy = (float)(O.y - (T)sc.ctr_y), fz = (float)(O.z - (T)sc.ctr_z);
    const float k2 = __builtin_fmaf(fz, fz, __builtin_fmaf(fy, fy, fx * fx));
    const float af = (float)a;
    const bool sane = af > 1e-30f && af < 1e30f && k2 < 1e30f;        // false for NaN as well
    const bool near = sane && k2 <= g.far2;
    const float ox = (float)O.x - g.x0, oy = (float)O.y, oz = (float)O.z - g.z0;
    const float dx = (float)D.x, dy = (float)D.y, dz = (float)D.z;
    float t0 = 0.0f, t1 = __builtin_huge_valf();
    float xlo = 0.0f, xhi = (float)g.nx * g.cell, zlo = 0.0f, zhi = (float)g.nz * g.cell, ylo = g.ylo, yhi = g.yhi;
    if (__builtin_amdgcn_ballot_w64(!near) != 0) {
        const float reach = fast_sqrt(k2) * 1.001f + g.cmax;
        const float E = 9.5367431640625e-07f * __builtin_fmaf(reach, reach, g.rmax2);
        const float rho = fast_sqrt(g.rmax2 + E) * 1.001f;
        if (!near) {
            xlo = g.core_lo[0] - g.x0 - rho; xhi = g.core_hi[0] - g.x0 + rho;
            ylo = g.core_lo[1] - rho;        yhi = g.core_hi[1] + rho;
            zlo = g.core_lo[2] - g.z0 - rho; zhi = g.core_hi[2] - g.z0 + rho;
        }
    }
    clip_axis(oy, dy, ylo, yhi, t0, t1);
    const float inv_dx = clip_axis(ox, dx, xlo, xhi, t0, t1);
    const float inv_dz = clip_axis(oz, dz, zlo, zhi, t0, t1);
    const bool crosses = !sane || t0 <= t1;
    if (__builtin_amdgcn_ballot_w64(!near && crosses) != 0) {
        // a far ray that skims the scene, a NaN or a huge one: the exact loop over the device table, for every lane of the wave
        hit_world_direct<T, RTIOW_SCENE_SCALAR>(p, lds_direct, O, D, a, closest, hit);
        if (COUNT) visited = -1;
        return;
    }
    // ---- one reciprocal for every quotient of this segment (FastDiv above ieee_roots)
    FastDiv<T> fd = {(T)0, false};
    if (p.range_flags & 2) {
        fd.on = __builtin_amdgcn_ballot_w64(!(a >= (T)0x1p-40 && a <= (T)0x1p40)) == 0;
        fd.ra = refined_reciprocal(a);
    }
    auto direct_list_and_walk = [&](auto fast_tag) __attribute__((always_inline)) {
        const FastDiv<T> fdc = {fd.ra, decltype(fast_tag)::value};
        // ---- the direct list, from LDS: packed trips, every ray
        {
            const int* ids = reinterpret_cast<const int*>(lds_direct + 4 * g.n_direct_padded);
            const LoopRay<T> r = make_loop_ray(O.x, O.y, O.z, D.x, D.y, D.z, a);
            for (int s = 0; s < g.n_direct_padded; s += 4) direct_trip<T>(lds_direct, ids, s, r, closest, hit, fdc);
        }
        // ---- the walk, from device memory
        bool walking = near && crosses;
        if (__builtin_amdgcn_ballot_w64(walking) == 0) return;
        // one base pointer and 32-bit byte offsets from it (the blob is under 2 GiB): every gather is `base + offset`, and the walk
        // carries one pointer in scalar registers instead of three
        const unsigned char* __restrict__ blob = g.blob;
        const int nx = g.nx, nz = g.nz;
        const unsigned cells_at = (unsigned)g.cells_offset;
        const unsigned idx_at = cells_at + (unsigned)((nx * nz * 8 + 15) & ~15);          // the indices follow the cells
        const unsigned aos_at = (unsigned)g.aos_offset;
        auto cell_record = [&](int ix, int iz) __attribute__((always_inline)) { return *reinterpret_cast<const uint2*>(blob + (cells_at + (unsigned)(iz * nx + ix) * 8u)); };
        const int pad = p.n;
        const float px = __builtin_fmaf(t0, dx, ox), pz = __builtin_fmaf(t0, dz, oz);
        int cx = (int)__builtin_floorf(px * g.inv_cell), cz = (int)__builtin_floorf(pz * g.inv_cell);
        cx = cx < 0 ? 0 : (cx >= nx ? nx - 1 : cx);
        cz = cz < 0 ? 0 : (cz >= nz ? nz - 1 : cz);
        const bool step_x = __builtin_fabsf(dx) >= 1e-30f, step_z = __builtin_fabsf(dz) >= 1e-30f;
        const int sx = dx > 0.0f ? 1 : -1, sz = dz > 0.0f ? 1 : -1;
        uint2 rec = {0u, 0u};
        if (walking) rec = cell_record(cx, cz);
        while (__builtin_amdgcn_ballot_w64(walking) != 0) {
            if (walking) {
                if (COUNT) ++visited;
                // where the ray leaves this cell, per axis, in closed form (the bound above), and the record of the cell it enters
                // next -- asked for before this cell's tests, whose gathers it then overlaps.  Always a cell of the table.
                const float bx = (float)(cx + (sx > 0 ? 1 : 0)) * g.cell, bz = (float)(cz + (sz > 0 ? 1 : 0)) * g.cell;
                const float tx = step_x ? (bx - ox) * inv_dx : __builtin_huge_valf();
                const float tz = step_z ? (bz - oz) * inv_dz : __builtin_huge_valf();
                const float tnext = __builtin_fminf(tx, tz);
                const bool x_first = tx <= tz;
                const int ncx = cx + (x_first ? sx : 0), ncz = cz + (x_first ? 0 : sz);
                const bool enters = (unsigned)ncx < (unsigned)nx && (unsigned)ncz < (unsigned)nz && tnext < t1;
                uint2 next = {0u, 0u};
                if (enters) next = cell_record(ncx, ncz);
                cell_list_tests<T>(blob, aos_at, idx_at + rec.x * 4u, rec.y, pad, O, D, a, closest, hit, fdc);
                const float tend = __builtin_fminf(t1, (float)closest);               // (float) rounds to nearest: covered by eps
                if (!enters || tnext >= tend) walking = false;                        // leaves the slab / the grid, or a nearer hit is known
                else { cx = ncx; cz = ncz; rec = next; }
            }
        }
    };
    if (fd.on) direct_list_and_walk(std::true_type{});
    else direct_list_and_walk(std::false_type{});
}

template <>
__device__ __forceinline__ void hit_world<float, RTIOW_SCENE_DEVICE_GRID>(const RenderParams<float>& p, const float* lds_geom, V3<float> O, V3<float> D,
                                                                          float a, float& closest, int& hit) {
    int visited = 0;
    hit_world_device_grid<float, false>(p, lds_geom, O, D, a, closest, hit, visited);
}
template <>
__device__ __forceinline__ void hit_world<double, RTIOW_SCENE_DEVICE_GRID>(const RenderParams<double>& p, const double* lds_geom, V3<double> O, V3<double> D,
                                                                           double a, double& closest, int& hit) {
    int visited = 0;
    hit_world_device_grid<double, false>(p, lds_geom, O, D, a, closest, hit, visited);
}

// ---- rtiow_render_large's kernels: persistent_body (render_kernels.h) over the new source -- the persistent hand-out in tile order,
// fp64's rotated trip, the drain; under names of their own, so that a profile tells them from rtiow_render's.
template <class T, bool BOUND_F32>
__global__ void __launch_bounds__(1024) large_scene_kernel(const RenderParams<T> p) { persistent_body<T, RTIOW_SCENE_DEVICE_GRID, false, false, BOUND_F32>(p); }

#ifdef RTIOW_DEBUG_API
// hit_world through the device grid on caller-supplied rays, one per lane (rtiow_debug_hit_world_large), with the cells each ray visited.
template <class T>
__global__ void __launch_bounds__(256) large_hit_probe_kernel(const RenderParams<T> p, const T* __restrict__ rays, int n, T* __restrict__ out_t, int* __restrict__ out_idx,
                                                              int* __restrict__ out_cells) {
    const T* lds_direct = stage_scene<T, RTIOW_SCENE_DEVICE_GRID>(p);
    for (int base = (int)blockIdx.x * (int)blockDim.x; base < n; base += (int)gridDim.x * (int)blockDim.x) {
        const int k = base + (int)threadIdx.x;
        if (k < n) {
            const V3<T> O = {rays[6 * (size_t)k], rays[6 * (size_t)k + 1], rays[6 * (size_t)k + 2]};
            const V3<T> D = {rays[6 * (size_t)k + 3], rays[6 * (size_t)k + 4], rays[6 * (size_t)k + 5]};
            T closest = __builtin_huge_val();
            int hit = -1, visited = 0;
            hit_world_device_grid<T, true>(p, lds_direct, O, D, dot3(D, D), closest, hit, visited);
            out_t[k] = closest; out_idx[k] = hit; out_cells[k] = visited;
        }
    }
}
#endif

}  // namespace
