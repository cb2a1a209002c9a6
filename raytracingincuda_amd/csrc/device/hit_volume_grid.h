// hit_volume_grid.h -- hit_world over a THREE-axis uniform grid that stays in device memory (RTIOW_SCENE_VOLUME_GRID, rtiow_render_volume
// and the _volume preview calls).  Included by rtiow_volume.hip, rtiow_volume_preview.hip and rtiow_volume_upscale.hip alone, behind the headers every unit shares and device/hit_device_grid.h, whose staging
// (stage_device_grid), sphere gather (list_slot) and cell tests (cell_list_tests) it calls as they are: the other code objects do not
// see it and keep their kernels.
#pragma once
#include "hit_device_grid.h"

namespace {

// =====================================================================================
// The device grid (hit_device_grid.h) runs over x and z; y is one slab, so a scene that fills a volume puts a whole column of spheres
// into every cell's list.  Here y is an axis like the other two (library/volume_grid.h):
//     cells {first, count} x nx ny nz | indices (32 bit) | AoS spheres {cx, cy, cz, r^2} x (n + 1) | direct table | direct ids
// with the record of cell (ix, iy, iz) at index (iy nz + iz) nx + ix.  GridParams carries the third axis in the two fields this source
// leaves free (params.h): ylo = y0, the origin of the cells along y, and yhi = (float)ny.
//
// Why the result is unchanged: hit_world_device_grid's argument with y treated like x and z.  The registration is against the cube
// [c - w - eps, c + w + eps]^3 and the fp32 edges used below, the setup is the same (near / sane / crosses, clip_axis on three axes),
// every listed sphere is tested with the reference's arithmetic and the ANYORDER tie rule, so the result is the lexicographic minimum
// of (root, index) over a superset of the spheres the reference could accept.  Far, NaN and huge rays send the wave through the exact
// loop over the device table.
//
// The walk's boundaries are in closed form at every step, per axis, as in hit_device_grid.h: b = (float)(c + 1 or c) * cell,
// t = (b - o) * inv_d, under eps / 16 as a position along the ray at every step with nothing accumulating; the bound holds for each
// axis alone, so a third one adds nothing to it.  The ray steps along the axis with the smallest t; ties go to x, then y, then z.
// =====================================================================================

template <>
__device__ __forceinline__ float* stage_scene<float, RTIOW_SCENE_VOLUME_GRID>(const RenderParams<float>& p) { return stage_device_grid<float>(p); }
template <>
__device__ __forceinline__ double* stage_scene<double, RTIOW_SCENE_VOLUME_GRID>(const RenderParams<double>& p) { return stage_device_grid<double>(p); }

// visited (COUNT only): the cells this lane's walk read, or -1 when its wave took the exact loop.
template <class T, bool COUNT>
__device__ __forceinline__ void hit_world_volume_grid(const RenderParams<T>& p, const T* lds_direct, V3<T> O, V3<T> D, T a, T& closest, int& hit, int& visited) {
    const auto& g = grid_of(p);
    // ---- which rays the registration margins cover: hit_world_grid's setup
    const auto& sc = screen_of(p);
    const float fx = (float)(O.x - (T)sc.ctr_x), fy = (float)(O.y - (T)sc.ctr_y), fz = (float)(O.z - (T)sc.ctr_z);
    const float k2 = __builtin_fmaf(fz, fz, __builtin_fmaf(fy, fy, fx * fx));
    const float af = (float)a;
    const bool sane = af > 1e-30f && af < 1e30f && k2 < 1e30f;        // false for NaN as well
    const bool near = sane && k2 <= g.far2;
    const float y0 = g.ylo;                                           // the third axis (params.h)
    const int ny = (int)g.yhi;
    const float ox = (float)O.x - g.x0, oy = (float)O.y - y0, oz = (float)O.z - g.z0;
    const float dx = (float)D.x, dy = (float)D.y, dz = (float)D.z;
    float t0 = 0.0f, t1 = __builtin_huge_valf();
    float xlo = 0.0f, xhi = (float)g.nx * g.cell, ylo = 0.0f, yhi = (float)ny * g.cell, zlo = 0.0f, zhi = (float)g.nz * g.cell;
    if (__builtin_amdgcn_ballot_w64(!near) != 0) {
        const float reach = fast_sqrt(k2) * 1.001f + g.cmax;
        const float E = 9.5367431640625e-07f * __builtin_fmaf(reach, reach, g.rmax2);
        const float rho = fast_sqrt(g.rmax2 + E) * 1.001f;
        if (!near) {
            xlo = g.core_lo[0] - g.x0 - rho; xhi = g.core_hi[0] - g.x0 + rho;
            ylo = g.core_lo[1] - y0 - rho;   yhi = g.core_hi[1] - y0 + rho;
            zlo = g.core_lo[2] - g.z0 - rho; zhi = g.core_hi[2] - g.z0 + rho;
        }
    }
    const float inv_dy = clip_axis(oy, dy, ylo, yhi, t0, t1);
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
        // one base pointer and 32-bit byte offsets from it (the blob is under 2 GiB, the records under 8 MB): every gather is `base + offset`
        const unsigned char* __restrict__ blob = g.blob;
        const int nx = g.nx, nz = g.nz;
        const unsigned cells_at = (unsigned)g.cells_offset;
        const unsigned idx_at = cells_at + (unsigned)((nx * ny * nz * 8 + 15) & ~15);     // the indices follow the cells
        const unsigned aos_at = (unsigned)g.aos_offset;
        auto cell_record = [&](int ix, int iy, int iz) __attribute__((always_inline)) {
            return *reinterpret_cast<const uint2*>(blob + (cells_at + (unsigned)((iy * nz + iz) * nx + ix) * 8u));
        };
        const int pad = p.n;
        const float px = __builtin_fmaf(t0, dx, ox), py = __builtin_fmaf(t0, dy, oy), pz = __builtin_fmaf(t0, dz, oz);
        int cx = (int)__builtin_floorf(px * g.inv_cell), cy = (int)__builtin_floorf(py * g.inv_cell), cz = (int)__builtin_floorf(pz * g.inv_cell);
        cx = cx < 0 ? 0 : (cx >= nx ? nx - 1 : cx);
        cy = cy < 0 ? 0 : (cy >= ny ? ny - 1 : cy);
        cz = cz < 0 ? 0 : (cz >= nz ? nz - 1 : cz);
        // clip_axis returns 0 for an axis the ray is parallel to (|d| < 1e-30): that axis never steps
        const int sx = dx > 0.0f ? 1 : -1, sy = dy > 0.0f ? 1 : -1, sz = dz > 0.0f ? 1 : -1;
        uint2 rec = {0u, 0u};
        if (walking) rec = cell_record(cx, cy, cz);
        while (__builtin_amdgcn_ballot_w64(walking) != 0) {
            if (walking) {
                if (COUNT) ++visited;
                // where the ray leaves this cell, per axis, in closed form, and the record of the cell it enters next -- asked for before
                // this cell's tests, whose gathers it then overlaps.  Always a cell of the table.
                const float bx = (float)(cx + (sx > 0 ? 1 : 0)) * g.cell, by = (float)(cy + (sy > 0 ? 1 : 0)) * g.cell, bz = (float)(cz + (sz > 0 ? 1 : 0)) * g.cell;
                const float tx = inv_dx != 0.0f ? (bx - ox) * inv_dx : __builtin_huge_valf();
                const float ty = inv_dy != 0.0f ? (by - oy) * inv_dy : __builtin_huge_valf();
                const float tz = inv_dz != 0.0f ? (bz - oz) * inv_dz : __builtin_huge_valf();
                const bool x_first = tx <= ty && tx <= tz;                          // ties: x, then y, then z
                const bool y_first = !x_first && ty <= tz;
                const float tnext = x_first ? tx : (y_first ? ty : tz);
                const int ncx = cx + (x_first ? sx : 0), ncy = cy + (y_first ? sy : 0), ncz = cz + (x_first || y_first ? 0 : sz);
                const bool enters = (unsigned)ncx < (unsigned)nx && (unsigned)ncy < (unsigned)ny && (unsigned)ncz < (unsigned)nz && tnext < t1;
                uint2 next = {0u, 0u};
                if (enters) next = cell_record(ncx, ncy, ncz);
                cell_list_tests<T>(blob, aos_at, idx_at + rec.x * 4u, rec.y, pad, O, D, a, closest, hit, fdc);
                const float tend = __builtin_fminf(t1, (float)closest);               // (float) rounds to nearest: covered by eps
                if (!enters || tnext >= tend) walking = false;                        // leaves the grid, or a nearer hit is known
                else { cx = ncx; cy = ncy; cz = ncz; rec = next; }
            }
        }
    };
    if (fd.on) direct_list_and_walk(std::true_type{});
    else direct_list_and_walk(std::false_type{});
}

template <>
__device__ __forceinline__ void hit_world<float, RTIOW_SCENE_VOLUME_GRID>(const RenderParams<float>& p, const float* lds_geom, V3<float> O, V3<float> D,
                                                                          float a, float& closest, int& hit) {
    int visited = 0;
    hit_world_volume_grid<float, false>(p, lds_geom, O, D, a, closest, hit, visited);
}
template <>
__device__ __forceinline__ void hit_world<double, RTIOW_SCENE_VOLUME_GRID>(const RenderParams<double>& p, const double* lds_geom, V3<double> O, V3<double> D,
                                                                           double a, double& closest, int& hit) {
    int visited = 0;
    hit_world_volume_grid<double, false>(p, lds_geom, O, D, a, closest, hit, visited);
}

// ---- rtiow_render_volume's kernels: persistent_body (render_kernels.h) over the new source, as large_scene_kernel is.
constexpr int VOLUME_LAUNCH_BOUNDS = 1024;
template <class T, bool BOUND_F32>
__global__ void __launch_bounds__(VOLUME_LAUNCH_BOUNDS) volume_scene_kernel(const RenderParams<T> p) { persistent_body<T, RTIOW_SCENE_VOLUME_GRID, false, false, BOUND_F32>(p); }

#ifdef RTIOW_DEBUG_API
// hit_world through the volume grid on caller-supplied rays, one per lane (rtiow_debug_hit_world_volume), with the cells each ray visited.
template <class T>
__global__ void __launch_bounds__(256) volume_hit_probe_kernel(const RenderParams<T> p, const T* __restrict__ rays, int n, T* __restrict__ out_t, int* __restrict__ out_idx,
                                                               int* __restrict__ out_cells) {
    const T* lds_direct = stage_scene<T, RTIOW_SCENE_VOLUME_GRID>(p);
    for (int base = (int)blockIdx.x * (int)blockDim.x; base < n; base += (int)gridDim.x * (int)blockDim.x) {
        const int k = base + (int)threadIdx.x;
        if (k < n) {
            const V3<T> O = {rays[6 * (size_t)k], rays[6 * (size_t)k + 1], rays[6 * (size_t)k + 2]};
            const V3<T> D = {rays[6 * (size_t)k + 3], rays[6 * (size_t)k + 4], rays[6 * (size_t)k + 5]};
            T closest = __builtin_huge_val();
            int hit = -1, visited = 0;
            hit_world_volume_grid<T, true>(p, lds_direct, O, D, dot3(D, D), closest, hit, visited);
            out_t[k] = closest; out_idx[k] = hit; out_cells[k] = visited;
        }
    }
}
#endif

}  // namespace
