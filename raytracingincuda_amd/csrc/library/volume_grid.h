// volume_grid.h -- the plan and the device blob of the THREE-axis uniform grid that is walked in device memory (RTIOW_SCENE_VOLUME_GRID,
// rtiow_render_volume; device/hit_volume_grid.h walks it).  device_grid.h's grid runs over x and z and holds the y extent as one slab: a
// scene that fills a volume (a particle cloud, a stack of layers) is registered there column by column.  Here y is an axis like the other
// two.  The argument for exactness, the candidates, the margins and the tables are grid_plan.h's, unchanged; what is stated here is the
// frame, the registration and the cells over three axes.
// Plain C++ (no HIP): also built on its own by tests/native/volume_grid_plan_main.cpp.
#pragma once
#include "grid_plan.h"

// The exactness argument is the one at the top of grid_plan.h with y treated like x and z:
//  registration    sphere i goes into every cell its cube [c - w - eps, c + w + eps]^3 touches, against the fp32 edges the kernel uses
//                  (x0f, y0f, z0f, cellf);
//  cell            >= lower = 2 (wmax + eps) 1.02, so a sphere lies in at most 2 x 2 x 2 cells;
//  direct list     every other sphere, one whose cube leaves the grid included (cannot happen by the extents; kept exact if it does).
// What differs from plan_device_grid:
//  frame           ext_y = (hi[1] - lo[1]) + 2 wmax, y0f = (float)(lo[1] - wmax - 0.25 cell), ny = ceil(ext_y / cell) + 1; nx, nz as in
//                  frame_grid; the cell is widened by 1.25 until nx ny nz <= max_cells.  Unlike the 2-D loop this one can run: at the
//                  natural cell the cell count is about spheres / K, and a scene of more than a million spheres meets the cap;
//  cell size       natural = cbrt(K ext_x ext_y ext_z / count), cell = max(natural, lower): about K spheres' centres a cell, each sphere
//                  of the r = 0.2, pitch 1 lattices in about 2.8 cells;
//  ranking         direct + 12 (cell / natural)^3: the direct list's spheres against the ~12 a walk meets in cells of the natural size,
//                  growing with the cell's volume;
//  cells           {first, count} at record index (iy nz + iz) nx + ix.
// VOLUME_GRID_MAX_CELLS = 2^20 is 8 MB of records: a record's byte offset stays inside 32 bits.
constexpr long long VOLUME_GRID_MAX_CELLS = 1ll << 20;
constexpr int VOLUME_GRID_MAX_DIRECT = 2048;
#ifndef RTIOW_VOLUME_GRID_K
#define RTIOW_VOLUME_GRID_K 1.0                       // scripts/volume_scene_probe.py builds 1.5 and 2.0 beside it (profiles/volume_scenes)
#endif
constexpr double VOLUME_GRID_K = RTIOW_VOLUME_GRID_K; // spheres' centres per cell of the natural size

struct VolumeGridPlan : GridPlanBase {
    int ny = 0;
    float y0f = 0;
    int longest = 0;
    size_t occupied = 0;                // cells with a list
    std::vector<uint32_t> cells;        // [ny][nz][nx]{first, count}: the cell's slice of `indices`
    std::vector<uint32_t> indices;      // sphere indices, ascending within a cell
};

struct VolumeCellSpan { int lo[3], hi[3]; };           // x, y, z

inline VolumeGridPlan plan_volume_grid(int m, const std::vector<double>& cr, const double* ctr, long long max_cells = VOLUME_GRID_MAX_CELLS) {
    VolumeGridPlan none;
    if (m < 24 || max_cells < 1) return none;
    const std::vector<int> all = grid_candidates(m, cr);
    // ---- the candidates: pure arithmetic over the set, no registration yet
    std::vector<int> small = all;
    GridCandidate best;
    double best_cell = 0, best_score = 0;
    bool have = false;
    const int direct_cap = std::min(VOLUME_GRID_MAX_DIRECT, std::max(8, m / 6));
    auto ext_y_of = [](const GridCandidate& c) { return (c.hi[1] - c.lo[1]) + 2 * c.wmax; };
    for (int attempt = 0; attempt < 16 && small.size() >= 16; ++attempt) {
        const GridCandidate c = grid_candidate(small, cr, ctr);
        const double natural = std::cbrt(VOLUME_GRID_K * c.ext_x * ext_y_of(c) * c.ext_z / (double)c.count);
        const double cell = std::max(natural, c.lower);
        const int direct = m - (int)c.count;
        const double q = cell / natural;
        const double score = (double)direct + 12.0 * q * q * q;
        if (c.L < 1e6 && std::isfinite(cell) && cell > 0 && std::isfinite(score) && direct <= direct_cap && (!have || score < best_score)) { best = c; best_cell = cell; best_score = score; have = true; }
        drop_largest_radii(small, cr, c);
    }
    if (!have) return none;
    // ---- the winner's frame: origin, cell width and size as the kernel will use them
    VolumeGridPlan pl;
    double cell = best_cell;
    const double ext_y = ext_y_of(best);
    for (;;) {
        const double fx = std::ceil(best.ext_x / cell) + 1, fy = std::ceil(ext_y / cell) + 1, fz = std::ceil(best.ext_z / cell) + 1;
        if (fx * fy * fz <= (double)max_cells) { pl.nx = (int)fx; pl.ny = (int)fy; pl.nz = (int)fz; break; }
        cell *= 1.25;
    }
    pl.cellf = (float)cell; pl.rfar = best.rfar; pl.eps = best.eps;
    pl.x0f = (float)(best.lo[0] - best.wmax - 0.25 * cell); pl.y0f = (float)(best.lo[1] - best.wmax - 0.25 * cell); pl.z0f = (float)(best.lo[2] - best.wmax - 0.25 * cell);
    // ---- registered in index order against the cell edges the KERNEL will use (fp32 origin and width), widened by eps again: every
    // cell's count first ...  The loop is grid_plan.h's register_spheres over three axes (that header stays as it is): what it does to
    // the direct list, halfwidth, the slab, the core box, rmax_g and cmax_g must stay what register_spheres does.
    const int nx = pl.nx, ny = pl.ny, nz = pl.nz;
    const size_t ncells = (size_t)nx * ny * nz;
    const float origin[3] = {pl.x0f, pl.y0f, pl.z0f};
    const int dims[3] = {nx, ny, nz};
    auto record = [&](int ix, int iy, int iz) { return ((size_t)iy * nz + iz) * nx + ix; };
    std::vector<char> is_small(m, 0);
    for (size_t k = 0; k < best.count; ++k) is_small[all[k]] = 1;
    std::vector<uint32_t> count(ncells, 0);
    std::vector<VolumeCellSpan> span(m, VolumeCellSpan{{0, 0, 0}, {-1, -1, -1}});
    pl.halfwidth.assign(m, 0.0);
    for (int i = 0; i < m; ++i) {
        if (!is_small[i]) { pl.direct.push_back(i); continue; }
        const double* s = &cr[4 * (size_t)i];
        const double w = best.w(s[3]);
        VolumeCellSpan sp;
        bool inside = true;
        for (int k = 0; k < 3; ++k) {
            const long long a = (long long)std::floor((s[k] - w - best.eps - (double)origin[k]) / (double)pl.cellf);
            const long long b = (long long)std::floor((s[k] + w + best.eps - (double)origin[k]) / (double)pl.cellf);
            inside = inside && a >= 0 && b < dims[k];
            sp.lo[k] = (int)a; sp.hi[k] = (int)b;
        }
        if (!inside) { pl.direct.push_back(i); continue; }
        span[i] = sp;
        for (int iy = sp.lo[1]; iy <= sp.hi[1]; ++iy)
            for (int iz = sp.lo[2]; iz <= sp.hi[2]; ++iz)
                for (int ix = sp.lo[0]; ix <= sp.hi[0]; ++ix) ++count[record(ix, iy, iz)];
        ++pl.registered;
        pl.halfwidth[i] = w;
        pl.ylo = std::min(pl.ylo, s[1] - w); pl.yhi = std::max(pl.yhi, s[1] + w);
        double d2 = 0;
        for (int k = 0; k < 3; ++k) { pl.core_lo[k] = std::min(pl.core_lo[k], s[k]); pl.core_hi[k] = std::max(pl.core_hi[k], s[k]); const double d = s[k] - ctr[k]; d2 += d * d; }
        pl.rmax_g = std::max(pl.rmax_g, s[3]);
        pl.cmax_g = std::max(pl.cmax_g, std::sqrt(d2));
    }
    // ... then {first, count} by a running sum, and the indices in sphere order: ascending within every cell
    pl.cells.assign(2 * ncells, 0);
    uint64_t total = 0;
    for (size_t c = 0; c < ncells; ++c) {
        pl.cells[2 * c] = (uint32_t)total; pl.cells[2 * c + 1] = 0;
        total += count[c];
        pl.longest = std::max(pl.longest, (int)count[c]);
        pl.occupied += count[c] ? 1 : 0;
    }
    if (total > 0x7fffffffull) return none;
    pl.indices.assign((size_t)total, 0);
    for (int i = 0; i < m; ++i)
        for (int iy = span[i].lo[1]; iy <= span[i].hi[1]; ++iy)
            for (int iz = span[i].lo[2]; iz <= span[i].hi[2]; ++iz)
                for (int ix = span[i].lo[0]; ix <= span[i].hi[0]; ++ix) {
                    const size_t c = record(ix, iy, iz);
                    pl.indices[pl.cells[2 * c] + pl.cells[2 * c + 1]++] = (uint32_t)i;
                }
    pl.usable = pl.registered >= 16 && (int)pl.direct.size() <= direct_cap;
    return pl;
}

// The device blob of a plan, in the handle's precision T; build_device_grid_blob's layout:
//   cells {first, count} x nx ny nz | indices | AoS table {cx, cy, cz, r^2} (+ the never-hit entry m) | direct table | direct ids | 16 spare bytes
// stage_scene copies the direct table and the ids to LDS; the rest is read where it lies.  The caller refuses a blob of 2 GiB or more.
typedef GridBlob VolumeGridBlob;

template <class T>
VolumeGridBlob build_volume_grid_blob(const VolumeGridPlan& pl, int m, const std::vector<double>& cr) {
    VolumeGridBlob b;
    b.cells_offset = append_section(b.bytes, pl.cells);
    b.indices_offset = append_section(b.bytes, pl.indices);
    b.aos_offset = append_section(b.bytes, aos_table<T>(m, cr));
    append_direct_sections<T>(b, pl, m, cr);
    b.bytes.resize(b.bytes.size() + 16, 0);                          // one spare line: an empty section still has an address inside the blob
    return b;
}

// GridParams of a plan (fill_grid_params, then the two fields the third axis needs; device/params.h says where they ride).
template <class G>
void fill_volume_grid_params(G& g, const VolumeGridPlan& pl) {
    fill_grid_params(g, pl);
    g.ylo = pl.y0f;                     // y0: the origin of the cells along y
    g.yhi = (float)pl.ny;               // ny <= 2^20: exact in fp32
}
