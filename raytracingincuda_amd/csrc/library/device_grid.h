// device_grid.h -- the plan and the device blob of the uniform grid that is walked in device memory (RTIOW_SCENE_DEVICE_GRID,
// rtiow_render_large; device/hit_device_grid.h walks it).  The argument for exactness, the candidates, the registration and the tables
// are grid_plan.h's, shared with the LDS grid; here the capacity limits are lifted: cells are variable-length lists of 32-bit sphere
// indices, so no sphere is pushed to the direct list by a full cell, no index has to fit 16 bits, and the cell count is bounded by
// memory, not by LDS.
// Plain C++ (no HIP): also built on its own by tests/native/large_grid_plan_main.cpp.
#pragma once
#include "grid_plan.h"

// What differs from plan_grid:
//  cells                    {first, count} per cell into ONE array of 32-bit sphere indices, ascending within a cell;
//  cell size                a mean of about two spheres per occupied cell: cell^2 = 1.5 x (area / spheres) -- a sphere of the r = 0.2, pitch 1
//                           lattices is in ~1.3 cells -- or the cell's lower bound when that is wider (large scenes: E grows with Cmax^2);
//  cell-count cap           DEVICE_GRID_MAX_CELLS = 2^20, a guard that no scene reaches.  The cell's lower bound grows with the scene:
//                           w >= sqrt(E) >= sqrt(18 * 2^-24 * 1.01) (Rfar + Cmax) >= 5.2e-3 Cmax (Rfar >= 4 Cmax, Cmax the plan's
//                           1.0001 Cmax), so cell > 2.04 w > 0.0106 Cmax, while an axis extends over at most 2 Cmax + 2 wmax: nx and nz
//                           are at most about 190 each, the grid about 36 000 cells (0.3 MB of records), and beyond that many cells'
//                           worth of spheres the LISTS grow instead (1.6 million lattice spheres: 128 x 128 cells, a longest list of
//                           about 400).  The loop that widens the cells by 1.25 under the cap is kept as the guard's other half and does not
//                           run; (iz nx + ix) 8 stays far inside an int (the kernel computes the record's byte offset in 32 bits);
//  which spheres are small  candidates as in plan_grid (every finite sphere, then without the largest radii, ...), but a candidate whose
//                           natural cell is narrower than its lower bound is kept with the bound instead of dropped -- a lattice of equal
//                           spheres has no smaller radii to fall back to.  The candidates are ranked by an estimate of a ray's tests:
//                           direct + 12 (cell / natural cell)^2, i.e. the direct list's spheres against the ~12 a walk meets in cells of
//                           the natural size, growing with the cell's area.  The ground and the three unit spheres lose to it, a scene
//                           of equal spheres keeps all of them;
//  direct list              only the spheres too big for a cell.  It lives in LDS; the plan is unusable when it is longer than
//                           max(8, m / 6) (the walk would not pay) or than DEVICE_GRID_MAX_DIRECT = 2048 (32 KB of fp64 table + 8 KB of
//                           ids: what leaves the shade records of a small scene and the drain scratch their room in a workgroup's LDS).
constexpr long long DEVICE_GRID_MAX_CELLS = 1ll << 20;
constexpr int DEVICE_GRID_MAX_DIRECT = 2048;

struct DeviceGridPlan : GridPlanBase {
    int longest = 0;
    std::vector<uint32_t> cells;        // [nz][nx]{first, count}: the cell's slice of `indices`
    std::vector<uint32_t> indices;      // sphere indices, ascending within a cell
};

inline DeviceGridPlan plan_device_grid(int m, const std::vector<double>& cr, const double* ctr) {
    DeviceGridPlan none;
    if (m < 24) return none;
    const std::vector<int> all = grid_candidates(m, cr);
    // ---- the candidates: pure arithmetic over the set, no registration yet
    std::vector<int> small = all;
    GridCandidate best;
    double best_cell = 0, best_score = 0;
    bool have = false;
    const int direct_cap = std::min(DEVICE_GRID_MAX_DIRECT, std::max(8, m / 6));
    for (int attempt = 0; attempt < 16 && small.size() >= 16; ++attempt) {
        const GridCandidate c = grid_candidate(small, cr, ctr);
        const double natural = std::sqrt(1.5 * c.ext_x * c.ext_z / (double)c.count);
        const double cell = std::max(natural, c.lower);
        const int direct = m - (int)c.count;
        const double score = (double)direct + 12.0 * (cell / natural) * (cell / natural);
        if (c.L < 1e6 && std::isfinite(cell) && cell > 0 && direct <= direct_cap && (!have || score < best_score)) { best = c; best_cell = cell; best_score = score; have = true; }
        drop_largest_radii(small, cr, c);
    }
    if (!have) return none;
    // ---- the winner, registered: every cell's count first ...
    small.assign(all.begin(), all.begin() + best.count);
    DeviceGridPlan pl;
    frame_grid(pl, best, best_cell, DEVICE_GRID_MAX_CELLS);
    const int nx = pl.nx;
    const size_t ncells = (size_t)nx * pl.nz;
    std::vector<uint32_t> count(ncells, 0);
    std::vector<CellSpan> span(m, CellSpan{0, -1, 0, -1});
    register_spheres(pl, m, cr, ctr, small, best, [&](int i, CellSpan s) {
        span[i] = s;
        for (int iz = s.iz0; iz <= s.iz1; ++iz)
            for (int ix = s.ix0; ix <= s.ix1; ++ix) ++count[(size_t)iz * nx + ix];
        return true;
    });
    // ... then {first, count} by a running sum, and the indices in sphere order: ascending within every cell
    pl.cells.assign(2 * ncells, 0);
    uint64_t total = 0;
    for (size_t c = 0; c < ncells; ++c) { pl.cells[2 * c] = (uint32_t)total; pl.cells[2 * c + 1] = 0; total += count[c]; pl.longest = std::max(pl.longest, (int)count[c]); }
    if (total > 0x7fffffffull) return none;
    pl.indices.assign((size_t)total, 0);
    for (int i = 0; i < m; ++i)
        for (int iz = span[i].iz0; iz <= span[i].iz1; ++iz)
            for (int ix = span[i].ix0; ix <= span[i].ix1; ++ix) {
                const size_t c = (size_t)iz * nx + ix;
                pl.indices[pl.cells[2 * c] + pl.cells[2 * c + 1]++] = (uint32_t)i;
            }
    pl.usable = pl.registered >= 16 && (int)pl.direct.size() <= direct_cap;
    return pl;
}

// The device blob of a plan, in the handle's precision T:
//   cells {first, count} x nx nz | indices | AoS table (both precisions) | direct table | direct ids | 16 spare bytes
// stage_scene copies the direct table and the ids to LDS; the rest is read where it lies.
typedef GridBlob DeviceGridBlob;

template <class T>
DeviceGridBlob build_device_grid_blob(const DeviceGridPlan& pl, int m, const std::vector<double>& cr) {
    DeviceGridBlob b;
    b.cells_offset = append_section(b.bytes, pl.cells);
    b.indices_offset = append_section(b.bytes, pl.indices);
    b.aos_offset = append_section(b.bytes, aos_table<T>(m, cr));
    append_direct_sections<T>(b, pl, m, cr);
    b.bytes.resize(b.bytes.size() + 16, 0);                          // one spare line: an empty section still has an address inside the blob
    return b;
}
