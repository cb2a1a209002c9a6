// device_grid.h -- the plan and the device blob of the uniform grid that is walked in device memory (RTIOW_SCENE_DEVICE_GRID,
// rtiow_render_large; device/hit_device_grid.h walks it).  plan_device_grid is plan_grid's argument for exactness (scene_tables.h) with
// its capacity limits lifted: cells are variable-length lists of 32-bit sphere indices, so no sphere is pushed to the direct list by a
// full cell, no index has to fit 16 bits, and the cell count is bounded by memory, not by LDS.
// Plain C++ (no HIP): also built on its own by tests/native/large_grid_plan_main.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

// What stays of plan_grid, to the letter:
//  registration half-width  w_i = sqrt(r_i^2 + E_i) + eps, E_i = 18 * 2^-24 * 1.01 ((Rfar + Cmax)^2 + r_i^2), Rfar = max(64, 4 Cmax),
//                           eps = 2^-16 L, L = 2 (Rfar + Cmax) + |ctr|_inf + rmax;
//  registration             sphere i goes into every cell its square [c - w - eps, c + w + eps]^2 touches, against the fp32 cell edges
//                           the kernel uses;
//  cell                     >= 2 (wmax + eps) 1.02, so a sphere lies in at most 2 x 2 cells.
// What differs:
//  cells                    {first, count} per cell into ONE array of 32-bit sphere indices, ascending within a cell;
//  cell size                a mean of about two spheres per occupied cell: cell^2 = 1.5 x (area / spheres) -- a sphere of the r = 0.2, pitch 1
//                           lattices is in ~1.3 cells -- or the lower bound above when that is wider (large scenes: E grows with Cmax^2);
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

struct DeviceGridPlan {
    bool usable = false;
    int nx = 0, nz = 0, registered = 0, longest = 0;
    float cellf = 0, x0f = 0, z0f = 0;
    double rfar = 0, eps = 0, ylo = 1e300, yhi = -1e300, core_lo[3] = {1e300, 1e300, 1e300}, core_hi[3] = {-1e300, -1e300, -1e300}, rmax_g = 0, cmax_g = 0;
    std::vector<uint32_t> cells;        // [nz][nx]{first, count}: the cell's slice of `indices`
    std::vector<uint32_t> indices;      // sphere indices, ascending within a cell
    std::vector<int> direct;
    std::vector<double> halfwidth;      // w_i of the registered spheres (0 for the direct list)
};

inline DeviceGridPlan plan_device_grid(int m, const std::vector<double>& cr, const double* ctr) {
    DeviceGridPlan none;
    if (m < 24) return none;
    std::vector<double> radii(m);
    for (int i = 0; i < m; ++i) radii[i] = cr[4 * (size_t)i + 3];
    std::vector<int> small;
    for (int i = 0; i < m; ++i) {
        bool ok = radii[i] > 0 && std::isfinite(radii[i]);
        for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(cr[4 * (size_t)i + k]);
        if (ok) small.push_back(i);
    }
    std::sort(small.begin(), small.end(), [&](int a, int b) { return radii[a] < radii[b] || (radii[a] == radii[b] && a < b); });
    const double u18 = 18.0 * std::ldexp(1.0, -24) * 1.01;
    // ---- the candidates: pure arithmetic over the set, no registration yet
    struct Candidate { size_t count = 0; double cell = 0, rfar = 0, eps = 0, cmax = 0, wmax = 0, lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, score = 0; };
    Candidate best;
    bool have = false;
    const int direct_cap = std::min(DEVICE_GRID_MAX_DIRECT, std::max(8, m / 6));
    for (int attempt = 0; attempt < 16 && small.size() >= 16; ++attempt) {
        Candidate c;
        c.count = small.size();
        double rmax = 0;
        for (int k = 0; k < 3; ++k) { c.lo[k] = 1e300; c.hi[k] = -1e300; }
        for (int i : small) {
            double d2 = 0;
            for (int k = 0; k < 3; ++k) { const double v = cr[4 * (size_t)i + k], d = v - ctr[k]; d2 += d * d; c.lo[k] = std::min(c.lo[k], v); c.hi[k] = std::max(c.hi[k], v); }
            c.cmax = std::max(c.cmax, std::sqrt(d2));
            rmax = std::max(rmax, radii[i]);
        }
        const double cut = 0.9 * rmax;                                   // the next candidate drops the largest radii
        c.cmax *= 1.0001;
        c.rfar = std::max(64.0, 4.0 * c.cmax);
        double cabs = 0;
        for (int k = 0; k < 3; ++k) cabs = std::max(cabs, std::fabs(ctr[k]));
        const double L = 2.0 * (c.rfar + c.cmax) + cabs + rmax;          // every coordinate the walk handles is smaller
        c.eps = std::ldexp(L, -16);
        const double E = u18 * ((c.rfar + c.cmax) * (c.rfar + c.cmax) + rmax * rmax);
        c.wmax = std::sqrt(rmax * rmax + E) + c.eps;                      // w grows with r: the largest radius has the widest square
        const double ext_x = (c.hi[0] - c.lo[0]) + 2 * c.wmax, ext_z = (c.hi[2] - c.lo[2]) + 2 * c.wmax;
        const double natural = std::sqrt(1.5 * ext_x * ext_z / (double)c.count);
        const double lower = 2.0 * (c.wmax + c.eps) * 1.02;
        c.cell = std::max(natural, lower);
        const int direct = m - (int)c.count;
        c.score = (double)direct + 12.0 * (c.cell / natural) * (c.cell / natural);
        if (L < 1e6 && std::isfinite(c.cell) && c.cell > 0 && direct <= direct_cap && (!have || c.score < best.score)) { best = c; have = true; }
        while (!small.empty() && radii[small.back()] >= cut) small.pop_back();
    }
    if (!have) return none;
    // ---- the winner, registered
    small.clear();
    {
        std::vector<int> order;
        for (int i = 0; i < m; ++i) {
            bool ok = radii[i] > 0 && std::isfinite(radii[i]);
            for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(cr[4 * (size_t)i + k]);
            if (ok) order.push_back(i);
        }
        std::sort(order.begin(), order.end(), [&](int a, int b) { return radii[a] < radii[b] || (radii[a] == radii[b] && a < b); });
        order.resize(best.count);
        small.swap(order);
    }
    DeviceGridPlan pl;
    double cell = best.cell;
    const double ext_x = (best.hi[0] - best.lo[0]) + 2 * best.wmax, ext_z = (best.hi[2] - best.lo[2]) + 2 * best.wmax;
    for (;;) {
        const double fx = std::ceil(ext_x / cell) + 1, fz = std::ceil(ext_z / cell) + 1;
        if (fx * fz <= (double)DEVICE_GRID_MAX_CELLS) { pl.nx = (int)fx; pl.nz = (int)fz; break; }
        cell *= 1.25;
    }
    pl.cellf = (float)cell; pl.rfar = best.rfar; pl.eps = best.eps;
    pl.x0f = (float)(best.lo[0] - best.wmax - 0.25 * cell); pl.z0f = (float)(best.lo[2] - best.wmax - 0.25 * cell);
    // registration against the cell edges the KERNEL will use (fp32 origin and width), widened by eps again
    auto cell_of = [&](double v, float origin) { return (long long)std::floor((v - (double)origin) / (double)pl.cellf); };
    const int nx = pl.nx, nz = pl.nz;
    const size_t ncells = (size_t)nx * nz;
    std::vector<char> is_small(m, 0);
    for (int i : small) is_small[i] = 1;
    pl.halfwidth.assign(m, 0.0);
    std::vector<uint32_t> count(ncells, 0);
    struct Span { int ix0, ix1, iz0, iz1; };
    std::vector<Span> span(m, Span{0, -1, 0, -1});
    const double eps = best.eps;
    for (int i = 0; i < m; ++i) {
        if (!is_small[i]) { pl.direct.push_back(i); continue; }
        const double cx = cr[4 * (size_t)i], cy = cr[4 * (size_t)i + 1], cz = cr[4 * (size_t)i + 2];
        const double E = u18 * ((best.rfar + best.cmax) * (best.rfar + best.cmax) + radii[i] * radii[i]);
        const double w = std::sqrt(radii[i] * radii[i] + E) + eps;
        const long long ix0 = cell_of(cx - w - eps, pl.x0f), ix1 = cell_of(cx + w + eps, pl.x0f);
        const long long iz0 = cell_of(cz - w - eps, pl.z0f), iz1 = cell_of(cz + w + eps, pl.z0f);
        if (!(ix0 >= 0 && iz0 >= 0 && ix1 < nx && iz1 < nz)) { pl.direct.push_back(i); continue; }     // cannot happen by the extents; kept exact if it does
        span[i] = Span{(int)ix0, (int)ix1, (int)iz0, (int)iz1};
        for (int iz = (int)iz0; iz <= (int)iz1; ++iz)
            for (int ix = (int)ix0; ix <= (int)ix1; ++ix) ++count[(size_t)iz * nx + ix];
        ++pl.registered;
        pl.halfwidth[i] = w;
        pl.ylo = std::min(pl.ylo, cy - w); pl.yhi = std::max(pl.yhi, cy + w);
        const double c3[3] = {cx, cy, cz};
        double d2 = 0;
        for (int k = 0; k < 3; ++k) { pl.core_lo[k] = std::min(pl.core_lo[k], c3[k]); pl.core_hi[k] = std::max(pl.core_hi[k], c3[k]); const double d = c3[k] - ctr[k]; d2 += d * d; }
        pl.rmax_g = std::max(pl.rmax_g, radii[i]);
        pl.cmax_g = std::max(pl.cmax_g, std::sqrt(d2));
    }
    // {first, count} by a running sum, then the indices in sphere order: ascending within every cell
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
//   cells {first, count} x nx nz | indices | AoS spheres {cx, cy, cz, r^2} x (m + 1): entry m never hits | direct table | direct ids
// every section padded to 16 bytes.  The direct table is laid out as geom_a is (fp32: pair-interleaved for the packed trips; padded to a
// multiple of four with never-hit entries, their id m): stage_scene copies it and the ids to LDS.  The offsets are bytes from the blob's
// start, as GridParams carries them (cells_offset, aos_offset, direct_offset, direct_ids_offset; the indices follow the cells).
struct DeviceGridBlob {
    std::vector<unsigned char> bytes;
    size_t cells_offset = 0, indices_offset = 0, aos_offset = 0, direct_offset = 0, direct_ids_offset = 0;
    int n_direct_padded = 0;
};
inline size_t device_grid_align16(size_t v) { return (v + 15) / 16 * 16; }

template <class T>
DeviceGridBlob build_device_grid_blob(const DeviceGridPlan& pl, int m, const std::vector<double>& cr) {
    DeviceGridBlob b;
    const int nd = (int)pl.direct.size(), ndp = (nd + 3) / 4 * 4;
    std::vector<T> dtab((size_t)ndp * 4);
    std::vector<int32_t> ids(ndp, m);
    for (int k = 0; k < ndp; ++k) {
        if (k < nd) {
            const int i = pl.direct[k];
            const T r = (T)cr[4 * (size_t)i + 3];
            dtab[4 * k] = (T)cr[4 * (size_t)i]; dtab[4 * k + 1] = (T)cr[4 * (size_t)i + 1]; dtab[4 * k + 2] = (T)cr[4 * (size_t)i + 2]; dtab[4 * k + 3] = (T)(r * r);   // as upload_scene
            ids[k] = i;
        } else { dtab[4 * k] = dtab[4 * k + 1] = dtab[4 * k + 2] = (T)0; dtab[4 * k + 3] = (T)-1e12; }
    }
    if (sizeof(T) == 4) {                                    // pair-interleave like geom_a (trip_discriminants)
        std::vector<T> pi(dtab.size());
        for (int q = 0; q < ndp / 2; ++q)
            for (int k = 0; k < 4; ++k) { pi[8 * q + 2 * k] = dtab[8 * q + k]; pi[8 * q + 2 * k + 1] = dtab[8 * q + 4 + k]; }
        dtab.swap(pi);
    }
    std::vector<T> aos((size_t)(m + 1) * 4);
    for (int i = 0; i < m; ++i) {
        const T r = (T)cr[4 * (size_t)i + 3];
        aos[4 * (size_t)i] = (T)cr[4 * (size_t)i]; aos[4 * (size_t)i + 1] = (T)cr[4 * (size_t)i + 1]; aos[4 * (size_t)i + 2] = (T)cr[4 * (size_t)i + 2]; aos[4 * (size_t)i + 3] = (T)(r * r);
    }
    aos[4 * (size_t)m] = aos[4 * (size_t)m + 1] = aos[4 * (size_t)m + 2] = (T)0; aos[4 * (size_t)m + 3] = (T)-1e12;
    const size_t cells_bytes = device_grid_align16(pl.cells.size() * sizeof(uint32_t));
    const size_t idx_bytes = device_grid_align16(pl.indices.size() * sizeof(uint32_t));
    const size_t aos_bytes = device_grid_align16(aos.size() * sizeof(T));
    const size_t dtab_bytes = device_grid_align16(dtab.size() * sizeof(T));
    const size_t ids_bytes = device_grid_align16(ids.size() * sizeof(int32_t));
    b.cells_offset = 0;
    b.indices_offset = cells_bytes;
    b.aos_offset = b.indices_offset + idx_bytes;
    b.direct_offset = b.aos_offset + aos_bytes;
    b.direct_ids_offset = b.direct_offset + dtab_bytes;
    b.n_direct_padded = ndp;
    b.bytes.assign(b.direct_ids_offset + ids_bytes + 16, 0);         // one spare line: an empty section still has an address inside the blob
    if (!pl.cells.empty()) std::memcpy(b.bytes.data() + b.cells_offset, pl.cells.data(), pl.cells.size() * sizeof(uint32_t));
    if (!pl.indices.empty()) std::memcpy(b.bytes.data() + b.indices_offset, pl.indices.data(), pl.indices.size() * sizeof(uint32_t));
    std::memcpy(b.bytes.data() + b.aos_offset, aos.data(), aos.size() * sizeof(T));
    if (!dtab.empty()) std::memcpy(b.bytes.data() + b.direct_offset, dtab.data(), dtab.size() * sizeof(T));
    if (!ids.empty()) std::memcpy(b.bytes.data() + b.direct_ids_offset, ids.data(), ids.size() * sizeof(int32_t));
    return b;
}
