// grid_plan.h -- the uniform grids over a scene's small spheres, on the host: what the LDS grid (RTIOW_SCENE_GRID, device/hit_grid.h) and
// the device-memory grid (RTIOW_SCENE_DEVICE_GRID, device/hit_device_grid.h; its plan is device_grid.h's) share, each stated once -- the
// candidates and their margins, the registration against the kernel's fp32 cell edges, the tables of a blob and its 16-byte sections,
// GridParams from a plan, the recentring point -- and the LDS grid's own plan (plan_grid) and blob (build_grid_blob).
// Plain C++ (no HIP): also built on its own by tests/native/grid_plan_main.cpp and tests/native/large_grid_plan_main.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

// The exactness argument both walks rest on (device/hit_grid.h has the kernel's half):
//  small sphere    : registration half-width w_i = sqrt(r_i^2 + E_i) + eps <= cell / 2, where
//                    E_i = 18 * 2^-24 * 1.01 ((Rfar + Cmax)^2 + r_i^2) bounds the reference's discriminant noise for every origin within
//                    Rfar = max(64, 4 Cmax) of the recentring point, eps = 2^-16 L, L = 2 (Rfar + Cmax) + |ctr|_inf + rmax;
//  registration    : sphere i goes into every cell its square [c - w - eps, c + w + eps]^2 touches, against the fp32 cell edges the
//                    kernel uses;
//  cell            : >= 2 (wmax + eps) 1.02, so a sphere lies in at most 2 x 2 cells;
//  direct list     : everything else (ground, big spheres, non-finite or non-positive ones), tested exactly by every ray.
// Candidate "small" sets: every finite sphere, then without the radii >= 0.9 rmax, and so on.  What a plan does with a candidate --
// the cell size, the choice among candidates, the cells' form, the caps -- is its own (plan_grid below, plan_device_grid).

// What every plan has; everything downstream of a plan (GridParams, the direct table, the debug hooks) reads these alone.
struct GridPlanBase {
    bool usable = false;
    int nx = 0, nz = 0, registered = 0;
    float cellf = 0, x0f = 0, z0f = 0;
    double rfar = 0, eps = 0, ylo = 1e300, yhi = -1e300, core_lo[3] = {1e300, 1e300, 1e300}, core_hi[3] = {-1e300, -1e300, -1e300}, rmax_g = 0, cmax_g = 0;
    std::vector<int> direct;
    std::vector<double> halfwidth;      // w_i of the registered spheres (0 for the direct list)
};

// The spheres that may be gridded at all (finite centre, finite positive radius), by radius, then index.
inline std::vector<int> grid_candidates(int m, const std::vector<double>& cr) {
    std::vector<int> small;
    for (int i = 0; i < m; ++i) {
        const double* s = &cr[4 * (size_t)i];
        if (s[3] > 0 && std::isfinite(s[3]) && std::isfinite(s[0]) && std::isfinite(s[1]) && std::isfinite(s[2])) small.push_back(i);
    }
    std::sort(small.begin(), small.end(), [&](int a, int b) { const double ra = cr[4 * (size_t)a + 3], rb = cr[4 * (size_t)b + 3]; return ra < rb || (ra == rb && a < b); });
    return small;
}

// The statistics and margins of one candidate set.
struct GridCandidate {
    size_t count = 0;
    double cmax = 0, rmax = 0, rfar = 0, L = 0, eps = 0, wmax = 0, lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    double ext_x = 0, ext_z = 0;        // the grid's extents: the centres' box widened by wmax
    double lower = 0;                   // the cell's lower bound
    double w(double r) const {
        const double E = 18.0 * 0x1p-24 * 1.01 * ((rfar + cmax) * (rfar + cmax) + r * r);
        return std::sqrt(r * r + E) + eps;
    }
};
inline GridCandidate grid_candidate(const std::vector<int>& small, const std::vector<double>& cr, const double* ctr) {
    GridCandidate c;
    c.count = small.size();
    for (int i : small) {
        double d2 = 0;
        for (int k = 0; k < 3; ++k) { const double v = cr[4 * (size_t)i + k], d = v - ctr[k]; d2 += d * d; c.lo[k] = std::min(c.lo[k], v); c.hi[k] = std::max(c.hi[k], v); }
        c.cmax = std::max(c.cmax, std::sqrt(d2));
        c.rmax = std::max(c.rmax, cr[4 * (size_t)i + 3]);
    }
    c.cmax *= 1.0001;
    c.rfar = std::max(64.0, 4.0 * c.cmax);
    double cabs = 0;
    for (int k = 0; k < 3; ++k) cabs = std::max(cabs, std::fabs(ctr[k]));
    c.L = 2.0 * (c.rfar + c.cmax) + cabs + c.rmax;                     // every coordinate the walk handles is smaller
    c.eps = std::ldexp(c.L, -16);
    c.wmax = c.w(c.rmax);                                              // w grows with r: the largest radius has the widest square
    c.ext_x = (c.hi[0] - c.lo[0]) + 2 * c.wmax; c.ext_z = (c.hi[2] - c.lo[2]) + 2 * c.wmax;
    c.lower = 2.0 * (c.wmax + c.eps) * 1.02;
    return c;
}
// The next candidate: without the radii >= 0.9 rmax of this one.
inline void drop_largest_radii(std::vector<int>& small, const std::vector<double>& cr, const GridCandidate& c) {
    const double cut = 0.9 * c.rmax;
    while (!small.empty() && cr[4 * (size_t)small.back() + 3] >= cut) small.pop_back();
}

// Origin, cell width (widened by 1.25 until the grid has at most max_cells) and size of a candidate's grid, as the kernel will use them.
inline void frame_grid(GridPlanBase& pl, const GridCandidate& c, double cell, long long max_cells) {
    for (;;) {
        const double fx = std::ceil(c.ext_x / cell) + 1, fz = std::ceil(c.ext_z / cell) + 1;
        if (fx * fz <= (double)max_cells) { pl.nx = (int)fx; pl.nz = (int)fz; break; }
        cell *= 1.25;
    }
    pl.cellf = (float)cell; pl.rfar = c.rfar; pl.eps = c.eps;
    pl.x0f = (float)(c.lo[0] - c.wmax - 0.25 * cell); pl.z0f = (float)(c.lo[2] - c.wmax - 0.25 * cell);
}

// Registers the spheres of `small` in index order; every other sphere, one whose square leaves the grid (cannot happen by the extents;
// kept exact if it does) and one that place(i, span) turns away join the direct list.  place stores sphere i in the cells of its span.
struct CellSpan { int ix0, ix1, iz0, iz1; };
template <class Place>
void register_spheres(GridPlanBase& pl, int m, const std::vector<double>& cr, const double* ctr, const std::vector<int>& small, const GridCandidate& c, Place place) {
    // against the cell edges the KERNEL will use (fp32 origin and width), widened by eps again
    auto cell_of = [&](double v, float origin) { return (long long)std::floor((v - (double)origin) / (double)pl.cellf); };
    std::vector<char> is_small(m, 0);
    for (int i : small) is_small[i] = 1;
    pl.halfwidth.assign(m, 0.0);
    for (int i = 0; i < m; ++i) {
        if (!is_small[i]) { pl.direct.push_back(i); continue; }
        const double* s = &cr[4 * (size_t)i];
        const double w = c.w(s[3]);
        const long long ix0 = cell_of(s[0] - w - c.eps, pl.x0f), ix1 = cell_of(s[0] + w + c.eps, pl.x0f);
        const long long iz0 = cell_of(s[2] - w - c.eps, pl.z0f), iz1 = cell_of(s[2] + w + c.eps, pl.z0f);
        if (!(ix0 >= 0 && iz0 >= 0 && ix1 < pl.nx && iz1 < pl.nz) || !place(i, CellSpan{(int)ix0, (int)ix1, (int)iz0, (int)iz1})) { pl.direct.push_back(i); continue; }
        ++pl.registered;
        pl.halfwidth[i] = w;
        pl.ylo = std::min(pl.ylo, s[1] - w); pl.yhi = std::max(pl.yhi, s[1] + w);
        double d2 = 0;
        for (int k = 0; k < 3; ++k) { pl.core_lo[k] = std::min(pl.core_lo[k], s[k]); pl.core_hi[k] = std::max(pl.core_hi[k], s[k]); const double d = s[k] - ctr[k]; d2 += d * d; }
        pl.rmax_g = std::max(pl.rmax_g, s[3]);
        pl.cmax_g = std::max(pl.cmax_g, std::sqrt(d2));
    }
}

// ---- the LDS grid's plan: about one sphere per cell, four 16-bit slots a cell; a sphere that meets a full cell joins the direct list.
// A candidate whose natural cell is narrower than the lower bound is dropped; of at most 12 candidates the plan with the shortest direct
// list wins.  nx nz <= 4096 (LDS), 24 <= m <= 60000 (16-bit indices, m itself the pad).  `usable` stays false when the grid would not pay
// (few small spheres, or a direct list that is no shorter than a fraction of the scene): the scene keeps the screened loop.
struct GridPlan : GridPlanBase {
    std::vector<uint16_t> cells;        // [nz][nx][4]: sphere indices, 0xffff x4 = empty cell, index m = never-hit pad
};

inline GridPlan plan_grid(int m, const std::vector<double>& cr, const double* ctr) {
    GridPlan best;
    if (m < 24 || m > 60000) return best;
    std::vector<int> small = grid_candidates(m, cr);
    bool have = false;
    for (int attempt = 0; attempt < 12 && (int)small.size() >= 16; ++attempt) {
        const GridCandidate c = grid_candidate(small, cr, ctr);
        const double cell = std::sqrt(c.ext_x * c.ext_z / (double)c.count);
        if (c.L < 1e6 && cell >= c.lower) {
            GridPlan pl;
            frame_grid(pl, c, cell, 4096);
            const int nx = pl.nx;
            pl.cells.assign((size_t)nx * pl.nz * 4, 0xffff);
            std::vector<int> count((size_t)nx * pl.nz, 0);
            register_spheres(pl, m, cr, ctr, small, c, [&](int i, CellSpan s) {
                for (int iz = s.iz0; iz <= s.iz1; ++iz)
                    for (int ix = s.ix0; ix <= s.ix1; ++ix) if (count[(size_t)iz * nx + ix] >= 4) return false;
                for (int iz = s.iz0; iz <= s.iz1; ++iz)
                    for (int ix = s.ix0; ix <= s.ix1; ++ix) { const size_t at = (size_t)iz * nx + ix; pl.cells[4 * at + count[at]++] = (uint16_t)i; }
                return true;
            });
            // a partly filled cell pads with index m, the never-hit entry behind the table (upload_scene)
            for (size_t at = 0; at < count.size(); ++at)
                if (count[at] > 0) for (int k = count[at]; k < 4; ++k) pl.cells[4 * at + k] = (uint16_t)m;
            if (pl.registered >= 16 && (!have || pl.direct.size() < best.direct.size())) { best = std::move(pl); have = true; }
        }
        drop_largest_radii(small, cr, c);
    }
    best.usable = have && (int)best.direct.size() <= std::max(8, m / 6);
    return best;
}

// ---- tables
// fp32 tables of {cx, cy, cz, w} entries are pair-interleaved for v_pk_*_f32 (trip_discriminants): entries 2q and 2q + 1 become
// {cx, cx', cy, cy', cz, cz', w, w'}.  The table holds an even number of entries.
template <class T>
void pair_interleave(std::vector<T>& t) {
    std::vector<T> pi(t.size());
    for (size_t q = 0; q < t.size() / 8; ++q)
        for (int k = 0; k < 4; ++k) { pi[8 * q + 2 * k] = t[8 * q + k]; pi[8 * q + 2 * k + 1] = t[8 * q + 4 + k]; }
    t.swap(pi);
}

// {cx, cy, cz, r * r} of sphere i in T as upload_scene stores it, and the entry that never hits: c = |oc|^2 + 1e12 => disc < 0.
template <class T>
void push_sphere(std::vector<T>& t, const std::vector<double>& cr, int i) {
    const double* s = &cr[4 * (size_t)i];
    const T r = (T)s[3];
    t.insert(t.end(), {(T)s[0], (T)s[1], (T)s[2], (T)(r * r)});
}
template <class T>
void push_never_hit(std::vector<T>& t) { t.insert(t.end(), {(T)0, (T)0, (T)0, (T)-1e12}); }

// The direct table of a plan, laid out as geom_a is (padded to a multiple of four with never-hit entries, their id m; fp32:
// pair-interleaved), and its ids.
template <class T>
std::vector<T> direct_table(const std::vector<int>& direct, int m, const std::vector<double>& cr, std::vector<int32_t>& ids) {
    std::vector<T> t;
    ids.assign(direct.begin(), direct.end());
    for (int i : direct) push_sphere(t, cr, i);
    while (ids.size() % 4) { push_never_hit(t); ids.push_back(m); }
    if (sizeof(T) == 4) pair_interleave(t);
    return t;
}
// The AoS table of the walk's per-lane gathers: every sphere, then entry m, which never hits.
template <class T>
std::vector<T> aos_table(int m, const std::vector<double>& cr) {
    std::vector<T> t;
    t.reserve(4 * ((size_t)m + 1));
    for (int i = 0; i < m; ++i) push_sphere(t, cr, i);
    push_never_hit(t);
    return t;
}

// ---- blobs: sections padded to 16 bytes; the offsets are bytes from the blob's start, named as GridParams names them (the device
// grid's indices follow its cells).
struct GridBlobOffsets {
    size_t cells_offset = 0, indices_offset = 0, aos_offset = 0, direct_offset = 0, direct_ids_offset = 0;
    int n_direct_padded = 0;
};
struct GridBlob : GridBlobOffsets {
    std::vector<unsigned char> bytes;
};
inline size_t device_grid_align16(size_t v) { return (v + 15) / 16 * 16; }

// Appends a section and returns its offset.
template <class E>
size_t append_section(std::vector<unsigned char>& blob, const std::vector<E>& section) {
    const size_t at = blob.size(), bytes = section.size() * sizeof(E);
    blob.resize(at + device_grid_align16(bytes), 0);
    if (bytes) std::memcpy(blob.data() + at, section.data(), bytes);
    return at;
}
// The direct table and its ids, the last two sections of either blob.
template <class T>
void append_direct_sections(GridBlob& b, const GridPlanBase& pl, int m, const std::vector<double>& cr) {
    std::vector<int32_t> ids;
    const std::vector<T> table = direct_table<T>(pl.direct, m, cr, ids);
    b.n_direct_padded = (int)ids.size();
    b.direct_offset = append_section(b.bytes, table);
    b.direct_ids_offset = append_section(b.bytes, ids);
}

// The LDS grid's blob in the handle's precision T: cells | AoS table (fp32 only: fp64 gathers from geom_a, which is AoS already) |
// direct table | direct ids.  layout_lds places it behind the other tables in LDS.
template <class T>
GridBlob build_grid_blob(const GridPlan& pl, int m, const std::vector<double>& cr) {
    GridBlob b;
    b.cells_offset = append_section(b.bytes, pl.cells);
    b.aos_offset = append_section(b.bytes, sizeof(T) == 4 ? aos_table<T>(m, cr) : std::vector<T>());
    append_direct_sections<T>(b, pl, m, cr);
    return b;
}

// ---- GridParams (device/params.h; G stands for it here, this header knows no HIP) from a plan: the slab and the box of the centres
// rounded outwards, the squares and Cmax with the slack that covers the kernel's raw roots.  The blob's pointer, size and offsets are
// the caller's.
template <class G>
void fill_grid_params(G& g, const GridPlanBase& pl) {
    g.use_grid = 1;
    g.nx = pl.nx; g.nz = pl.nz;
    g.x0 = pl.x0f; g.z0 = pl.z0f; g.cell = pl.cellf; g.inv_cell = (float)(1.0 / (double)pl.cellf);
    g.ylo = std::nextafter((float)pl.ylo, -INFINITY); g.yhi = std::nextafter((float)pl.yhi, INFINITY);
    g.far2 = (float)(pl.rfar * pl.rfar * 0.999);
    for (int k = 0; k < 3; ++k) { g.core_lo[k] = std::nextafter((float)pl.core_lo[k], -INFINITY); g.core_hi[k] = std::nextafter((float)pl.core_hi[k], INFINITY); }
    g.rmax2 = (float)(pl.rmax_g * pl.rmax_g * 1.0001);
    g.cmax = (float)(pl.cmax_g * 1.0001);
}
// ... and the offsets of a blob that starts `base` bytes into what the kernel addresses (LDS, or the blob itself: 0).
template <class G>
void place_grid_blob(G& g, const GridBlobOffsets& at, size_t base) {
    g.n_direct_padded = at.n_direct_padded;
    g.cells_offset = (int)(base + at.cells_offset); g.aos_offset = (int)(base + at.aos_offset);
    g.direct_offset = (int)(base + at.direct_offset); g.direct_ids_offset = (int)(base + at.direct_ids_offset);
}

// The recentring point: the centroid of the spheres that are not ground-like (r < 100), zero without any; finite_only leaves out
// spheres with a non-finite centre.  The callers round it to the handle's precision.
inline void recentring_point(int m, const std::vector<double>& cr, bool finite_only, double* ctr) {
    double sum[3] = {0, 0, 0};
    int cnt = 0;
    for (int i = 0; i < m; ++i) {
        const double* s = &cr[4 * (size_t)i];
        if (!(s[3] < 100.0) || (finite_only && !(std::isfinite(s[0]) && std::isfinite(s[1]) && std::isfinite(s[2])))) continue;
        for (int k = 0; k < 3; ++k) sum[k] += s[k];
        ++cnt;
    }
    for (int k = 0; k < 3; ++k) ctr[k] = cnt ? sum[k] / cnt : 0.0;
}
