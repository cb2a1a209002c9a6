// Stand-alone check of the device grid's plan and blob (raytracingincuda_amd/csrc/library/device_grid.h), built with
// -fsanitize=address,undefined by tests/test_large_grid_plan.py and run directly.  The invariants held here are what keeps the kernel's
// gathers inside the blob: every {first, count} inside the index array, every index <= m, lists ascending, every finite sphere on the
// direct list or in every cell its inflated square touches, offsets and sizes of the blob consistent in both precisions.  Also pinned:
// the reachable size of the grid (nx, nz <= 192 whatever the scene; see main).
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "device_grid.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Lcg {
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
};

static void push(std::vector<double>& cr, double x, double y, double z, double r) { cr.insert(cr.end(), {x, y, z, r}); }

// A jittered lattice of n spheres (r = 0.2, pitch 1) on the ground, with the ground and three unit spheres in front.
static std::vector<double> lattice(int n, uint64_t seed) {
    std::vector<double> cr;
    push(cr, 0, -1000, 0, 1000);
    push(cr, 0, 1, 0, 1.0); push(cr, -4, 1, 0, 1.0); push(cr, 4, 1, 0, 1.0);
    Lcg g{seed};
    int side = 1;
    while (side * side < n) ++side;
    for (int k = 0; k < n; ++k) {
        const int ix = k % side, iz = k / side;
        push(cr, ix - 0.5 * side + 0.5 * (g.next() - 0.5), 0.2, iz - 0.5 * side + 0.5 * (g.next() - 0.5), 0.2);
    }
    return cr;
}
static std::vector<double> line(int n, double r = 0.2, double pitch = 1.0) {
    std::vector<double> cr;
    push(cr, 0, -1000, 0, 1000);
    for (int k = 0; k < n; ++k) push(cr, (k - 0.5 * n) * pitch, r, 0.0, r);
    return cr;
}

// One scene of each kind of tests/large_scene.py's EDGE_SCENES (the same shapes, this file's generator).
// clusters: the ground, 600 spheres over 40 x 40 and clusters of 1 .. 24 within 0.05 of a point, the last of every third an exact copy of its first.
static std::vector<double> clusters(uint64_t seed) {
    std::vector<double> cr;
    push(cr, 0, -1000, 0, 1000);
    Lcg g{seed};
    for (int k = 0; k < 600; ++k) { const double x = 40 * g.next() - 20, z = 40 * g.next() - 20; push(cr, x, 0.2, z, 0.2); }
    for (int k = 1; k <= 24; ++k) {
        const double px = 36 * g.next() - 18, pz = 36 * g.next() - 18;
        const size_t first = cr.size();
        for (int j = 0; j < k; ++j) { const double r = 0.15 + 0.05 * g.next(); push(cr, px + 0.07 * (g.next() - 0.5), r + 0.3 * g.next(), pz + 0.07 * (g.next() - 0.5), r); }
        if (k % 3 == 2) for (int q = 0; q < 4; ++q) cr[cr.size() - 4 + q] = cr[first + q];
    }
    return cr;
}
// equal_no_ground: 900 equal spheres on a jittered lattice at heights in [0, 3] and nothing else.
static std::vector<double> equal_no_ground(uint64_t seed) {
    std::vector<double> cr;
    Lcg g{seed};
    for (int k = 0; k < 900; ++k) { const double x = k % 30 - 15 + 0.5 * (g.next() - 0.5), z = k / 30 - 15 + 0.5 * (g.next() - 0.5); push(cr, x, 3 * g.next(), z, 0.2); }
    return cr;
}
// mixed_with_bad: the ground, four big spheres, 800 of mixed radii and heights; four of them r < 0, r = NaN, cx = inf and r = 0.
static std::vector<double> mixed_with_bad(uint64_t seed) {
    std::vector<double> cr;
    push(cr, 0, -1000, 0, 1000);
    push(cr, 0, 1, 0, 1.0); push(cr, -6, 1, 3, 1.0); push(cr, 7, 1, -4, 1.0); push(cr, 2, 1.5, 9, 1.5);
    Lcg g{seed};
    for (int k = 0; k < 800; ++k) { const double x = 30 * g.next() - 15, y = 4 * g.next() - 1, z = 30 * g.next() - 15; push(cr, x, y, z, 0.05 + 0.3 * g.next()); }
    cr[4 * 105 + 3] = -0.3; cr[4 * 305 + 3] = NAN; cr[4 * 505] = INFINITY; cr[4 * 705 + 3] = 0.0;
    return cr;
}
// far_centre: 900 equal spheres on a jittered lattice on a ground, translated by (3000, 0, -2000).
static std::vector<double> far_centre(uint64_t seed) {
    std::vector<double> cr;
    push(cr, 3000, -1000, -2000, 1000);
    Lcg g{seed};
    for (int k = 0; k < 900; ++k) { const double x = k % 30 - 15 + 0.5 * (g.next() - 0.5), z = k / 30 - 15 + 0.5 * (g.next() - 0.5); push(cr, 3000 + x, 0.2, -2000 + z, 0.2); }
    return cr;
}
// sparse_wide: the ground and 1 000 spheres of r = 0.2 over 4000 x 4000.
static std::vector<double> sparse_wide(uint64_t seed) {
    std::vector<double> cr;
    push(cr, 0, -1000, 0, 1000);
    Lcg g{seed};
    for (int k = 0; k < 1000; ++k) { const double x = 4000 * g.next() - 2000, z = 4000 * g.next() - 2000; push(cr, x, 0.2, z, 0.2); }
    return cr;
}

// The recentring point the library uses: the centroid of the finite spheres with r < 100, rounded to fp32.
static void centre(const std::vector<double>& cr, double* ctr) {
    const size_t m = cr.size() / 4;
    double s[3] = {0, 0, 0};
    size_t cnt = 0;
    for (size_t i = 0; i < m; ++i)
        if (cr[4 * i + 3] < 100.0 && std::isfinite(cr[4 * i]) && std::isfinite(cr[4 * i + 1]) && std::isfinite(cr[4 * i + 2])) { for (int k = 0; k < 3; ++k) s[k] += cr[4 * i + k]; ++cnt; }
    for (int k = 0; k < 3; ++k) ctr[k] = (double)(float)(cnt ? s[k] / (double)cnt : 0.0);
}

template <class T>
static void check_blob(const DeviceGridPlan& pl, int m, const std::vector<double>& cr) {
    const DeviceGridBlob b = build_device_grid_blob<T>(pl, m, cr);
    const size_t ncells = (size_t)pl.nx * pl.nz, nd = pl.direct.size();
    CHECK(b.cells_offset == 0);
    CHECK(b.indices_offset % 16 == 0 && b.aos_offset % 16 == 0 && b.direct_offset % 16 == 0 && b.direct_ids_offset % 16 == 0);
    CHECK(b.indices_offset >= b.cells_offset + ncells * 8);
    CHECK(b.indices_offset == device_grid_align16(ncells * 8));                      // where the kernel looks for the indices
    CHECK(b.aos_offset >= b.indices_offset + pl.indices.size() * 4);
    CHECK(b.direct_offset >= b.aos_offset + (size_t)(m + 1) * 4 * sizeof(T));
    CHECK(b.n_direct_padded % 4 == 0 && (size_t)b.n_direct_padded >= nd && (size_t)b.n_direct_padded < nd + 4);
    CHECK(b.direct_ids_offset >= b.direct_offset + (size_t)b.n_direct_padded * 4 * sizeof(T));
    CHECK(b.bytes.size() >= b.direct_ids_offset + (size_t)b.n_direct_padded * 4);
    CHECK(b.bytes.size() < 0x7fffffffull);                                            // GridParams::blob_bytes and the offsets are ints
    if (b.bytes.size() < b.direct_ids_offset + (size_t)b.n_direct_padded * 4) return;
    CHECK(std::memcmp(b.bytes.data() + b.cells_offset, pl.cells.data(), ncells * 8) == 0);
    CHECK(pl.indices.empty() || std::memcmp(b.bytes.data() + b.indices_offset, pl.indices.data(), pl.indices.size() * 4) == 0);
    T pad[4];
    std::memcpy(pad, b.bytes.data() + b.aos_offset + (size_t)m * 4 * sizeof(T), sizeof pad);
    CHECK(pad[3] < (T)-1e11);                                                          // the never-hit entry at index m
    for (int k = 0; k < b.n_direct_padded; ++k) {
        int32_t id;
        std::memcpy(&id, b.bytes.data() + b.direct_ids_offset + (size_t)k * 4, 4);
        CHECK((size_t)k < nd ? id == pl.direct[k] : id == m);
    }
    // a registered sphere's AoS entry is its {c, r^2} in T
    for (int i = 0; i < m; i += m / 7 + 1) {
        T e[4];
        std::memcpy(e, b.bytes.data() + b.aos_offset + (size_t)i * 4 * sizeof(T), sizeof e);
        const T r = (T)cr[4 * (size_t)i + 3];
        CHECK(e[0] == (T)cr[4 * (size_t)i] && e[1] == (T)cr[4 * (size_t)i + 1] && e[2] == (T)cr[4 * (size_t)i + 2] && e[3] == (T)(r * r));
    }
}

static DeviceGridPlan check_scene(const char* name, const std::vector<double>& cr, bool want_usable) {
    const int m = (int)(cr.size() / 4);
    double ctr[3];
    centre(cr, ctr);
    const DeviceGridPlan pl = plan_device_grid(m, cr, ctr);
    std::printf("%s: m %d usable %d nx %d nz %d cell %.4f registered %d direct %zu entries %zu longest %d rfar %.1f eps %.5f\n", name, m, (int)pl.usable, pl.nx, pl.nz,
                (double)pl.cellf, pl.registered, pl.direct.size(), pl.indices.size(), pl.longest, pl.rfar, pl.eps);
    CHECK(pl.usable == want_usable);
    if (!pl.usable) return pl;
    const size_t ncells = (size_t)pl.nx * pl.nz;
    CHECK((long long)pl.nx * pl.nz <= DEVICE_GRID_MAX_CELLS && pl.nx >= 1 && pl.nz >= 1);
    CHECK(pl.cells.size() == 2 * ncells);
    CHECK(pl.registered + (int)pl.direct.size() == m);
    // every {first, count} inside the index array; the lists tile it; ascending; every index < m (<= m: the pad entry is never listed)
    size_t expect_first = 0;
    int longest = 0;
    for (size_t c = 0; c < ncells; ++c) {
        const size_t first = pl.cells[2 * c], count = pl.cells[2 * c + 1];
        CHECK(first == expect_first);
        CHECK(first + count <= pl.indices.size());
        if (first + count > pl.indices.size()) return pl;
        for (size_t k = 0; k < count; ++k) {
            CHECK(pl.indices[first + k] < (uint32_t)m);
            if (k) CHECK(pl.indices[first + k - 1] < pl.indices[first + k]);
        }
        expect_first = first + count;
        longest = std::max(longest, (int)count);
    }
    CHECK(expect_first == pl.indices.size());
    CHECK(longest == pl.longest);
    // the cell is wide enough for 2 x 2 and every sphere is on the direct list or in every cell its inflated square touches
    std::vector<char> is_direct(m, 0);
    for (int i : pl.direct) { CHECK(i >= 0 && i < m); if (i >= 0 && i < m) is_direct[i] = 1; }
    for (size_t k = 1; k < pl.direct.size(); ++k) CHECK(pl.direct[k - 1] < pl.direct[k]);
    double wmax = 0;
    for (int i = 0; i < m; ++i) wmax = std::max(wmax, pl.halfwidth[i]);
    CHECK((double)pl.cellf >= 2.0 * (wmax + pl.eps) * 1.0199);
    for (int i = 0; i < m; ++i) {
        if (is_direct[i]) { CHECK(pl.halfwidth[i] == 0.0); continue; }
        const double w = pl.halfwidth[i], r = cr[4 * (size_t)i + 3];
        CHECK(w >= r + pl.eps);                                                        // sqrt(r^2 + E) + eps
        const double reach = w + pl.eps;
        const long long ix0 = (long long)std::floor((cr[4 * (size_t)i] - reach - (double)pl.x0f) / (double)pl.cellf), ix1 = (long long)std::floor((cr[4 * (size_t)i] + reach - (double)pl.x0f) / (double)pl.cellf);
        const long long iz0 = (long long)std::floor((cr[4 * (size_t)i + 2] - reach - (double)pl.z0f) / (double)pl.cellf), iz1 = (long long)std::floor((cr[4 * (size_t)i + 2] + reach - (double)pl.z0f) / (double)pl.cellf);
        CHECK(ix0 >= 0 && iz0 >= 0 && ix1 < pl.nx && iz1 < pl.nz && ix1 - ix0 <= 1 && iz1 - iz0 <= 1);
        if (!(ix0 >= 0 && iz0 >= 0 && ix1 < pl.nx && iz1 < pl.nz)) continue;
        for (long long iz = iz0; iz <= iz1; ++iz)
            for (long long ix = ix0; ix <= ix1; ++ix) {
                const size_t c = (size_t)iz * pl.nx + (size_t)ix;
                const uint32_t* b = pl.indices.data() + pl.cells[2 * c];
                CHECK(std::binary_search(b, b + pl.cells[2 * c + 1], (uint32_t)i));
            }
        CHECK(cr[4 * (size_t)i + 1] - w >= pl.ylo && cr[4 * (size_t)i + 1] + w <= pl.yhi);
    }
    check_blob<float>(pl, m, cr);
    check_blob<double>(pl, m, cr);
    return pl;
}

int main() {
    for (int n : {6000, 20000}) {
        const DeviceGridPlan pl = check_scene("lattice", lattice(n, 7u + (unsigned)n), true);
        CHECK(pl.registered >= (int)(0.9 * n) && pl.direct.size() <= 8);              // what tests/test_render_large.py asserts of large_grid()
        CHECK(pl.indices.size() <= 4 * (size_t)pl.registered);
    }
    {
        const DeviceGridPlan pl = check_scene("line", line(2000), true);
        CHECK(pl.nx + pl.nz > 128);                                                   // longer than any walk of the LDS grid
    }
    {   // the five kinds of tests/large_scene.py's edge scenes, each with the property it exists for
        DeviceGridPlan pl = check_scene("clusters", clusters(21), true);
        int long_lists = 0, odd = 0, even = 0;
        for (size_t c = 0; c < (size_t)pl.nx * pl.nz; ++c)
            if (pl.cells[2 * c + 1] >= 7) { ++long_lists; (pl.cells[2 * c + 1] % 2 ? odd : even)++; }
        CHECK(pl.longest >= 24 && long_lists >= 20 && odd > 0 && even > 0 && pl.direct.size() == 1);
        pl = check_scene("equal_no_ground", equal_no_ground(22), true);
        CHECK(pl.direct.empty() && pl.registered == 900 && pl.yhi - pl.ylo > 3.3);
        CHECK(build_device_grid_blob<float>(pl, 900, equal_no_ground(22)).n_direct_padded == 0);     // an LDS table of size 0
        pl = check_scene("mixed_with_bad", mixed_with_bad(23), true);
        CHECK(pl.direct.size() % 4 != 0 && pl.direct.size() >= 5);
        for (int bad : {105, 305, 505, 705}) CHECK(std::find(pl.direct.begin(), pl.direct.end(), bad) != pl.direct.end());
        pl = check_scene("far_centre", far_centre(24), true);
        CHECK(pl.eps >= 0.04);
        pl = check_scene("sparse_wide", sparse_wide(25), true);
        CHECK(pl.cellf > 100 && pl.yhi - pl.ylo > 20);
    }
    {   // The reachable size of the grid.  With Cmax' = 1.0001 Cmax and Rfar >= 4 Cmax', the half-width of any registered sphere is
        //   w >= sqrt(E) >= sqrt(18 * 2^-24 * 1.01) (Rfar + Cmax') >= 1.04e-3 * 5 Cmax' = 5.2e-3 Cmax',
        // so cell >= 2 (wmax + eps) 1.02 > 2.04 w > 0.0106 Cmax', while the extent of an axis is at most 2 Cmax + 2 wmax: nx and nz are
        // each at most about 2 / 0.0106 + 3 = 191, the grid at most about 36 000 cells, whatever the scene.  DEVICE_GRID_MAX_CELLS
        // (2^20) is never reached and the loop that widens the cells under it never runs; beyond that many cells' worth of spheres
        // it is the lists that grow.
        DeviceGridPlan pl = check_scene("lattice 100000", lattice(100000, 3), true);
        CHECK(pl.nx <= 192 && pl.nz <= 192);
        pl = check_scene("line 200000", line(200000, 0.02, 0.05), true);
        CHECK(pl.nx <= 192 && pl.nz <= 192);
        CHECK(pl.longest > 2000);                                                     // check_blob above: a list of more than 2 000 entries
    }
    {
        const DeviceGridPlan pl = check_scene("lattice 70000", lattice(70000, 5), true);
        bool wide = false;
        for (uint32_t i : pl.indices) wide = wide || i > 0xffffu;
        CHECK(wide);                                                                  // indices that need more than 16 bits
    }
    {
        std::vector<double> cr;
        push(cr, 0, -1000, 0, 1000);
        for (int k = 0; k < 9; ++k) push(cr, k, 0.2, 0, 0.2);
        check_scene("ten spheres", cr, false);
    }
    {   // non-finite and non-positive radii go to the direct list, never into a cell
        std::vector<double> cr = lattice(400, 11);
        cr[4 * 50 + 3] = -1.0; cr[4 * 60] = INFINITY; cr[4 * 70 + 3] = NAN;
        const DeviceGridPlan pl = check_scene("lattice with bad spheres", cr, true);
        for (int bad : {50, 60, 70}) CHECK(std::find(pl.direct.begin(), pl.direct.end(), bad) != pl.direct.end());
    }
    std::printf("%d large-grid-plan failure(s)\n", failures);
    return failures ? 1 : 0;
}
