// Stand-alone check of the volume grid's plan and blob (raytracingincuda_amd/csrc/library/volume_grid.h), built with
// -fsanitize=address,undefined by tests/test_volume_grid_plan.py and run directly.  The invariants held here are what keeps the kernel's
// gathers inside the blob: every record inside the cell table, every {first, count} inside the index array, every index < m, lists
// ascending, every finite sphere on the direct list or in every cell its inflated cube touches, offsets and sizes of the blob consistent
// in both precisions -- on cubes of 18^3 and 46^3 spheres, the column, a cube with spheres the plan cannot grid, a scene the plan
// refuses and a cap on the cell count small enough for the loop that widens the cells to run.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "volume_grid.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Lcg {
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
};

static void push(std::vector<double>& cr, double x, double y, double z, double r) { cr.insert(cr.end(), {x, y, z, r}); }

// The ground and side^3 spheres (r = 0.2, pitch 1, jitter +-0.3) above it, y from 0.5 up: the shape of tests/volume_scene.py's cube.
static std::vector<double> cube(int side, uint64_t seed, bool ground = true) {
    std::vector<double> cr;
    if (ground) push(cr, 0, -1000, 0, 1000);
    Lcg g{seed};
    for (int iy = 0; iy < side; ++iy)
        for (int iz = 0; iz < side; ++iz)
            for (int ix = 0; ix < side; ++ix)
                push(cr, ix - 0.5 * (side - 1) + 0.6 * (g.next() - 0.5), iy + 0.5 + 0.6 * (g.next() - 0.5), iz - 0.5 * (side - 1) + 0.6 * (g.next() - 0.5), 0.2);
    return cr;
}
// 2 000 spheres stacked along y at pitch 0.5.
static std::vector<double> column(uint64_t seed) {
    std::vector<double> cr;
    Lcg g{seed};
    for (int k = 0; k < 2000; ++k) push(cr, 0.1 * (g.next() - 0.5), 0.5 * k, 0.1 * (g.next() - 0.5), 0.2);
    return cr;
}
// cube(14) plus r < 0, r = NaN, cx = inf, r = 0 and two unit spheres.
static std::vector<double> with_bad(uint64_t seed) {
    std::vector<double> cr = cube(14, seed);
    push(cr, -3, 16, 2, 1.0); push(cr, 4, 7.5, -9.5, 1.0);
    cr[4 * 105 + 3] = -0.3; cr[4 * 305 + 3] = NAN; cr[4 * 505] = INFINITY; cr[4 * 705 + 3] = 0.0;
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
static void check_blob(const VolumeGridPlan& pl, int m, const std::vector<double>& cr) {
    const VolumeGridBlob b = build_volume_grid_blob<T>(pl, m, cr);
    const size_t ncells = (size_t)pl.nx * pl.ny * pl.nz, nd = pl.direct.size();
    CHECK(b.cells_offset == 0);
    CHECK(b.indices_offset % 16 == 0 && b.aos_offset % 16 == 0 && b.direct_offset % 16 == 0 && b.direct_ids_offset % 16 == 0);
    CHECK(b.indices_offset == device_grid_align16(ncells * 8));                      // where the kernel looks for the indices
    CHECK(ncells * 8 <= 0x7fffffffull);                                               // a record's byte offset in 32 bits
    CHECK(b.aos_offset >= b.indices_offset + pl.indices.size() * 4);
    CHECK(b.direct_offset >= b.aos_offset + (size_t)(m + 1) * 4 * sizeof(T));
    CHECK(b.n_direct_padded % 4 == 0 && (size_t)b.n_direct_padded >= nd && (size_t)b.n_direct_padded < nd + 4);
    CHECK(b.direct_ids_offset >= b.direct_offset + (size_t)b.n_direct_padded * 4 * sizeof(T));
    CHECK(b.bytes.size() >= b.direct_ids_offset + (size_t)b.n_direct_padded * 4 + 16);
    CHECK(b.bytes.size() < 0x7fffffffull);                                            // GridParams::blob_bytes and the offsets are ints
    if (b.bytes.size() < b.direct_ids_offset + (size_t)b.n_direct_padded * 4) return;
    CHECK(std::memcmp(b.bytes.data() + b.cells_offset, pl.cells.data(), ncells * 8) == 0);
    CHECK(pl.indices.empty() || std::memcmp(b.bytes.data() + b.indices_offset, pl.indices.data(), pl.indices.size() * 4) == 0);
    // every gather of the walk, from the blob's own bytes: record -> slice of the index array -> sphere entry, all inside the blob
    for (size_t c = 0; c < ncells; ++c) {
        uint32_t rec[2];
        std::memcpy(rec, b.bytes.data() + b.cells_offset + c * 8, 8);
        const size_t list_end = b.indices_offset + ((size_t)rec[0] + rec[1]) * 4;
        CHECK(list_end <= b.aos_offset);
        if (list_end > b.aos_offset) return;
        for (uint32_t k = 0; k < rec[1]; ++k) {
            uint32_t i;
            std::memcpy(&i, b.bytes.data() + b.indices_offset + ((size_t)rec[0] + k) * 4, 4);
            CHECK(b.aos_offset + ((size_t)i + 1) * 4 * sizeof(T) <= b.direct_offset);
        }
    }
    T pad[4];
    std::memcpy(pad, b.bytes.data() + b.aos_offset + (size_t)m * 4 * sizeof(T), sizeof pad);
    CHECK(pad[3] < (T)-1e11);                                                          // the never-hit entry at index m
    for (int k = 0; k < b.n_direct_padded; ++k) {
        int32_t id;
        std::memcpy(&id, b.bytes.data() + b.direct_ids_offset + (size_t)k * 4, 4);
        CHECK((size_t)k < nd ? id == pl.direct[k] : id == m);
    }
    for (int i = 0; i < m; i += m / 7 + 1) {
        T e[4];
        std::memcpy(e, b.bytes.data() + b.aos_offset + (size_t)i * 4 * sizeof(T), sizeof e);
        const T r = (T)cr[4 * (size_t)i + 3];
        const bool same = (e[0] == (T)cr[4 * (size_t)i] || cr[4 * (size_t)i] != cr[4 * (size_t)i]) && e[1] == (T)cr[4 * (size_t)i + 1] && e[2] == (T)cr[4 * (size_t)i + 2];
        CHECK(same && (e[3] == (T)(r * r) || r != r));
    }
}

static VolumeGridPlan check_scene(const char* name, const std::vector<double>& cr, bool want_usable, long long max_cells = VOLUME_GRID_MAX_CELLS) {
    const int m = (int)(cr.size() / 4);
    double ctr[3];
    centre(cr, ctr);
    const VolumeGridPlan pl = plan_volume_grid(m, cr, ctr, max_cells);
    std::printf("%s: m %d usable %d grid %d x %d x %d cell %.4f registered %d direct %zu entries %zu occupied %zu longest %d rfar %.1f eps %.5f\n", name, m, (int)pl.usable,
                pl.nx, pl.ny, pl.nz, (double)pl.cellf, pl.registered, pl.direct.size(), pl.indices.size(), pl.occupied, pl.longest, pl.rfar, pl.eps);
    CHECK(pl.usable == want_usable);
    if (!pl.usable) return pl;
    const size_t ncells = (size_t)pl.nx * pl.ny * pl.nz;
    CHECK((long long)ncells <= max_cells && pl.nx >= 1 && pl.ny >= 1 && pl.nz >= 1);
    CHECK(pl.cells.size() == 2 * ncells);
    CHECK(pl.registered + (int)pl.direct.size() == m);
    // every {first, count} inside the index array; the lists tile it; ascending; every index < m (the pad entry is never listed)
    size_t expect_first = 0, occupied = 0;
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
        occupied += count ? 1 : 0;
    }
    CHECK(expect_first == pl.indices.size());
    CHECK(longest == pl.longest && occupied == pl.occupied);
    CHECK(pl.indices.size() <= 8 * (size_t)pl.registered);
    // the cell is wide enough for 2 x 2 x 2 and every sphere is on the direct list or in every cell its inflated cube touches
    std::vector<char> is_direct(m, 0);
    for (int i : pl.direct) { CHECK(i >= 0 && i < m); if (i >= 0 && i < m) is_direct[i] = 1; }
    for (size_t k = 1; k < pl.direct.size(); ++k) CHECK(pl.direct[k - 1] < pl.direct[k]);
    double wmax = 0;
    for (int i = 0; i < m; ++i) wmax = std::max(wmax, pl.halfwidth[i]);
    CHECK((double)pl.cellf >= 2.0 * (wmax + pl.eps) * 1.0199);
    const float origin[3] = {pl.x0f, pl.y0f, pl.z0f};
    const int dims[3] = {pl.nx, pl.ny, pl.nz};
    for (int i = 0; i < m; ++i) {
        if (is_direct[i]) { CHECK(pl.halfwidth[i] == 0.0); continue; }
        const double w = pl.halfwidth[i], r = cr[4 * (size_t)i + 3];
        CHECK(w >= r + pl.eps);                                                        // sqrt(r^2 + E) + eps
        const double reach = w + pl.eps;
        long long a[3], b[3];
        bool inside = true;
        for (int k = 0; k < 3; ++k) {
            a[k] = (long long)std::floor((cr[4 * (size_t)i + k] - reach - (double)origin[k]) / (double)pl.cellf);
            b[k] = (long long)std::floor((cr[4 * (size_t)i + k] + reach - (double)origin[k]) / (double)pl.cellf);
            inside = inside && a[k] >= 0 && b[k] < dims[k] && b[k] - a[k] <= 1;
        }
        CHECK(inside);
        if (!inside) continue;
        for (long long iy = a[1]; iy <= b[1]; ++iy)
            for (long long iz = a[2]; iz <= b[2]; ++iz)
                for (long long ix = a[0]; ix <= b[0]; ++ix) {
                    const size_t c = ((size_t)iy * pl.nz + (size_t)iz) * pl.nx + (size_t)ix;
                    const uint32_t* s = pl.indices.data() + pl.cells[2 * c];
                    CHECK(std::binary_search(s, s + pl.cells[2 * c + 1], (uint32_t)i));
                }
    }
    check_blob<float>(pl, m, cr);
    check_blob<double>(pl, m, cr);
    return pl;
}

int main() {
    {
        const VolumeGridPlan pl = check_scene("cube 18", cube(18, 7), true);
        CHECK(pl.registered == 18 * 18 * 18 && pl.direct.size() == 1);
        CHECK((double)pl.indices.size() / (double)pl.occupied <= 6.0);
    }
    {
        const VolumeGridPlan pl = check_scene("cube 46", cube(46, 9), true);
        CHECK(pl.registered == 46 * 46 * 46 && pl.direct.size() == 1);
        bool wide = false;
        for (uint32_t i : pl.indices) wide = wide || i > 0xffffu;
        CHECK(wide);                                                                  // indices that need more than 16 bits
    }
    {
        const VolumeGridPlan pl = check_scene("column", column(11), true);
        CHECK(pl.ny > 128 && pl.direct.empty());
        CHECK(build_volume_grid_blob<float>(pl, 2000, column(11)).n_direct_padded == 0);     // an LDS table of size 0
    }
    {
        const VolumeGridPlan pl = check_scene("with bad", with_bad(13), true);
        CHECK(pl.direct.size() == 7);
        for (int bad : {0, 105, 305, 505, 705, 2745, 2746}) CHECK(std::find(pl.direct.begin(), pl.direct.end(), bad) != pl.direct.end());
    }
    {
        std::vector<double> cr;
        push(cr, 0, -1000, 0, 1000);
        for (int k = 0; k < 9; ++k) push(cr, k, 0.2, 0, 0.2);
        check_scene("ten spheres", cr, false);
    }
    {   // a cap the natural cell does not meet: the loop that widens the cells runs, and every invariant still holds
        const VolumeGridPlan wide = check_scene("cube 27", cube(27, 15), true);
        const VolumeGridPlan capped = check_scene("cube 27, at most 4096 cells", cube(27, 15), true, 4096);
        CHECK((long long)wide.nx * wide.ny * wide.nz > 4096);
        CHECK((long long)capped.nx * capped.ny * capped.nz <= 4096 && capped.cellf > wide.cellf && capped.registered == wide.registered);
    }
    std::printf("%d volume-grid-plan failure(s)\n", failures);
    return failures ? 1 : 0;
}
