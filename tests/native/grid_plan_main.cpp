// Stand-alone check of the LDS grid's plan and blob (raytracingincuda_amd/csrc/library/grid_plan.h), built with
// -fsanitize=address,undefined by tests/test_grid_plan_digests.py and run directly.  plan_grid writes 16-bit indices into a [nz][nx][4]
// table at computed cell coordinates, and hit_world_grid reads the blob at the offsets recorded here: the invariants held are that
// every sphere is on the direct list or in every cell its inflated square touches and never both, that cells fill from slot 0 and pad
// with m, that the sections tile the blob at multiples of 16, and that the tables hold the spheres upload_scene's way.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "grid_plan.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Lcg {
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
};

static void push(std::vector<double>& cr, double x, double y, double z, double r) { cr.insert(cr.end(), {x, y, z, r}); }

// A jittered lattice of n spheres (r = 0.2, pitch 1) on the ground around (ox, oz), with the ground and three unit spheres in front.
static std::vector<double> lattice(int n, uint64_t seed, double ox = 0, double oz = 0) {
    std::vector<double> cr;
    push(cr, ox, -1000, oz, 1000);
    push(cr, ox, 1, oz, 1.0); push(cr, ox - 4, 1, oz, 1.0); push(cr, ox + 4, 1, oz, 1.0);
    Lcg g{seed};
    int side = 1;
    while (side * side < n) ++side;
    for (int k = 0; k < n; ++k) push(cr, ox + k % side - 0.5 * side + 0.5 * (g.next() - 0.5), 0.2, oz + k / side - 0.5 * side + 0.5 * (g.next() - 0.5), 0.2);
    return cr;
}

// The recentring point build_screen_table uses: no finiteness test, rounded to fp32.
static void centre(const std::vector<double>& cr, double* ctr) {
    recentring_point((int)(cr.size() / 4), cr, false, ctr);
    for (int k = 0; k < 3; ++k) ctr[k] = (double)(float)ctr[k];
}

template <class T>
static bool same(T a, T b) { return a == b || (a != a && b != b); }

// The inverse of pair_interleave.
template <class T>
static std::vector<T> deinterleaved(const std::vector<T>& t) {
    std::vector<T> out(t.size());
    for (size_t q = 0; q < t.size() / 8; ++q)
        for (int k = 0; k < 4; ++k) { out[8 * q + k] = t[8 * q + 2 * k]; out[8 * q + 4 + k] = t[8 * q + 2 * k + 1]; }
    return out;
}

template <class T>
static void check_interleave() {
    for (size_t entries : {0u, 4u, 10u}) {
        std::vector<T> v(4 * entries);
        for (size_t k = 0; k < v.size(); ++k) v[k] = (T)(k + 1);
        std::vector<T> w = v;
        pair_interleave(w);
        CHECK(w.size() == v.size() && deinterleaved(w) == v);
        if (entries == 4) {
            const std::vector<T> expect = {1, 5, 2, 6, 3, 7, 4, 8, 9, 13, 10, 14, 11, 15, 12, 16};
            CHECK(w == expect);
        }
        pair_interleave(w); pair_interleave(w);
        w = deinterleaved(deinterleaved(deinterleaved(w)));
        CHECK(w == v);
    }
}

template <class T>
static std::vector<T> section(const GridBlob& b, size_t at, size_t count) {
    std::vector<T> out(count);
    if (count && at + count * sizeof(T) <= b.bytes.size()) std::memcpy(out.data(), b.bytes.data() + at, count * sizeof(T));
    return out;
}

template <class T>
static void check_blob(const GridPlan& pl, int m, const std::vector<double>& cr) {
    const GridBlob b = build_grid_blob<T>(pl, m, cr);
    const size_t nd = pl.direct.size(), ndp = (nd + 3) / 4 * 4, aos_entries = sizeof(T) == 4 ? (size_t)m + 1 : 0;
    // every offset a multiple of 16, the sections tile the blob exactly
    CHECK(b.cells_offset == 0 && b.aos_offset % 16 == 0 && b.direct_offset % 16 == 0 && b.direct_ids_offset % 16 == 0 && b.bytes.size() % 16 == 0);
    CHECK(b.aos_offset == device_grid_align16(pl.cells.size() * 2));
    CHECK(b.direct_offset == b.aos_offset + device_grid_align16(aos_entries * 4 * sizeof(T)));
    CHECK((size_t)b.n_direct_padded == ndp);
    CHECK(b.direct_ids_offset == b.direct_offset + device_grid_align16(ndp * 4 * sizeof(T)));
    CHECK(b.bytes.size() == b.direct_ids_offset + device_grid_align16(ndp * 4));
    if (b.bytes.size() != b.direct_ids_offset + device_grid_align16(ndp * 4)) return;
    CHECK(section<uint16_t>(b, b.cells_offset, pl.cells.size()) == pl.cells);
    auto entry_is = [&](const std::vector<T>& t, size_t k, int i) {                     // entry k of a table against sphere i, or the never-hit entry (i == m)
        if (i == m) return t[4 * k] == (T)0 && t[4 * k + 1] == (T)0 && t[4 * k + 2] == (T)0 && t[4 * k + 3] == (T)-1e12;
        const double* s = &cr[4 * (size_t)i];
        const T r = (T)s[3];
        return same(t[4 * k], (T)s[0]) && same(t[4 * k + 1], (T)s[1]) && same(t[4 * k + 2], (T)s[2]) && same(t[4 * k + 3], (T)(r * r));
    };
    // the direct table, de-interleaved, and its ids: the listed spheres, then never-hit pads with id m
    std::vector<T> table = section<T>(b, b.direct_offset, ndp * 4);
    if (sizeof(T) == 4) table = deinterleaved(table);
    const std::vector<int32_t> ids = section<int32_t>(b, b.direct_ids_offset, ndp);
    for (size_t k = 0; k < ndp; ++k) {
        const int want = k < nd ? pl.direct[k] : m;
        CHECK(ids[k] == want);
        CHECK(entry_is(table, k, want));
    }
    // fp32 carries the AoS table, entry m never hits; fp64 gathers from geom_a and carries none
    const std::vector<T> aos = section<T>(b, b.aos_offset, aos_entries * 4);
    for (size_t i = 0; i < aos_entries; ++i) CHECK(entry_is(aos, i, (int)i));
    if (sizeof(T) == 8) CHECK(b.direct_offset == b.aos_offset);
}

// What fill_grid_params and place_grid_blob write: the fields of GridParams they touch.
struct Params {
    int use_grid = 0, nx = 0, nz = 0;
    float x0 = 0, z0 = 0, cell = 0, inv_cell = 0, ylo = 0, yhi = 0, far2 = 0, core_lo[3] = {0, 0, 0}, core_hi[3] = {0, 0, 0}, rmax2 = 0, cmax = 0;
    int n_direct_padded = 0, cells_offset = 0, aos_offset = 0, direct_offset = 0, direct_ids_offset = 0;
};

static GridPlan check_scene(const char* name, const std::vector<double>& cr, bool want_usable, bool want_plan, const double* centre_given = nullptr) {
    const int m = (int)(cr.size() / 4);
    double ctr[3];
    centre(cr, ctr);
    if (centre_given) std::memcpy(ctr, centre_given, sizeof ctr);
    const GridPlan pl = plan_grid(m, cr, ctr);
    std::printf("%s: m %d usable %d nx %d nz %d cell %.4f registered %d direct %zu rfar %.1f eps %.5f\n", name, m, (int)pl.usable, pl.nx, pl.nz, (double)pl.cellf,
                pl.registered, pl.direct.size(), pl.rfar, pl.eps);
    CHECK(pl.usable == want_usable);
    CHECK((pl.nx > 0) == want_plan);
    if (pl.nx <= 0) {                                                                  // no candidate was registered at all
        CHECK(!pl.usable && pl.nz == 0 && pl.cells.empty() && pl.direct.empty() && pl.registered == 0);
        return pl;
    }
    const int nx = pl.nx, nz = pl.nz;
    CHECK(nz > 0 && (long long)nx * nz <= 4096);
    CHECK(pl.cells.size() == (size_t)nx * nz * 4 && pl.halfwidth.size() == (size_t)m);
    if (pl.cells.size() != (size_t)nx * nz * 4 || pl.halfwidth.size() != (size_t)m) return pl;
    // cells: at most four spheres, filled from slot 0, padded with m; an empty cell is 0xffff x 4
    std::vector<char> in_cells(m, 0);
    for (size_t c = 0; c < (size_t)nx * nz; ++c) {
        const uint16_t* rec = &pl.cells[4 * c];
        int real = 0;
        while (real < 4 && rec[real] < m) ++real;
        if (real == 0) { CHECK(rec[0] == 0xffff && rec[1] == 0xffff && rec[2] == 0xffff && rec[3] == 0xffff); continue; }
        for (int k = 0; k < 4; ++k) {
            if (k >= real) { CHECK(rec[k] == m); continue; }
            in_cells[rec[k]] = 1;
            if (k) CHECK(rec[k - 1] < rec[k]);                                         // index order: no sphere twice
        }
    }
    // every sphere on the direct list or registered, never both
    std::vector<char> is_direct(m, 0);
    for (int i : pl.direct) { CHECK(i >= 0 && i < m); if (i >= 0 && i < m) is_direct[i] = 1; }
    for (size_t k = 1; k < pl.direct.size(); ++k) CHECK(pl.direct[k - 1] < pl.direct[k]);
    int registered = 0;
    double wmax = 0;
    for (int i = 0; i < m; ++i) {
        CHECK(is_direct[i] != in_cells[i]);
        registered += in_cells[i];
        CHECK((pl.halfwidth[i] > 0) == (in_cells[i] != 0));
        wmax = std::max(wmax, pl.halfwidth[i]);
    }
    CHECK(registered == pl.registered && pl.registered + (int)pl.direct.size() == m);
    CHECK((double)pl.cellf >= 2.0 * (wmax + pl.eps) * 1.0199);
    // a registered sphere is in EVERY cell its square touches, against the kernel's fp32 edges; the box and the slab hold it
    auto cell_of = [&](double v, float origin) { return (long long)std::floor((v - (double)origin) / (double)pl.cellf); };
    for (int i = 0; i < m; ++i) {
        if (!in_cells[i]) continue;
        const double* s = &cr[4 * (size_t)i];
        const double w = pl.halfwidth[i];
        CHECK(std::isfinite(s[0]) && std::isfinite(s[1]) && std::isfinite(s[2]) && std::isfinite(s[3]) && s[3] > 0);
        CHECK(w >= s[3] + pl.eps);                                                     // sqrt(r^2 + E) + eps
        const long long ix0 = cell_of(s[0] - w - pl.eps, pl.x0f), ix1 = cell_of(s[0] + w + pl.eps, pl.x0f);
        const long long iz0 = cell_of(s[2] - w - pl.eps, pl.z0f), iz1 = cell_of(s[2] + w + pl.eps, pl.z0f);
        CHECK(ix0 >= 0 && iz0 >= 0 && ix1 < nx && iz1 < nz && ix1 - ix0 <= 1 && iz1 - iz0 <= 1);
        if (!(ix0 >= 0 && iz0 >= 0 && ix1 < nx && iz1 < nz)) continue;
        for (long long iz = iz0; iz <= iz1; ++iz)
            for (long long ix = ix0; ix <= ix1; ++ix) {
                const uint16_t* rec = &pl.cells[4 * ((size_t)iz * nx + (size_t)ix)];
                CHECK(rec[0] == i || rec[1] == i || rec[2] == i || rec[3] == i);
            }
        CHECK(s[1] - w >= pl.ylo && s[1] + w <= pl.yhi);
        for (int k = 0; k < 3; ++k) CHECK(pl.core_lo[k] <= s[k] && s[k] <= pl.core_hi[k]);
        CHECK(s[3] <= pl.rmax_g);
    }
    // the kernel's parameters round outwards
    Params g;
    fill_grid_params(g, pl);
    CHECK(g.use_grid == 1 && g.nx == nx && g.nz == nz && g.cell == pl.cellf && g.x0 == pl.x0f && g.z0 == pl.z0f);
    CHECK((double)g.ylo < pl.ylo && (double)g.yhi > pl.yhi && (double)g.far2 < pl.rfar * pl.rfar && (double)g.rmax2 > pl.rmax_g * pl.rmax_g && (double)g.cmax > pl.cmax_g);
    for (int k = 0; k < 3; ++k) CHECK((double)g.core_lo[k] < pl.core_lo[k] && (double)g.core_hi[k] > pl.core_hi[k]);
    const GridBlob b = build_grid_blob<float>(pl, m, cr);
    place_grid_blob(g, b, 4096);
    CHECK(g.cells_offset == 4096 && g.aos_offset == 4096 + (int)b.aos_offset && g.direct_offset == 4096 + (int)b.direct_offset);
    CHECK(g.direct_ids_offset == 4096 + (int)b.direct_ids_offset && g.n_direct_padded == b.n_direct_padded);
    check_blob<float>(pl, m, cr);
    check_blob<double>(pl, m, cr);
    return pl;
}

int main() {
    check_interleave<float>();
    check_interleave<double>();
    {
        const GridPlan pl = check_scene("lattice 400", lattice(400, 3), true, true);
        CHECK(pl.direct.size() >= 4 && pl.direct[0] == 0 && pl.direct[1] == 1 && pl.direct[2] == 2 && pl.direct[3] == 3);     // the ground and the three unit spheres
    }
    {   // 60 000 spheres, the most plan_grid takes.  The cell's lower bound grows with the extent of the candidates (E with Cmax^2):
        // a square lattice of more than about 17 000 equal spheres has no plan at all.  So: the ground and 47 999 unit spheres
        // first, which the third candidate drops, then a lattice of 12 000 small ones -- the cells hold indices 48 000 .. 59 999, the
        // highest a cell can, and the pad m = 60000 is the 16-bit value closest to the empty mark 0xffff.  Four slots a cell under
        // nx nz <= 4096 cannot hold them all: the plan is made and is not usable.
        std::vector<double> cr;
        push(cr, 0, -1000, 0, 1000);
        for (int k = 0; k < 47999; ++k) push(cr, 2.0 * (k % 220) - 220, 1, 2.0 * (k / 220) - 220, 1.0);
        Lcg g{5};
        for (int k = 0; k < 12000; ++k) push(cr, k % 110 - 55 + 0.5 * (g.next() - 0.5), 0.2, k / 110 - 55 + 0.5 * (g.next() - 0.5), 0.2);
        const GridPlan pl = check_scene("lattice 12000 behind 48000 big spheres", cr, false, true);
        uint16_t highest = 0;
        for (uint16_t v : pl.cells) if (v < 60000) highest = std::max(highest, v);
        CHECK(highest > 59000);
        CHECK(std::find(pl.cells.begin(), pl.cells.end(), (uint16_t)60000) != pl.cells.end());
    }
    {   // eight knots of six spheres within 0.02 of a point: the fifth and sixth of each, at the least, meet a full cell and join the direct list
        std::vector<double> cr = lattice(400, 7);
        Lcg g{9};
        for (int k = 0; k < 8; ++k) {
            const double x = 16 * g.next() - 8, z = 16 * g.next() - 8;
            for (int j = 0; j < 6; ++j) push(cr, x + 0.02 * g.next(), 0.2, z + 0.02 * g.next(), 0.2);
        }
        const GridPlan pl = check_scene("lattice with knots", cr, true, true);
        int overflow = 0;
        for (int i : pl.direct) overflow += cr[4 * (size_t)i + 3] == 0.2;
        CHECK(overflow >= 16);
    }
    {   // non-finite and non-positive spheres go to the direct list, never into a cell
        std::vector<double> cr = lattice(400, 11);
        cr[4 * 50 + 3] = -1.0; cr[4 * 60] = INFINITY; cr[4 * 70 + 3] = NAN; cr[4 * 80 + 3] = 0.0; cr[4 * 90 + 3] = INFINITY; cr[4 * 100 + 1] = NAN;
        const double origin[3] = {0, 0, 0};                                            // the centroid over centres that are not finite is not a point
        const GridPlan pl = check_scene("lattice with bad spheres", cr, true, true, origin);
        for (int bad : {50, 60, 70, 80, 90, 100}) CHECK(std::find(pl.direct.begin(), pl.direct.end(), bad) != pl.direct.end());
    }
    {
        const GridPlan pl = check_scene("lattice far from the origin", lattice(900, 13, 3000, -2000), true, true);
        CHECK(pl.eps >= 0.04 && std::fabs((double)pl.x0f) > 2900 && std::fabs((double)pl.z0f) > 1900);
    }
    check_scene("23 spheres", lattice(19, 17), false, false);
    {
        const std::vector<double> cr = lattice(59997, 19);                             // 60 001 spheres
        const GridPlan pl = check_scene("lattice 59997", cr, false, false);
        check_blob<float>(pl, 60001, cr);                                              // never built by the library; an empty plan still has a well-formed blob
    }
    std::printf("%d grid-plan failure(s)\n", failures);
    return failures ? 1 : 0;
}
