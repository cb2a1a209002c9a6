// The per-sphere tables and the edit list of a mapped scene edit (csrc/library/edit_list.h) on the CPU, with no
// GPU and no library.  stdin, as text:
//   line 1:  elem spheres snap_spheres        elem: 4 or 8 (bytes of T)
//   line 2:  from_snapshot, one int per sphere of the current scene
//   then per sphere of the current scene one line of 4 + 6 hexadecimal words: {C, r} and {type, albedo_fuzz x 4, refraction_index}, every
//   real as the bits of T, the type as an int32; then the same per sphere of the snapshot;
//   then any number of compositions: "compose n current_slots", valid x n, origin x n, current_kept x current_slots, from_snapshot x kept.
// stdout: "flags f0 f1 ...", one line "snap w0 w1 w2 w3" per sphere (the motion plane's table), one line per entry "owner w0 w1 w2 w3",
// "entries N", and one line "map ..." per composition.  A "RULE BROKEN" line where the functions without a map are not the identity case.
// Built by tests/test_scene_mapped_abi.py with ASan + UBSan and run directly.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "edit_list.h"

namespace {

bool word(uint64_t& out) {
    char buf[32];
    if (std::scanf("%31s", buf) != 1) return false;
    out = std::strtoull(buf, nullptr, 16);
    return true;
}
void put(std::vector<unsigned char>& to, uint64_t w, size_t bytes) {
    unsigned char b[8];
    std::memcpy(b, &w, 8);                                       // little endian, as the tables are on the host
    to.insert(to.end(), b, b + bytes);
}
bool ints(std::vector<int32_t>& to, size_t count) {
    to.resize(count);
    for (int32_t& v : to) if (std::scanf("%" SCNd32, &v) != 1) return false;
    return true;
}
void print_words(const unsigned char* from, size_t elem) {
    for (int i = 0; i < 4; ++i) {
        uint64_t w = 0;
        std::memcpy(&w, from + i * elem, elem);
        std::printf(" %" PRIx64, w);
    }
    std::printf("\n");
}

}  // namespace

int main() {
    size_t elem = 0, spheres = 0, snap_spheres = 0;
    if (std::scanf("%zu %zu %zu", &elem, &spheres, &snap_spheres) != 3 || (elem != 4 && elem != 8)) { std::fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int32_t> from;
    if (!ints(from, spheres)) return 2;
    for (int32_t j : from) if (j < -1 || j >= (int32_t)snap_spheres) { std::fprintf(stderr, "bad map\n"); return 2; }
    std::vector<unsigned char> geom, mat, snap_geom, snap_mat;
    for (int side = 0; side < 2; ++side)
        for (size_t k = 0; k < (side ? snap_spheres : spheres); ++k) {
            std::vector<unsigned char>& g = side ? snap_geom : geom;
            std::vector<unsigned char>& m = side ? snap_mat : mat;
            uint64_t w = 0;
            for (int i = 0; i < 4; ++i) { if (!word(w)) return 2; put(g, w, elem); }
            if (!word(w)) return 2;
            put(m, w, sizeof(int32_t));
            for (int i = 0; i < 5; ++i) { if (!word(w)) return 2; put(m, w, elem); }
        }
    const size_t gs = 4 * elem, ms = sizeof(int32_t) + 5 * elem;
    const std::vector<int32_t> flags = edit_flags_mapped(geom.data(), snap_geom.data(), gs, mat.data(), snap_mat.data(), ms, spheres, from.data());
    const std::vector<unsigned char> table = motion_snap_table(snap_geom.data(), gs, spheres, from.data());
    const EditList list = build_edit_list_mapped(geom.data(), snap_geom.data(), gs, flags, from.data(), snap_spheres);
    int failures = 0;
    bool identity = spheres == snap_spheres;
    for (size_t k = 0; identity && k < spheres; ++k) identity = from[k] == (int32_t)k;
    if (identity) {                                              // the functions without a map are this case
        const std::vector<int32_t> plain = edit_flags(geom.data(), snap_geom.data(), gs, mat.data(), snap_mat.data(), ms, spheres);
        const EditList plain_list = build_edit_list(geom.data(), snap_geom.data(), gs, plain);
        if (plain != flags || plain_list.geom != list.geom || plain_list.owner != list.owner || table != snap_geom) { ++failures; std::printf("RULE BROKEN: the identity map is not the plain edit\n"); }
    }
    if (list.geom.size() != list.entries() * gs || table.size() != spheres * gs) { ++failures; std::printf("RULE BROKEN: %zu bytes for %zu entries\n", list.geom.size(), list.entries()); }
    std::printf("flags");
    for (int32_t f : flags) std::printf(" %d", f);
    std::printf("\n");
    for (size_t k = 0; k < spheres; ++k) { std::printf("snap"); print_words(table.data() + k * gs, elem); }
    for (size_t e = 0; e < list.entries() && list.geom.size() == list.entries() * gs; ++e) { std::printf("%d", list.owner[e]); print_words(list.geom.data() + e * gs, elem); }
    std::printf("entries %zu\n", list.entries());
    char name[16];
    while (std::scanf("%15s", name) == 1) {
        int n = 0, current_slots = 0;
        if (std::string(name) != "compose" || std::scanf("%d %d", &n, &current_slots) != 2 || n <= 0 || current_slots <= 0) return 2;
        std::vector<int32_t> valid, origin, kept_in, map_in;
        if (!ints(valid, (size_t)n) || !ints(origin, (size_t)n) || !ints(kept_in, (size_t)current_slots)) return 2;
        std::vector<unsigned char> kept(kept_in.begin(), kept_in.end());
        size_t kept_count = 0;
        for (unsigned char c : kept) kept_count += c != 0;
        if (!ints(map_in, kept_count)) return 2;
        const std::vector<int32_t> out = compose_origin(n, valid.data(), origin.data(), kept.data(), current_slots, map_in.data());
        std::printf("map");
        for (int32_t v : out) std::printf(" %d", v);
        std::printf("\n");
    }
    return failures ? 1 : 0;
}
