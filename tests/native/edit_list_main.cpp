// The edit list (csrc/library/edit_list.h) on the CPU, with no GPU and no library.  stdin: tables as text,
//   line 1:  elem spheres        elem: 4 or 8 (bytes of T)
//   then per sphere one line of 4 + 6 + 4 + 6 hexadecimal words: {C, r} and {type, albedo_fuzz x 4, refraction_index} of the current scene,
//   then the same of the snapshot; every real as the bits of T (8 or 16 hex digits), the type as an int32.
// stdout: "flags f0 f1 ...", then one line per entry "owner w0 w1 w2 w3" (the bits of {C, r}), then "entries N".
// Built by tests/test_edit_influence_abi.py with ASan + UBSan and run directly.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

}  // namespace

int main() {
    size_t elem = 0, spheres = 0;
    if (std::scanf("%zu %zu", &elem, &spheres) != 2 || (elem != 4 && elem != 8)) { std::fprintf(stderr, "bad header\n"); return 2; }
    std::vector<unsigned char> geom, mat, snap_geom, snap_mat;
    for (size_t k = 0; k < spheres; ++k)
        for (int side = 0; side < 2; ++side) {
            std::vector<unsigned char>& g = side ? snap_geom : geom;
            std::vector<unsigned char>& m = side ? snap_mat : mat;
            uint64_t w = 0;
            for (int i = 0; i < 4; ++i) { if (!word(w)) return 2; put(g, w, elem); }
            if (!word(w)) return 2;
            put(m, w, sizeof(int32_t));
            for (int i = 0; i < 5; ++i) { if (!word(w)) return 2; put(m, w, elem); }
        }
    const size_t gs = 4 * elem, ms = sizeof(int32_t) + 5 * elem;
    const std::vector<int32_t> flags = edit_flags(geom.data(), snap_geom.data(), gs, mat.data(), snap_mat.data(), ms, spheres);
    const EditList list = build_edit_list(geom.data(), snap_geom.data(), gs, flags);
    std::printf("flags");
    for (int32_t f : flags) std::printf(" %d", f);
    std::printf("\n");
    if (list.geom.size() != list.entries() * gs) { std::printf("RULE BROKEN: %zu bytes for %zu entries\n", list.geom.size(), list.entries()); return 1; }
    for (size_t e = 0; e < list.entries(); ++e) {
        std::printf("%d", list.owner[e]);
        for (int i = 0; i < 4; ++i) {
            uint64_t w = 0;
            std::memcpy(&w, list.geom.data() + e * gs + i * elem, elem);
            std::printf(" %" PRIx64, w);
        }
        std::printf("\n");
    }
    std::printf("entries %zu\n", list.entries());
    return 0;
}
