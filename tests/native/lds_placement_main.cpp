// The LDS of the upscalers over the device grid (csrc/library/lds_placement.h) on the CPU, with no GPU and no
// library: what a launch over the device grid lays out (place_large_lds) and the kernels' own bytes behind it (place_own_lds), for a
// direct list of zero, of nine (padded to twelve) and of the plan's maximum of 2 048 entries, in both precisions, with the shade records
// in LDS and not.  Every piece is written into a buffer of exactly the launch's size, byte by byte under its owner's name: a byte with two
// owners is an overlap (upscale_wide_kernel stages its footprint in front of stage_device_grid's barrier, so footprint, direct list,
// shade records and tally words are all written before the one barrier that publishes them), a byte outside the buffer is ASan's.
// stdout: one "RULE BROKEN" line per failure, the count last.  Built by tests/test_large_upscale_abi.py with ASan + UBSan, run directly.
#include <cstdio>
#include <string>
#include <vector>

#include "lds_placement.h"

namespace {

int failures = 0;
void expect(bool ok, const std::string& what) { if (!ok) { ++failures; std::printf("RULE BROKEN: %s\n", what.c_str()); } }

// device/upscale.h and device/upscale_wide.h: one word per wave of four; 144 staged pixels of three Vec4<T> and one int4
constexpr size_t TALLY_BYTES = 4 * sizeof(unsigned);
constexpr size_t wide_stage_bytes(size_t elem) { return 144 * (3 * 4 * elem + 16); }

struct Lds {
    std::vector<char> owner;
    std::string where;
    void claim(size_t from, size_t bytes, char who) {
        for (size_t k = from; k < from + bytes; ++k) {
            expect(owner[k] == 0, where + ": byte " + std::to_string(k) + " of '" + who + "' belongs to '" + owner[k] + "'");
            owner[k] = who;
        }
    }
};

void launch(int ndp, size_t elem, int n, bool wide) {
    const std::string where = std::to_string(ndp) + " direct, " + std::to_string(8 * elem) + " bit, " + std::to_string(n) + " spheres, " + (wide ? "wide" : "narrow");
    const LargeLds at = place_large_lds(ndp, elem, n, 256, 0);                    // the tile kernels' layout: no drain scratch
    const size_t shade_bytes = (elem * 12 * (size_t)n + 15) / 16 * 16;
    expect(at.direct_bytes == (size_t)ndp * (4 * elem + 4) && at.direct_bytes % 16 == 0, where + ": the direct table and its ids");
    expect(at.shade_offset == at.direct_bytes && at.shade_offset % 16 == 0, where + ": the shade records follow the ids");
    expect(at.coop_offset == at.lds && at.lds == at.direct_bytes + (at.shade_in_lds ? shade_bytes : 0), where + ": the size");
    expect(!at.shade_in_lds || at.lds <= 32 * 1024, where + ": shade records only within a fifth of the LDS");
    const size_t own_bytes = (wide ? wide_stage_bytes(elem) : 0) + TALLY_BYTES;
    const OwnLds own = place_own_lds(at.lds, own_bytes);
    expect(own.offset % 16 == 0 && own.offset >= at.lds && own.offset < at.lds + 16, where + ": 16-byte aligned, right behind the scene");
    expect(own.end == own.offset + own_bytes && own.fits && own.end <= LDS_WORKGROUP_LIMIT, where + ": within a compute unit's LDS");
    Lds lds{std::vector<char>(own.end, 0), where};
    const size_t stage_offset = own.offset, tally_offset = own.offset + (wide ? wide_stage_bytes(elem) : 0);     // launch_upscale(_wide)
    if (wide) lds.claim(stage_offset, wide_stage_bytes(elem), 'f');                // the footprint, staged first
    lds.claim(0, (size_t)ndp * 4 * elem, 'd');                                     // stage_device_grid: the table at offset 0 ...
    lds.claim((size_t)ndp * 4 * elem, (size_t)ndp * sizeof(int), 'i');             // ... its ids behind it
    if (at.shade_in_lds) lds.claim(at.shade_offset, elem * 12 * (size_t)n, 's');
    lds.claim(tally_offset, TALLY_BYTES, 't');                                     // upscale_count, behind the barrier
    expect(tally_offset % 4 == 0 && stage_offset % 16 == 0, where + ": alignment of the kernel's own pieces");
}

}  // namespace

int main() {
    for (const bool wide : {false, true})
        for (const size_t elem : {sizeof(float), sizeof(double)})
            for (const int ndp : {0, 12, 2048})
                for (const int n : {24, 100, 900, 6004, 20004}) launch(ndp, elem, n, wide);
    // the shade records do ride along on a small scene and do not on a large one
    expect(place_large_lds(12, 4, 100, 256, 0).shade_in_lds && !place_large_lds(12, 4, 6004, 256, 0).shade_in_lds, "shade records by size");
    expect(!place_large_lds(2048, 8, 24, 256, 0).shade_in_lds, "a long direct list leaves no room for shade records");
    // a persistent launch: the drain scratch last
    {
        const LargeLds at = place_large_lds(12, 8, 6004, 256, 4096);
        expect(at.coop_offset == at.direct_bytes && at.lds == at.coop_offset + 4096, "drain scratch behind the scene");
    }
    // own bytes that do not fit are said not to
    expect(place_own_lds(LDS_WORKGROUP_LIMIT - 16, 16).fits && !place_own_lds(LDS_WORKGROUP_LIMIT - 16, 17).fits, "the limit itself fits");
    expect(!place_own_lds(LDS_WORKGROUP_LIMIT - 8, 16).fits && place_own_lds(5, 16).offset == 16 && place_own_lds(0, 16).offset == 0, "alignment counts");
    std::printf("%d lds-placement failure(s)\n", failures);
    return failures ? 1 : 0;
}
