// lds_placement.h -- where the pieces of a launch's dynamic LDS go, as pure functions of their sizes: what a launch over the device grid
// lays out (place_large_lds: the direct table and its ids from offset 0, the shade records while they fit, the drain scratch), and a
// kernel's own bytes behind the scene of whichever binding (place_own_lds: the upscalers' tally words and footprint).  large_launch.h
// and launch.h ask these and fill the parameters; nothing here touches the device.
// Plain C++ (no HIP): also built on its own by tests/native/lds_placement_main.cpp.
#pragma once
#include <cstddef>

constexpr size_t LDS_WORKGROUP_LIMIT = 160 * 1024;      // a compute unit's LDS, the most one workgroup may be given

// A kernel's own `own_lds` bytes behind the `scene_lds` bytes its scene binding laid out: 16-byte aligned.  fits: the whole is within a
// compute unit's LDS.
struct OwnLds {
    size_t offset, end;
    bool fits;
};
inline OwnLds place_own_lds(size_t scene_lds, size_t own_lds) {
    const size_t offset = (scene_lds + 15) / 16 * 16;
    return OwnLds{offset, offset + own_lds, offset + own_lds <= LDS_WORKGROUP_LIMIT};
}

// The LDS of a launch over the device grid, for n_direct_padded entries (a multiple of 4) of the direct list, elements of `elem` bytes
// (4 or 8), n spheres, workgroups of `threads` lanes and coop_bytes of drain scratch (0: a tile kernel, which has none): the direct
// table {cx, cy, cz, r^2} at offset 0 with its ids behind it (device/hit_device_grid.h: stage_device_grid), the shade records at
// shade_offset while they fit by layout_lds's rule (a workgroup's share within 1/5 of the LDS, a wave's under 6.5 KB), the drain scratch
// at coop_offset; lds bytes in all.  Every offset is a multiple of 16.
struct LargeLds {
    size_t direct_bytes, shade_offset, coop_offset, lds;
    bool shade_in_lds;
};
inline LargeLds place_large_lds(int n_direct_padded, size_t elem, int n, int threads, size_t coop_bytes) {
    LargeLds o{};
    o.direct_bytes = (size_t)n_direct_padded * 4 * elem + (size_t)n_direct_padded * sizeof(int);       // a multiple of 16
    size_t lds = o.direct_bytes;
    const size_t waves_in_block = (size_t)((threads + 63) / 64);
    const size_t shade_bytes = (elem * 12 * (size_t)n + 15) / 16 * 16;
    o.shade_offset = lds;
    o.shade_in_lds = lds + shade_bytes + coop_bytes <= 32 * 1024 && (lds + shade_bytes + coop_bytes) / waves_in_block <= 6656;
    if (o.shade_in_lds) lds += shade_bytes;
    o.coop_offset = lds;
    o.lds = lds + coop_bytes;
    return o;
}
