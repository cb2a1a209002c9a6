// edit_list.h -- the edit list of an rtiow_edit_scene: the spheres an edit touched, as the entries whose share of
// a pixel's surroundings bounds how much of its incoming light the edit can have changed (edit_influence_kernel, device/edit_influence.h).
// Built on the host from the comparison of the current tables with the snapshot that upload_motion_table (scene_tables.h) makes.
// Plain C++ (no HIP): also built on its own by tests/native/edit_list_main.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// Flags of a kept sphere k against the snapshot, bits against bits.  MOVED: any of the 4 T of {C_k, r_k} differs; CHANGED: the material
// record differs.  The values of MOTION_MOVED / MOTION_CHANGED (device/scene_motion.h); scene_tables.h asserts them equal.
constexpr int EDIT_MOVED = 1, EDIT_CHANGED = 2;
// Entries edit_influence_kernel stages in LDS at a time.  A list longer than one chunk is an ordinary case.
constexpr int EDIT_LIST_CHUNK = 32;

// The tables are the handle's: per kept sphere geom_bytes of {C, r} (4 T) and mat_bytes of the material record, as the bits of T.
inline std::vector<int32_t> edit_flags(const unsigned char* geom, const unsigned char* snap_geom, size_t geom_bytes, const unsigned char* mat,
                                       const unsigned char* snap_mat, size_t mat_bytes, size_t spheres) {
    std::vector<int32_t> flags(spheres, 0);
    for (size_t k = 0; k < spheres; ++k) {
        if (std::memcmp(geom + k * geom_bytes, snap_geom + k * geom_bytes, geom_bytes) != 0) flags[k] |= EDIT_MOVED;
        if (std::memcmp(mat + k * mat_bytes, snap_mat + k * mat_bytes, mat_bytes) != 0) flags[k] |= EDIT_CHANGED;
    }
    return flags;
}

// One entry: {C.xyz, r} as the bits of T (geom_bytes) and the kept sphere k it belongs to.  Through the kept spheres in ascending k:
//   MOVED, with or without CHANGED: two entries, {C'_k, r'_k} of the snapshot, then {C_k, r_k} of the current scene;
//   CHANGED only:                   one entry, {C_k, r_k};
//   neither:                        none.
// Old and new places are separate entries, which leaves room for spheres that exist on one side of an edit only.
struct EditList {
    std::vector<unsigned char> geom;
    std::vector<int32_t> owner;
    size_t entries() const { return owner.size(); }
};

inline EditList build_edit_list(const unsigned char* geom, const unsigned char* snap_geom, size_t geom_bytes, const std::vector<int32_t>& flags) {
    EditList list;
    auto entry = [&](const unsigned char* from, size_t k) {
        list.geom.insert(list.geom.end(), from + k * geom_bytes, from + (k + 1) * geom_bytes);
        list.owner.push_back((int32_t)k);
    };
    for (size_t k = 0; k < flags.size(); ++k) {
        if (flags[k] & EDIT_MOVED) { entry(snap_geom, k); entry(geom, k); }
        else if (flags[k] & EDIT_CHANGED) entry(geom, k);
    }
    return list;
}
