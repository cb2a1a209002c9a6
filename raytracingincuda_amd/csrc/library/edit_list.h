// edit_list.h -- the edit list of an rtiow_edit_scene: the spheres an edit touched, as the entries whose share of
// a pixel's surroundings bounds how much of its incoming light the edit can have changed (edit_influence_kernel, device/edit_influence.h).
// Built on the host from the comparison of the current tables with the snapshot that upload_motion_table (scene_tables.h) makes.
// With rtiow_edit_scene_mapped the current scene and the snapshot may differ in shape: the map from_snapshot
// says which sphere of the snapshot each kept sphere of the current scene continues.  The arithmetic is stated once, for a map; the
// functions without one are its identity case.
// Plain C++ (no HIP): also built on its own by tests/native/edit_list_main.cpp and tests/native/scene_mapped_list_main.cpp.
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
// from_snapshot[k] of a sphere the snapshot does not hold (an added sphere), and the owner of an entry that belongs to no sphere of the
// current scene (a removed sphere's): a hit pixel's id is >= 0 and a miss is never lit, so no pixel skips such an entry as its own.
constexpr int32_t EDIT_NO_ORIGIN = -1, EDIT_OWNER_REMOVED = -2;

// The sphere of the snapshot that kept sphere k continues: from_snapshot[k], or k itself without a map (the identity).
inline int32_t edit_origin(const int32_t* from_snapshot, size_t k) { return from_snapshot ? from_snapshot[k] : (int32_t)k; }

// The tables are the handle's: per kept sphere geom_bytes of {C, r} (4 T) and mat_bytes of the material record, as the bits of T.
// Per kept sphere k of the current scene, with j = from_snapshot[k]: j >= 0: the current record of k against snapshot record j;
// j == -1 (added): CHANGED alone, which carries nothing and reads no snapshot record.
inline std::vector<int32_t> edit_flags_mapped(const unsigned char* geom, const unsigned char* snap_geom, size_t geom_bytes, const unsigned char* mat,
                                              const unsigned char* snap_mat, size_t mat_bytes, size_t spheres, const int32_t* from_snapshot) {
    std::vector<int32_t> flags(spheres, 0);
    for (size_t k = 0; k < spheres; ++k) {
        const int32_t j = edit_origin(from_snapshot, k);
        if (j < 0) { flags[k] = EDIT_CHANGED; continue; }
        if (std::memcmp(geom + k * geom_bytes, snap_geom + (size_t)j * geom_bytes, geom_bytes) != 0) flags[k] |= EDIT_MOVED;
        if (std::memcmp(mat + k * mat_bytes, snap_mat + (size_t)j * mat_bytes, mat_bytes) != 0) flags[k] |= EDIT_CHANGED;
    }
    return flags;
}
inline std::vector<int32_t> edit_flags(const unsigned char* geom, const unsigned char* snap_geom, size_t geom_bytes, const unsigned char* mat,
                                       const unsigned char* snap_mat, size_t mat_bytes, size_t spheres) {
    return edit_flags_mapped(geom, snap_geom, geom_bytes, mat, snap_mat, mat_bytes, spheres, nullptr);
}

// The table surface_motion_kernel reads beside the flags, indexed by the kept spheres of the current scene: {C'_j, r'_j} of the snapshot
// for j = from_snapshot[k] >= 0, four zeros of T for an added sphere (never read: its flag is CHANGED).
inline std::vector<unsigned char> motion_snap_table(const unsigned char* snap_geom, size_t geom_bytes, size_t spheres, const int32_t* from_snapshot) {
    std::vector<unsigned char> table(spheres * geom_bytes, 0);
    for (size_t k = 0; k < spheres; ++k) {
        const int32_t j = edit_origin(from_snapshot, k);
        if (j >= 0) std::memcpy(table.data() + k * geom_bytes, snap_geom + (size_t)j * geom_bytes, geom_bytes);
    }
    return table;
}

// One entry: {C.xyz, r} as the bits of T (geom_bytes) and its owner.  Pass 1, through the kept spheres of the current scene in ascending k,
// owner k, with j = from_snapshot[k]:
//   MOVED, with or without CHANGED: two entries, {C'_j, r'_j} of the snapshot, then {C_k, r_k} of the current scene;
//   CHANGED only:                   one entry, {C_k, r_k} (an added sphere is this case);
//   neither:                        none.
// Pass 2, through the spheres j of the snapshot in ascending order that no current sphere continues (the removed ones): one entry
// {C'_j, r'_j} with the owner EDIT_OWNER_REMOVED.  Under the identity pass 2 finds none.
// Old and new places are separate entries, which is what lets a sphere exist on one side of an edit only.
struct EditList {
    std::vector<unsigned char> geom;
    std::vector<int32_t> owner;
    size_t entries() const { return owner.size(); }
};

inline EditList build_edit_list_mapped(const unsigned char* geom, const unsigned char* snap_geom, size_t geom_bytes, const std::vector<int32_t>& flags,
                                       const int32_t* from_snapshot, size_t snap_spheres) {
    EditList list;
    auto entry = [&](const unsigned char* from, size_t k, int32_t owner) {
        list.geom.insert(list.geom.end(), from + k * geom_bytes, from + (k + 1) * geom_bytes);
        list.owner.push_back(owner);
    };
    std::vector<unsigned char> continued(snap_spheres, 0);
    for (size_t k = 0; k < flags.size(); ++k) {
        const int32_t j = edit_origin(from_snapshot, k);
        if (j >= 0) continued[(size_t)j] = 1;
        if (flags[k] & EDIT_MOVED) { entry(snap_geom, (size_t)j, (int32_t)k); entry(geom, k, (int32_t)k); }
        else if (flags[k] & EDIT_CHANGED) entry(geom, k, (int32_t)k);
    }
    for (size_t j = 0; j < snap_spheres; ++j)
        if (!continued[j]) entry(snap_geom, j, EDIT_OWNER_REMOVED);
    return list;
}
inline EditList build_edit_list(const unsigned char* geom, const unsigned char* snap_geom, size_t geom_bytes, const std::vector<int32_t>& flags) {
    return build_edit_list_mapped(geom, snap_geom, geom_bytes, flags, nullptr, flags.size());
}

// The map after an rtiow_edit_scene_mapped.  The new scene has n slots, of which `valid` keeps some (nullptr: all), numbered k' in slot
// order; origin[i] names the slot of the current scene that slot i continues, or -1; current_kept[s] != 0 says that the current scene
// keeps its slot s, and from_snapshot is the current map, by kept sphere.  from_snapshot'[k'] = -1 for origin[i] == -1, else
// from_snapshot[k] for the number k of slot origin[i] among the current scene's kept slots.  The caller has checked the arguments
// (check_scene_mapped, preview_state.h): every origin of a kept slot is -1 or a kept slot of the current scene.
inline std::vector<int32_t> compose_origin(int n, const int32_t* valid, const int32_t* origin, const unsigned char* current_kept, int current_slots,
                                           const int32_t* from_snapshot) {
    std::vector<int32_t> number((size_t)current_slots, -1);      // slot of the current scene -> its number among the kept
    int32_t kept = 0;
    for (int s = 0; s < current_slots; ++s)
        if (current_kept[s]) number[(size_t)s] = kept++;
    std::vector<int32_t> out;
    for (int i = 0; i < n; ++i) {
        if (valid && !valid[i]) continue;
        out.push_back(origin[i] < 0 ? EDIT_NO_ORIGIN : from_snapshot[number[(size_t)origin[i]]]);
    }
    return out;
}
