// scene_tables.h -- device tables of a scene: exact / shade tables (upload_scene), motion table, screening table, and the upload of the
// LDS grid (its plan and blob are grid_plan.h's, plain C++)
// Host side of librtiow_hip.so; part of the single translation unit rtiow_hip.hip (internal linkage).
#pragma once
#include "handle.h"
#include "edit_list.h"

namespace {

static_assert(EDIT_MOVED == MOTION_MOVED && EDIT_CHANGED == MOTION_CHANGED, "edit_list.h states the flags of device/scene_motion.h");

template <class T>
int upload_scene(rtiow_handle_s* h, int n, const T* cr, const T* af, const T* ri, const int32_t* type, const int32_t* valid) {
    std::vector<T> ga, st;
    int m = 0;
    for (int i = 0; i < n; ++i) {
        if (valid && !valid[i]) continue;
        const T cx = cr[4 * i], cy = cr[4 * i + 1], cz = cr[4 * i + 2], r = cr[4 * i + 3];
        if (type[i] < 0 || type[i] > 2) return fail_arg(h, RTIOW_E_BADARG, "material type out of range");
        ga.insert(ga.end(), {cx, cy, cz, (T)(r * r)});          // hittable.h:45 radius*radius
        // words 4..7: albedo and fuzz; a dielectric uses neither (material.h:70), its record carries Schlick's
        // r0^2 = ((1 - ri) / (1 + ri))^2 for ri = 1/eta (front face) and ri = eta (back face) instead, computed here
        // with the operations of material.h:62-66 in T (no contraction on the host either)
        auto r0sq = [](T ri_) { T r0 = ((T)1 - ri_) / ((T)1 + ri_); return (T)(r0 * r0); };
        const bool glass = type[i] == RTIOW_DIELECTRIC;
        st.insert(st.end(), {cx, cy, cz, (T)((T)1 / r),         // vec3.h:89-91 (1/t)*v
                             glass ? r0sq((T)((T)1 / ri[i])) : af[4 * i], glass ? r0sq(ri[i]) : af[4 * i + 1], af[4 * i + 2], af[4 * i + 3],
                             ri[i], (T)((T)1 / ri[i]),          // material.h:73 1.0f/refraction_index
                             (T)type[i], (T)0});
        ++m;
    }
    if (m == 0) return fail_arg(h, RTIOW_E_BADARG, "scene has no valid spheres");
    const int mp = (m + 4) / 4 * 4;                         // >= one padding entry: index m is the never-hit sphere that grid cells pad with
    for (int i = m; i < mp; ++i) ga.insert(ga.end(), {(T)0, (T)0, (T)0, (T)-1e12});   // c = |oc|^2 + 1e12 => disc < 0: never hit
    if (sizeof(T) == 4) pair_interleave(ga);                 // fp32: for v_pk_*_f32 (trip_discriminants)
    h->host_cr.clear();
    for (int i = 0; i < n; ++i)
        if (!valid || valid[i]) for (int k = 0; k < 4; ++k) h->host_cr.push_back((double)cr[4 * i + k]);
    h->screen_dirty = true;
    h->large_dirty = true;
    h->volume_dirty = true;
    HIP_TRY(h, h->geom_a.reset());
    HIP_TRY(h, h->shade_tbl.reset());
    HIP_TRY(h, h->geom_a.ensure(sizeof(T) * 4 * mp));
    HIP_TRY(h, h->shade_tbl.ensure(sizeof(T) * 12 * m));
    HIP_TRY(h, hipMemcpy(h->geom_a, ga.data(), sizeof(T) * 4 * mp, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->shade_tbl, st.data(), sizeof(T) * 12 * m, hipMemcpyHostToDevice));
    h->n = m; h->n_padded = mp;
    // what rtiow_edit_scene compares and the commits snapshot: the kept spheres' tables as the bits of T, and the kept pattern
    h->scene_slots = n;
    h->scene_kept.assign((size_t)n, 0);
    h->scene_geom.clear(); h->scene_mat.clear();
    for (int i = 0; i < n; ++i) {
        if (valid && !valid[i]) continue;
        h->scene_kept[i] = 1;
        auto bytes = [](std::vector<unsigned char>& to, const void* from, size_t count) { to.insert(to.end(), (const unsigned char*)from, (const unsigned char*)from + count); };
        bytes(h->scene_geom, cr + 4 * i, 4 * sizeof(T));
        bytes(h->scene_mat, type + i, sizeof(int32_t));
        bytes(h->scene_mat, af + 4 * i, 4 * sizeof(T));
        bytes(h->scene_mat, ri + i, sizeof(T));
    }
    on_scene_uploaded(h->preview);
    h->stats.num_spheres = m;
    h->stats.scene_prepare_ms = 0;
    return 0;
}

// The per-sphere table of the motion plane (surface_motion_kernel) after an rtiow_edit_scene or rtiow_edit_scene_mapped on a handle with a
// base, indexed by the h->n kept spheres of the current scene: for the sphere j = h->from_snapshot[k] of the snapshot that k continues,
// {C'_j, r'_j} and MOTION_MOVED / MOTION_CHANGED from comparing the current record of k with the snapshot's of j, bits against bits; for
// an added sphere (j == -1) zeros and MOTION_CHANGED alone.  The snapshot may hold another number of spheres than the scene.  Beside it,
// from the same comparison, the edit list of edit_influence_kernel (edit_list.h), which may be empty.  The copies are synchronous: the
// vectors are gone on return.
template <class T>
int upload_motion_table(rtiow_handle_s* h) {
    const size_t m = (size_t)h->n, gs = 4 * sizeof(T), ms = sizeof(int32_t) + 5 * sizeof(T);
    if (h->from_snapshot.size() != m) return fail_arg(h, RTIOW_E_STATE, "scene edit: the map does not cover the scene (a base without a snapshot)");
    const int32_t* from = h->from_snapshot.data();       // m entries: the commit's identity, composed by every mapped edit since
    const std::vector<int32_t> flags = edit_flags_mapped(h->scene_geom.data(), h->snap_geom.data(), gs, h->scene_mat.data(), h->snap_mat.data(), ms, m, from);
    const std::vector<unsigned char> snap = motion_snap_table(h->snap_geom.data(), gs, m, from);
    const EditList list = build_edit_list_mapped(h->scene_geom.data(), h->snap_geom.data(), gs, flags, from, h->snap_geom.size() / gs);
    HIP_TRY(h, hipStreamSynchronize(h->stream));         // a plane of the previous edit may still be reading the tables
    HIP_TRY(h, h->motion_snap.ensure(m * gs));
    HIP_TRY(h, h->motion_flags.ensure(m * sizeof(int32_t)));
    HIP_TRY(h, hipMemcpy(h->motion_snap, snap.data(), m * gs, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->motion_flags, flags.data(), m * sizeof(int32_t), hipMemcpyHostToDevice));
    h->edit_entries = 0;
    if (list.entries()) {
        HIP_TRY(h, h->edit_list.ensure(list.geom.size()));
        HIP_TRY(h, h->edit_owner.ensure(list.entries() * sizeof(int32_t)));
        HIP_TRY(h, hipMemcpy(h->edit_list, list.geom.data(), list.geom.size(), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->edit_owner, list.owner.data(), list.entries() * sizeof(int32_t), hipMemcpyHostToDevice));
        h->edit_entries = (int)list.entries();
    }
    return 0;
}

// Builds the screening table of hit_world_screened for the current scene: centres recentred on
// the scene's centroid (ground-like spheres excluded), q' = |C'|^2 - r^2 - 2^-17 (|C'|^2 + r^2)
// rounded DOWN; always fp32 and pair-interleaved like the fp32 geom_a (the fp64 kernel screens in
// fp32 too).  2 Cmax goes to the kernel for the per-ray share of the margin.
template <class T>
int build_screen_table(rtiow_handle_s* h) {
    typedef float S;                                        // the screen runs in fp32 for both precisions
    const int m = h->n, mp = h->n_padded;
    const std::vector<double>& cr = h->host_cr;
    double ctr[3];
    recentring_point(m, cr, false, ctr);
    for (int k = 0; k < 3; ++k) h->ctr[k] = (double)(T)ctr[k];
    std::vector<S> lin((size_t)mp * 4);
    double cmax = 0;                                        // max |C'| over the spheres that are screened
    for (int i = 0; i < mp; ++i) {
        if (i >= m) { lin[4 * i] = lin[4 * i + 1] = lin[4 * i + 2] = 0; lin[4 * i + 3] = (S)1e12; continue; }   // padding: c~ huge => never a candidate
        double c2 = 0;
        for (int k = 0; k < 3; ++k) {
            const S cp = (S)(cr[4 * i + k] - h->ctr[k]);    // what the kernel will use as C'
            lin[4 * i + k] = cp;
            c2 += (double)cp * (double)cp;
        }
        if (std::sqrt(c2) > 64.0) { lin[4 * i + 3] = (S)-1e30; continue; }         // e.g. the ground: always re-tested exactly
        cmax = std::max(cmax, std::sqrt(c2));
        const double r = cr[4 * i + 3], r2 = r * r;
        const double kappa = std::ldexp(1.0, -17) * (c2 + r2);                     // the sphere's share of the margin
        S q = (S)(c2 - r2 - kappa);
        if ((double)q > c2 - r2 - kappa) q = std::nextafter(q, (S)-INFINITY);
        lin[4 * i + 3] = q;
    }
    h->omax2 = 2.0 * cmax * 1.000001;                       // per-ray share uses 2 Cmax |O'| + |O'|^2; the slack covers the raw sqrt (<= 2^-22 relative) in the kernel
    pair_interleave(lin);
    HIP_TRY(h, h->geom_s.reset());
    HIP_TRY(h, h->geom_s.ensure(lin.size() * sizeof(S)));
    HIP_TRY(h, hipMemcpy(h->geom_s, lin.data(), lin.size() * sizeof(S), hipMemcpyHostToDevice));
    h->screen_dirty = false;
    return 0;
}

// Builds the device tables of hit_world_grid for the current scene (after build_screen_table, whose recentring point the plan
// shares): grid_plan.h's plan and blob, uploaded.  On return h->grid.use_grid says whether the scene has a grid; its offsets stay
// relative to the blob (h->grid_at) until layout_lds places it in LDS.
template <class T>
int build_grid_tables(rtiow_handle_s* h) {
    GridParams& g = h->grid;
    g = GridParams{};
    HIP_TRY(h, h->grid_blob.reset());
    const GridPlan pl = plan_grid(h->n, h->host_cr, h->ctr);
    if (!pl.usable) return 0;
    const GridBlob b = build_grid_blob<T>(pl, h->n, h->host_cr);
    HIP_TRY(h, h->grid_blob.ensure(b.bytes.size()));
    HIP_TRY(h, hipMemcpy(h->grid_blob, b.bytes.data(), b.bytes.size(), hipMemcpyHostToDevice));
    h->grid_at = b;
    h->grid_direct = (int)pl.direct.size(); h->grid_registered = pl.registered;
    fill_grid_params(g, pl);
    place_grid_blob(g, b, 0);
    g.blob = h->grid_blob;
    g.blob_bytes = (int)b.bytes.size();
    return 0;
}

template <class T>
void fill_screen_params(RenderParams<T>& p, const rtiow_handle_s* h) {
    p.screen.geom_s = h->geom_s;
    p.use_screen = ((h->scene_source == RTIOW_SCENE_LDS || h->scene_source == RTIOW_SCENE_GRID) && h->geom_s) ? 1 : 0;
    p.screen.ctr_x = (T)h->ctr[0]; p.screen.ctr_y = (T)h->ctr[1]; p.screen.ctr_z = (T)h->ctr[2]; p.screen.omax2 = (T)h->omax2;
}

}  // namespace
