// preview_state.h -- the policy of the preview chain (INTEGRATION.md sections 7 to 20): what the handle holds that is current
// (PreviewState), what every event makes current or stale (on_*: one function per event, each stating everything that event touches),
// what a call needs (need_*: a predicate that carries its refusal) and the argument checks the calls share (check_*).
// rtiow_hip.hip and launch.h ask here and write none of these fields themselves; nothing here touches the device.
// Plain C++ (no HIP): also built on its own by tests/native/preview_state_main.cpp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

constexpr int PREVIEW_E_BADARG = -1, PREVIEW_E_STATE = -2;   // RTIOW_E_BADARG, RTIOW_E_STATE (include/rtiow.h); handle.h asserts them equal
enum { ACC_MODE_NONE = 0, ACC_MODE_PLAIN = 1, ACC_MODE_ADAPTIVE = 2 };   // PreviewState::acc_mode: no chunk since the reset, rtiow_accumulate, rtiow_accumulate_adaptive / _budget
enum { DENOISED_FROM_ACCUMULATION = 0, DENOISED_FROM_TEMPORAL = 1 };     // PreviewState::denoised_from: rtiow_denoise(_variance), rtiow_denoise_history(_variance)

struct PreviewState {
    bool scene = false;                           // rtiow_set_scene has uploaded one (the handle's n != 0); a scene never goes away again
    bool have_camera = false;
    int nranks = 1;                               // rtiow_set_shard: the filters and the history refuse nranks > 1
    bool rng_ready = false;
    // progressive rendering: the samples rtiow_accumulate has accumulated since the last reset, and the mode the first chunk after a
    // reset fixed (ACC_MODE_*: rtiow_accumulate or rtiow_accumulate_adaptive)
    int acc_samples = 0, acc_mode = ACC_MODE_NONE;
    // denoised previews: guides_ok: the guides belong to the current scene, camera and shard (with RTIOW_GUIDES_SPECULAR it covers the
    // chain's set too); denoised_ok: rtiow_denoise has filled the denoised image since the last set_*
    bool guides_ok = false, denoised_ok = false;
    // temporal history.  hist_base_ok: there is a base, what rtiow_history_commit kept of an earlier camera; it survives rtiow_set_camera,
    // rtiow_accumulate_reset and rtiow_init_rng, and is emptied by rtiow_history_reset, rtiow_set_scene and rtiow_set_shard.
    // hist_ok: rtiow_history_update has written the temporal image of the current camera since the last set_* / reset / commit.
    bool hist_base_ok = false, hist_ok = false;
    // variance-guided filtering of the temporal image.  hist_var_ok: rtiow_denoise_history_variance has written the plane V^0 for the
    // temporal image the handle holds -- it goes stale with hist_ok and with every update.  acc_gen counts the chunks and resets of the
    // accumulation; hist_gen is its value at the update that wrote the temporal image, whose alpha = n / Mout holds only while the two agree.
    bool hist_var_ok = false;
    uint64_t acc_gen = 0, hist_gen = 0;
    // history-guided sample budgets.  plan_ok: rtiow_history_plan has written the plan since the last set_* / history reset / commit --
    // it goes stale with the temporal image
    bool plan_ok = false;
    // edge resolve.  coverage_ok: the coverage layers belong to the current scene, camera and shard;
    // coverage_grid: the sub-samples per side of the last rtiow_render_coverage, 0 before the first (it survives everything).
    // denoised_from: which image the filter that wrote the denoised image read (DENOISED_FROM_*), and denoised_gen: acc_gen at that
    // filter -- the counts behind the image are the accumulation's only while the two agree.  resolved: rtiow_resolve_edges has rewritten
    // the denoised image since that filter.
    bool coverage_ok = false;
    int coverage_grid = 0;
    int denoised_from = DENOISED_FROM_ACCUMULATION;
    uint64_t denoised_gen = 0;
    bool resolved = false;
    // scene edits that keep the history.  scene_edited: rtiow_edit_scene has changed the scene since the commit
    // that made the base -- motion is in effect; it is cleared wherever the base is made or emptied.  motion_ok: the motion plane belongs to
    // the current scene, camera and shard; it is written wherever the guides are while motion is in effect and goes stale with them.
    bool scene_edited = false, motion_ok = false;
    // edit influence.  influence_on: rtiow_set_edit_influence holds a kappa > 0.  While it does, the influence
    // plane is written wherever the motion plane is, and the motion plane's fourth T holds the fade: both are current exactly when motion_ok.
    bool influence_on = false;
    // guided upscaling.  upscaled_ok: rtiow_upscale has written the upscaled image of the current scene, camera
    // and shard; upscale_factor: its F (0 before the first; it survives everything).  A finished output: only a new frame makes it stale.
    bool upscaled_ok = false;
    int upscale_factor = 0;
};

// ---- events.  Flags are raised behind a successful enqueue, never before it; on_chunk_begin alone comes before its launch.
// Every reset of the accumulation bumps acc_gen, as every chunk does (need_same_accumulation compares it with the update's).
inline void on_accumulation_reset(PreviewState& s) { s.acc_samples = 0; s.acc_mode = ACC_MODE_NONE; ++s.acc_gen; }
// A new guide mode (rtiow_set_guide_mode) or lens lattice (rtiow_set_guide_lens) makes the guides and the denoised image stale and nothing else.
inline void on_guide_mode_changed(PreviewState& s) { s.guides_ok = false; s.motion_ok = false; s.denoised_ok = false; }
// What a new scene, camera or shard has in common: the accumulation, the guides and the denoised image, the temporal image and the
// history plan, the coverage layers and the upscaled image are of the old frame.  (rtiow_hip.hip drops the carried hand-out order beside
// it: its cost map is of the old frame too.)
inline void on_frame_changed(PreviewState& s) {
    on_accumulation_reset(s); on_guide_mode_changed(s);
    s.hist_ok = false; s.plan_ok = false; s.coverage_ok = false; s.upscaled_ok = false;
}
// rtiow_set_scene, before the upload: also the history base goes, which a new camera keeps.  The RNG states stay.
inline void on_set_scene(PreviewState& s) { on_frame_changed(s); s.hist_base_ok = false; s.scene_edited = false; }
// rtiow_edit_scene and rtiow_edit_scene_mapped, before the upload: rtiow_set_scene's event without emptying the base; with a base, motion
// is in effect from here on.
inline void on_scene_edited(PreviewState& s) { on_frame_changed(s); s.scene_edited = s.hist_base_ok; }
inline void on_scene_uploaded(PreviewState& s) { s.scene = true; }
// rtiow_set_edit_influence with another kappa than the handle has (`on`: the new one is > 0): everything that depends on the motion plane
// is stale -- the plane, the guides it is rendered with, the plan, the temporal image and the denoised image.  The knob itself survives
// every other event.
inline void on_edit_influence_changed(PreviewState& s, bool on) { s.influence_on = on; on_guide_mode_changed(s); s.hist_ok = false; s.plan_ok = false; }
// rtiow_set_camera: a bad image size takes the camera away and leaves everything else; a good one -- the very camera the handle
// already has is no exception -- also asks for new RNG states.  The base survives.
inline void on_set_camera(PreviewState& s, bool good_size) { s.have_camera = good_size; if (good_size) { on_frame_changed(s); s.rng_ready = false; } }
inline void on_set_shard(PreviewState& s, int nranks) { s.nranks = nranks; on_frame_changed(s); s.rng_ready = false; s.hist_base_ok = false; s.scene_edited = false; }
// rtiow_init_rng resets the accumulation where it starts (on_accumulation_reset) and ends here.
inline void on_rng_initialised(PreviewState& s) { s.rng_ready = true; }
// A chunk of either kind, before its launch; then the chunk itself: a plain one counts its samples, the first of a kind fixes the mode.
inline void on_chunk_begin(PreviewState& s) { ++s.acc_gen; }
inline void on_plain_chunk(PreviewState& s, int samples) { s.acc_samples += samples; s.acc_mode = ACC_MODE_PLAIN; }
inline void on_adaptive_chunk(PreviewState& s) { s.acc_mode = ACC_MODE_ADAPTIVE; }
// The motion plane is rendered with the guides while motion is in effect, and only then.
inline void on_guides_rendered(PreviewState& s) { s.guides_ok = true; s.motion_ok = s.scene_edited; }
// Any of the four filters: the image is new, so not resolved, and its counts are those of the accumulation as it stands.
inline void on_denoised(PreviewState& s, int from = DENOISED_FROM_ACCUMULATION) { s.denoised_ok = true; s.denoised_from = from; s.denoised_gen = s.acc_gen; s.resolved = false; }
inline void on_coverage_rendered(PreviewState& s, int grid) { s.coverage_ok = true; s.coverage_grid = grid; }
inline void on_edges_resolved(PreviewState& s) { s.resolved = true; }
inline void on_upscaled(PreviewState& s, int factor) { s.upscaled_ok = true; s.upscale_factor = factor; }
// rtiow_history_update / _clipped: V^0 was of the image this one replaces.
inline void on_history_updated(PreviewState& s) { s.hist_ok = true; s.hist_var_ok = false; s.hist_gen = s.acc_gen; }
inline void on_plan_written(PreviewState& s) { s.plan_ok = true; }
inline void on_temporal_variance_written(PreviewState& s) { s.hist_var_ok = true; }
inline void on_history_reset(PreviewState& s) { s.hist_base_ok = false; s.hist_ok = false; s.plan_ok = false; s.scene_edited = false; s.motion_ok = false; }
// Both commits: the temporal image and the guides became the base by changing owners, so what they leave behind is stale.
// The base is of the scene as it stands now: motion is off until the next rtiow_edit_scene.
inline void on_commit(PreviewState& s) { s.hist_base_ok = true; s.hist_ok = false; s.plan_ok = false; s.guides_ok = false; s.scene_edited = false; s.motion_ok = false; }

// ---- refusals: the code a call returns and the text it leaves in rtiow_last_error_string, `call` first.  code 0: not refused.
struct Refusal {
    int code = 0;
    std::string text;
};
inline Refusal refuse_unless(bool ok, int code, const char* call, const std::string& text) { return ok ? Refusal{} : Refusal{code, call + text}; }

// ---- preconditions.  ASKS_SCENE: the call also asks for a scene, under the same text.  A chunk needs one (need_scene) and a scene never
// goes away, so acc_mode != ACC_MODE_NONE and hist_ok each imply it; the calls differ in whether they ask all the same, and keep to that.
enum Asks { ASKS_CAMERA, ASKS_SCENE };
inline bool frame_set(const PreviewState& s, Asks asks) { return s.have_camera && (asks == ASKS_CAMERA || s.scene); }
inline Refusal need_scene(const PreviewState& s, const char* call) { return refuse_unless(frame_set(s, ASKS_SCENE), PREVIEW_E_STATE, call, " before rtiow_set_scene/rtiow_set_camera"); }
inline Refusal need_rng(const PreviewState& s, const char* call) { return refuse_unless(s.rng_ready, PREVIEW_E_STATE, call, " before rtiow_init_rng"); }
// neighbours: the wording of the calls that filter or reproject (the others read or forget what those wrote).
inline Refusal need_unsharded(const PreviewState& s, const char* call, bool neighbours) {
    return refuse_unless(s.nranks <= 1, PREVIEW_E_STATE, call, neighbours ? ": not on a sharded handle (the strips of a shard are not image neighbours)" : ": not on a sharded handle");
}
inline Refusal need_chunk(const PreviewState& s, const char* call, Asks asks) {
    return refuse_unless(frame_set(s, asks) && s.acc_mode != ACC_MODE_NONE, PREVIEW_E_STATE, call, ": no chunk since the last reset");
}
inline Refusal need_adaptive_chunk(const PreviewState& s, const char* call, Asks asks) {
    return refuse_unless(frame_set(s, asks) && s.acc_mode == ACC_MODE_ADAPTIVE, PREVIEW_E_STATE, call, ": no adaptive chunk since the last reset (plain chunks keep no second moment)");
}
// A chunk of one kind refuses an accumulation of the other (`other`: ACC_MODE_PLAIN or ACC_MODE_ADAPTIVE).
inline Refusal need_no_chunk_of(const PreviewState& s, const char* call, int other) {
    return refuse_unless(s.acc_mode != other, PREVIEW_E_STATE, call, std::string(" after ") + (other == ACC_MODE_PLAIN ? "rtiow_accumulate" : "rtiow_accumulate_adaptive") + ": reset the accumulation first");
}
inline Refusal need_guides(const PreviewState& s, const char* call) {
    return refuse_unless(s.have_camera && s.guides_ok, PREVIEW_E_STATE, call, ": no guides for the current scene, camera and shard (rtiow_render_guides)");
}
inline Refusal need_denoised(const PreviewState& s, const char* call) { return refuse_unless(s.have_camera && s.denoised_ok, PREVIEW_E_STATE, call, " before rtiow_denoise"); }
inline Refusal need_temporal_image(const PreviewState& s, const char* call, Asks asks) {
    return refuse_unless(frame_set(s, asks) && s.hist_ok, PREVIEW_E_STATE, call, ": no temporal image for the current camera (rtiow_history_update)");
}
// The accumulation is still the one the update read.
inline Refusal need_same_accumulation(const PreviewState& s, const char* call) {
    return refuse_unless(s.hist_gen == s.acc_gen, PREVIEW_E_STATE, call, ": a chunk or a reset since the update that wrote the temporal image (update again)");
}
inline Refusal need_temporal_variance(const PreviewState& s, const char* call) {
    return refuse_unless(s.have_camera && s.hist_ok && s.hist_var_ok, PREVIEW_E_STATE, call, ": no variance plane for the temporal image (rtiow_denoise_history_variance)");
}
inline Refusal need_base(const PreviewState& s, const char* call) { return refuse_unless(s.hist_base_ok, PREVIEW_E_STATE, call, ": no history base (rtiow_history_commit)"); }
inline Refusal need_plan(const PreviewState& s, const char* call) {
    return refuse_unless(s.have_camera && s.plan_ok, PREVIEW_E_STATE, call, ": no history plan for the current camera (rtiow_history_plan)");
}
inline Refusal need_coverage(const PreviewState& s, const char* call) {
    return refuse_unless(s.have_camera && s.coverage_ok, PREVIEW_E_STATE, call, ": no coverage layers for the current scene, camera and shard (rtiow_render_coverage)");
}
// rtiow_resolve_edges: the denoised image is a filter's own (a second pass would blend twice), the temporal image it came from is still
// there to be read for its lengths, and the accumulation still holds the counts the filter saw.
inline Refusal need_unresolved(const PreviewState& s, const char* call) { return refuse_unless(!s.resolved, PREVIEW_E_STATE, call, ": the denoised image is already resolved (filter again)"); }
inline Refusal need_denoised_source(const PreviewState& s, const char* call) {
    return refuse_unless(s.denoised_from != DENOISED_FROM_TEMPORAL || s.hist_ok, PREVIEW_E_STATE, call,
                         ": the temporal image the denoised image came from is stale (resolve before rtiow_history_commit)");
}
inline Refusal need_denoised_accumulation(const PreviewState& s, const char* call) {
    return refuse_unless(s.denoised_gen == s.acc_gen, PREVIEW_E_STATE, call, ": a chunk or a reset since the filter that wrote the denoised image (filter again)");
}
// rtiow_read_upscaled, rtiow_upscaled_device_ptr: an rtiow_upscale since the last new scene, camera or shard.
inline Refusal need_upscaled(const PreviewState& s, const char* call) {
    return refuse_unless(s.have_camera && s.upscaled_ok, PREVIEW_E_STATE, call, ": no upscaled image for the current scene, camera and shard (rtiow_upscale)");
}
// Motion is in effect: from an rtiow_edit_scene on a handle with a base until the next commit, history reset, set_scene or set_shard.
inline bool motion_in_effect(const PreviewState& s) { return s.hist_base_ok && s.scene_edited; }
// rtiow_edit_scene: a scene to edit.  (Its argument checks compare with the tables the handle holds: check_scene_edit.)
inline Refusal need_scene_to_edit(const PreviewState& s, const char* call) { return refuse_unless(s.scene, PREVIEW_E_STATE, call, " before rtiow_set_scene"); }
// rtiow_read_scene_motion: motion in effect and the plane of the current scene, camera and shard.
inline Refusal need_motion(const PreviewState& s, const char* call) {
    if (Refusal r = refuse_unless(motion_in_effect(s), PREVIEW_E_STATE, call, ": motion is not in effect (rtiow_edit_scene on a handle with a history base)"); r.code) return r;
    return refuse_unless(s.have_camera && s.guides_ok && s.motion_ok, PREVIEW_E_STATE, call, ": no motion plane for the current scene, camera and shard (rtiow_render_guides)");
}
// rtiow_read_scene_origin: motion in effect, in rtiow_read_scene_motion's words; the map is the host's, so no plane is asked for.
inline Refusal need_motion_in_effect(const PreviewState& s, const char* call) {
    return refuse_unless(motion_in_effect(s), PREVIEW_E_STATE, call, ": motion is not in effect (rtiow_edit_scene on a handle with a history base)");
}
// rtiow_read_edit_influence: motion in effect, the knob on (no plane is made while it is off), and the plane current with the motion plane.
inline Refusal need_edit_influence(const PreviewState& s, const char* call) {
    if (Refusal r = refuse_unless(motion_in_effect(s), PREVIEW_E_STATE, call, ": motion is not in effect (rtiow_edit_scene on a handle with a history base)"); r.code) return r;
    if (Refusal r = refuse_unless(s.influence_on, PREVIEW_E_STATE, call, ": edit influence is off (rtiow_set_edit_influence with kappa > 0)"); r.code) return r;
    return refuse_unless(s.have_camera && s.guides_ok && s.motion_ok, PREVIEW_E_STATE, call, ": no influence plane for the current scene, camera and shard (rtiow_render_guides)");
}
// Does the influence plane follow the motion plane at the next guide render?
inline bool influence_in_effect(const PreviewState& s) { return motion_in_effect(s) && s.influence_on; }
// rtiow_set_edit_influence: kappa >= 0 (+inf: any influence at all drops the history); NaN is refused by the same comparison.
inline Refusal check_edit_influence(const char* call, double kappa) { return refuse_unless(kappa >= 0, PREVIEW_E_BADARG, call, ": need kappa >= 0 (0: off, +inf: any influence drops the history)"); }
// The grid the layers would be rendered with when they are stale: the last one asked for, else COVERAGE_DEFAULT_GRID.
constexpr int COVERAGE_DEFAULT_GRID = 4;
inline int coverage_grid_or_default(const PreviewState& s) { return s.coverage_grid ? s.coverage_grid : COVERAGE_DEFAULT_GRID; }

// ---- argument checks
// The filters: levels in 1..8, then sigma[4] (colour or variance, normal, albedo, depth) each > 0; inv2[k] = 1 / sigma[k]^2.  A call
// without levels (rtiow_history_commit_filtered) passes 1.
inline Refusal check_filter(const char* call, int levels, const double (&sigma)[4], double (&inv2)[4]) {
    if (levels < 1 || levels > 8) return Refusal{PREVIEW_E_BADARG, std::string(call) + ": levels must be 1..8"};
    for (int k = 0; k < 4; ++k) {
        if (!(sigma[k] > 0)) return Refusal{PREVIEW_E_BADARG, std::string(call) + ": every sigma must be > 0 (+inf turns its term off)"};
        inv2[k] = 1.0 / (sigma[k] * sigma[k]);
    }
    return Refusal{};
}
inline Refusal check_history_tolerances(const char* call, double depth_tol, double normal_cos, double max_history) {
    return refuse_unless(depth_tol >= 0 && normal_cos >= -1 && normal_cos <= 1 && max_history > 0, PREVIEW_E_BADARG, call,
                         ": need depth_tol >= 0, normal_cos in [-1, 1], max_history > 0 (+inf: no cap)");
}
// clip_radius and variance_radius (`name`) in 1..max_radius, which the kernel's LDS tile is sized for; rest: what else the text asks for.
inline Refusal check_radius(const char* call, const char* name, int radius, int max_radius, bool rest_ok = true, const char* rest = "") {
    return refuse_unless(radius >= 1 && radius <= max_radius && rest_ok, PREVIEW_E_BADARG, call, std::string(": need ") + name + " in 1.." + std::to_string(max_radius) + rest);
}
inline Refusal check_coverage_grid(const char* call, int subsamples_per_side) {
    return refuse_unless(subsamples_per_side == 2 || subsamples_per_side == 4, PREVIEW_E_BADARG, call, ": subsamples_per_side must be 2 or 4");
}
// rtiow_edit_scene, in the order it asks: the tables are there (check_scene_tables, rtiow_set_scene's own refusal); a scene to edit
// (need_scene_to_edit); n is the current scene's and `valid` keeps the slots the current scene keeps (kept[i] != 0; valid == nullptr
// keeps every slot), so that kept spheres correspond index for index (check_scene_edit).
inline Refusal check_scene_tables(const char* call, bool tables, int n) { return refuse_unless(tables && n > 0, PREVIEW_E_BADARG, call, ": null or empty table"); }
inline Refusal check_scene_edit(const char* call, int n, const int32_t* valid, int current_n, const unsigned char* kept) {
    if (n != current_n) return Refusal{PREVIEW_E_BADARG, std::string(call) + ": n must be the current scene's (rtiow_set_scene changes the shape)"};
    for (int i = 0; i < n; ++i)
        if ((!valid || valid[i] != 0) != (kept[i] != 0)) return Refusal{PREVIEW_E_BADARG, std::string(call) + ": valid must keep the slots the current scene keeps"};
    return Refusal{};
}
// rtiow_edit_scene_mapped, in the order it asks after check_scene_tables and need_scene_to_edit: an origin
// table; for every slot i that `valid` keeps, origin[i] is -1 (a new sphere) or a slot the current scene keeps; no two kept slots continue
// the same sphere; then upload_scene's own refusals, in its words: a material type in 0..2 on every kept slot, and a kept slot at all.
// origin[i] of a slot `valid` drops is not read.  The new scene may have any n and any `valid`.
inline Refusal check_scene_mapped(const char* call, int n, const int32_t* valid, const int32_t* type, const int32_t* origin, int current_n,
                                  const unsigned char* kept) {
    if (!origin) return Refusal{PREVIEW_E_BADARG, std::string(call) + ": origin must not be NULL (-1 per slot: every sphere is new)"};
    auto keeps = [&](int i) { return !valid || valid[i] != 0; };
    for (int i = 0; i < n; ++i)
        if (keeps(i) && origin[i] != -1 && (origin[i] < -1 || origin[i] >= current_n || !kept[origin[i]]))
            return Refusal{PREVIEW_E_BADARG, std::string(call) + ": origin must be -1 or a slot the current scene keeps"};
    std::vector<unsigned char> continued((size_t)(current_n > 0 ? current_n : 0), 0);
    for (int i = 0; i < n; ++i) {
        if (!keeps(i) || origin[i] < 0) continue;
        if (continued[(size_t)origin[i]]) return Refusal{PREVIEW_E_BADARG, std::string(call) + ": two slots continue the same sphere (a sphere is continued at most once)"};
        continued[(size_t)origin[i]] = 1;
    }
    int spheres = 0;
    for (int i = 0; i < n; ++i) {
        if (!keeps(i)) continue;
        if (type[i] < 0 || type[i] > 2) return Refusal{PREVIEW_E_BADARG, "material type out of range"};
        ++spheres;
    }
    return spheres ? Refusal{} : Refusal{PREVIEW_E_BADARG, "scene has no valid spheres"};
}
// rtiow_resolve_edges: radius in 1..max_radius, sigma[2] (normal, depth) each > 0 with inv2[k] = 1 / sigma[k]^2, prior > 0.
inline Refusal check_edge_resolve(const char* call, int radius, int max_radius, const double (&sigma)[2], double prior, double (&inv2)[2]) {
    if (Refusal r = check_radius(call, "radius", radius, max_radius); r.code) return r;
    for (int k = 0; k < 2; ++k) {
        if (!(sigma[k] > 0)) return Refusal{PREVIEW_E_BADARG, std::string(call) + ": every sigma must be > 0 (+inf turns its term off)"};
        inv2[k] = 1.0 / (sigma[k] * sigma[k]);
    }
    return refuse_unless(prior > 0, PREVIEW_E_BADARG, call, ": need prior > 0 (+inf: the rebuilt colour alone)");
}
// rtiow_upscale: factor in min_factor..max_factor, source one of the `sources` RTIOW_UPSCALE_*, sigma[3] (normal, albedo, depth) each > 0
// with inv2[k] = 1 / sigma[k]^2, use_coverage 0 or 1.
inline Refusal check_upscale(const char* call, int factor, int min_factor, int max_factor, int source, int sources, const double (&sigma)[3], int use_coverage,
                             double (&inv2)[3]) {
    if (factor < min_factor || factor > max_factor)
        return Refusal{PREVIEW_E_BADARG, std::string(call) + ": factor must be " + std::to_string(min_factor) + ".." + std::to_string(max_factor)};
    if (source < 0 || source >= sources) return Refusal{PREVIEW_E_BADARG, std::string(call) + ": unknown source (RTIOW_UPSCALE_*)"};
    for (int k = 0; k < 3; ++k) {
        if (!(sigma[k] > 0)) return Refusal{PREVIEW_E_BADARG, std::string(call) + ": every sigma must be > 0 (+inf turns its term off)"};
        inv2[k] = 1.0 / (sigma[k] * sigma[k]);
    }
    return refuse_unless(use_coverage == 0 || use_coverage == 1, PREVIEW_E_BADARG, call, ": use_coverage must be 0 or 1");
}
// ... and its output, factor x the W x rows frame with elem_bytes per T.  The kernel's pixel coordinates are ints that it rounds up to
// whole 8 x 8 tiles (width and height at most 2^31 - 8), and it counts the tiles, rounded up to whole workgroups of four, in an int (at
// most 2^31 - 4 of them).  Within both limits the buffer has under 2^42 bytes, which the kernel indexes in size_t: *out_bytes.
inline Refusal check_upscale_extent(const char* call, int factor, int64_t W, int64_t rows, int64_t elem_bytes, uint64_t* out_bytes) {
    const uint64_t ow = (uint64_t)factor * (uint64_t)W, oh = (uint64_t)factor * (uint64_t)rows;
    if (ow > 0x7ffffff8ull || oh > 0x7ffffff8ull)
        return Refusal{PREVIEW_E_BADARG, std::string(call) + ": the output is wider or higher than the kernel's int coordinates count (2^31 - 8)"};
    const uint64_t tx = (ow + 7) / 8, ty = (oh + 7) / 8;
    if (ty != 0 && tx > 0x7ffffffcull / ty)
        return Refusal{PREVIEW_E_BADARG, std::string(call) + ": the output has more 8 x 8 tiles than the kernel's int counts (2^31 - 4)"};
    if (out_bytes) *out_bytes = ow * oh * 3 * (uint64_t)elem_bytes;
    return Refusal{};
}
