// The scene edit's share of the preview chain's policy (csrc/library/preview_state.h) on the CPU, with no GPU
// and no library: what puts motion in effect and what ends it, what makes the motion plane current and stale, and the entry checks of
// rtiow_edit_scene and rtiow_read_scene_motion, asked in the order the entry points in rtiow_hip.hip ask them.  stdout: one "RULE BROKEN"
// line per failure, the count last.  Built by tests/test_scene_motion_abi.py with ASan + UBSan, run directly.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "preview_state.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what) { if (!ok) { ++failures; std::printf("RULE BROKEN: %s\n", what); } }

const char* const EDIT = "rtiow_edit_scene";
const char* const READ = "rtiow_read_scene_motion";

// rtiow_edit_scene's checks, in its order: the tables, a scene to edit, the shape.
Refusal edit(const PreviewState& s, bool tables, int n, const int32_t* valid, int current_n, const std::vector<unsigned char>& kept) {
    const std::vector<Refusal> checks = {check_scene_tables(EDIT, tables, n), need_scene_to_edit(s, EDIT)};
    for (const Refusal& r : checks) if (r.code) return r;
    return check_scene_edit(EDIT, n, valid, current_n, kept.data());
}
bool has(const Refusal& r, int code, const char* call, const char* part) { return r.code == code && r.text.find(call) == 0 && r.text.find(part) != std::string::npos; }

PreviewState sampled() {
    PreviewState s;
    on_set_camera(s, true); on_set_scene(s); on_scene_uploaded(s);
    on_accumulation_reset(s); on_rng_initialised(s);
    on_chunk_begin(s); on_plain_chunk(s, 4);
    return s;
}
PreviewState committed() { PreviewState s = sampled(); on_guides_rendered(s); on_history_updated(s); on_commit(s); return s; }
PreviewState edited() { PreviewState s = committed(); on_scene_edited(s); return s; }

void event_rules() {
    PreviewState s = sampled();
    on_scene_edited(s);
    expect(!motion_in_effect(s) && !s.scene_edited && s.acc_mode == ACC_MODE_NONE && !s.guides_ok, "without a base an edit is a set_scene of the same shape");
    on_guides_rendered(s);
    expect(s.guides_ok && !s.motion_ok && need_motion(s, READ).code == PREVIEW_E_STATE, "... and guides rendered then come without a plane");
    s = committed();
    expect(s.hist_base_ok && !motion_in_effect(s) && !s.motion_ok, "a commit leaves motion off");
    // everything rtiow_set_scene makes stale, except the base
    s = committed(); on_set_camera(s, true); on_rng_initialised(s); on_chunk_begin(s); on_plain_chunk(s, 4); on_guides_rendered(s);
    on_history_updated(s); on_plan_written(s); on_denoised(s); on_coverage_rendered(s, 2);
    const uint64_t gen = s.acc_gen;
    on_scene_edited(s);
    expect(s.hist_base_ok && motion_in_effect(s), "an edit keeps the base and puts motion in effect");
    expect(s.acc_samples == 0 && s.acc_mode == ACC_MODE_NONE && s.acc_gen == gen + 1, "... with the accumulation back to 0");
    expect(!s.guides_ok && !s.motion_ok && !s.coverage_ok && !s.plan_ok && !s.hist_ok && !s.denoised_ok, "... guides, layers, plan, temporal and denoised image stale");
    expect(s.rng_ready && s.have_camera && s.scene && s.coverage_grid == 2, "... and camera, RNG states and the lattice kept, as rtiow_set_scene keeps them");
    // the plane follows the guides
    expect(has(need_motion(s, READ), PREVIEW_E_STATE, READ, "no motion plane"), "in effect but not rendered: the plane is stale");
    on_guides_rendered(s);
    expect(s.motion_ok && need_motion(s, READ).code == 0, "guides rendered while motion is in effect bring the plane");
    on_guide_mode_changed(s);
    expect(!s.motion_ok && motion_in_effect(s) && need_motion(s, READ).code == PREVIEW_E_STATE, "a new guide mode makes the plane stale with the guides");
    on_guides_rendered(s); on_set_camera(s, true);
    expect(!s.motion_ok && motion_in_effect(s), "a new camera makes the plane stale and leaves motion in effect");
    on_guides_rendered(s); on_scene_edited(s);
    expect(!s.motion_ok && motion_in_effect(s), "a second edit makes the plane stale and leaves motion in effect");
    // chunks, resets, updates, plans and filters leave both alone
    on_guides_rendered(s); on_chunk_begin(s); on_plain_chunk(s, 1); on_accumulation_reset(s); on_rng_initialised(s); on_history_updated(s);
    on_plan_written(s); on_denoised(s); on_coverage_rendered(s, 4); on_edges_resolved(s);
    expect(s.motion_ok && motion_in_effect(s), "chunks, resets, updates, plans, filters and resolves leave motion and its plane alone");
    // what ends it
    void (*const ends[])(PreviewState&) = {on_commit, on_history_reset, on_set_scene, [](PreviewState& t) { on_set_shard(t, 1); }, [](PreviewState& t) { on_set_shard(t, 2); }};
    for (auto event : ends) {
        PreviewState t = edited();
        on_guides_rendered(t);
        event(t);
        expect(!motion_in_effect(t) && !t.scene_edited && !t.motion_ok, "commit, history reset, set_scene and set_shard end motion");
        expect(has(need_motion(t, READ), PREVIEW_E_STATE, READ, "motion is not in effect"), "... and the read says so");
        on_guides_rendered(t);
        expect(!t.motion_ok, "... and guides rendered afterwards come without a plane");
    }
    s = edited(); on_commit(s);
    expect(s.hist_base_ok && !motion_in_effect(s), "a commit takes a new snapshot: the base stays, motion is off");
    on_scene_edited(s);
    expect(motion_in_effect(s), "... until the next edit");
    s = edited(); on_set_camera(s, false);
    expect(motion_in_effect(s) && need_motion(s, READ).code == PREVIEW_E_STATE, "no camera, no plane");
}

void check_rules() {
    const std::vector<unsigned char> kept = {1, 1, 0, 1};
    const int32_t same[4] = {1, 7, 0, 1}, other[4] = {1, 1, 1, 1}, fewer[4] = {1, 0, 0, 1};
    const PreviewState none, s = sampled();
    expect(has(edit(none, false, 4, same, 0, {}), PREVIEW_E_BADARG, EDIT, "null or empty table"), "a null table is refused first, whatever the state");
    expect(has(edit(s, true, 0, same, 4, kept), PREVIEW_E_BADARG, EDIT, "null or empty table"), "n <= 0 is an empty table");
    expect(has(edit(s, true, -3, same, 4, kept), PREVIEW_E_BADARG, EDIT, "null or empty table"), "... and so is n < 0");
    expect(has(edit(none, true, 4, same, 0, {}), PREVIEW_E_STATE, EDIT, "before rtiow_set_scene"), "no scene yet: RTIOW_E_STATE");
    expect(has(edit(s, true, 3, same, 4, kept), PREVIEW_E_BADARG, EDIT, "n must be the current scene's"), "another n is refused");
    expect(has(edit(s, true, 5, same, 4, kept), PREVIEW_E_BADARG, EDIT, "n must be the current scene's"), "... a larger one too");
    expect(has(edit(s, true, 4, other, 4, kept), PREVIEW_E_BADARG, EDIT, "valid must keep the slots"), "a valid that keeps one more slot is refused");
    expect(has(edit(s, true, 4, fewer, 4, kept), PREVIEW_E_BADARG, EDIT, "valid must keep the slots"), "... and one that keeps one less");
    expect(has(edit(s, true, 4, nullptr, 4, kept), PREVIEW_E_BADARG, EDIT, "valid must keep the slots"), "valid == NULL keeps every slot: refused when the scene drops one");
    expect(edit(s, true, 4, same, 4, kept).code == 0, "the same pattern is accepted (any non-zero value keeps a slot)");
    expect(edit(s, true, 4, nullptr, 4, {1, 1, 1, 1}).code == 0 && edit(s, true, 4, other, 4, {1, 1, 1, 1}).code == 0, "valid == NULL matches a scene that keeps every slot");
    expect(edit(committed(), true, 4, same, 4, kept).code == 0 && edit(edited(), true, 4, same, 4, kept).code == 0, "with a base, and again while motion is in effect");
    PreviewState sharded = sampled(); on_set_shard(sharded, 2);
    expect(edit(sharded, true, 4, same, 4, kept).code == 0, "a sharded handle may edit: it has no base, so no motion");
}

}  // namespace

int main() {
    event_rules();
    check_rules();
    std::printf("%d scene-motion rule failure(s)\n", failures);
    return failures ? 1 : 0;
}
