// The mapped scene edit's share of the preview chain's policy (csrc/library/preview_state.h) on the CPU, with no
// GPU and no library: the entry checks of rtiow_edit_scene_mapped with their wording, asked in the order the entry point in rtiow_hip.hip
// asks them, what rtiow_read_scene_origin needs, and that the call's event is rtiow_edit_scene's.  stdout: one "RULE BROKEN" line per
// failure, the count last.  Built by tests/test_scene_mapped_abi.py with ASan + UBSan, run directly.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "preview_state.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what) { if (!ok) { ++failures; std::printf("RULE BROKEN: %s\n", what); } }

const char* const EDIT = "rtiow_edit_scene_mapped";
const char* const READ = "rtiow_read_scene_origin";

struct Args {
    bool tables = true;
    int n = 3;
    std::vector<int32_t> valid, type = {0, 1, 2}, origin = {0, -1, 3};
    bool have_valid = false, have_origin = true;
};
// the scene the handle holds: 4 slots, slot 2 dropped
const std::vector<unsigned char> KEPT = {1, 1, 0, 1};

// rtiow_edit_scene_mapped's checks, in its order: the tables, a scene to edit, the map's arguments.
Refusal edit(const PreviewState& s, const Args& a, const std::vector<unsigned char>& kept = KEPT) {
    if (Refusal r = check_scene_tables(EDIT, a.tables, a.n); r.code) return r;
    if (Refusal r = need_scene_to_edit(s, EDIT); r.code) return r;
    return check_scene_mapped(EDIT, a.n, a.have_valid ? a.valid.data() : nullptr, a.type.data(), a.have_origin ? a.origin.data() : nullptr, (int)kept.size(), kept.data());
}
bool is(const Refusal& r, int code, const std::string& text) { return r.code == code && r.text == text; }
std::string said(const char* rest) { return std::string(EDIT) + rest; }

PreviewState sampled() {
    PreviewState s;
    on_set_camera(s, true); on_set_scene(s); on_scene_uploaded(s);
    on_accumulation_reset(s); on_rng_initialised(s);
    on_chunk_begin(s); on_plain_chunk(s, 4);
    return s;
}
PreviewState committed() { PreviewState s = sampled(); on_guides_rendered(s); on_history_updated(s); on_commit(s); return s; }

void check_rules() {
    const PreviewState none, s = sampled();
    const std::string TABLE = said(": null or empty table"), SCENE = said(" before rtiow_set_scene");
    const std::string ORIGIN = said(": origin must not be NULL (-1 per slot: every sphere is new)");
    const std::string SLOT = said(": origin must be -1 or a slot the current scene keeps");
    const std::string TWICE = said(": two slots continue the same sphere (a sphere is continued at most once)");
    Args a;
    expect(edit(s, a).code == 0 && edit(committed(), a).code == 0, "three slots continuing slots 0 and 3 and adding one are accepted, with a base or without");
    // the order: tables, scene, origin, range, duplicates, type / no kept slot -- each refusal with everything behind it wrong too
    Args all_bad; all_bad.tables = false; all_bad.have_origin = false; all_bad.type = {9, 9, 9};
    expect(is(edit(none, all_bad), PREVIEW_E_BADARG, TABLE), "a null table is refused first, whatever the state");
    all_bad.tables = true; all_bad.n = 0;
    expect(is(edit(none, all_bad), PREVIEW_E_BADARG, TABLE), "n <= 0 is an empty table");
    all_bad.n = -4;
    expect(is(edit(none, all_bad), PREVIEW_E_BADARG, TABLE), "... and so is n < 0");
    all_bad.n = 3;
    expect(is(edit(none, all_bad), PREVIEW_E_STATE, SCENE), "no scene yet: RTIOW_E_STATE, before the origin is looked at");
    expect(is(edit(s, all_bad), PREVIEW_E_BADARG, ORIGIN), "origin == NULL is refused before the types are looked at");
    for (int32_t bad : {-2, 4, 2, INT32_MAX, INT32_MIN}) {
        Args b; b.origin = {0, bad, 0}; b.type = {9, 9, 9};
        expect(is(edit(s, b), PREVIEW_E_BADARG, SLOT), "an origin below -1, past the current slots or naming a dropped slot is refused before duplicates and types");
    }
    Args twice; twice.origin = {3, 1, 3}; twice.type = {0, 9, 0};
    expect(is(edit(s, twice), PREVIEW_E_BADARG, TWICE), "two kept slots naming one origin are refused before the types");
    Args fresh; fresh.origin = {-1, -1, -1};
    expect(edit(s, fresh).code == 0, "-1 may repeat: every sphere new");
    for (int32_t bad : {-1, 3, 1 << 20}) {
        Args b; b.type = {0, bad, 2};
        expect(is(edit(s, b), PREVIEW_E_BADARG, "material type out of range"), "a material type outside 0..2 on a kept slot, in upload_scene's words");
    }
    Args nothing; nothing.have_valid = true; nothing.valid = {0, 0, 0}; nothing.origin = {77, 77, 77}; nothing.type = {9, 9, 9};
    expect(is(edit(s, nothing), PREVIEW_E_BADARG, "scene has no valid spheres"), "no kept slot at all, in upload_scene's words");
    // a dropped slot is not read
    Args dropped; dropped.have_valid = true; dropped.valid = {5, 0, 1}; dropped.origin = {0, -9, 3}; dropped.type = {0, 9, 0};
    expect(edit(s, dropped).code == 0, "origin and type of a slot valid drops are not read (any non-zero value keeps a slot)");
    dropped.origin = {0, 0, 3};
    expect(edit(s, dropped).code == 0, "... so it names no origin twice either");
    // any n and any valid
    Args more; more.n = 6; more.type = {0, 0, 0, 0, 0, 0}; more.origin = {3, -1, 1, -1, 0, -1};
    expect(edit(s, more).code == 0, "more slots than the current scene has");
    Args one; one.n = 1; one.type = {2}; one.origin = {1};
    expect(edit(s, one).code == 0, "fewer slots than the current scene has");
    expect(is(edit(s, one, {1, 0, 0, 1}), PREVIEW_E_BADARG, SLOT), "... against the scene the handle holds now");
}

void event_rules() {
    // the call's event is rtiow_edit_scene's
    PreviewState s = committed();
    on_set_camera(s, true); on_rng_initialised(s); on_chunk_begin(s); on_plain_chunk(s, 4); on_guides_rendered(s);
    on_history_updated(s); on_plan_written(s); on_denoised(s); on_coverage_rendered(s, 2);
    const uint64_t gen = s.acc_gen;
    expect(is(need_motion_in_effect(s, READ), PREVIEW_E_STATE, std::string(READ) + ": motion is not in effect (rtiow_edit_scene on a handle with a history base)"),
           "before any edit the map cannot be read, in rtiow_read_scene_motion's words");
    expect(need_motion(s, READ).text == need_motion_in_effect(s, READ).text, "... the very words");
    on_scene_edited(s);
    expect(s.hist_base_ok && motion_in_effect(s) && need_motion_in_effect(s, READ).code == 0, "a mapped edit on a committed handle: the base stays, motion is in effect, the map can be read");
    expect(s.acc_samples == 0 && s.acc_mode == ACC_MODE_NONE && s.acc_gen == gen + 1, "... with the accumulation back to 0");
    expect(!s.guides_ok && !s.motion_ok && !s.coverage_ok && !s.plan_ok && !s.hist_ok && !s.denoised_ok, "... guides, layers, plan, temporal and denoised image stale");
    expect(s.rng_ready && s.have_camera && s.scene, "... camera and RNG states kept");
    on_guides_rendered(s);
    expect(s.motion_ok && need_motion_in_effect(s, READ).code == 0, "the map needs no plane, and is there with one");
    void (*const ends[])(PreviewState&) = {on_commit, on_history_reset, on_set_scene, [](PreviewState& t) { on_set_shard(t, 1); }, [](PreviewState& t) { on_set_shard(t, 2); }};
    for (auto event : ends) {
        PreviewState t = committed();
        on_scene_edited(t);
        event(t);
        expect(!motion_in_effect(t) && need_motion_in_effect(t, READ).code == PREVIEW_E_STATE, "commit, history reset, set_scene and set_shard end motion and the map's read");
    }
    PreviewState u = sampled();
    on_guides_rendered(u); on_history_updated(u);
    on_scene_edited(u);
    expect(!motion_in_effect(u) && !u.scene_edited && u.acc_mode == ACC_MODE_NONE && !u.hist_ok && need_motion_in_effect(u, READ).code == PREVIEW_E_STATE,
           "on an uncommitted handle a mapped edit is a set_scene: motion is not in effect");
    PreviewState sharded = sampled();
    on_set_shard(sharded, 2); on_rng_initialised(sharded); on_chunk_begin(sharded); on_plain_chunk(sharded, 1);
    Args a;
    expect(edit(sharded, a).code == 0, "a sharded handle may edit");
    on_scene_edited(sharded);
    expect(!motion_in_effect(sharded) && need_motion_in_effect(sharded, READ).code == PREVIEW_E_STATE, "... it has no base, so motion is not in effect");
    PreviewState was = committed();
    on_set_shard(was, 2); on_scene_edited(was);
    expect(!motion_in_effect(was), "... and a shard set after a commit took the base away");
}

}  // namespace

int main() {
    check_rules();
    event_rules();
    std::printf("%d scene-mapped rule failure(s)\n", failures);
    return failures ? 1 : 0;
}
