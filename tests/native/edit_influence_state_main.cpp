// Edit influence's share of the preview chain's policy (csrc/library/preview_state.h) on the CPU, with no GPU
// and no library: what a new kappa makes stale and what it leaves alone, and what rtiow_read_edit_influence needs.
// First the rules on the events alone: one "RULE BROKEN" line per failure.  Then stdin: one line of steps per state (the steps of
// tests/preview_refusals.py's STATES, and edit / guides / kappa_on / kappa_off); for each, a fresh PreviewState goes through the steps'
// events and rtiow_read_edit_influence's check is asked: stdout "code | message".  The count of rule failures comes last.
// Built by tests/test_edit_influence_abi.py with ASan + UBSan, run directly.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>

#include "preview_state.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what) { if (!ok) { ++failures; std::printf("RULE BROKEN: %s\n", what); } }

const char* const SET = "rtiow_set_edit_influence";
const char* const READ = "rtiow_read_edit_influence";

// What a pass does to the state before its own event: guides that are not current are rendered first (run_pass in rtiow_hip.hip).
void pass(PreviewState& s) { if (!s.guides_ok) on_guides_rendered(s); }

void step(PreviewState& s, const std::string& name) {
    if (name == "scene_camera") { on_set_camera(s, true); on_set_scene(s); on_scene_uploaded(s); }
    else if (name == "rng") { on_accumulation_reset(s); on_rng_initialised(s); }
    else if (name == "plain") { on_chunk_begin(s); on_plain_chunk(s, 1); }
    else if (name == "adaptive") { on_chunk_begin(s); on_adaptive_chunk(s); }
    else if (name == "update") { pass(s); on_history_updated(s); }
    else if (name == "plan") { pass(s); on_plan_written(s); }
    else if (name == "commit") on_commit(s);
    else if (name == "move") on_set_camera(s, true);
    else if (name == "history_variance") { pass(s); on_temporal_variance_written(s); on_denoised(s); }
    else if (name == "shard") on_set_shard(s, 3);
    else if (name == "edit") on_scene_edited(s);
    else if (name == "guides") on_guides_rendered(s);
    else if (name == "kappa_on") { if (!s.influence_on) on_edit_influence_changed(s, true); }      // the entry point: the same value changes nothing
    else if (name == "kappa_off") { if (s.influence_on) on_edit_influence_changed(s, false); }
    else { std::fprintf(stderr, "unknown step %s\n", name.c_str()); std::exit(2); }
}

PreviewState after(const char* steps) {
    PreviewState s;
    std::istringstream in(steps);
    for (std::string name; in >> name;) step(s, name);
    return s;
}
bool has(const Refusal& r, int code, const char* call, const char* part) { return r.code == code && r.text.find(call) == 0 && r.text.find(part) != std::string::npos; }

void event_rules() {
    const char* const EDITED = "scene_camera rng plain update commit edit rng plain";
    PreviewState s;
    expect(!s.influence_on && !influence_in_effect(s), "a handle starts with the knob off");
    // everything that depends on the motion plane goes stale, and nothing else
    s = after(EDITED);
    pass(s); on_history_updated(s); on_plan_written(s); on_denoised(s); on_coverage_rendered(s, 2);
    const PreviewState before = s;
    on_edit_influence_changed(s, true);
    expect(s.influence_on && influence_in_effect(s), "kappa > 0 on an edited handle: the plane follows the motion plane");
    expect(!s.guides_ok && !s.motion_ok && !s.plan_ok && !s.hist_ok && !s.denoised_ok, "a new kappa: motion plane, guides, plan, temporal image and denoised image stale");
    expect(s.acc_samples == before.acc_samples && s.acc_mode == before.acc_mode && s.acc_gen == before.acc_gen, "... the accumulation stays");
    expect(s.hist_base_ok && s.scene_edited && motion_in_effect(s), "... the base stays and motion stays in effect");
    expect(s.rng_ready && s.have_camera && s.scene && s.coverage_ok && s.coverage_grid == 2 && s.nranks == before.nranks, "... camera, scene, RNG states and coverage layers stay");
    expect(has(need_edit_influence(s, READ), PREVIEW_E_STATE, READ, "no influence plane"), "on, but the planes are stale");
    on_guides_rendered(s);
    expect(s.motion_ok && need_edit_influence(s, READ).code == 0, "guides rendered with the knob on bring the plane");
    on_edit_influence_changed(s, false);
    expect(!s.influence_on && !s.guides_ok && !s.motion_ok, "back to 0: the faded motion plane is stale");
    on_guides_rendered(s);
    expect(s.motion_ok && need_motion(s, "rtiow_read_scene_motion").code == 0, "... the motion plane comes back with the guides");
    expect(has(need_edit_influence(s, READ), PREVIEW_E_STATE, READ, "edit influence is off"), "... and no influence plane is made while the knob is off");
    // the knob survives every other event
    void (*const events[])(PreviewState&) = {on_set_scene, on_scene_edited, on_commit, on_history_reset, on_accumulation_reset, on_guide_mode_changed,
                                            [](PreviewState& t) { on_set_camera(t, true); }, [](PreviewState& t) { on_set_shard(t, 2); }};
    for (auto event : events) {
        PreviewState t = after(EDITED);
        on_edit_influence_changed(t, true);
        event(t);
        expect(t.influence_on, "the knob survives set_scene, edit_scene, commit, history reset, accumulation reset, guide mode, set_camera and set_shard");
    }
    // what ends motion ends the plane
    void (*const ends[])(PreviewState&) = {on_commit, on_history_reset, on_set_scene, [](PreviewState& t) { on_set_shard(t, 2); }};
    for (auto event : ends) {
        PreviewState t = after(EDITED);
        on_edit_influence_changed(t, true); on_guides_rendered(t);
        event(t);
        expect(!influence_in_effect(t) && has(need_edit_influence(t, READ), PREVIEW_E_STATE, READ, "motion is not in effect"), "commit, history reset, set_scene and set_shard end the plane");
    }
    // allowed in every state: on a handle without anything, and on a shard
    s = PreviewState{};
    on_edit_influence_changed(s, true);
    expect(s.influence_on && !s.guides_ok && !influence_in_effect(s), "the knob is recorded on a fresh handle");
    s = after("scene_camera shard rng plain");
    on_edit_influence_changed(s, true);
    expect(s.influence_on && s.nranks == 3 && s.acc_mode == ACC_MODE_PLAIN, "... and on a shard, which keeps its accumulation");
}

void check_rules() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    for (double good : {0.0, 1e-300, 0.5, 1.0, 1e300, inf}) expect(check_edit_influence(SET, good).code == 0, "kappa >= 0 is accepted, +inf too");
    for (double bad : {-1e-300, -1.0, -inf, nan}) expect(has(check_edit_influence(SET, bad), PREVIEW_E_BADARG, SET, "need kappa >= 0"), "negative and NaN are RTIOW_E_BADARG");
    expect(check_edit_influence(SET, -0.0).code == 0, "-0 is 0");
}

}  // namespace

int main() {
    event_rules();
    check_rules();
    for (std::string line; std::getline(std::cin, line);) {
        if (line.empty()) continue;
        const Refusal r = need_edit_influence(after(line.c_str()), READ);
        std::printf("%d | %s\n", r.code, r.text.c_str());
    }
    std::printf("%d edit-influence rule failure(s)\n", failures);
    return failures ? 1 : 0;
}
