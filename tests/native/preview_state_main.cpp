// The policy of the preview chain (csrc/library/preview_state.h) on the CPU, with no GPU and no library: a reader of the header.
// stdin: lines of "steps | call | name=value ..." (tests/preview_refusals.py: program_line); for each, a fresh PreviewState goes through
// the steps' events and the call's checks are asked in the order its entry point in rtiow_hip.hip asks them; stdout: "code | message".
// Before that, the invalidation rules tests/test_history.py::test_states_and_error_codes states in its comments are checked on the
// events alone; the last line of stdout counts their failures.  Built by tests/test_preview_state.py with ASan + UBSan, run directly.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "preview_state.h"

namespace {

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
    else { std::fprintf(stderr, "unknown step %s\n", name.c_str()); std::exit(2); }
}

using Args = std::map<std::string, double>;

// The first refusal of `checks`, or none.
Refusal first(std::vector<Refusal> checks) {
    for (Refusal& r : checks) if (r.code) return r;
    return Refusal{};
}

Refusal ask(const PreviewState& s, const std::string& name, Args& a) {
    const char* c = name.c_str();
    const double sigma[4] = {a["sigma_first"], a["sigma_normal"], a["sigma_albedo"], a["sigma_depth"]};
    double inv2[4];
    auto filter = [&](int levels) { return check_filter(c, levels, sigma, inv2); };
    auto tolerances = [&] { return check_history_tolerances(c, a["depth_tol"], a["normal_cos"], a["max_history"]); };
    if (name == "rtiow_read_linear") return need_chunk(s, c, ASKS_CAMERA);
    if (name == "rtiow_render_guides") return need_scene(s, c);
    if (name == "rtiow_read_guides" || name == "rtiow_read_filter_guides") return need_guides(s, c);
    if (name == "rtiow_denoise") return first({filter((int)a["levels"]), need_chunk(s, c, ASKS_SCENE), need_unsharded(s, c, true)});
    if (name == "rtiow_read_denoised" || name == "rtiow_denoised_device_ptr") return need_denoised(s, c);
    if (name == "rtiow_read_variance") return need_adaptive_chunk(s, c, ASKS_CAMERA);
    if (name == "rtiow_denoise_variance") return first({filter((int)a["levels"]), need_adaptive_chunk(s, c, ASKS_SCENE), need_unsharded(s, c, true)});
    if (name == "rtiow_history_reset") return need_unsharded(s, c, false);
    if (name == "rtiow_history_update") return first({tolerances(), need_chunk(s, c, ASKS_SCENE), need_unsharded(s, c, true)});
    if (name == "rtiow_history_update_clipped")
        return first({tolerances(), check_radius(c, "clip_radius", (int)a["clip_radius"], 3, a["clip_gamma"] >= 0, ", clip_gamma >= 0 (+inf: no clamp)"),
                      need_chunk(s, c, ASKS_SCENE), need_unsharded(s, c, true)});
    if (name == "rtiow_history_plan") return first({tolerances(), need_scene(s, c), need_unsharded(s, c, true)});
    if (name == "rtiow_read_history_plan") return first({need_unsharded(s, c, false), need_plan(s, c)});
    if (name == "rtiow_accumulate_budget") return first({need_scene(s, c), need_rng(s, c), need_no_chunk_of(s, c, ACC_MODE_PLAIN), need_plan(s, c)});
    if (name == "rtiow_history_commit" || name == "rtiow_read_history" || name == "rtiow_history_device_ptr")
        return first({need_unsharded(s, c, false), need_temporal_image(s, c, ASKS_CAMERA)});
    if (name == "rtiow_history_commit_filtered") return first({filter(1), need_unsharded(s, c, false), need_temporal_image(s, c, ASKS_SCENE)});
    if (name == "rtiow_read_history_base") return first({need_unsharded(s, c, false), need_base(s, c)});
    if (name == "rtiow_denoise_history") return first({filter((int)a["levels"]), need_unsharded(s, c, true), need_temporal_image(s, c, ASKS_SCENE)});
    if (name == "rtiow_denoise_history_variance")
        return first({filter((int)a["levels"]), check_radius(c, "variance_radius", (int)a["variance_radius"], 3), need_unsharded(s, c, true),
                      need_temporal_image(s, c, ASKS_SCENE), need_same_accumulation(s, c)});
    if (name == "rtiow_read_history_variance") return first({need_unsharded(s, c, false), need_temporal_variance(s, c)});
    if (name == "rtiow_set_guide_mode") return Refusal{};                    // its checks are its own; it refuses no state
    std::fprintf(stderr, "unknown call %s\n", c);
    std::exit(2);
}

// ---- the invalidation rules, on the events alone
int failures = 0;
void expect(bool ok, const char* what) { if (!ok) { ++failures; std::printf("RULE BROKEN: %s\n", what); } }

PreviewState updated() {
    PreviewState s;
    for (const char* n : {"scene_camera", "rng", "plain", "update"}) step(s, n);
    return s;
}
PreviewState committed() { PreviewState s = updated(); on_commit(s); return s; }

void rules() {
    PreviewState s = updated();
    expect(s.hist_ok && s.guides_ok && s.hist_gen == s.acc_gen && !s.hist_var_ok, "an update leaves a temporal image of this accumulation and no V^0");
    // the temporal image survives a further chunk, an accumulation reset and init_rng ...
    step(s, "plain"); on_accumulation_reset(s); step(s, "rng");
    expect(s.hist_ok, "the temporal image survives a chunk, an accumulation reset and init_rng");
    expect(s.hist_gen != s.acc_gen && s.acc_mode == ACC_MODE_NONE && s.acc_samples == 0, "... but is no longer of this accumulation, which is empty");
    // ... and goes stale on commit, set_camera, set_scene, set_shard and history_reset
    void (*const stale[])(PreviewState&) = {on_commit, [](PreviewState& t) { on_set_camera(t, true); }, on_set_scene, [](PreviewState& t) { on_set_shard(t, 1); }, on_history_reset};
    for (auto event : stale) { s = updated(); on_plan_written(s); event(s); expect(!s.hist_ok && !s.plan_ok, "commit, set_camera, set_scene, set_shard and history_reset leave no temporal image and no plan"); }
    // the base survives set_camera, reset_accumulation and init_rng; set_scene, set_shard and history_reset empty it
    s = committed(); on_set_camera(s, true); on_accumulation_reset(s); step(s, "rng");
    expect(s.hist_base_ok, "the base survives set_camera, an accumulation reset and init_rng");
    void (*const empties[])(PreviewState&) = {on_set_scene, [](PreviewState& t) { on_set_shard(t, 1); }, on_history_reset};
    for (auto event : empties) { s = committed(); event(s); expect(!s.hist_base_ok, "set_scene, set_shard and history_reset empty the base"); }
    // what else the set_* calls ask for again, and what they keep
    s = updated(); on_set_camera(s, true);
    expect(!s.rng_ready && !s.guides_ok && !s.denoised_ok && s.acc_mode == ACC_MODE_NONE && s.scene, "a new camera asks for RNG states, guides and samples, and keeps the scene");
    s = updated(); on_set_scene(s);
    expect(s.rng_ready && s.have_camera && !s.guides_ok && s.acc_mode == ACC_MODE_NONE, "a new scene keeps the camera and the RNG states");
    s = updated(); on_set_camera(s, false);
    expect(!s.have_camera && s.hist_ok && s.rng_ready, "a camera of a bad size takes the camera away and nothing else");
    s = committed();
    expect(!s.guides_ok && s.hist_base_ok, "a commit takes the guides with it");
    s = updated(); on_denoised(s); on_guide_mode_changed(s);
    expect(!s.guides_ok && !s.denoised_ok && s.hist_ok, "a new guide mode makes the guides and the denoised image stale and nothing else");
}

}  // namespace

int main() {
    rules();
    std::string line;
    while (std::getline(std::cin, line)) {
        const size_t bar1 = line.find(" | "), bar2 = line.find(" | ", bar1 + 3);
        if (bar1 == std::string::npos || bar2 == std::string::npos) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        PreviewState s;
        std::istringstream steps(line.substr(0, bar1)), args(line.substr(bar2 + 3));
        for (std::string w; steps >> w;) step(s, w);
        Args a;
        for (std::string w; args >> w;) a[w.substr(0, w.find('='))] = std::strtod(w.c_str() + w.find('=') + 1, nullptr);
        const Refusal r = ask(s, line.substr(bar1 + 3, bar2 - bar1 - 3), a);
        std::printf("%d | %s\n", r.code, r.text.c_str());
    }
    std::printf("%d preview-state rule failure(s)\n", failures);
    return failures ? 1 : 0;
}
