// The edge resolve's share of the preview chain's policy (csrc/library/preview_state.h) on the CPU, with no
// GPU and no library: what makes the coverage layers current and stale, what rtiow_resolve_edges needs of the denoised image, and its
// argument checks, asked in the order the entry points in rtiow_hip.hip ask them.  stdout: one "RULE BROKEN" line per failure, the count
// last.  Built by tests/test_edge_resolve_abi.py with ASan + UBSan, run directly.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "preview_state.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what) { if (!ok) { ++failures; std::printf("RULE BROKEN: %s\n", what); } }

const char* const CALL = "rtiow_resolve_edges";
constexpr double INF = std::numeric_limits<double>::infinity();

// rtiow_resolve_edges's checks, in its order: arguments, then state.
Refusal resolve(const PreviewState& s, int radius = 2, double sigma_normal = 0.3, double sigma_depth = 0.5, double prior = 8.0) {
    double inv2[2];
    const std::vector<Refusal> checks = {check_edge_resolve(CALL, radius, 3, {sigma_normal, sigma_depth}, prior, inv2), need_unsharded(s, CALL, true),
                                         need_denoised(s, CALL), need_unresolved(s, CALL), need_denoised_source(s, CALL), need_denoised_accumulation(s, CALL)};
    for (const Refusal& r : checks) if (r.code) return r;
    return Refusal{};
}

PreviewState sampled() {
    PreviewState s;
    on_set_camera(s, true); on_set_scene(s); on_scene_uploaded(s);
    on_accumulation_reset(s); on_rng_initialised(s);
    on_chunk_begin(s); on_plain_chunk(s, 4);
    return s;
}
PreviewState denoised() { PreviewState s = sampled(); on_guides_rendered(s); on_denoised(s); return s; }
PreviewState denoised_from_history() {
    PreviewState s = sampled();
    on_guides_rendered(s); on_history_updated(s); on_denoised(s, DENOISED_FROM_TEMPORAL);
    return s;
}
bool has(const Refusal& r, int code, const char* part) { return r.code == code && r.text.find(CALL) == 0 && r.text.find(part) != std::string::npos; }

void coverage_rules() {
    PreviewState s;
    expect(need_coverage(s, "rtiow_read_coverage").code == PREVIEW_E_STATE && coverage_grid_or_default(s) == 4, "no layers on a new handle; the resolve would render 4 x 4");
    expect(check_coverage_grid("c", 2).code == 0 && check_coverage_grid("c", 4).code == 0, "2 and 4 sub-samples a side are accepted");
    for (int g : {-1, 0, 1, 3, 5, 8, 16}) expect(check_coverage_grid("c", g).code == PREVIEW_E_BADARG, "every other lattice is refused");
    expect(need_scene(s, "rtiow_render_coverage").code == PREVIEW_E_STATE, "rtiow_render_coverage needs scene and camera");
    s = sampled();
    expect(need_scene(s, "rtiow_render_coverage").code == 0, "... and nothing else");
    on_coverage_rendered(s, 2);
    expect(need_coverage(s, "c").code == 0 && coverage_grid_or_default(s) == 2, "rendered layers are current and remember their lattice");
    // they survive chunks, resets, the guide mode, updates and commits ...
    on_chunk_begin(s); on_plain_chunk(s, 1); on_accumulation_reset(s); on_rng_initialised(s); on_guide_mode_changed(s);
    on_guides_rendered(s); on_history_updated(s); on_commit(s); on_history_reset(s); on_denoised(s); on_edges_resolved(s);
    expect(need_coverage(s, "c").code == 0, "the layers survive chunks, resets, rtiow_set_guide_mode, updates, commits, filters and resolves");
    // ... and go stale with scene, camera and shard, keeping their lattice for the next render
    void (*const stale[])(PreviewState&) = {on_set_scene, [](PreviewState& t) { on_set_camera(t, true); }, [](PreviewState& t) { on_set_shard(t, 2); }};
    for (auto event : stale) {
        PreviewState t = s;
        event(t);
        expect(need_coverage(t, "c").code == PREVIEW_E_STATE && coverage_grid_or_default(t) == 2, "set_scene, set_camera and set_shard make the layers stale");
    }
    PreviewState t = s;
    on_set_camera(t, false);
    expect(need_coverage(t, "c").code == PREVIEW_E_STATE, "no camera, no layers");
}

void resolve_rules() {
    expect(has(resolve(sampled()), PREVIEW_E_STATE, "before rtiow_denoise"), "no denoised image: refused");
    PreviewState s = denoised();
    expect(resolve(s).code == 0 && s.denoised_from == DENOISED_FROM_ACCUMULATION && !s.resolved, "a filtered accumulation can be resolved");
    on_edges_resolved(s);
    expect(has(resolve(s), PREVIEW_E_STATE, "already resolved"), "a second resolve is refused");
    on_denoised(s);
    expect(resolve(s).code == 0, "... until a filter has run again");
    // a chunk or a reset since the filter
    s = denoised(); on_chunk_begin(s); on_plain_chunk(s, 1);
    expect(has(resolve(s), PREVIEW_E_STATE, "a chunk or a reset since the filter"), "a chunk after the filter: refused");
    s = denoised(); on_accumulation_reset(s);
    expect(has(resolve(s), PREVIEW_E_STATE, "a chunk or a reset since the filter"), "a reset after the filter: refused");
    // the temporal image
    s = denoised_from_history();
    expect(resolve(s).code == 0 && s.denoised_from == DENOISED_FROM_TEMPORAL, "a filtered temporal image can be resolved");
    on_commit(s);
    expect(has(resolve(s), PREVIEW_E_STATE, "resolve before rtiow_history_commit"), "... but not after the commit took the temporal image");
    s = denoised_from_history(); on_history_reset(s);
    expect(has(resolve(s), PREVIEW_E_STATE, "resolve before rtiow_history_commit"), "... or after a history reset");
    s = denoised(); on_guides_rendered(s); on_history_updated(s); on_commit(s);
    expect(resolve(s).code == 0, "a commit does not matter to a filtered accumulation");
    // sharded handles, new frames, a new guide mode
    s = denoised(); on_set_shard(s, 2);
    expect(has(resolve(s), PREVIEW_E_STATE, "not on a sharded handle"), "a sharded handle is refused as such");
    s = denoised(); on_set_camera(s, true);
    expect(has(resolve(s), PREVIEW_E_STATE, "before rtiow_denoise"), "a new camera leaves nothing to resolve");
    s = denoised(); on_guide_mode_changed(s);
    expect(has(resolve(s), PREVIEW_E_STATE, "before rtiow_denoise"), "a new guide mode leaves nothing to resolve");
    // arguments come first, whatever the state
    const double nan = std::nan("");
    s = denoised();
    for (const PreviewState& t : {PreviewState{}, s}) {
        for (int radius : {-1, 0, 4, 100}) expect(has(resolve(t, radius), PREVIEW_E_BADARG, "radius in 1..3"), "radius outside 1..3");
        for (double bad : {0.0, -1.0, nan, -INF}) {
            expect(has(resolve(t, 2, bad), PREVIEW_E_BADARG, "sigma"), "sigma_normal <= 0 or NaN");
            expect(has(resolve(t, 2, 0.3, bad), PREVIEW_E_BADARG, "sigma"), "sigma_depth <= 0 or NaN");
            expect(has(resolve(t, 2, 0.3, 0.5, bad), PREVIEW_E_BADARG, "prior > 0"), "prior <= 0 or NaN");
        }
    }
    for (int radius : {1, 2, 3}) expect(resolve(s, radius, INF, INF, INF).code == 0, "radius 1..3 and +inf everywhere are accepted");
    double inv2[2] = {-1, -1};
    expect(check_edge_resolve(CALL, 1, 3, {0.5, INF}, 1.0, inv2).code == 0 && inv2[0] == 4.0 && inv2[1] == 0.0, "inv2 = 1 / sigma^2; +inf turns the term off");
}

}  // namespace

int main() {
    coverage_rules();
    resolve_rules();
    std::printf("%d edge-resolve rule failure(s)\n", failures);
    return failures ? 1 : 0;
}
