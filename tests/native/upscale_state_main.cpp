// Guided upscaling's share of the preview chain's policy (csrc/library/preview_state.h) on the CPU, with no GPU
// and no library: what makes the upscaled image current and stale -- every event of the chain against upscaled_ok --, what rtiow_upscale
// needs of each source, and its argument checks, asked in the order the entry points in rtiow_hip.hip ask them.  stdout: one "RULE BROKEN"
// line per failure, the count last.  Built by tests/test_upscale_abi.py with ASan + UBSan, run directly.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "preview_state.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what) { if (!ok) { ++failures; std::printf("RULE BROKEN: %s\n", what); } }

const char* const CALL = "rtiow_upscale";
constexpr double INF = std::numeric_limits<double>::infinity();
enum { DENOISED = 0, LINEAR = 1, HISTORY = 2, SOURCES = 3 };

// rtiow_upscale's checks, in its order: arguments, scene and camera, shard, the source, the output's extent.
Refusal upscale(const PreviewState& s, int factor = 2, int source = DENOISED, double sn = 0.3, double sa = 0.1, double sz = 0.5, int use_coverage = 1,
                int64_t W = 64, int64_t rows = 40, int64_t elem = 4) {
    double inv2[3];
    uint64_t bytes = 0;
    const std::vector<Refusal> checks = {
        check_upscale(CALL, factor, 2, 4, source, SOURCES, {sn, sa, sz}, use_coverage, inv2), need_scene(s, CALL), need_unsharded(s, CALL, true),
        source == DENOISED ? need_denoised(s, CALL) : source == LINEAR ? need_chunk(s, CALL, ASKS_SCENE) : need_temporal_image(s, CALL, ASKS_SCENE),
        check_upscale_extent(CALL, factor, W, rows, elem, &bytes)};
    for (const Refusal& r : checks) if (r.code) return r;
    return Refusal{};
}

PreviewState framed() {
    PreviewState s;
    on_set_camera(s, true); on_set_scene(s); on_scene_uploaded(s);
    on_accumulation_reset(s); on_rng_initialised(s);
    return s;
}
PreviewState sampled() { PreviewState s = framed(); on_chunk_begin(s); on_plain_chunk(s, 4); return s; }
PreviewState denoised() { PreviewState s = sampled(); on_guides_rendered(s); on_denoised(s); return s; }
PreviewState updated() { PreviewState s = sampled(); on_guides_rendered(s); on_history_updated(s); return s; }
PreviewState upscaled(int factor = 2) { PreviewState s = denoised(); on_upscaled(s, factor); return s; }
bool has(const Refusal& r, int code, const char* part) { return r.code == code && r.text.find(CALL) == 0 && r.text.find(part) != std::string::npos; }
bool readable(const PreviewState& s) { return need_upscaled(s, "rtiow_read_upscaled").code == 0; }

void staleness_rules() {
    PreviewState s;
    expect(need_upscaled(s, "r").code == PREVIEW_E_STATE && s.upscale_factor == 0, "no upscaled image on a new handle");
    expect(!readable(denoised()), "... nor before the first rtiow_upscale");
    s = upscaled(3);
    expect(readable(s) && s.upscale_factor == 3, "an upscaled image is current and remembers its factor");
    // a finished output: every event but a new frame leaves it alone
    struct Event { const char* name; void (*apply)(PreviewState&); };
    const Event keep[] = {
        {"on_accumulation_reset", on_accumulation_reset}, {"on_guide_mode_changed", on_guide_mode_changed},
        {"on_scene_uploaded", on_scene_uploaded}, {"on_edit_influence_changed", [](PreviewState& t) { on_edit_influence_changed(t, true); }},
        {"on_rng_initialised", on_rng_initialised}, {"on_chunk_begin", on_chunk_begin}, {"on_plain_chunk", [](PreviewState& t) { on_plain_chunk(t, 2); }},
        {"on_adaptive_chunk", on_adaptive_chunk}, {"on_guides_rendered", on_guides_rendered}, {"on_denoised", [](PreviewState& t) { on_denoised(t); }},
        {"on_denoised from the temporal image", [](PreviewState& t) { on_denoised(t, DENOISED_FROM_TEMPORAL); }},
        {"on_coverage_rendered", [](PreviewState& t) { on_coverage_rendered(t, 4); }}, {"on_edges_resolved", on_edges_resolved},
        {"on_history_updated", on_history_updated}, {"on_plan_written", on_plan_written}, {"on_temporal_variance_written", on_temporal_variance_written},
        {"on_history_reset", on_history_reset}, {"on_commit", on_commit}, {"on_upscaled", [](PreviewState& t) { on_upscaled(t, 3); }},
    };
    for (const Event& e : keep) {
        PreviewState t = s;
        e.apply(t);
        if (!(readable(t) && t.upscale_factor == 3)) { ++failures; std::printf("RULE BROKEN: %s must leave the upscaled image current\n", e.name); }
    }
    const Event stale[] = {
        {"on_frame_changed", on_frame_changed}, {"on_set_scene", on_set_scene}, {"on_scene_edited", on_scene_edited},
        {"on_set_camera", [](PreviewState& t) { on_set_camera(t, true); }}, {"on_set_shard", [](PreviewState& t) { on_set_shard(t, 1); }},
        {"on_set_shard to several ranks", [](PreviewState& t) { on_set_shard(t, 3); }},
    };
    for (const Event& e : stale) {
        PreviewState t = s;
        e.apply(t);
        if (!(!readable(t) && t.upscale_factor == 3)) { ++failures; std::printf("RULE BROKEN: %s must make the upscaled image stale and keep its factor\n", e.name); }
    }
    PreviewState t = s;
    on_set_camera(t, false);
    expect(!readable(t), "no camera, no upscaled image");
    expect(need_upscaled(PreviewState{}, "rtiow_read_upscaled").text.find("rtiow_read_upscaled: no upscaled image") == 0, "the readers' refusal names the call and rtiow_upscale");
}

void source_rules() {
    expect(has(upscale(PreviewState{}), PREVIEW_E_STATE, "before rtiow_set_scene/rtiow_set_camera"), "before scene and camera: refused");
    for (int source : {DENOISED, LINEAR, HISTORY})
        expect(has(upscale(PreviewState{}, 2, source), PREVIEW_E_STATE, "before rtiow_set_scene/rtiow_set_camera"), "... whatever the source");
    PreviewState s = framed();
    expect(has(upscale(s, 2, DENOISED), PREVIEW_E_STATE, "before rtiow_denoise"), "DENOISED before a filter: refused");
    expect(has(upscale(s, 2, LINEAR), PREVIEW_E_STATE, "no chunk since the last reset"), "LINEAR without a chunk: refused");
    expect(has(upscale(s, 2, HISTORY), PREVIEW_E_STATE, "no temporal image"), "HISTORY without a temporal image: refused");
    s = sampled();
    expect(upscale(s, 2, LINEAR).code == 0 && upscale(s, 2, DENOISED).code == PREVIEW_E_STATE && upscale(s, 2, HISTORY).code == PREVIEW_E_STATE, "a chunk serves LINEAR alone");
    on_accumulation_reset(s);
    expect(has(upscale(s, 2, LINEAR), PREVIEW_E_STATE, "no chunk"), "a reset takes LINEAR's colour away");
    s = denoised();
    expect(upscale(s, 2, DENOISED).code == 0 && upscale(s, 3, DENOISED, INF, INF, INF, 0).code == 0, "a filtered image can be upscaled");
    on_edges_resolved(s);
    expect(upscale(s, 2, DENOISED).code == 0, "... and so can a resolved one");
    on_guide_mode_changed(s);
    expect(has(upscale(s, 2, DENOISED), PREVIEW_E_STATE, "before rtiow_denoise") && upscale(s, 2, LINEAR).code == 0, "a new guide mode leaves no denoised image, but the accumulation");
    s = updated();
    expect(upscale(s, 4, HISTORY).code == 0, "a temporal image can be upscaled");
    on_commit(s);
    expect(has(upscale(s, 4, HISTORY), PREVIEW_E_STATE, "no temporal image"), "... but not after the commit took it");
    s = updated(); on_history_reset(s);
    expect(has(upscale(s, 4, HISTORY), PREVIEW_E_STATE, "no temporal image"), "... or after a history reset");
    // a sharded handle is refused as such, before its source is asked for
    s = denoised(); on_set_shard(s, 3);
    for (int source : {DENOISED, LINEAR, HISTORY}) expect(has(upscale(s, 2, source), PREVIEW_E_STATE, "not on a sharded handle"), "a sharded handle is refused as such");
    // coverage and guides are not preconditions: the call renders them
    s = denoised(); s.coverage_ok = false;
    expect(upscale(s, 2, DENOISED, 0.3, 0.1, 0.5, 1).code == 0 && coverage_grid_or_default(s) == 4, "stale layers are rendered by the call, 4 x 4 before any");
}

void argument_rules() {
    const double nan = std::nan("");
    const PreviewState s = denoised();
    for (const PreviewState& t : {PreviewState{}, s}) {      // arguments come first, whatever the state
        for (int factor : {-1, 0, 1, 5, 8, 100}) expect(has(upscale(t, factor), PREVIEW_E_BADARG, "factor must be 2..4"), "factor outside 2..4");
        for (int source : {-1, 3, 7}) expect(has(upscale(t, 2, source), PREVIEW_E_BADARG, "unknown source"), "source outside 0..2");
        for (double bad : {0.0, -1.0, nan, -INF}) {
            expect(has(upscale(t, 2, DENOISED, bad), PREVIEW_E_BADARG, "sigma"), "sigma_normal <= 0 or NaN");
            expect(has(upscale(t, 2, DENOISED, 0.3, bad), PREVIEW_E_BADARG, "sigma"), "sigma_albedo <= 0 or NaN");
            expect(has(upscale(t, 2, DENOISED, 0.3, 0.1, bad), PREVIEW_E_BADARG, "sigma"), "sigma_depth <= 0 or NaN");
        }
        for (int flag : {-1, 2, 16}) expect(has(upscale(t, 2, DENOISED, 0.3, 0.1, 0.5, flag), PREVIEW_E_BADARG, "use_coverage must be 0 or 1"), "use_coverage not 0 or 1");
        // the first bad argument in the order factor, source, sigmas, flag decides the text
        expect(has(upscale(t, 9, 9, -1.0, 0.1, 0.5, 9), PREVIEW_E_BADARG, "factor"), "factor is asked first");
        expect(has(upscale(t, 2, 9, -1.0, 0.1, 0.5, 9), PREVIEW_E_BADARG, "source"), "then the source");
        expect(has(upscale(t, 2, 1, -1.0, 0.1, 0.5, 9), PREVIEW_E_BADARG, "sigma"), "then the sigmas");
    }
    for (int factor : {2, 3, 4}) for (int flag : {0, 1}) expect(upscale(s, factor, DENOISED, INF, INF, INF, flag).code == 0, "factors 2..4, +inf everywhere and both flags are accepted");
    double inv2[3] = {-1, -1, -1};
    expect(check_upscale(CALL, 2, 2, 4, 0, 3, {0.5, INF, 0.25}, 0, inv2).code == 0 && inv2[0] == 4.0 && inv2[1] == 0.0 && inv2[2] == 16.0, "inv2 = 1 / sigma^2; +inf turns the term off");
    // the extent comes last, behind the state: width and height in the kernel's ints, then its tile count
    expect(has(upscale(PreviewState{}, 4, DENOISED, 0.3, 0.1, 0.5, 1, 1ll << 30, 1), PREVIEW_E_STATE, "before rtiow_set_scene"), "the state is asked before the extent");
    expect(has(upscale(s, 4, DENOISED, 0.3, 0.1, 0.5, 1, 1ll << 30, 1), PREVIEW_E_BADARG, "wider or higher"), "an output wider than an int's pixels");
    expect(has(upscale(s, 2, DENOISED, 0.3, 0.1, 0.5, 1, 1, 0x7fffffffll), PREVIEW_E_BADARG, "wider or higher"), "... or higher");
    expect(has(upscale(s, 4, DENOISED, 0.3, 0.1, 0.5, 1, 1 << 19, 1 << 19), PREVIEW_E_BADARG, "8 x 8 tiles"), "an output of 2^36 tiles");
    expect(has(upscale(s, 2, DENOISED, 0.3, 0.1, 0.5, 1, 1 << 18, 1 << 18), PREVIEW_E_BADARG, "8 x 8 tiles"), "2^32 tiles");
    uint64_t bytes = 0;
    expect(check_upscale_extent(CALL, 2, 1920, 1080, 4, &bytes).code == 0 && bytes == 3840ull * 2160 * 12, "3840 x 2160 fp32: its bytes");
    expect(check_upscale_extent(CALL, 3, 1, 1, 8, &bytes).code == 0 && bytes == 9ull * 24, "1 x 1 at F = 3 in fp64: 216 bytes");
    expect(check_upscale_extent(CALL, 4, 46340, 46340, 8, &bytes).code == 0 && bytes == 185360ull * 185360 * 24, "the largest square frame rtiow_set_camera takes fits at F = 4");
    expect(check_upscale_extent(CALL, 2, 0x3ffffffcll, 1, 4, &bytes).code == 0 && check_upscale_extent(CALL, 2, 0x3ffffffdll, 1, 4, &bytes).code == PREVIEW_E_BADARG,
           "the width limit is 2^31 - 8 output pixels");
    expect(check_upscale_extent(CALL, 2, 0, 0, 4, &bytes).code == 0 && bytes == 0, "an empty frame has no bytes");
}

}  // namespace

int main() {
    staleness_rules();
    source_rules();
    argument_rules();
    std::printf("%d upscale rule failure(s)\n", failures);
    return failures ? 1 : 0;
}
