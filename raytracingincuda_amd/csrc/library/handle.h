// handle.h -- rtiow_handle_s, the device buffers it owns (DeviceBuffer) and the small helpers every host file uses (error text, frame size,
// shard rows, operand-range checks, make_params); what of the preview chain is current is preview_state.h's
// Host side of librtiow_hip.so; part of the single translation unit rtiow_hip.hip (internal linkage).
#pragma once
#include "../device/params.h"
#include "order_key.h"
#include "launch_plan.h"
#include "preview_state.h"
#include "grid_plan.h"

// A device allocation owned by the handle or by one call: freed when it goes out of scope.  ensure() grows it to at least `bytes`
// and never shrinks it; the old allocation is freed before the new one is made, so its contents are lost.
template <class E = unsigned char>
class DeviceBuffer {
  public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : ptr_(o.ptr_), bytes_(o.bytes_) { o.ptr_ = nullptr; o.bytes_ = 0; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { std::swap(ptr_, o.ptr_); std::swap(bytes_, o.bytes_); return *this; }
    ~DeviceBuffer() { (void)reset(); }
    hipError_t ensure(size_t bytes) {
        if (ptr_ && bytes_ >= bytes) return hipSuccess;
        if (hipError_t e = reset()) return e;
        if (hipError_t e = hipMalloc((void**)&ptr_, bytes)) return e;
        bytes_ = bytes;
        return hipSuccess;
    }
    hipError_t reset() {
        if (!ptr_) return hipSuccess;
        const hipError_t e = hipFree(ptr_);
        ptr_ = nullptr; bytes_ = 0;
        return e;
    }
    operator E*() const { return ptr_; }
    size_t bytes() const { return bytes_; }
    template <class U> U* as() const { return (U*)ptr_; }       // buffers whose element type is the handle's precision
  private:
    E* ptr_ = nullptr;
    size_t bytes_ = 0;
};

static_assert(PREVIEW_E_BADARG == RTIOW_E_BADARG && PREVIEW_E_STATE == RTIOW_E_STATE, "preview_state.h refuses in the C-ABI's codes");

struct rtiow_handle_s {
    int device = 0;
    int precision = 32;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_a = nullptr, ev_b = nullptr, ev_c = nullptr;   // ev_a: prepass done, ev_b: main launch starts, ev_c: main launch done (place_pixels_kernel follows)
    bool time_phases = false;
    bool render_pending = false;                  // rtiow_render_async recorded its stop event, rtiow_render_wait has not read it yet
    std::string err;

    // scene
    int n = 0, n_padded = 0;
    DeviceBuffer<> geom_a, shade_tbl;
    DeviceBuffer<float> geom_s;                   // screening table (built lazily at the first render of a scene)
    std::vector<double> host_cr;                  // compact {cx,cy,cz,r} kept for building it
    bool screen_dirty = true;
    double ctr[3] = {0, 0, 0}, omax2 = 0;
    // uniform grid over the small spheres (RTIOW_SCENE_GRID; built with the screening table)
    DeviceBuffer<> grid_blob;
    GridParams grid{};                            // offsets are relative to the blob until layout_lds places it in LDS
    GridBlobOffsets grid_at;                      // where the blob's sections start
    int grid_direct = 0, grid_registered = 0;
    // what of the preview chain is current: every rule that reads or writes it is in preview_state.h
    PreviewState preview;
    // camera (preview.have_camera)
    rtiow_camera_f32 cam32{};
    rtiow_camera_f64 cam64{};
    // shard (preview.nranks)
    int rank = 0, strip_rows = 8;
    int local_rows = 0;
    // rng
    DeviceBuffer<uint32_t> rng;
    DeviceBuffer<uint32_t> rng_low_table;         // J^lo * s0 for lo < 2^XW_LOW_BITS (xw_low_table_kernel), per rtiow_init_rng
    DeviceBuffer<uint32_t> jump;
    int jump_count = 0;                           // matrices of `jump` that are filled: enough for the bits of the largest pixel index so far
    // framebuffer: allocated here (freed by rtiow_destroy) or the caller's (fb_external: rtiow_bind_framebuffer, never freed here)
    void* fb = nullptr;
    size_t fb_bytes = 0;
    bool fb_external = false;
    // knobs / stats
    int scene_source = RTIOW_SCENE_GRID;
    int schedule = RTIOW_SCHED_SORTED;
    DeviceBuffer<> mid;                           // SCHED_SORTED: MidState records parked between the launches
    DeviceBuffer<uint32_t> cost;
    DeviceBuffer<> levels;                        // rtiow_read_levels: one byte per channel + an 8-byte NaN counter behind them
    DeviceBuffer<uint32_t> cost_rank;             // the smoothed cost the sort ranks by
    DeviceBuffer<int> order;
    DeviceBuffer<int> slot_of;                    // SCHED_SORTED: pixel -> slot (the inverse of `order`)
    DeviceBuffer<> staged;                        // SCHED_SORTED: finished pixels in slot order (place_pixels_kernel writes the image)
    DeviceBuffer<unsigned> sort_scratch;
    // SCHED_SORTED: the order a two-phase render left in `order` / `slot_of` is carried to the next renders of the same frame, which then
    // launch once from sample 0 (order_key.h).  Cleared by whatever changes the cost map (scene, camera, shard) or
    // overwrites the two buffers (counting runs, rtiow_accumulate, rtiow_accumulate_adaptive); launch_render compares the key itself.
    CarriedOrder carried;
    OrderRecord order_rec;                        // what `order` holds now (launch_plan.h: plan_ranking_record, plan_adaptive_record)
    bool order_reuse = true;                      // RTIOW_ORDER_REUSE=0 at rtiow_create: every sorted render ranks again (A/B runs, studies)
    // progressive rendering (rtiow_accumulate): the per-pixel MidState records of the last chunk (two buffers, ping-pong: acc_mid[acc_cur]
    // holds them) and the segments each pixel ran in that chunk (the next chunk's ranking)
    int acc_cur = 0;
    DeviceBuffer<> acc_mid[2];
    DeviceBuffer<uint32_t> acc_cost;
    // adaptive progressive rendering (rtiow_accumulate_adaptive): the per-pixel count and relative error the last adaptive chunk left,
    // and {active pixels, largest count} of that chunk
    DeviceBuffer<int32_t> adapt_counts;
    DeviceBuffer<float> adapt_err;
    DeviceBuffer<unsigned> adapt_ctr;
    // denoised previews (rtiow_render_guides / rtiow_read_linear / rtiow_denoise), all allocated at first use: the guides ({normal, depth}
    // and {albedo, 0}, 4 T per pixel each), the linear image, the filter's two ping-pong colour buffers and its gamma-encoded output
    DeviceBuffer<> guide_nd, guide_alb;
    DeviceBuffer<> linear;
    DeviceBuffer<> dn_tmp[2];
    DeviceBuffer<> denoised;
    // filter guides (rtiow_set_guide_mode): what the three filters steer by.  RTIOW_GUIDES_FIRST_HIT: guide_nd / guide_alb themselves.
    // RTIOW_GUIDES_SPECULAR: the specular chain's {normal', depth'} and {albedo', (T)bounces}, 4 T per pixel each, allocated at first use
    // and written wherever the first-hit guides are.  The knob survives set_scene / _camera / _shard.
    int guide_mode = RTIOW_GUIDES_FIRST_HIT;
    int guide_max_bounces = 0;
    double guide_max_fuzz = 0;
    DeviceBuffer<> chain_nd, chain_alb;
    // lens-sampled filter guides (rtiow_set_guide_lens): lens points per side of the lattice, 0 (off), 2 or 4.  While the lattice is in
    // effect (lens_in_effect) the second pair of buffers holds the lens guides in either guide mode.  The knob survives set_scene / _camera / _shard.
    int guide_lens = 0;
    // variance-guided denoising (rtiow_read_variance / rtiow_denoise_variance), allocated at first use: the variance plane of the adaptive
    // accumulation (1 T per pixel, rewritten by every call) and the filter's two ping-pong variance planes
    DeviceBuffer<> variance;
    DeviceBuffer<> dn_var[2];
    // temporal history (rtiow_history_*), allocated at first use.  The base: what rtiow_history_commit kept of an earlier camera --
    // {H.rgb, M} and {normal', depth'}, 4 T per pixel each, and that camera.  The temporal image of the current camera: {C.rgb, M},
    // 4 T per pixel, and its colour alone as the 3-T plane the filter reads.  hist_ctr: the reprojected-pixel count and, behind it, the
    // count of those the clamp changed.
    DeviceBuffer<> hist_base_hm, hist_base_nd;
    rtiow_camera_f32 hist_cam32{};
    rtiow_camera_f64 hist_cam64{};
    DeviceBuffer<> hist_cm, hist_rgb;
    DeviceBuffer<unsigned> hist_ctr;
    // variance-guided filtering of the temporal image (rtiow_denoise_history_variance), allocated at first use: its level-0 variance
    // plane V^0, 1 T per pixel, which the filter's ping-pong leaves alone
    DeviceBuffer<> hist_var;
    // history-guided sample budgets (rtiow_history_plan / rtiow_accumulate_budget), allocated at first use: the plan, i.e. the history
    // length m every pixel of the current camera will carry, 1 T per pixel, and its count of pixels with m > 0
    DeviceBuffer<> plan_m;
    DeviceBuffer<unsigned> plan_ctr;
    // edge resolve (rtiow_render_coverage / rtiow_resolve_edges), allocated at first use: the coverage layers of every local pixel --
    // {id_0, id_1, c_0, c_1} as four int32 and {n_l, z_l}, 4 T, for l = 0, 1 -- and the count of pixels the last resolve rewrote.  The
    // buffers never change owners.
    DeviceBuffer<> cov_ic, cov_nz;
    DeviceBuffer<unsigned> edge_ctr;
    // scene edits that keep the history (rtiow_edit_scene).  On the host, as the bits of T and per kept sphere: the tables of the current
    // scene (scene_geom: {C, r}, 4 T; scene_mat: type as int32, then the 4 T of albedo_fuzz and refraction_index), written by every
    // upload, and the snapshot of them both commits take (snap_geom, snap_mat), which goes wherever the base goes.  scene_slots and
    // scene_kept: the n and the kept pattern of the last upload, which an edit must repeat.  On the device, allocated at first use: the
    // per-sphere table of the motion plane ({C', r'} and the MOTION_* flags, written by rtiow_edit_scene) and the plane itself ({Q, carry}
    // as 4 T and the id per local pixel, written wherever the guides are while motion is in effect).
    std::vector<unsigned char> scene_geom, scene_mat, snap_geom, snap_mat, scene_kept;
    int scene_slots = 0;
    // rtiow_edit_scene_mapped: per kept sphere of the current scene, the number of the sphere it continues among the kept spheres of the
    // snapshot, or -1 (added since).  The identity from both commits, composed by every mapped edit, left alone by rtiow_edit_scene, and
    // gone wherever the snapshot goes; without a base it is empty.
    std::vector<int32_t> from_snapshot;
    DeviceBuffer<> motion_snap, motion_qc;
    DeviceBuffer<int32_t> motion_flags, motion_ids;
    // edit influence (rtiow_set_edit_influence): the knob (0: off; preview.influence_on says whether it is > 0; it survives set_scene /
    // _camera / _shard), the edit list of the last rtiow_edit_scene with motion in effect ({C, r} as 4 T and the owner per entry, written
    // beside motion_snap / motion_flags; edit_entries may be 0) and the influence plane lambda, 1 T per local pixel, written wherever the
    // motion plane is while the knob is on.  All allocated at first use.
    double edit_kappa = 0;
    int edit_entries = 0;
    DeviceBuffer<> edit_list, edit_lambda;
    DeviceBuffer<int32_t> edit_owner;
    // guided upscaling (rtiow_upscale), allocated at first use and regrown for a larger factor: the upscaled image, (F local_rows) x (F W)
    // x 3 T, gamma-encoded, with F = preview.upscale_factor and upscaled_bytes its size; the count of output pixels the share decided
    DeviceBuffer<> upscaled;
    size_t upscaled_bytes = 0;
    DeviceBuffer<unsigned> upscale_ctr;
    // large scenes (rtiow_render_large, rtiow_large.hip): the device grid of the current scene -- blob, its description with offsets
    // relative to the blob, the recentring point and what rtiow_read_large_grid reports -- built at first use after an upload
    // (large_dirty, set by upload_scene)
    DeviceBuffer<> large_blob;
    GridParams large_grid{};
    double large_ctr[3] = {0, 0, 0};
    bool large_dirty = true;
    rtiow_large_grid_info large_info{};
    // volume scenes (rtiow_render_volume, rtiow_volume.hip): the three-axis grid of the current scene, kept beside the device grid in
    // the same form (volume_dirty, set by upload_scene; the recentring point is large_centre's, held here so that either grid may be
    // built without the other)
    DeviceBuffer<> volume_blob;
    GridParams volume_grid{};
    double volume_ctr[3] = {0, 0, 0};
    bool volume_dirty = true;
    rtiow_volume_grid_info volume_info{};
    int waves_per_simd = 0;
    int num_cus = 256;
    int last_count_blocks = 0, last_count_waves_per_block = 0;
    size_t timeline_cap_waves = 0;            // waves the debug timeline buffer holds
    DeviceBuffer<unsigned int> work_counter;      // the persistent hand-out's two slot counters (persistent_setup)
    int warmup_us = 0;                               // RTIOW_CLOCK_WARMUP_US: busy kernel in front of the handle's FIRST timed render (before its start event), see clock_warmup_kernel
    bool warmed = false;
    unsigned long long* clock_stamps = nullptr;      // pinned + mapped host memory, 8 words: {memtime, realtime} x {start, end} of the prepass [0..3] and the main launch [4..7]
    unsigned long long* clock_stamps_dev = nullptr;  // its device address
    unsigned long long* timeline = nullptr;   // debug: set only during rtiow_debug_timeline
    uint32_t* pixel_times = nullptr;          // debug: set only during rtiow_debug_pixel_times
    rtiow_stats stats{};
};

namespace {

size_t elem_size(const rtiow_handle_s* h) { return h->precision == 64 ? 8 : 4; }

int fail(rtiow_handle_s* h, hipError_t e, const char* file, int line) {
    char buf[512];
    // same text the reference's CUDA_SAFE_CALL prints (main.cu:16-17)
    std::snprintf(buf, sizeof buf, "HIP_SAFE_CALL: %s %s %d", hipGetErrorString(e), file, line);
    if (h) h->err = buf;
    return (int)e;
}
int fail_arg(rtiow_handle_s* h, int code, const char* msg) { if (h) h->err = msg; return code; }
// A precondition or argument check of preview_state.h: return its refusal, the text left for rtiow_last_error_string.
#define PREVIEW_TRY(h, check) do { Refusal r_ = (check); if (r_.code) { (h)->err = std::move(r_.text); return r_.code; } } while (0)

#define HIP_TRY(h, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail((h), e_, __FILE__, __LINE__); } while (0)

int compute_local_rows(int H, int rank, int nranks, int strip_rows) {
    int rows = 0;
    const int nstrips = (H + strip_rows - 1) / strip_rows;
    for (int s = rank; s < nstrips; s += nranks) {
        const int r0 = s * strip_rows;
        rows += (r0 + strip_rows <= H) ? strip_rows : (H - r0);
    }
    return rows;
}

int img_w(const rtiow_handle_s* h) { return h->precision == 64 ? h->cam64.img_width : h->cam32.img_width; }
int img_h(const rtiow_handle_s* h) { return h->precision == 64 ? h->cam64.img_height : h->cam32.img_height; }
// The camera in precision T, and f(T()) for the handle's precision: the one place a call picks float or double.
template <class T>
const auto& camera(const rtiow_handle_s* h) {
    if constexpr (sizeof(T) == 4) return h->cam32;
    else return h->cam64;
}
template <class F>
auto by_precision(const rtiow_handle_s* h, F f) { return h->precision == 32 ? f(float()) : f(double()); }

size_t local_pixels(const rtiow_handle_s* h) { return (size_t)img_w(h) * h->local_rows; }
// Is the lens lattice of rtiow_set_guide_lens in effect?  The knob is on and the camera has a lens: the test the render kernels make
// before they sample it.  A function of the knob and the camera alone, and a change of either makes the guides stale, so current guides
// were rendered under the answer given here.
bool lens_in_effect(const rtiow_handle_s* h) { return h->guide_lens > 0 && (h->precision == 64 ? (double)h->cam64.defocus_angle : (double)h->cam32.defocus_angle) > 0; }
// The filter guides live in the second pair of buffers: the specular chain's, or the lens lattice's in either mode.
bool filter_guides_in_second_pair(const rtiow_handle_s* h) { return h->guide_mode == RTIOW_GUIDES_SPECULAR || lens_in_effect(h); }
// The guides the filters read (rtiow_denoise, rtiow_denoise_variance, rtiow_denoise_history): the first-hit buffers themselves, or the
// second pair.  The history launch and the commit's swap use guide_nd whatever the mode.
const DeviceBuffer<>& filter_nd(const rtiow_handle_s* h) { return filter_guides_in_second_pair(h) ? h->chain_nd : h->guide_nd; }
const DeviceBuffer<>& filter_alb(const rtiow_handle_s* h) { return filter_guides_in_second_pair(h) ? h->chain_alb : h->guide_alb; }
size_t image_bytes(const rtiow_handle_s* h) { return local_pixels(h) * 3 * elem_size(h); }          // the local image, 3 T per pixel

int ensure_framebuffer(rtiow_handle_s* h) {
    const size_t need = image_bytes(h);
    if (h->fb_external) {
        if (h->fb_bytes < need) return fail_arg(h, RTIOW_E_BADARG, "bound framebuffer too small");
        return 0;
    }
    if (h->fb && h->fb_bytes >= need) return 0;
    if (h->fb) { HIP_TRY(h, hipFree(h->fb)); h->fb = nullptr; h->fb_bytes = 0; }
    if (need == 0) return 0;
    HIP_TRY(h, hipMalloc(&h->fb, need));
    h->fb_bytes = need;
    return 0;
}

// Can gen_primary take 1/sqrt(|D|^2) without range handling (inv_sqrt_accepted)?  D = pixel sample - lens point:
// the samples lie in the pixel plane (pixel00 + fi du + fj dv, fi in [-0.5, W - 0.5]), the lens points on the
// defocus disk around the centre (|px|, |py| <= 1).  |D| is at most the sum of the extents and at least the
// distance of the lens from the pixel plane; both with room for the fp32 rounding of coordinates up to M.
template <class CAM>
int primary_rays_in_range(const CAM& c) {
    auto v = [](const auto* a) { return std::array<double, 3>{(double)a[0], (double)a[1], (double)a[2]}; };
    auto dot = [](const std::array<double, 3>& a, const std::array<double, 3>& b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    auto len = [&](const std::array<double, 3>& a) { return std::sqrt(dot(a, a)); };
    const auto ctr = v(c.center), p00 = v(c.pixel00_loc), du = v(c.pixel_delta_u), dv = v(c.pixel_delta_v);
    std::array<double, 3> ddu = v(c.defocus_disk_u), ddv = v(c.defocus_disk_v);
    if (c.defocus_angle <= 0) ddu = ddv = {0, 0, 0};
    const std::array<double, 3> rel = {p00[0] - ctr[0], p00[1] - ctr[1], p00[2] - ctr[2]};
    std::array<double, 3> n = {du[1] * dv[2] - du[2] * dv[1], du[2] * dv[0] - du[0] * dv[2], du[0] * dv[1] - du[1] * dv[0]};
    const double nl = len(n);
    if (!(nl > 0) || !std::isfinite(nl)) return 0;
    n = {n[0] / nl, n[1] / nl, n[2] / nl};
    const double W = c.img_width + 1.0, H = c.img_height + 1.0;
    const double dmax = len(rel) + W * len(du) + H * len(dv) + len(ddu) + len(ddv);
    const double dmin = std::fabs(dot(rel, n)) - std::fabs(dot(ddu, n)) - std::fabs(dot(ddv, n));
    const double M = len(ctr) + len(p00) + W * len(du) + H * len(dv) + len(ddu) + len(ddv);   // largest coordinate in play
    const double slack = M * 0x1p-18;                                                          // >> the fp32 rounding of ps, org and D
    return std::isfinite(dmax) && dmax + slack < 0x1p30 && dmin - slack > 0x1p-30;
}

// FastDiv (above ieee_roots): every sphere (centre +- radius) and the lens within 2^18 of the origin.
template <class CAM>
int scene_in_range(const rtiow_handle_s* h, const CAM& c) {
    double reach = 0;
    for (size_t i = 0; i + 3 < h->host_cr.size(); i += 4)
        for (int k = 0; k < 3; ++k) reach = std::fmax(reach, std::fabs(h->host_cr[i + k]) + std::fabs(h->host_cr[i + 3]));
    for (int k = 0; k < 3; ++k)
        reach = std::fmax(reach, std::fabs((double)c.center[k]) + std::fabs((double)c.defocus_disk_u[k]) + std::fabs((double)c.defocus_disk_v[k]));
    return !h->host_cr.empty() && std::isfinite(reach) && reach < 0x1p18;
}

// The parameters of a single-phase launch of the whole local frame in tile order, every field defined: samples [0, S) from the states of
// rtiow_init_rng, no hand-out order, no solo waves, no staging.  Each launch sets what it changes.
template <class T>
RenderParams<T> make_params(const rtiow_handle_s* h) {
    const auto& c = camera<T>(h);
    RenderParams<T> p{};
    p.range_flags = primary_rays_in_range(c) | (scene_in_range(h, c) << 1);
    p.cold.W = c.img_width; p.cold.H = c.img_height; p.cold.S = c.samples_per_pixel; p.B = c.max_depth;
    p.cold.pixel_samples_scale = c.pixel_samples_scale;
    p.cam.center = {c.center[0], c.center[1], c.center[2]};
    p.cam.pixel00 = {c.pixel00_loc[0], c.pixel00_loc[1], c.pixel00_loc[2]};
    p.cam.du = {c.pixel_delta_u[0], c.pixel_delta_u[1], c.pixel_delta_u[2]};
    p.cam.dv = {c.pixel_delta_v[0], c.pixel_delta_v[1], c.pixel_delta_v[2]};
    p.cam.defocus_angle = c.defocus_angle;
    p.cam.ddu = {c.defocus_disk_u[0], c.defocus_disk_u[1], c.defocus_disk_u[2]};
    p.cam.ddv = {c.defocus_disk_v[0], c.defocus_disk_v[1], c.defocus_disk_v[2]};
    p.n = h->n; p.n_padded = h->n_padded;
    p.geom_a = h->geom_a.as<const T>(); p.screen.shade_tbl = h->shade_tbl.as<const T>();
    p.cold.rng = h->rng; p.cold.fb = (T*)h->fb;
    p.cold.local_rows = h->local_rows; p.cold.rank = h->rank; p.cold.nranks = h->preview.nranks; p.cold.strip_rows = h->strip_rows;
    p.cold.s_begin = 0; p.s_end = p.cold.S; p.cold.rng_in = h->rng; p.cold.solo_lanes = 1;
    return p;
}

}  // namespace
