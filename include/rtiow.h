/* rtiow.h -- C-ABI of librtiow_hip.so: the MI355X (gfx950) `render` hot path of the
 * RayTracingInOneWeekend tracer, as a drop-in for the launch sequence in the reference's
 *   src/GlobalFloatCUDAInOneWeekend/main.cu  (fp32)  and
 *   src/GlobalDoubleCUDAInOneWeekend/main.cu (fp64).
 *
 * The reference has no FFI: it launches its kernels inline.  Each entry point below replaces
 * one phase of that inline sequence (cited as main.cu:LINE, relative to
 * /root/reference/src/GlobalFloatCUDAInOneWeekend/ unless noted) so that a host `main` keeps
 * the reference's ordering and timing semantics.  INTEGRATION.md shows the host-side binding.
 *
 * Conventions: plain C, no C++ types, no exceptions.  Every function returns an int:
 * 0 on success, otherwise the hipError_t value of the failing runtime call (or a negative
 * RTIOW_E_* code for argument errors); rtiow_last_error_string() gives the text that the
 * reference's CUDA_SAFE_CALL (main.cu:14-21) would have printed.  The caller owns host
 * memory; the library owns device memory behind the opaque handle.  A handle is not
 * thread-safe.  One handle == one GPU; multi-GPU jobs use either one handle per rank (process;
 * raytracingincuda_amd/distributed.py gathers with torch.distributed) or one rtiow_group (below)
 * in a single process.
 */
#ifndef RTIOW_H
#define RTIOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTIOW_ABI_VERSION 6

#define RTIOW_E_BADARG   (-1)
#define RTIOW_E_STATE    (-2)   /* call order violated (e.g. render before set_scene) */
#define RTIOW_E_NOMEM    (-3)

/* MaterialType (material.h:11-15). */
#define RTIOW_LAMBERTIAN 0
#define RTIOW_METAL      1
#define RTIOW_DIELECTRIC 2

/* Scene-table source selected for the sphere loop (the AMD analogue of the reference's
 * global / constant / texture variants, README.md:7-12). */
#define RTIOW_SCENE_LDS       0 /* sphere list staged into LDS per workgroup, with the packed-
                                 * fp32 8-operation conservative screen in front of the exact test
                                 * (both precisions)                                             */
#define RTIOW_SCENE_SCALAR    1 /* wave-uniform scalar loads through the scalar cache, exact loop */
#define RTIOW_SCENE_LDS_EXACT 2 /* LDS, the reference's 12-operation test on every sphere        */
#define RTIOW_SCENE_GRID      3 /* default: LDS tables plus a uniform grid over the small spheres -- a
                                 * lane walks the cells its ray crosses and tests only their spheres,
                                 * exactly; big spheres are tested by every ray.  Same image bit for
                                 * bit.  Scenes the grid does not suit run as RTIOW_SCENE_LDS.     */
#define RTIOW_SCENE_DEVICE_GRID 4 /* rtiow_render_large and the _large preview calls only (rtiow_set_scene_source refuses it): a uniform grid
                                 * whose cells, index lists and spheres stay in device memory; what
                                 * rtiow_stats.scene_source reads after that call                    */
#define RTIOW_SCENE_VOLUME_GRID 5 /* rtiow_render_volume and the _volume preview calls only (rtiow_set_scene_source refuses it): a uniform
                                 * grid over x, y and z in device memory; what rtiow_stats.scene_source reads after such a call */

/* Pixel scheduling (same image either way):
 * STATIC     = the reference's launch geometry: grid of T x T blocks, one lane per pixel
 *              (main.cu:137-139, camera.h:131-134);
 * PERSISTENT = resident waves pull 64-pixel pools from a global counter and hand a new pixel
 *              to every lane the moment it finishes one (lanes are not pixels here, so
 *              --threads has no effect: workgroups are always four waves). */
#define RTIOW_SCHED_STATIC     0
#define RTIOW_SCHED_PERSISTENT 1
/* SORTED = PERSISTENT in two launches: a prepass renders the first 3 samples of every pixel and
 * records their path-segment counts; the pixels are then ranked heavy-first into balanced pools
 * of neighbouring pixels and the main launch renders the remaining samples in that order (RNG
 * state and colour sum carried exactly, so the image is unchanged).  Removes the drain tail of
 * late heavy pixels.  Default.  The hand-out order packs a pixel as (local row << 16 | column): a frame wider than 65535
 * columns or a shard taller than 32767 rows (or smaller than 4096 pixels) is rendered like RTIOW_SCHED_PERSISTENT, in one
 * launch in tile order (same image; rtiow_stats.phases then reads 1).
 * The order is carried across renders: it depends on scene, camera, shard, bounce limit and sample count, not on the seed, so after
 * a handle's first two-phase render every further rtiow_render of the same frame skips prepass and ranking and launches once, from
 * sample 0, in that order (rtiow_stats.phases 1, order_reused 1; the same image bit for bit -- the order is a scheduling hint).
 * rtiow_set_scene, rtiow_set_shard and rtiow_set_camera with another camera drop the order (the identical camera keeps it), as do
 * rtiow_count_segments, rtiow_accumulate and rtiow_accumulate_adaptive, which write the same buffers; rtiow_init_rng keeps it.  Any
 * change of the launch geometry (schedule, scene source, waves_per_simd) is caught by a key compared on every render.  The
 * environment variable RTIOW_ORDER_REUSE=0, read by rtiow_create, makes every render rank again. */
#define RTIOW_SCHED_SORTED     2

typedef struct rtiow_handle_s* rtiow_handle;

/* The fields of `struct camera` that `render` reads (camera.h:10-30), produced by
 * camera::initialize (camera.h:33-68).  Scalars are in the handle's precision: pass
 * rtiow_camera_f32 to a 32-bit handle and rtiow_camera_f64 to a 64-bit one. */
typedef struct {
    int32_t img_width, img_height, samples_per_pixel, max_depth;
    float   pixel_samples_scale;
    float   center[3], pixel00_loc[3], pixel_delta_u[3], pixel_delta_v[3];
    float   defocus_angle;
    float   defocus_disk_u[3], defocus_disk_v[3];
} rtiow_camera_f32;

typedef struct {
    int32_t img_width, img_height, samples_per_pixel, max_depth;
    double  pixel_samples_scale;
    double  center[3], pixel00_loc[3], pixel_delta_u[3], pixel_delta_v[3];
    double  defocus_angle;
    double  defocus_disk_u[3], defocus_disk_v[3];
} rtiow_camera_f64;

typedef struct {
    double   rng_init_ms;        /* last rtiow_init_rng kernel time (HIP events)           */
    double   render_ms;          /* last rtiow_render kernel time (HIP events)             */
    uint64_t primary_rays;       /* local_rows * width * samples of the last render        */
    int32_t  local_rows;         /* rows of the image this handle renders                  */
    int32_t  num_spheres;        /* spheres uploaded (invalid slots already dropped)       */
    int32_t  block_x, block_y;   /* thread-block shape used by the last render             */
    int32_t  vgprs, sgprs;       /* register use of the render kernel variant (0: unknown) */
    int32_t  lds_bytes;          /* dynamic+static LDS per workgroup of the last render    */
    int32_t  scene_source;       /* RTIOW_SCENE_*                                          */
    int32_t  schedule;           /* RTIOW_SCHED_*                                          */
    int32_t  grid_blocks;        /* workgroups launched by the last render                 */
    int32_t  phases;             /* 2 when RTIOW_SCHED_SORTED split the render, else 1     */
    int32_t  prepass_samples;    /* samples per pixel rendered by the prepass launch (0: none) */
    double   prepass_ms;         /* HIP-event time of the prepass launch of the last timed render */
    double   main_ms;            /* HIP-event time of the main launch (render_persistent_kernel /
                                  * render_kernel): the dominant kernel of the roofline      */
    uint64_t segments_prepass;   /* last rtiow_count_segments: hit_world calls per launch   */
    uint64_t segments_main;
    uint64_t max_chain_prepass;  /* last rtiow_count_segments: the longest per-pixel chain of      */
    uint64_t max_chain_main;     /* segments in each launch (a pixel's samples are sequential: one
                                  * RNG stream, so no schedule finishes before its longest chain)  */
    /* RTIOW_SCENE_GRID, last render (all 0 when the scene runs without a grid): */
    int32_t  grid_nx, grid_nz;   /* cells along x and z                                           */
    int32_t  grid_registered;    /* spheres binned into cells (each in up to 2 x 2 of them)       */
    int32_t  grid_direct;        /* spheres every ray tests exactly (too big for a cell / overflow) */
    double   grid_cell;          /* cell width                                                    */
    /* RTIOW_SCHED_SORTED on a partly filled GPU (small frame, shard): waves that held only the top-ranked
     * pixels, and how many each (0: the plain kernel ran) */
    int32_t  solo_waves, solo_lanes;
    /* Host time of the per-scene pre-processing the render kernels rely on -- screening table + uniform-grid plan
     * and blob (build_screen_table, build_grid_tables) -- spent once per rtiow_set_scene, at the first render after
     * it, BEFORE the start event of that render: like the reference's scene set-up (main.cu:148-321) it is outside
     * render_only and inside end_to_end.  0 when the last scene needed no tables (scalar / exact sources). */
    double   scene_prepare_ms;
    /* RTIOW_SCHED_SORTED: 1 when the main launch stored finished pixels in slot order into a staging buffer and
     * place_pixels_kernel wrote the image in whole lines (coalesced framebuffer writes); place_ms = HIP-event time of
     * that kernel in the last timed render (inside render_ms, outside main_ms). */
    int32_t  staged_stores;
    int32_t  num_cus;            /* compute units of the handle's device (hipDeviceProp_t::multiProcessorCount)              */
    double   place_ms;
    int32_t  clock_mhz;          /* its nominal shader clock (hipDeviceProp_t::clockRate): what an issue-slot figure is rated against */
    int32_t  order_reused;       /* RTIOW_SCHED_SORTED: 1 when the last render skipped prepass and ranking and launched once, from sample 0, in the
                                  * order an earlier render of the same frame left (phases 1, prepass_ms 0, staged_stores 1; main_ms and place_ms
                                  * still split render_ms).  Was reserved0: same offset and size, no ABI change. */
    /* ABI 6.  EFFECTIVE shader clock of the last timed render's launches (persistent schedules; 0: none taken): one wave of each launch --
     * the first dispatched, resident until the hand-out runs dry -- stamps s_memtime and s_memrealtime when it starts and ends, the clock is
     * d(s_memtime) / d(s_memrealtime) x 100 MHz over that wave's life.  A cold process whose render takes 16 ms instead of 11.6 shows here
     * whether the chip was still ramping its clock (profiles/r05/cold_process_study.md). */
    double   main_clock_mhz, prepass_clock_mhz;
    double   main_wave0_ms;      /* that wave's life in the main launch (s_memrealtime), for reading main_clock_mhz against main_ms */
} rtiow_stats;

/* ---- lifetime -------------------------------------------------------------------------
 * rtiow_create replaces cudaSetDevice(0) + event creation (main.cu:81-92).
 * precision is 32 (GlobalFloat) or 64 (GlobalDouble). */
int rtiow_abi_version(void);
/* SHA-256 (hex) of the sources and compiler flags this library was built from (raytracingincuda_amd/build.py
 * passes it in; "unknown" for a hand build).  Profiles record it, and bench.py reports counter-derived figures
 * only from records taken with the very build that is loaded. */
const char* rtiow_build_id(void);
int rtiow_create(int device, int precision, rtiow_handle* out);
int rtiow_destroy(rtiow_handle h);                                   /* main.cu:384-388 */
const char* rtiow_last_error_string(rtiow_handle h);                 /* main.cu:14-21   */

/* Run on an existing hipStream_t (e.g. torch's current stream) instead of the handle's own. */
int rtiow_set_stream(rtiow_handle h, void* hip_stream);

/* ---- scene: replaces cudaMalloc/cudaMemcpy of materials+spheres+world and the two
 * pointer fix-up kernels (main.cu:301-321).  Arrays are host arrays in the handle's
 * precision T:  center_radius[4n] = {cx,cy,cz,r}, albedo_fuzz[4n] = {r,g,b,fuzz},
 * refraction_index[n]; type[n] = RTIOW_*; valid[n] (may be NULL = all valid): slots the
 * reference leaves default-constructed (skipped grid cells, main.cu:168) are dropped. */
int rtiow_set_scene(rtiow_handle h, int n, const void* center_radius, const void* albedo_fuzz,
                    const void* refraction_index, const int32_t* type, const int32_t* valid);

/* ---- camera: replaces passing `cam` by value to render (main.cu:335). */
int rtiow_set_camera(rtiow_handle h, const void* camera /* rtiow_camera_f32 | _f64 */);

/* ---- multi-GPU row sharding (new; the reference is single-GPU, main.cu:81).
 * The image is cut into strips of strip_rows rows dealt round-robin: this handle renders
 * the strips s with s % nranks == rank.  Default (0,1,8) = the whole image.  RNG streams
 * are keyed by the GLOBAL pixel index, so the assembled image does not depend on nranks. */
int rtiow_set_shard(rtiow_handle h, int rank, int nranks, int strip_rows);
int rtiow_local_rows(rtiow_handle h, int* rows);
/* Global row index of each local row (rows_out has rtiow_local_rows entries). */
int rtiow_local_row_map(rtiow_handle h, int32_t* rows_out);

/* ---- RNG: replaces cudaMalloc(rand_states) + init_rng<<<>>> (main.cu:326-330,
 * rtweekend.h:43-50): XORWOW, curand_init(seed, global_pixel_index, 0). */
int rtiow_init_rng(rtiow_handle h, uint64_t seed);

/* ---- render: replaces render<<<dimGrid,dimBlock>>> + sync (main.cu:334-341).
 * threads_per_block_row is the reference's --threads (block = T x T pixels, main.cu:137-139;
 * the grid is ceil-divided, unlike main.cu:137-138): it shapes the launch of RTIOW_SCHED_STATIC and
 * is accepted and ignored by the dynamic schedules.  0 selects the library's own tiling.
 * kernel_ms (may be NULL) receives the HIP-event time around the kernel only; passing NULL
 * makes the call asynchronous on the handle's stream. */
int rtiow_render(rtiow_handle h, int threads_per_block_row, float* kernel_ms);

/* The two halves of a timed rtiow_render, for callers that drive several GPUs from one thread
 * (rtiow_group_*, below): rtiow_render_async enqueues start event, launches and stop event on the
 * handle's stream and returns; rtiow_render_wait blocks on the stop event and returns the
 * HIP-event time of the kernels alone (the same figure rtiow_render reports). */
int rtiow_render_async(rtiow_handle h, int threads_per_block_row);
int rtiow_render_wait(rtiow_handle h, float* kernel_ms);

/* Same render with a path-segment counter (hit_world calls, hittable.h:80) added: untimed,
 * used by bench.py for the algorithmic-flop figure and by tests against the oracle's count.
 * The image it leaves in the framebuffer is identical to rtiow_render's. */
int rtiow_count_segments(rtiow_handle h, int threads_per_block_row, uint64_t* segments);

/* ---- Progressive rendering: the frame in chunks of samples.  After a reset, rtiow_accumulate(h, k1, ...), rtiow_accumulate(h, k2, ...),
 * ... each leave in the framebuffer the exact bits rtiow_render leaves with the same camera and samples_per_pixel = k1 + ... + ki (same
 * seed), whatever the chunk sizes, schedule, scene source or shard layout: a pixel's samples are one sequential RNG chain summed in
 * sample order, and each chunk resumes every pixel from its exact RNG state and colour sum.  The preview is scaled by (T)1 / (T)n, n = the
 * samples accumulated so far; the camera's samples_per_pixel and pixel_samples_scale are not used, max_depth and the rest are.
 *
 * rtiow_accumulate renders samples [n, n + samples) of every local pixel and writes the preview to the framebuffer (the library's or the
 * bound one).  Chunks always use the persistent hand-out: threads_per_block_row is accepted and ignored.  kernel_ms as in rtiow_render
 * (NULL: asynchronous on the handle's stream).  RTIOW_E_BADARG for samples <= 0 or n + samples > INT32_MAX; RTIOW_E_STATE before scene,
 * camera and RNG are set up.  A handle without local rows launches nothing (n still advances).
 * n goes back to 0 -- the next chunk starts from the RNG states of rtiow_init_rng -- on rtiow_accumulate_reset, rtiow_set_camera,
 * rtiow_set_scene, rtiow_set_shard and rtiow_init_rng; rtiow_set_scene_source, rtiow_set_schedule and rtiow_bind_framebuffer keep it.
 * The accumulation has buffers of its own (48 B fp32 / 64 B fp64 per pixel, twice): rtiow_render and rtiow_count_segments between two
 * chunks do not disturb it.  Not available on groups (rtiow_group_*). */
int rtiow_accumulate_reset(rtiow_handle h);
int rtiow_accumulate(rtiow_handle h, int samples, int threads_per_block_row, float* kernel_ms);
int rtiow_accumulated_samples(rtiow_handle h, int* samples);

/* ---- Adaptive progressive rendering: every pixel has its own sample count n_p.  Each pixel keeps its colour sum, s2 = the sum of the
 * squared luminance Y = 0.2126 r + 0.7152 g + 0.0722 b of its samples (in the handle's precision, in sample order) and n_p; after every
 * adaptive chunk the library computes, in double, err_p = sqrt(var / n) / (m + 1e-3) with m = Y(sum) / n and
 * var = max(0, (s2 - n m^2) / (n - 1)) -- the relative standard error of the mean luminance; +inf for n < 2 -- and stores it as float.
 *
 * rtiow_accumulate_adaptive renders `samples` more samples of every ACTIVE local pixel: one with (n_p < min_samples or
 * (double)err_p > rel_error) and n_p + samples <= max_samples, err_p being what the previous call left (+inf before the first), so no count
 * passes max_samples.  Inactive pixels are not traced.  The framebuffer then holds the preview of every local pixel, the exact bits
 * rtiow_render leaves for that pixel with samples_per_pixel = n_p (same camera and seed): a pixel's samples are one sequential RNG chain
 * summed in sample order.  The whole image is rewritten by every call.  *active_pixels (may be NULL) receives the number of pixels that
 * ran: 0 = converged (no render kernel is launched; the preview is still written).  The call blocks once, to read the active count back
 * before the render launch.  kernel_ms (NULL: not timed) = HIP-event time of the select, render and finish kernels, without that read-back.
 * rtiow_accumulated_samples reports the largest n_p in this mode.
 * RTIOW_E_BADARG: samples <= 0, min_samples < 0, max_samples < min_samples, rel_error < 0 or NaN, a frame 65536 or more pixels wide or
 * a shard of 32768 or more local rows (the hand-out order packs a pixel as row << 16 | column).  RTIOW_E_STATE before scene, camera
 * and RNG are set up.  A handle without local rows launches nothing.
 * The first chunk after a reset fixes the mode: rtiow_accumulate after adaptive chunks, and rtiow_accumulate_adaptive after plain ones,
 * return RTIOW_E_STATE until rtiow_accumulate_reset.  Resets, isolation from rtiow_render and the state kept by set_scene_source,
 * set_schedule and bind_framebuffer are those of rtiow_accumulate.  The adaptive chunk always uses the persistent hand-out (the schedule
 * does not change the image).  Not available on groups.
 *
 * rtiow_read_adaptive_state copies n_p and err_p of every local pixel (row-major local order) to host memory; either pointer may be NULL.
 * npix must equal local_rows x width (RTIOW_E_BADARG).  Before an adaptive chunk: n = 0 and err = +inf. */
int rtiow_accumulate_adaptive(rtiow_handle h, int samples, int min_samples, double rel_error, int max_samples, float* kernel_ms, int* active_pixels);
int rtiow_read_adaptive_state(rtiow_handle h, int32_t* counts, float* rel_err, size_t npix);

/* ---- Denoised previews of progressive rendering.  Every value below is computed in T, left to right as
 * written, with plain * + - / and a correctly rounded sqrt (no fused multiply-add), so a restatement in numpy gives the same bits.
 *
 * rtiow_read_linear copies the linear (pre-gamma) mean colour of the current accumulation, local_rows x width x 3 T:
 * c_p = n_p > 0 ? acc_p * ((T)1 / (T)n_p) : 0 per channel, n_p = rtiow_accumulated_samples (plain chunks) or the pixel's own count
 * (adaptive chunks).  (c > 0 ? sqrt(c) : 0) is the preview's bits.  RTIOW_E_STATE when no chunk has run since the last reset.
 *
 * rtiow_render_guides computes first-hit guide buffers for the handle's camera, scene and shard.  Local pixel (i, jl), global row j,
 * has the ray O = camera centre, D = ((pixel00 + i du) + j dv) - O (no jitter, no defocus) and (t, k) = hit_world(O, D).  On a hit:
 * P = O + t D, outward = (P - C_k) * ((T)1 / r_k), normal = ((D.x o.x + D.y o.y) + D.z o.z) < 0 ? outward : -outward, albedo = the
 * material's {r,g,b} (lambertian, metal) or {1,1,1} (dielectric), depth = t; on a miss all zero.  kernel_ms as in rtiow_render.
 * rtiow_read_guides copies them as planes (npix = local_rows x width; normal and albedo npix x 3 T, depth npix T; each may be NULL).
 * The guides go stale on rtiow_set_scene, rtiow_set_camera and rtiow_set_shard: rtiow_read_guides then returns RTIOW_E_STATE.
 *
 * rtiow_denoise filters the linear colour c of the current accumulation with `levels` levels of an edge-avoiding a-trous filter
 * (Dammertz et al. 2010) into a buffer of its own: level k (step s = 1 << k) gives every pixel p, over the taps q = p + (dx s, dy s),
 * dy then dx in -2..2, those outside the frame skipped: kern = K[dx+2] K[dy+2], K = {1/16, 1/4, 3/8, 1/4, 1/16};
 * e = ((ec ic_k + en i_n) + ea i_a) + ez i_z with ec = (d.x d.x + d.y d.y) + d.z d.z of colour q - p, en and ea likewise of normal and
 * albedo, ez = dz dz of depth; w = kern / (1 + e); out_p = (sum w c_q) / (sum w) per channel, sums in tap order from 0.
 * ic_k = (T)((1 / (sigma_color^2)) 4^k), i_n = (T)(1 / sigma_normal^2), i_a and i_z likewise (computed in double); sigma = +inf turns
 * its term off.  The output is the last level gamma-encoded like the preview (x > 0 ? sqrt(x) : 0).  Stale guides are rendered first,
 * inside kernel_ms (NULL: asynchronous).  RTIOW_E_BADARG: levels outside 1..8, a sigma <= 0 or NaN.  RTIOW_E_STATE: no chunk since the
 * last reset, or a sharded handle (nranks > 1: its strips are not image neighbours).  The framebuffer, the accumulation and the next
 * chunk's bits are untouched.  rtiow_read_denoised copies the output (local_rows x width x 3 T); rtiow_denoised_device_ptr gives its
 * device address (valid until a later rtiow_denoise on a larger frame).  Both return RTIOW_E_STATE before an rtiow_denoise or after
 * rtiow_set_scene / _camera / _shard.  All these buffers are allocated at first use.  Not available on groups. */
/* Linear (pre-gamma) mean colour of the current accumulation, local_rows x width x 3 T. */
int rtiow_read_linear(rtiow_handle h, void* host_rgb, size_t bytes);
/* First-hit guide buffers for the handle's camera, scene and shard. */
int rtiow_render_guides(rtiow_handle h, float* kernel_ms);
int rtiow_read_guides(rtiow_handle h, void* normal /* npix*3 T */, void* albedo /* npix*3 T */, void* depth /* npix T */, size_t npix);
/* Edge-avoiding a-trous filter of the current accumulation into a buffer of its own. */
int rtiow_denoise(rtiow_handle h, int levels, double sigma_color, double sigma_normal, double sigma_albedo, double sigma_depth, float* kernel_ms);
int rtiow_read_denoised(rtiow_handle h, void* host_rgb, size_t bytes);
int rtiow_denoised_device_ptr(rtiow_handle h, void** device_ptr, size_t* bytes);

/* ---- Variance-guided denoising: the colour edge-stop of the filter follows the noise each pixel measured.
 * Both calls need the second moment s2 that only adaptive chunks keep: after plain chunks, and with no chunk since the last reset, they
 * return RTIOW_E_STATE.  (rtiow_accumulate_adaptive(h, k, INT32_MAX, 0.0, INT32_MAX, ...) samples uniformly and keeps s2; its preview
 * is rtiow_accumulate's bit for bit.)
 *
 * rtiow_read_variance copies V_p, the estimated variance of the pixel's MEAN luminance, one T per local pixel (npix = local_rows x
 * width, else RTIOW_E_BADARG).  With n = n_p, the colour sum acc and s2 as stored, in double and in this order -- the expressions of
 * err_p above --: m = Y(acc) / n, var = max(0, (s2 - n m^2) / (n - 1)), V_p = (T)(var / n); V_p = 0 for n_p < 2 (no estimate).
 * sqrt(var / n) / (m + 1e-3) is err_p.  Works on shards.
 *
 * rtiow_denoise_variance filters the linear colour C^0 = c of the accumulation (rtiow_read_linear) together with V^0 = V.  Frame,
 * taps, tap order, kern, the guide terms en, ea, ez with i_n, i_a, i_z, the skipping of taps outside the frame, the gamma of the last
 * level, `levels`, stale guides, kernel_ms and the refusal of shards are rtiow_denoise's; everything in T, left to right as written,
 * plain * + - /.  Level k, step s = 1 << k, gives every pixel p:
 *   g_p = (sum b V^k_q) / (sum b) over q = p + (dx, dy), dy then dx in -1..1 (step 1 at every level), b = B[dx+1] B[dy+1],
 *         B = {1/4, 1/2, 1/4}, those outside the frame skipped, sums from 0;
 *   i_p = f_k / (sv2 g_p + eps), sv2 = (T)(sigma_variance^2) (the square in double), f_k = (T)(4^k), eps = (T)1e-8;
 *   per tap q = p + (dx s, dy s), dy then dx in -2..2:  ec = (d.x d.x + d.y d.y) + d.z d.z with d = C^k_q - C^k_p,
 *         e = ((ec i_p + en i_n) + ea i_a) + ez i_z,  w = kern / (1 + e),  S = S + w C^k_q,  W = W + w,  U = U + (w w) V^k_q;
 *   C^(k+1)_p = S / W per channel,  V^(k+1)_p = U / (W W).
 * sigma_variance = +inf turns the colour term off: i_p = 0 by definition (decided on the host, also when sv2 is not finite in T); the
 * colour output is then rtiow_denoise's with sigma_color = +inf.  The output goes to the buffer rtiow_denoise writes:
 * rtiow_read_denoised and rtiow_denoised_device_ptr return the image of whichever of the two calls ran last.
 * RTIOW_E_BADARG: levels outside 1..8, a sigma <= 0 or NaN.  RTIOW_E_STATE: as said above, or a sharded handle.  The framebuffer,
 * the accumulation, its counts and errors and the next chunk's bits are untouched.  Not available on groups. */
int rtiow_read_variance(rtiow_handle h, void* host_var /* npix T */, size_t npix);
int rtiow_denoise_variance(rtiow_handle h, int levels, double sigma_variance, double sigma_normal, double sigma_albedo, double sigma_depth, float* kernel_ms);

/* ---- Temporal history for progressive previews: samples survive a camera move.  The handle keeps a BASE
 * -- per pixel {H.rgb, M} (history colour, history length in samples) and {normal', depth'} of an earlier camera, with that camera
 * (primed below) -- and a TEMPORAL IMAGE {C.rgb, M} of the current camera.  rtiow_history_update reprojects every pixel of the current
 * camera into the base, gathers the matching history bilinearly and blends it with the current accumulation by sample count;
 * rtiow_history_commit makes the result the new base.  Everything in T, left to right as written, plain * + - / (no fused
 * multiply-add), so a restatement in numpy gives the same bits.
 *
 * Host constants of the base camera, in double from its stored fields, each rounded once to T: a = pixel00' - O', w = du' x dv',
 * f = (a.x w.x + a.y w.y) + a.z w.z (f < 0: w and f negated), iu = 1 / ((du'.x du'.x + du'.y du'.y) + du'.z du'.z), iv likewise.
 * Pixel p = (x, y) has the colour c and count n_p of rtiow_read_linear and the guides N_p, t_p:
 *   D = ((pixel00 + x du) + y dv) - O;  hit (t_p > 0): d = (O + t_p D) - O';  miss: d = D;
 *   den = (d.x w.x + d.y w.y) + d.z w.z;  s = f / den;  e = s d - a;  u = ((e.x du'.x + e.y du'.y) + e.z du'.z) iu, v with dv', iv;
 *   te = den / f;  x0 = floor(u), y0 = floor(v), fx = u - x0, fy = v - y0.
 * Taps (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1) with b = (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy, those outside the frame skipped.
 * A tap q counts when M_q > 0 and -- hit: depth'_q > 0, |depth'_q - te| <= (T)depth_tol te, (N_p.x N'_q.x + N_p.y N'_q.y) + N_p.z
 * N'_q.z >= (T)normal_cos -- miss: depth'_q == 0.  From 0 over the taps that count: S = S + b H_q, L = L + b M_q, Bs = Bs + b;
 * Bs > 0: h = S / Bs, m = L / Bs, else h = 0, m = 0;  m = min(m, (T)max_history).  There are no taps (m = 0) unless den > 0,
 * -1 < u < W and -1 < v < H, nor when the base is empty, was committed at another frame size, or f is 0 or not finite.
 *   nT = (T)n_p, Mout = m + nT;  Mout > 0: alpha = nT / Mout, Cout = h + alpha (c - h), else Cout = 0.
 * Without history Cout is c bit for bit and Mout is n_p.  *reprojected_pixels (may be NULL) = the pixels with m > 0.
 *
 * rtiow_history_update writes the temporal image.  It always combines the base with the WHOLE current accumulation, so it may be
 * called after every chunk.  Stale guides are rendered first, inside kernel_ms (NULL: not timed; with reprojected_pixels NULL too
 * the call is asynchronous).  RTIOW_E_BADARG: depth_tol < 0 or NaN, normal_cos outside [-1, 1] or NaN, max_history <= 0 or NaN
 * (+inf: no cap).  RTIOW_E_STATE: no chunk since the last accumulation reset.
 * rtiow_history_commit makes the temporal image, the current guides and the current camera the base: the buffers change owners,
 * nothing is copied.  The temporal image and the guides are stale afterwards.  Commit, then move the camera (or reset the
 * accumulation): an update over the accumulation that was committed would count its samples twice.  RTIOW_E_STATE when the temporal
 * image is stale.
 * rtiow_history_reset empties the base.  So do rtiow_set_scene and rtiow_set_shard; the base survives rtiow_set_camera, rtiow_init_rng
 * and rtiow_accumulate_reset.  The temporal image goes stale on rtiow_set_camera, rtiow_set_scene, rtiow_set_shard, rtiow_history_reset
 * and rtiow_history_commit: rtiow_read_history (planes: rgb npix x 3 T linear, length npix T; either may be NULL; npix = height x width),
 * rtiow_history_device_ptr (npix x 4 T {C.rgb, M}; valid until the next commit or an update on a larger frame) and
 * rtiow_denoise_history then return RTIOW_E_STATE.
 * rtiow_denoise_history is rtiow_denoise with level 0 reading Cout instead of the accumulation: arguments, errors, stale guides and
 * the output buffer (rtiow_read_denoised, rtiow_denoised_device_ptr) are rtiow_denoise's.
 * None of these touches the framebuffer, the accumulation, its counts or the bits of the next chunk.  All return RTIOW_E_STATE on a
 * sharded handle (nranks > 1).  Buffers are allocated at first use.  Not available on groups. */
int rtiow_history_reset(rtiow_handle h);
int rtiow_history_update(rtiow_handle h, double depth_tol, double normal_cos, double max_history, float* kernel_ms, uint64_t* reprojected_pixels);
int rtiow_history_commit(rtiow_handle h);
int rtiow_read_history(rtiow_handle h, void* rgb /* npix*3 T, linear */, void* length /* npix T */, size_t npix);
int rtiow_history_device_ptr(rtiow_handle h, void** device_ptr, size_t* bytes);   /* npix x 4 T: {C.rgb, M} */
int rtiow_denoise_history(rtiow_handle h, int levels, double sigma_color, double sigma_normal, double sigma_albedo, double sigma_depth, float* kernel_ms);

/* ---- Filter guides that follow mirrors and glass to the first diffuse surface.  The handle has two sets
 * of guides.  The FIRST-HIT guides are those of rtiow_render_guides / rtiow_read_guides above, in either mode; rtiow_history_update and
 * rtiow_history_commit use them alone (reprojection needs the real first surface).  The FILTER guides are what rtiow_denoise,
 * rtiow_denoise_variance and rtiow_denoise_history steer by.  RTIOW_GUIDES_FIRST_HIT (default): they are the first-hit buffers
 * themselves -- no extra memory, no extra launch, every output as without this call.  RTIOW_GUIDES_SPECULAR: a second pair of buffers,
 * allocated at first use and written wherever the first-hit guides are rendered (rtiow_render_guides, and the stale guides a filter
 * or rtiow_history_update renders first), by following each pixel's centre ray through the specular surfaces it meets:
 *
 * Everything in T, left to right as written, plain * + - / and a correctly rounded sqrt, no fused multiply-add.  O_0, D_0 = the ray of
 * rtiow_render_guides; A = {1,1,1}, Z = 0, b = 0.  Repeat (t, k) = hit_world(O_b, D_b) (D for D_b below):
 *   miss, b == 0: normal' = albedo' = 0, depth' = 0.   miss, b > 0: normal' = 0, albedo' = A, depth' = Z.
 *   hit: P = O_b + t D, outward = (P - C_k) * ((T)1 / r_k), dn = (D.x o.x + D.y o.y) + D.z o.z, front = dn < 0, N = front ? outward :
 *   -outward; a_k = the material's {r,g,b}, {1,1,1} for a dielectric.  The surface is specular when it is a dielectric, or a metal with
 *   (double)fuzz_k <= max_fuzz.  Not specular, or b == max_bounces: normal' = N, albedo' = A a_k per channel (A for a dielectric),
 *   depth' = Z + t, and the chain ends.  Otherwise A = A a_k (A kept for a dielectric), Z = Z + t, O_(b+1) = P, b = b + 1 and
 *     metal:      dN = (D.x N.x + D.y N.y) + D.z N.z, c2 = 2 dN, D' = D - c2 N per component;
 *     dielectric: dd = (D.x D.x + D.y D.y) + D.z D.z, len = sqrt(dd), il = 1 / len, u = D il, m = -((u.x N.x + u.y N.y) + u.z N.z),
 *                 ct = m < 1 ? m : 1, st = sqrt(1 - ct ct), ri = front ? (T)1 / eta_k (as the shade table holds it) : eta_k;
 *                 ri st > 1 (total internal reflection): c2 = 2 (-ct), r = u - c2 N;  else perp = ri (u + ct N) per component,
 *                 kk = -sqrt(|1 - ((perp.x perp.x + perp.y perp.y) + perp.z perp.z)|), r = perp + kk N;  D' = r len.
 * Schlick's reflectance is not consulted: the refracted branch is taken whenever there is one.  Through `len` every t of a chain is in
 * the units of the primary ray, so depth' compares with the first-hit depth.  bounces = b at the end.  A sky seen in a mirror has the
 * colour A x (the primary ray's sky), hence albedo' = A on a miss.
 *
 * rtiow_set_guide_mode is a knob like rtiow_set_scene_source: it survives rtiow_set_scene, rtiow_set_camera and rtiow_set_shard.  A call
 * that changes nothing does nothing; one that changes mode, max_bounces or max_fuzz makes the guides (both sets: rtiow_read_guides too
 * returns RTIOW_E_STATE until they are rendered again) and the denoised image stale and leaves the accumulation, the history base and
 * the temporal image alone.  RTIOW_E_BADARG: a mode other than 0 or 1; in mode 1 max_bounces outside 1..16, max_fuzz < 0 or NaN (+inf:
 * every metal is a mirror).  In mode 0 the other arguments are ignored.
 * rtiow_read_filter_guides copies the filter guides as planes: arguments, RTIOW_E_STATE when stale, layout and shards as
 * rtiow_read_guides, plus bounces (npix int32); any pointer may be NULL.  In mode 0 it gives the first-hit planes and bounces = 0. */
#define RTIOW_GUIDES_FIRST_HIT 0   /* default: the filters steer by the first-hit guides */
#define RTIOW_GUIDES_SPECULAR  1
int rtiow_set_guide_mode(rtiow_handle h, int mode /* RTIOW_GUIDES_* */, int max_bounces, double max_fuzz);
int rtiow_read_filter_guides(rtiow_handle h, void* normal /* npix*3 T */, void* albedo /* npix*3 T */, void* depth /* npix T */,
                             int32_t* bounces /* npix */, size_t npix);

/* ---- History-guided sample budgets: sample where the history is short.  After a camera move most pixels
 * will carry up to max_history samples from the base; the few that were just disoccluded will carry none.  Which is which is known
 * before the first sample of the new frame is traced, because the history length m of rtiow_history_update depends on the current
 * camera, the first-hit guides and the base alone, not on the accumulation.
 * rtiow_history_plan computes the PLAN: for every pixel p, m_p = the m of the block above, to the letter -- the ray, the reprojection,
 * te, the four taps, the tests on M_q, depth'_q and the normals, L / Bs and min(m, (T)max_history), in T with plain * + - /, floor and
 * fabs -- and 0 in every case listed there as "no taps".  An empty base or a base of another frame size gives m = 0 everywhere, not an
 * error.  *reprojected_pixels (may be NULL) = the pixels with m_p > 0.  An rtiow_history_update with the same three arguments later
 * gives Mout = m_p + (T)n_p bit for bit.  Arguments, their errors, the rendering of stale guides inside kernel_ms and the asynchronous
 * form (both pointers NULL) are rtiow_history_update's.  It needs scene and camera (else RTIOW_E_STATE), no RNG and no chunk; RTIOW_E_STATE
 * on a sharded handle.
 * The plan goes stale exactly when the temporal image does -- rtiow_set_camera, rtiow_set_scene, rtiow_set_shard, rtiow_history_reset,
 * rtiow_history_commit -- and survives rtiow_init_rng, rtiow_accumulate_reset, rtiow_set_guide_mode (it uses the first-hit guides) and
 * every chunk.  rtiow_read_history_plan copies it (npix T, npix = height x width; NULL: only the checks): RTIOW_E_STATE when stale.
 *
 * rtiow_accumulate_budget is rtiow_accumulate_adaptive with another rule.  A local pixel is active iff
 *     (n_p < min_samples  or  (T)n_p + m_p < (T)target)  and  n_p + samples <= max_samples
 * with the sum and the comparison in T and n_p = 0 in the first chunk after a reset.  Everything else is that call's: inactive pixels
 * are not traced, the whole preview is rewritten, every pixel holds the bits rtiow_render leaves at samples_per_pixel = n_p (never
 * sampled: 0), the second moment and err_p are kept (rtiow_read_adaptive_state, rtiow_read_variance, rtiow_denoise_variance work
 * afterwards), one blocking read-back of the active count, kernel_ms, and *active_pixels == 0 meaning that nothing but the finish was
 * launched.  The chunk belongs to the adaptive mode: it alternates freely with rtiow_accumulate_adaptive between two resets and returns
 * RTIOW_E_STATE after plain chunks.  RTIOW_E_STATE also when the plan is stale or scene, camera and RNG are not set up.  RTIOW_E_BADARG:
 * samples <= 0, min_samples < 0, max_samples < min_samples, target <= 0 or NaN (+inf: everybody, up to max_samples), or a frame beyond
 * rtiow_accumulate_adaptive's limits.  A failing call leaves the handle as it was.
 * The loop of a moving camera: rtiow_set_camera, rtiow_init_rng, rtiow_history_plan, rtiow_accumulate_budget until *active_pixels == 0,
 * rtiow_history_update with the plan's three arguments, rtiow_history_commit.  With max_history < target no pixel ever reaches the
 * target and every frame adds target - max_history samples to a fully covered pixel; with min_samples = 0 a pixel whose m_p reaches
 * the target is not sampled at all and Cout there is the gathered history h.  Not available on groups. */
int rtiow_history_plan(rtiow_handle h, double depth_tol, double normal_cos, double max_history, float* kernel_ms, uint64_t* reprojected_pixels);
int rtiow_read_history_plan(rtiow_handle h, void* length /* npix T */, size_t npix);
int rtiow_accumulate_budget(rtiow_handle h, int samples, int min_samples, double target, int max_samples, float* kernel_ms, int* active_pixels);

/* ---- History clipped to the current frame's neighbourhood colours.  A reflection, a refraction or an
 * out-of-focus edge moves with the camera but is reprojected as if painted on the first surface; max_history only bounds how long such
 * a history lives.  rtiow_history_update_clipped is rtiow_history_update with one step inserted between "m = min(m, (T)max_history)"
 * and "nT = (T)n_p": the gathered colour h is clamped to what the current accumulation shows around the pixel.  Everything in T, left
 * to right as written, plain * + - / and a correctly rounded sqrt, no fused multiply-add.  For local pixel p = (x, y), r = clip_radius:
 *   Window: q = (x + dx, y + dy), dy then dx in -r..r.  A tap counts when q is inside the frame and n_q > 0; n_q and c_q are those
 *   of rtiow_read_linear.  From 0, per channel, over the taps that count: A = A + c_q, Q = Q + c_q c_q; the integer k = k + 1.
 *   kT = (T)k, mu = A / kT, s = Q / kT - mu mu, s = s > 0 ? s : 0, sd = sqrt(s), e = (T)clip_gamma sd, lo = mu - e, hi = mu + e.
 *   When m > 0 and k >= 2, per channel: h = h < lo ? lo : (h > hi ? hi : h); otherwise h stays.  Comparisons with NaN are false, so a
 *   NaN bound leaves h alone.
 * m is not changed: Mout, the length plane and *reprojected_pixels are rtiow_history_update's bit for bit for the same first three
 * arguments, and rtiow_history_plan still predicts Mout.  *clipped_pixels (may be NULL) = the pixels with m > 0 in which at least one
 * channel of h changed value; every other pixel has rtiow_history_update's Cout bit for bit.  clip_gamma = +inf clips nothing: the whole
 * temporal image is rtiow_history_update's.  clip_gamma = 0 replaces the history by the neighbourhood mean.
 * RTIOW_E_BADARG: the errors of rtiow_history_update, clip_radius outside 1..3, clip_gamma < 0 or NaN.  RTIOW_E_STATE, the rendering of
 * stale guides inside kernel_ms, the asynchronous form (all three pointers NULL) and the refusal of sharded handles are
 * rtiow_history_update's.  The call writes the same temporal image and colour plane, so rtiow_history_commit, rtiow_read_history,
 * rtiow_history_device_ptr and rtiow_denoise_history work on its result unchanged, and it touches nothing else: framebuffer,
 * accumulation, counts and errors, base, guides, plan, the bits of the next chunk.  A failing call leaves the handle as it was.
 * Not available on groups. */
int rtiow_history_update_clipped(rtiow_handle h, double depth_tol, double normal_cos, double max_history, int clip_radius, double clip_gamma,
                                 float* kernel_ms, uint64_t* reprojected_pixels, uint64_t* clipped_pixels);

/* ---- Variance-guided filtering of the temporal image.  rtiow_denoise_variance steers its colour edge-stop
 * by each pixel's measured noise but reads the current accumulation only; rtiow_denoise_history reads the temporal image but has one
 * fixed sigma.  rtiow_denoise_history_variance is rtiow_denoise_variance with two changes at level 0: C^0 = Cout, the temporal colour
 * plane rtiow_denoise_history reads, and V^0 = the plane below.  Nothing is carried from frame to frame: the blend is
 * Cout = h + alpha (c - h), alpha = n / Mout, and if the history's samples have the per-sample variance the frame measured, the variance
 * of Cout's mean luminance is alpha^2 V + (1 - alpha)^2 V n / m = alpha V.  Everything in T, left to right as written, plain * + - /,
 * no fused multiply-add.  For local pixel p = (x, y), r = variance_radius:
 *   Measured -- the accumulation is adaptive and n_p >= 2: V_p = rtiow_read_variance's value, alpha = (T)n_p / Mout_p (the update's own
 *   expression and bits; Mout_p > 0 here), V^0_p = alpha V_p.
 *   Spatial -- every other pixel (never sampled, n_p < 2, every pixel after plain chunks): Y_q = the luminance of adaptive chunks
 *   ((0.2126 R + 0.7152 G) + 0.0722 B in T) of Cout_q.  Window: q = (x + dx, y + dy), dy then dx in -r..r; a tap counts when q is inside
 *   the frame and Mout_q > 0.  From 0 over the taps that count: A = A + Y_q, Q = Q + Y_q Y_q; the integer k = k + 1.  kT = (T)k,
 *   mu = A / kT, s = Q / kT - mu mu, s = s > 0 ? s : 0, V^0_p = k >= 2 ? s : 0.  s is the spread of per-pixel means already: it is not
 *   divided by a count.
 * levels, taps, tap order, kern, g_p, i_p, f_k, eps, the guide terms, the filter guides of the current guide mode, the skipping of taps
 * outside the frame, the gamma of the last level, the output buffer (rtiow_read_denoised, rtiow_denoised_device_ptr), the rendering of
 * stale guides inside kernel_ms, kernel_ms == NULL meaning asynchronous and sigma_variance = +inf decided on the host are
 * rtiow_denoise_variance's to the letter.  V^0 lives in a buffer of its own, which the levels do not overwrite; rtiow_read_history_variance
 * copies it out (npix = height x width, else RTIOW_E_BADARG; var == NULL runs only the checks).  It returns RTIOW_E_STATE until a
 * rtiow_denoise_history_variance has run, wherever the temporal image goes stale, and after a later rtiow_history_update(_clipped).
 * RTIOW_E_BADARG: rtiow_denoise_variance's errors, variance_radius outside 1..3.  RTIOW_E_STATE: the temporal image is stale; the handle
 * is sharded; a chunk (rtiow_accumulate, _adaptive, _budget) or a reset of the accumulation (rtiow_accumulate_reset, rtiow_init_rng) ran
 * after the update that wrote the temporal image -- alpha would no longer be the update's: update again.  A failing call leaves the
 * handle as it was.  The call touches nothing else: framebuffer, accumulation, counts and errors, base, temporal image, guides, plan,
 * the bits of the next chunk.  Not available on groups. */
int rtiow_denoise_history_variance(rtiow_handle h, int levels, double sigma_variance, double sigma_normal, double sigma_albedo, double sigma_depth,
                                   int variance_radius, float* kernel_ms);
int rtiow_read_history_variance(rtiow_handle h, void* var /* npix T */, size_t npix);

/* ---- Recurrent history: a filtered temporal image as the next base.  rtiow_history_commit hands the raw
 * temporal image to the next frame, so every frame starts from a history that still carries its full noise.
 * rtiow_history_commit_filtered is rtiow_history_commit with one step in front: the {C.rgb, M} of the temporal image, as the last
 * rtiow_history_update(_clipped) wrote it, is replaced by {H'.rgb, M} below before it becomes the base -- one level of the a-trous
 * filter at step 1, fed back (Schied et al. 2017).  The base keeps its format; nothing new is carried.  Everything in T, left to right
 * as written, plain * + - /, no fused multiply-add.  For pixel p = (x, y): C, M = the temporal image; N, A, Z = the filter guides of the
 * current guide mode (normal, albedo, depth), the ones rtiow_denoise_history steers by.
 *   M_p > 0 is false: H'_p = C_p (which is 0 there), M'_p = M_p, bit for bit.
 *   Otherwise the taps are q = p + (dx, dy), dy then dx in -2..2, at step 1.  A tap counts when q is inside the frame and M_q > 0.
 *   kern = K[dx+2] K[dy+2], K = {1/16, 1/4, 3/8, 1/4, 1/16};  ec, en, ea, ez, e = ((ec ic + en i_n) + ea i_a) + ez i_z and
 *   w = kern / (1 + e) exactly as level 0 of rtiow_denoise: ic = (T)(1 / sigma_color^2) and so on, computed in double and rounded
 *   once, sigma = +inf turning a term off.  From 0, in tap order, over the taps that count: S = S + w C_q per channel, Wt = Wt + w.
 *   F = S / Wt per channel.  feedback == 1 (decided on the host): H'_p = F; otherwise H'_p = C_p + (T)feedback (F - C_p) per channel.
 *   M'_p = M_p: the length is not touched, so rtiow_history_plan still predicts Mout bit for bit.  Comparisons with NaN are false.
 * After this step the call is rtiow_history_commit: the new base is {H', M'}, the current FIRST-HIT {normal, depth} and the current
 * camera; the temporal image, the plan and the guides go stale.  The result is written into the buffer that held the old base (the
 * first commit of a handle allocates it); the buffer of the temporal image is left behind, stale.  Stale guides (e.g. after
 * rtiow_set_guide_mode) are rendered first, inside kernel_ms; kernel_ms == NULL: asynchronous on the handle's stream.
 * RTIOW_E_BADARG: a sigma <= 0 or NaN, feedback outside (0, 1] or NaN.  RTIOW_E_STATE: the temporal image is stale; the handle is
 * sharded.  A failing call leaves the handle as it was.  The call touches nothing else: framebuffer, accumulation, counts and errors,
 * the denoised buffer, the bits of the next chunk.  Not available on groups.
 * rtiow_read_history_base copies the base's {H.rgb} and {M} as planes, in the layout of rtiow_read_history (either pointer may be
 * NULL; npix = height x width of the frame the base was committed at, else RTIOW_E_BADARG), after either commit.  RTIOW_E_STATE: the
 * base is empty or the handle is sharded. */
int rtiow_history_commit_filtered(rtiow_handle h, double sigma_color, double sigma_normal, double sigma_albedo, double sigma_depth, double feedback,
                                  float* kernel_ms);
int rtiow_read_history_base(rtiow_handle h, void* rgb /* npix*3 T, linear */, void* length /* npix T */, size_t npix);

/* ---- Edge resolve: silhouette pixels rebuilt from sub-pixel coverage layers.  The guides are one centre ray
 * per pixel, while the colour of a silhouette pixel is an area mix of two surfaces: such a pixel looks like neither neighbour and the
 * filters leave it almost alone.  rtiow_render_coverage finds, per pixel, which first-hit spheres share it and in what proportion;
 * rtiow_resolve_edges rebuilds each mixed pixel of the denoised image from what the filter produced on the pure pixels of its layers
 * nearby.  Everything in T, left to right as written, plain * + - /, no fused multiply-add.
 * Coverage layers.  They depend on scene, camera and shard only, like the guides.  G = subsamples_per_side in {2, 4}, S = G G.  For local
 * pixel (i, jl) with global row j and sub-sample s = a + G b (b outer): o_a = ((T)a + 0.5) / G - 0.5 and o_b likewise (-+0.25 for G = 2;
 * -+0.375, -+0.125 for G = 4: exact), fx = (T)i + o_a, fy = (T)j + o_b, D = ((pixel00 + fx du) + fy dv) - O with O the camera centre (no
 * lens sample), (t, k) = hit_world(O, D), and the normal N facing the ray to the letter of rtiow_render_guides.  A miss: k = -1, N = 0,
 * t = 0.  k counts the spheres rtiow_set_scene kept (invalid slots are not counted).  c_k = the number of sub-samples with that k.  The
 * distinct k are ordered by c_k descending, the smaller k first on a tie (the sky, -1, is the smallest).  Layer l in {0, 1} holds id_l,
 * c_l, n_l = (the sum of N over its sub-samples, from 0 in index order) * ((T)1 / (T)c_l) per component, and z_l the same of t.  One
 * distinct k: the pixel is PURE, with pid = id_0 and layer 1 = {-2, 0, 0, 0}.  Otherwise it is MIXED; a third surface and beyond is
 * dropped.
 * rtiow_render_coverage: RTIOW_E_BADARG unless G is 2 or 4; RTIOW_E_STATE before scene and camera are set.  It works on shards (rows are
 * global).  The layers go stale with rtiow_set_scene, rtiow_set_camera and rtiow_set_shard and survive chunks, resets,
 * rtiow_set_guide_mode, rtiow_history_update and both commits: their buffers, allocated at first use, never change owners.  Every call
 * renders, whatever G the layers have.  kernel_ms == NULL: asynchronous on the handle's stream.
 * rtiow_read_coverage copies planes: ids and counts npix x 2 int32, normal npix x 2 x 3 T, depth npix x 2 T (any pointer may be NULL).
 * npix != local_rows x width: RTIOW_E_BADARG; stale layers: RTIOW_E_STATE.
 * The resolve.  rtiow_resolve_edges rewrites, in place, the mixed pixels of the denoised image -- the buffer of rtiow_read_denoised /
 * rtiow_denoised_device_ptr, whichever of the four filters wrote it last.  g = that image, gamma-encoded as stored; N_q, Z_q = the
 * FIRST-HIT guides of pixel q in either guide mode; i_n = (T)(1 / sigma_normal^2) and i_z likewise, computed in double and rounded once,
 * sigma = +inf turning a term off.  Per mixed pixel p = (x, y), r = radius:
 *   L_p = g_p g_p per channel.  Taps q = p + (dx, dy), dy then dx in -r..r; a tap counts when q is inside the frame and q is pure.
 *   For layer l = 0 then 1, from 0 over the taps that count with pid_q == id_l: d = N_q - n_l, en = (d.x d.x + d.y d.y) + d.z d.z,
 *   dz = Z_q - z_l, e = en i_n + (dz dz) i_z, w = 1 / (1 + e), Sx = Sx + w (g_q g_q) per channel, Wt = Wt + w.
 *   A layer with Wt > 0 is FOUND: F_l = Sx / Wt, a_l = (T)c_l / (T)S.  R = 0, rest = 1; for each found layer in order R = R + a_l F_l,
 *   rest = rest - a_l; then R = R + rest L_p.
 *   n_eff = the count behind the filtered image: n_p of rtiow_read_linear when rtiow_denoise(_variance) wrote it, Mout_p of the temporal
 *   image when rtiow_denoise_history(_variance) did.  beta = (T)prior / ((T)prior + (T)n_eff) and out = L_p + beta (R - L_p); prior = +inf
 *   is decided on the host: out = R.  Stored: out > 0 ? sqrt(out) : 0.
 * A pure pixel keeps its stored bits, and so does a mixed pixel with no found layer.  The kernel reads only pure pixels and its own pixel
 * and writes only mixed pixels, so in place is race-free and deterministic.  *resolved_pixels (may be NULL) = the pixels rewritten.
 * Stale layers are rendered first, inside kernel_ms, with the G of the last rtiow_render_coverage, or 4 if there was none; so are stale
 * guides.  kernel_ms == NULL and resolved_pixels == NULL: asynchronous on the handle's stream.
 * RTIOW_E_BADARG: radius outside 1..3, a sigma <= 0 or NaN, prior <= 0 or NaN.  RTIOW_E_STATE: no denoised image; an image already
 * resolved (a second pass would blend twice: filter again); a sharded handle; the temporal image stale when the denoised image came from
 * it (resolve before rtiow_history_commit); a chunk or a reset of the accumulation since the filter ran.  A failing call leaves the
 * handle as it was.  The call touches nothing but the denoised buffer: framebuffer, accumulation, counts and errors, guides, temporal
 * image, base, plan, the bits of the next chunk.  Not available on groups. */
int rtiow_render_coverage(rtiow_handle h, int subsamples_per_side, float* kernel_ms);
int rtiow_read_coverage(rtiow_handle h, int32_t* ids /* npix*2 */, int32_t* counts /* npix*2 */, void* normal /* npix*2*3 T */, void* depth /* npix*2 T */,
                        size_t npix);
int rtiow_resolve_edges(rtiow_handle h, int radius, double sigma_normal, double sigma_depth, double prior, float* kernel_ms, uint64_t* resolved_pixels);

/* ---- Lens-sampled filter guides.  The guides above are traced through a pinhole, while the image the filters
 * work on is rendered through the camera's lens: where the circle of confusion spans pixels the colour is a smooth mix of what the
 * aperture sees and the guides still show one hard edge.  With this knob on, the FILTER guides -- what rtiow_denoise,
 * rtiow_denoise_variance, rtiow_denoise_history, rtiow_denoise_history_variance and rtiow_history_commit_filtered steer by and
 * rtiow_read_filter_guides reads -- are the mean of the guide values over S = G G rays from a fixed lattice of points on the defocus
 * disk through the pixel centre on the focus plane: the rays rtiow_render draws, without their randomness.
 * Everything in T, left to right as written, plain * + - / and a correctly rounded sqrt, no fused multiply-add.  Local pixel (i, jl) with
 * global row j, G = samples_per_side, lens sample s = a + G b (b outer), a, b in 0..G-1:
 *   o_a = (T)(2a + 1) / (T)G - 1 and o_b likewise (-+0.5 for G = 2; -+0.75, -+0.25 for G = 4: exact).
 *   kappa = (T)1 for G = 2, (T)0.8944271909999159 for G = 4 (sqrt(0.8): the lattice's second moment per axis is 1/4, the uniform unit
 *   disk's, and every point lies inside the disk).  lx = kappa o_a, ly = kappa o_b.
 *   O_s = (O + lx U) + ly V per component, O the camera centre, U, V = defocus_disk_u, defocus_disk_v as the camera struct holds them.
 *   ps = (pixel00 + (T)i du) + (T)j dv, the ray target of rtiow_render_guides.  D_s = ps - O_s.
 *   (normal'_s, albedo'_s, depth'_s, b_s) = the chain of rtiow_set_guide_mode's block above started from (O_s, D_s), with the handle's
 *   max_fuzz and max_bounces in RTIOW_GUIDES_SPECULAR; in RTIOW_GUIDES_FIRST_HIT with max_bounces = 0, i.e. ended at its first hit:
 *   rtiow_render_guides' values to the letter (normal facing the ray, albedo {r,g,b} or {1,1,1} for a dielectric, depth t, 0 on a miss).
 *   From 0 in s order, per component: Ns = Ns + normal'_s, As = As + albedo'_s, Zs = Zs + depth'_s.  q = (T)1 / (T)S (exact).
 *   normal = Ns q, albedo = As q, depth = Zs q, bounces = the largest b_s.  The normal is not renormalised: a blurred normal is shorter,
 *   and that is the information.  A ray that misses adds zeros.
 * rtiow_set_guide_lens(h, G): G = 0 (off, the default of a new handle), 2 or 4; anything else, or a NULL handle: RTIOW_E_BADARG.  A knob
 * like rtiow_set_guide_mode and orthogonal to it: it survives rtiow_set_scene, rtiow_set_camera and rtiow_set_shard; a call that changes
 * nothing does nothing; one that changes the value makes the guides (both sets) and the denoised image stale and leaves the accumulation
 * and its count, the history base, the temporal image, the plan and the coverage layers alone.  The lattice takes effect when guides are
 * rendered -- rtiow_render_guides, and the stale guides a filter, an update or a filtered commit renders first -- and only if
 * (double)defocus_angle > 0, the test rtiow_render makes before it samples the lens: with a pinhole camera the knob is accepted and
 * inert, the filter guides are the guide mode's bit for bit and no further kernel runs.  In effect, the lens guides live in the second
 * pair of buffers in either guide mode (allocated at first use; freed again in RTIOW_GUIDES_FIRST_HIT with the knob back at 0) and
 * rtiow_read_filter_guides returns them.  The first-hit guides, the reprojection, the plan, the coverage layers, rtiow_resolve_edges, the
 * accumulation and every output with the knob off are untouched.  Not available on groups. */
int rtiow_set_guide_lens(rtiow_handle h, int samples_per_side /* 0: off (default), 2 or 4 */);

/* ---- Scene edits that keep the history: reprojection through sphere motion.  rtiow_set_scene empties the
 * history base, so a viewer that nudges one sphere restarts every pixel from the noise of its few samples although almost every pixel
 * still shows the surface it showed a frame ago.  rtiow_edit_scene changes the spheres and keeps the base; the updates then carry the
 * history of a moved sphere along with it.  The base keeps its format and holds no ids.
 * The snapshot.  rtiow_history_commit and rtiow_history_commit_filtered also keep, on the host, the tables of the scene current at the
 * commit: per kept sphere k (invalid slots dropped, numbered as rtiow_read_coverage numbers them) {C'_k, r'_k} and the material record
 * -- type, the 4 T of albedo_fuzz, refraction_index -- as the bits of T.  It goes wherever the base goes: rtiow_history_reset,
 * rtiow_set_scene and rtiow_set_shard drop it.
 * rtiow_edit_scene takes rtiow_set_scene's arguments and is rtiow_set_scene in every respect -- tables uploaded, screen and grid tables
 * rebuilt at the next render, the accumulation back to 0, guides, coverage layers, plan, temporal image and denoised image stale, the
 * carried hand-out order dropped, the stats' meaning -- except that the history base and its snapshot survive.  With a base, MOTION IS
 * IN EFFECT from the call until the next commit (which takes a new snapshot), rtiow_history_reset, rtiow_set_scene or rtiow_set_shard,
 * whether or not any value changed.  Without a base the call is a rtiow_set_scene of the same shape.  Against the snapshot, bits against
 * bits: moved_k = any of the 4 T of {C_k, r_k} differs; changed_k = the material record differs.
 * RTIOW_E_BADARG: a NULL handle (-1 before any device work); a null or empty table; an n other than the current scene's; a `valid` that
 * keeps other slots than the current scene keeps (kept spheres must correspond index for index); a material type outside 0..2.
 * RTIOW_E_STATE: no scene yet.  A failing call leaves the handle as it was.  Not available on groups.
 * The motion plane.  While motion is in effect it is rendered wherever the first-hit guides are (rtiow_render_guides, and the stale guides
 * a filter, an update, a plan or a filtered commit renders first) and goes stale with them.  Everything in T, left to right as written,
 * plain * + - /, no fused multiply-add.  For local pixel p: (t, k) = hit_world(O, D) of rtiow_render_guides, the same ray and the same
 * values as the guides' depth.
 *   a miss:             id = -1, Q = 0, carry = 1.
 *   a hit, changed_k:   id = k,  Q = 0, carry = 0: a surface that changed colour or kind carries nothing.
 *   a hit, not moved_k: id = k,  Q = O + t D per component, carry = 1: the expression the update forms from the depth, so the same bits.
 *   a hit, moved_k:     id = k,  P = O + t D, o = (P - C_k) * ((T)1 / r_k) per component (the guides' outward), Q = C'_k + r'_k o per
 *                       component, carry = 1: the point of the sphere's old surface that this point came from, under translation and
 *                       scaling about the centre.
 * rtiow_read_scene_motion copies planes: prev_point npix x 3 T (Q), carry and ids npix int32 (any pointer may be NULL).
 * npix != local_rows x width: RTIOW_E_BADARG.  RTIOW_E_STATE: motion is not in effect, or the plane is stale.  Rows are global, as in
 * rtiow_read_guides; a base needs an unsharded handle, so a handle of several ranks never has motion in effect.
 * The gather through motion.  While motion is in effect rtiow_history_update, rtiow_history_update_clipped and rtiow_history_plan are
 * their definitions above with exactly two changes at a hit pixel: d = Q_p - O' instead of (O + t_p D) - O', and carry_p == 0 means no
 * taps (m = 0).  Everything after d is unchanged: den, s, u, v, te, the taps and their tests, the cap, the blend, the clip, the
 * counters.  The normal test needs no change: translation and scaling about the centre keep the normal of corresponding points.  So:
 * a pixel whose first hit is the sky or a sphere that neither moved nor changed has the plain call's bits; a pixel that now sees what
 * the moved sphere used to hide fails the depth test against the base and gets m = 0, so rtiow_accumulate_budget samples it; and the
 * plan still predicts Mout bit for bit.  With motion not in effect every call is what it was, bit for bit.
 * Out of scope: rotation (meaningless for uniform spheres), added or removed spheres, motion-aware coverage layers and lens guides.
 * Pixels that only reflect, refract or are shadowed by an edited sphere: rtiow_set_edit_influence, below. */
int rtiow_edit_scene(rtiow_handle h, int n, const void* center_radius, const void* albedo_fuzz,
                     const void* refraction_index, const int32_t* type, const int32_t* valid);
int rtiow_read_scene_motion(rtiow_handle h, void* prev_point /* npix*3 T */, int32_t* carry /* npix */, int32_t* ids /* npix */, size_t npix);

/* ---- Edit influence: shorten the history where a scene edit changes the light.  The motion plane looks at
 * a pixel's first hit only.  The ground under a moved sphere, a neighbour that took its colour bleed, a mirror that shows it: their first
 * hit was not edited, they pass every test of the gather and carry a full-length history of the wrong light.  The sky is the only light,
 * so the irradiance at a point changes by at most the share of its surroundings that the edited spheres occupy, before and after the edit.
 * rtiow_set_edit_influence records kappa: 0 is off (a handle's default; every call is then what it was, bit for bit), kappa > 0 is on,
 * +inf drops the history wherever there is any influence at all.  NaN or negative: RTIOW_E_BADARG; a NULL handle: -1.  Allowed in every
 * state, on shards too; the value survives set_scene / _camera / _shard.  Another value than the handle has makes the motion plane, the
 * guides it is rendered with, the plan, the temporal image and the denoised image stale; the same value changes nothing.
 * The edit list.  rtiow_edit_scene with motion in effect keeps, through the kept spheres in ascending k: moved_k (with or without
 * changed_k): two entries, {C'_k, r'_k} of the snapshot, then {C_k, r_k} of the current scene; changed_k only: one entry, {C_k, r_k};
 * neither: none.  Each entry has the owner k.
 * The influence plane.  While motion is in effect and kappa > 0 it is written wherever the motion plane is.  Everything in T, left to
 * right as written, plain * + - / and sqrt, no fused multiply-add.  For local pixel p with guides' depth t_p, motion plane carry_p, id k_p:
 *   a miss (depth == 0) or carry_p == 0:  lambda_p = 0
 *   otherwise:  P = O + t_p D per component (as rtiow_history_update forms it), s = 0, and for every entry e in list order with
 *               owner_e != k_p:  v = C_e - P, d2 = (v.x v.x + v.y v.y) + v.z v.z, q = (r_e r_e) / d2,
 *                                omega = q >= 1 ? 1 : 1 - sqrt(1 - q)  (NaN compares false),  s = s + omega;
 *               lambda_p = s > 0 ? min(1, kappa s) : 0, with kappa rounded once to T.
 *   fade_p = carry_p == 0 ? 0 : 1 - lambda_p replaces carry_p in the motion plane.
 * omega is twice the share of the full sphere of directions around P that the entry occupies.  A pixel's own sphere is skipped (its
 * history is the motion plane's business), sky pixels never fade, an empty list gives lambda = 0 everywhere.
 * The gathers.  rtiow_history_update, rtiow_history_update_clipped and rtiow_history_plan through the motion plane gain one operation
 * after the cap: m = m * fade_p.  fade_p == 0 takes no taps, as carry_p == 0 does.  The plan still predicts Mout - n bit for bit, so
 * rtiow_accumulate_budget samples the faded pixels more, and the clipped update clamps what is left.  rtiow_read_scene_motion answers
 * carry as (fourth component != 0).
 * rtiow_read_edit_influence copies lambda, npix T.  npix != local_rows x width: RTIOW_E_BADARG.  RTIOW_E_STATE: motion is not in effect,
 * kappa == 0 (no plane is made then), or the plane is stale (rtiow_render_guides).  Rows are global, as in rtiow_read_scene_motion.
 * Out of scope: added or removed spheres, a horizon or cosine term in omega, following the specular chain, fading coverage layers or
 * lens guides, groups. */
int rtiow_set_edit_influence(rtiow_handle h, double kappa /* 0: off; > 0: on */);
int rtiow_read_edit_influence(rtiow_handle h, void* lambda /* npix T */, size_t npix);

/* ---- Scene edits that add and remove spheres without restarting the history.  rtiow_edit_scene accepts a
 * scene of the current shape only, because it matches the spheres of the current scene with those of the snapshot index for index.
 * rtiow_edit_scene_mapped takes the correspondence from the caller, so the new scene may have any n and any `valid`.  No kernel is added
 * or changed: the motion plane and the edit influence read per-sphere tables that the host builds through the map.
 * rtiow_edit_scene_mapped is rtiow_edit_scene in every respect it documents -- tables uploaded, screen and grid tables rebuilt at the next
 * render, the accumulation back to 0, guides, coverage layers, plan, temporal image and denoised image stale, the carried hand-out order
 * dropped, the base and its snapshot kept, motion in effect from the call until the next commit, rtiow_history_reset, rtiow_set_scene or
 * rtiow_set_shard; without a base a rtiow_set_scene of the new tables -- except for the shape.  rtiow_edit_scene itself is unchanged.
 * origin[i], for every slot i that `valid` keeps, names the slot OF THE SCENE THE HANDLE HOLDS NOW that slot i continues, or is -1 for a
 * new sphere.  origin[i] of a dropped slot is not read.  A kept sphere of the current scene that no slot continues is removed.
 * The map.  The handle keeps from_snapshot[k] per kept sphere k of the current scene: the number j of the sphere it continues among the
 * kept spheres of the snapshot, or -1.
 *   both commits:               the identity (they take the snapshot).
 *   rtiow_edit_scene:           left alone.
 *   rtiow_history_reset, rtiow_set_scene, rtiow_set_shard: dropped with the snapshot.
 *   rtiow_edit_scene_mapped:    for kept slot i of the new scene, numbered k': origin[i] == -1: from_snapshot'[k'] = -1; origin[i] == s,
 *                               s numbered k in the current scene: from_snapshot'[k'] = from_snapshot[k].
 * So mapped edits between two commits compose, and a sphere added and then moved before the next commit still has no origin.  Without a
 * base no map is kept.
 * The tables.  Per kept sphere k of the current scene with j = from_snapshot[k]:
 *   j >= 0:   moved_k and changed_k from the current record of k against the snapshot's record of j, bits against bits, and {C'_j, r'_j}
 *             in the motion plane's table: section 19 with j in the place of k.
 *   j == -1:  changed_k alone and four zeros of T: the motion plane gives the sphere's pixels Q = 0, carry = 0, id = k.
 * A removed sphere has no entry in either table: the pixel that now sees what it hid reprojects to a base pixel that holds the removed
 * sphere's depth and normal, fails the gather's tests and gets m = 0, as a pixel does that a moved sphere uncovers.
 * The edit list (rtiow_set_edit_influence), in two passes.
 *   pass 1, the kept spheres of the current scene in ascending k, owner k: moved_k: {C'_j, r'_j}, then {C_k, r_k}; changed_k only -- an
 *           added sphere is this case: {C_k, r_k}; neither: none.
 *   pass 2, the kept spheres j of the snapshot in ascending order that no current sphere continues: {C'_j, r'_j} with the owner -2.
 * A hit pixel's id is >= 0 and a miss has lambda = 0, so no pixel skips an entry of owner -2 as its own.
 * RTIOW_E_BADARG and RTIOW_E_STATE, asked in this order before anything is touched: a NULL handle (-1 before any device work); a null or
 * empty table or n <= 0; no scene yet (RTIOW_E_STATE); origin == NULL; for a kept slot, an origin[i] below -1, at or above the current
 * scene's slot count, or naming a slot the current scene drops; two kept slots naming the same origin (a sphere is continued at most
 * once: no duplication); a material type outside 0..2 on a kept slot, or no kept slot at all.  A failing call leaves the handle as it
 * was.  Not available on groups; on a handle of several ranks there is never a base, so the call is a rtiow_set_scene there.
 * rtiow_read_scene_origin copies the map, `count` int32 (the pointer may be NULL).  RTIOW_E_STATE: motion is not in effect.  A count other
 * than the number of kept spheres: RTIOW_E_BADARG.
 * Out of scope: duplicating a sphere, motion-aware coverage layers and lens guides, groups and sharded bases. */
int rtiow_edit_scene_mapped(rtiow_handle h, int n, const void* center_radius, const void* albedo_fuzz,
                            const void* refraction_index, const int32_t* type, const int32_t* valid,
                            const int32_t* origin /* n */);
int rtiow_read_scene_origin(rtiow_handle h, int32_t* from_snapshot /* kept spheres */, size_t count);

/* ---- Guided upscaling: a preview at a multiple of the traced resolution.  Every buffer above has the
 * camera's img_width x img_height; rtiow_upscale writes an image F = factor times as wide and as high from the frame that was traced.
 * Every output pixel traces one primary ray of its own and gathers the colour of the four traced pixels around it, weighed by what that
 * ray hit.  Everything in T, left to right as written, plain * + - /, a correctly rounded sqrt, no fused multiply-add.
 * W, H = the camera's frame.  Output pixel (I, J) of the F W x F H image: i = I / F, a = I - F i; j, b likewise.
 * The ray is rtiow_render_coverage's sub-sample ray with G = F, to the letter: o_a = ((T)a + 0.5) / (T)F - 0.5 and o_b likewise,
 *   fx = (T)i + o_a, fy = (T)j + o_b, D = ((pixel00 + fx du) + fy dv) - O, (t, k) = hit_world(O, D).  On a hit N, A, Z are
 *   rtiow_render_guides' normal (facing the ray), albedo ({1,1,1} for a dielectric) and depth t; on a miss k = -1, N = A = 0, Z = 0.
 * The taps.  x0 = o_a < 0 ? i - 1 : i, gx = o_a < 0 ? (T)1 + o_a : o_a; y0, gy likewise.  The traced pixels q = (x0, y0), (x0 + 1, y0),
 *   (x0, y0 + 1), (x0 + 1, y0 + 1), in this order, with b = ((T)1 - gx)((T)1 - gy), gx ((T)1 - gy), ((T)1 - gx) gy, gx gy.  A tap counts
 *   when q is inside the frame, b > 0 and q holds colour.  By source:
 *     RTIOW_UPSCALE_DENOISED  always;                                c_q = g_q g_q per channel, g the denoised image as stored
 *     RTIOW_UPSCALE_LINEAR    n_q > 0 (rtiow_read_linear's count);   c_q = rtiow_read_linear's value
 *     RTIOW_UPSCALE_HISTORY   Mout_q > 0;                            c_q = Cout_q of the temporal image
 * The weight.  N_q, A_q, Z_q = the FIRST-HIT guides of q, in either guide mode and whatever rtiow_set_guide_lens is set to.  d = N_q - N,
 *   en = (d.x d.x + d.y d.y) + d.z d.z; ea the same of the albedo; dz = Z_q - Z, ez = dz dz; e = (en i_n + ea i_a) + ez i_z with
 *   i_* = (T)(1 / sigma_*^2) computed in double and rounded once (sigma = +inf turns a term off); w = b / ((T)1 + e).  From 0 in tap
 *   order: S1 = S1 + w c_q per channel, W1 = W1 + w.
 * The share, with use_coverage = 1.  (id_0, id_1, c_0, c_1) = the coverage layers of q, S their G G.  m = id_0 == k ? c_0 :
 *   (id_1 == k ? c_1 : 0); when m > 0: wp = w * ((T)m / (T)S), Sp = Sp + wp c_q, Wp = Wp + wp.  A traced pixel's colour is an area mix;
 *   this weighs a tap by how much of it is the surface the output pixel sees (the sky is k = -1 and matches sky layers).
 * The result.  Wp > 0: out = Sp / Wp; otherwise W1 > 0: out = S1 / W1; otherwise 0.  Stored per channel: out > 0 ? sqrt(out) : 0.
 *   *covered_pixels (may be NULL) = the output pixels with Wp > 0; 0 with use_coverage = 0.
 * Stale guides are rendered first, inside kernel_ms; with use_coverage = 1 so are stale layers, with the G of the last
 * rtiow_render_coverage, or 4 if there was none (G is independent of F).  kernel_ms == NULL and covered_pixels == NULL: asynchronous on
 * the handle's stream.  The output buffer is the handle's own: allocated at first use, regrown for a larger F, freed by rtiow_destroy.
 * rtiow_read_upscaled copies it, (F local_rows) x (F width) x 3 T, gamma-encoded like the preview; rtiow_upscaled_device_ptr gives its
 * address and size.
 * RTIOW_E_BADARG: factor outside 2..4; source outside 0..2; a sigma <= 0 or NaN; use_coverage not 0 or 1; an output wider or higher than
 * 2^31 - 8 pixels or of more than 2^31 - 4 8x8 tiles, the kernel's int coordinates and tile count (the text says which; within them the
 * byte size fits its size_t index); in the two readers, bytes other than the buffer's.
 * RTIOW_E_STATE: before scene and camera are set; DENOISED before a filter has run; LINEAR without a chunk; HISTORY with a stale temporal
 * image; a sharded handle; in the readers, before an rtiow_upscale or once the image is stale.  A NULL handle: -1 before any device work.
 * A failing call leaves the handle as it was.
 * The upscaled image goes stale with rtiow_set_scene, rtiow_edit_scene(_mapped), rtiow_set_camera and rtiow_set_shard and with nothing
 * else: it is a finished output and survives chunks, filters, updates, commits and the guide knobs.  The call reads the framebuffer's
 * sources -- accumulation and counts, denoised image, guides, layers, temporal image -- and writes only its own buffer: every existing
 * path keeps its bits.  Not available on groups. */
#define RTIOW_UPSCALE_DENOISED 0   /* the buffer of rtiow_read_denoised, whichever filter (or rtiow_resolve_edges) wrote it last */
#define RTIOW_UPSCALE_LINEAR   1   /* the linear colour of the accumulation (rtiow_read_linear) */
#define RTIOW_UPSCALE_HISTORY  2   /* the colour Cout of the temporal image (rtiow_read_history) */
int rtiow_upscale(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth,
                  int use_coverage, float* kernel_ms, uint64_t* covered_pixels);
int rtiow_read_upscaled(rtiow_handle h, void* host_rgb, size_t bytes);      /* (F rows) x (F W) x 3 T, gamma-encoded like the preview */
int rtiow_upscaled_device_ptr(rtiow_handle h, void** device_ptr, size_t* bytes);

/* ---- Wide-support guided upscaling: rtiow_upscale with a 4 x 4 cubic B-spline gather.  rtiow_upscale's four
 * bilinear taps average less than plain interpolation does once an edge-stop takes weight from some of them; sixteen taps under a smooth,
 * non-negative kernel average more where nothing stops them and still refuse taps across a silhouette.
 * Everything in T, left to right as written, plain * + - /, a correctly rounded sqrt, no fused multiply-add.
 * rtiow_upscale's, to the letter: the output pixel (I, J), i, a, j, b, o_a, o_b, the ray, hit_world, k, N, A, Z;
 *   x0 = o_a < 0 ? i - 1 : i, gx = o_a < 0 ? (T)1 + o_a : o_a; y0, gy likewise.
 * The taps.  The 16 traced pixels q = (x0 - 1 + u, y0 - 1 + v), u, v = 0..3, in row-major order (v outer, u inner).  Per axis, from
 *   g (gx or gy) and h = (T)1 - g, the cubic B-spline:
 *     c[0] = ((h*h)*h) / (T)6
 *     c[1] = ((((T)3*g - (T)6)*g)*g + (T)4) / (T)6
 *     c[2] = ((((T)3*h - (T)6)*h)*h + (T)4) / (T)6
 *     c[3] = ((g*g)*g) / (T)6
 *   b = cy[v] * cx[u].  The kernel is non-negative, so sqrt and the test b > 0 keep their meaning (g = 0: c[3] = 0, a 3 x 3 gather).
 *   A tap counts when q is inside the frame -- tested before any load --, b > 0 and q holds colour, by rtiow_upscale's rule per source.
 * rtiow_upscale's unchanged: c_q per source; e, w = b / ((T)1 + e), S1, W1 from 0 in tap order; the share (m, wp, Sp, Wp); the result;
 *   the gamma store; *covered_pixels; the guides are the FIRST-HIT buffers whatever the guide mode and lens knob; stale guides and, with
 *   the share, stale layers are rendered first inside kernel_ms; both out-pointers NULL: asynchronous on the handle's stream.
 * The call writes the handle's upscaled buffer: rtiow_read_upscaled and rtiow_upscaled_device_ptr serve whichever of rtiow_upscale and
 * rtiow_upscale_wide (or of their _large twins below) ran last, and the image goes stale by the same rule.
 * Refusals: rtiow_upscale's, in its order, under this call's name; a sharded handle is refused; not available on groups.  A NULL
 * handle: -1 before any device work.  A failing call leaves the handle as it was. */
int rtiow_upscale_wide(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth,
                       int use_coverage, float* kernel_ms, uint64_t* covered_pixels);

/* ---- Large scenes: rtiow_render through a uniform grid walked in device memory.
 * rtiow_render is fast while a scene's tables fit a compute unit's LDS; beyond that (about 5 100 spheres in fp32, 3 400 in fp64) it reads
 * the scene through the exact loop over every sphere (rtiow_stats.scene_source == RTIOW_SCENE_SCALAR).  rtiow_render_large renders the
 * same frame -- same framebuffer, shard, RNG states (read from where rtiow_init_rng left them and left there, as by rtiow_render), rtiow_stats -- with only the spheres too big for a grid cell in LDS and
 * everything else in a grid in device memory: variable-length cells of 32-bit sphere indices, no limit on spheres per cell, at most about
 * 190 x 190 cells (beyond that the lists grow).  Every pixel draws its numbers in the reference's order from its own state: the image is rtiow_render's bit for bit.
 * Opt-in: rtiow_render never selects it, the knobs of rtiow_set_scene_source and rtiow_set_schedule do not apply (the launch is the
 * persistent hand-out in tile order; rtiow_stats.schedule reads RTIOW_SCHED_PERSISTENT, scene_source RTIOW_SCENE_DEVICE_GRID, and the
 * grid_* fields describe the device grid).  Plan and device tables are built at the first call after rtiow_set_scene /
 * rtiow_edit_scene(_mapped), before the start event; the time goes to rtiow_stats.scene_prepare_ms.
 * kernel_ms NULL: asynchronous on the handle's stream.  RTIOW_E_BADARG, with the call's name in rtiow_last_error_string, without a
 * scene or a camera and when the grid does not suit the scene (fewer than 24 spheres, fewer than 16 of them small enough for a cell,
 * or a list of big spheres longer than max(8, n / 6) or 2048): use rtiow_render -- there is no silent fall-back.  RTIOW_E_STATE
 * before rtiow_init_rng.
 * The accumulate / adaptive / budget calls, every preview call and the groups keep rtiow_render's sources; the chunks, the guides, the
 * coverage layers and the two upscalers have _large twins of their own (below). */
int rtiow_render_large(rtiow_handle h, float* kernel_ms);
typedef struct {
    int32_t  usable;             /* 1: rtiow_render_large renders this scene; 0: it refuses (every other field is then 0)  */
    int32_t  nx, nz;             /* cells along x and z                                                                    */
    double   cell;               /* cell width                                                                             */
    double   rfar;               /* origins farther than this from the scene's centre send their wave through the exact loop */
    int32_t  registered;         /* spheres in cells (each in up to 2 x 2 of them)                                         */
    int32_t  direct;             /* spheres too big for a cell: in LDS, tested by every ray                                */
    uint64_t index_entries;      /* length of the index array: the sum of the cells' list lengths                          */
    int32_t  longest_list;       /* spheres in the fullest cell                                                            */
    int32_t  reserved;
    uint64_t blob_bytes;         /* device memory of cells, indices, sphere table and direct list                          */
} rtiow_large_grid_info;
/* The device grid of the handle's scene in the handle's precision, built here if no rtiow_render_large has built it yet (host work and one
 * upload; no kernel).  RTIOW_E_BADARG without a scene. */
int rtiow_read_large_grid(rtiow_handle h, rtiow_large_grid_info* out);

/* ---- The preview chain on large scenes: chunks, guides and coverage layers through the device grid.
 * Five opt-in calls, each the twin of the call it is named after: the same buffers, state, checks, refusals (under the new name) and bits,
 * with the scene read through the device grid of rtiow_render_large instead of the handle's scene source.  A _large call and its twin
 * are interchangeable at every point of a session: a chunk through the grid may follow a chunk through rtiow_accumulate and the other way
 * round, and every filter, the history, the plan, the edge resolve and the upscalers read what a _large call left exactly as they read
 * what the twin leaves.  rtiow_stats reports scene_source == RTIOW_SCENE_DEVICE_GRID and the grid_* fields as after rtiow_render_large.
 * A scene the device grid does not suit is refused as rtiow_render_large refuses it, RTIOW_E_BADARG with the text
 * "<call>: the device grid does not suit this scene (...); use <twin>", after the twin's own checks of state and arguments and before
 * anything changes; it is never rendered another way.  The calls remember nothing: a filter call that finds the guides or the layers
 * stale renders them through the handle's scene source, as today, so the caller renders them with the _large call after each change of
 * camera or scene.  Not available on groups. */
/* rtiow_accumulate (threads_per_block_row has no twin: chunks always run through the persistent hand-out). */
int rtiow_accumulate_large(rtiow_handle h, int samples, float* kernel_ms);
/* rtiow_accumulate_adaptive. */
int rtiow_accumulate_adaptive_large(rtiow_handle h, int samples, int min_samples, double rel_error, int max_samples, float* kernel_ms, int* active_pixels);
/* rtiow_accumulate_budget: RTIOW_E_STATE before a plan that is current. */
int rtiow_accumulate_budget_large(rtiow_handle h, int samples, int min_samples, double target, int max_samples, float* kernel_ms, int* active_pixels);
/* rtiow_render_guides: the first-hit guides, then the lens guides or else the specular chain, then the motion plane while an edit is in
 * effect and the edit influence behind it: what rtiow_render_guides launches, in its order and under its conditions. */
int rtiow_render_guides_large(rtiow_handle h, float* kernel_ms);
/* rtiow_render_coverage: subsamples_per_side 2 or 4. */
int rtiow_render_coverage_large(rtiow_handle h, int subsamples_per_side, float* kernel_ms);

/* ---- Guided upscaling on large scenes: the upscalers through the device grid.
 * rtiow_upscale and rtiow_upscale_wide trace one primary ray for every output pixel through the handle's scene source: on a scene beyond
 * the LDS that is the exact loop over every sphere, factor x factor times per traced pixel.  These two opt-in calls are their twins in
 * the sense of the five calls above -- the same buffers, state, checks, refusals (under the new name), image and *covered_pixels, bit for
 * bit -- with that ray traced through the device grid of rtiow_render_large.  They write the handle's upscaled buffer:
 * rtiow_read_upscaled and rtiow_upscaled_device_ptr serve whichever of the upscale calls ran last, and the image goes stale by
 * rtiow_upscale's rule and by nothing else.  Stale guides and, with use_coverage, stale layers are rendered first inside kernel_ms as by
 * the twin, but through rtiow_render_guides_large and rtiow_render_coverage_large (the layers at the twin's subsamples_per_side): other
 * kernels, the same bits.  rtiow_stats reports scene_source == RTIOW_SCENE_DEVICE_GRID and the grid_* fields afterwards.
 * Refusals: the twin's, in its order, under this call's name (a sharded handle among them); behind them, and before anything changes --
 * an image of an earlier call stays readable with its bits --, a scene the device grid does not suit: RTIOW_E_BADARG, "<call>: the
 * device grid does not suit this scene (...); use <twin>".  There is no silent fall-back.  The LDS refusal of the twin stays, in front
 * of the buffers.  A NULL handle: -1 before any device work.  Not available on groups. */
/* rtiow_upscale. */
int rtiow_upscale_large(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth,
                        int use_coverage, float* kernel_ms, uint64_t* covered_pixels);
/* rtiow_upscale_wide. */
int rtiow_upscale_wide_large(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth,
                             int use_coverage, float* kernel_ms, uint64_t* covered_pixels);

/* ---- Volume scenes: rtiow_render through a THREE-axis uniform grid walked in device memory.
 * The device grid of rtiow_render_large runs over x and z and holds the y extent as one slab: a scene that fills a volume (a particle
 * cloud, a molecule, a stack of layers) puts a whole column of spheres into every cell's list.  rtiow_render_volume is rtiow_render_large
 * over a grid of nx x ny x nz cells of its own: the same framebuffer, shard, RNG states (read from where rtiow_init_rng left them and
 * left there), timing and rtiow_stats, and the image is rtiow_render's bit for bit.  Opt-in: no call selects it, and the knobs of
 * rtiow_set_scene_source and rtiow_set_schedule do not apply (rtiow_stats.schedule reads RTIOW_SCHED_PERSISTENT, scene_source
 * RTIOW_SCENE_VOLUME_GRID; grid_nx, grid_nz, grid_cell, grid_registered and grid_direct describe the volume grid, rtiow_read_volume_grid
 * has ny).  Plan and device tables are built at the first call after rtiow_set_scene / rtiow_edit_scene(_mapped), before the start event;
 * the time goes to rtiow_stats.scene_prepare_ms.  The grid of rtiow_render_large and this one may both exist on a handle.
 * kernel_ms NULL: asynchronous on the handle's stream.  Refusals: rtiow_render_large's, in its order, under this call's name; a scene
 * the volume grid does not suit (fewer than 24 spheres, fewer than 16 small enough for a cell, or a list of big spheres longer than
 * max(8, n / 6) or 2048) gets RTIOW_E_BADARG and "rtiow_render_volume: the volume grid does not suit this scene (...); use rtiow_render"
 * -- there is no silent fall-back.  RTIOW_E_STATE before rtiow_init_rng.  A NULL handle: -1 before any device work.
 * The chunks, guides, coverage layers and upscalers have _volume twins of their own (below).  Not available on groups. */
int rtiow_render_volume(rtiow_handle h, float* kernel_ms);
typedef struct {
    int32_t  usable;             /* 1: rtiow_render_volume renders this scene; 0: it refuses (every other field is then 0)  */
    int32_t  nx, ny, nz;         /* cells along x, y and z                                                                  */
    double   cell;               /* cell width                                                                              */
    double   rfar;               /* origins farther than this from the scene's centre send their wave through the exact loop */
    int32_t  registered;         /* spheres in the grid                                                                     */
    int32_t  direct;             /* spheres too big for a cell: tested by every ray                                         */
    uint64_t index_entries;      /* entries of the index array (a sphere is listed in at most 8 cells)                      */
    uint64_t occupied_cells;     /* cells with a list                                                                       */
    int32_t  longest_list;       /* spheres in the fullest cell                                                             */
    int32_t  reserved;
    uint64_t blob_bytes;         /* device memory of cells, indices, sphere table and direct list                           */
} rtiow_volume_grid_info;
/* The volume grid of the handle's scene in the handle's precision, built here if no rtiow_render_volume has built it yet (host work and
 * one upload; no kernel).  RTIOW_E_BADARG without a scene. */
int rtiow_read_volume_grid(rtiow_handle h, rtiow_volume_grid_info* out);

/* ---- A session on a volume scene: chunks, guides, coverage layers and both upscalers through the volume grid (INTEGRATION.md
 * section 28).  Seven opt-in calls, each the twin of the call it is named after in the sense of the _large calls above: the same
 * parameters, buffers, preview state, checks, refusals (under the new name), statistics and bits, with the scene read through the volume
 * grid of rtiow_render_volume instead of the handle's scene source.  A _volume call, its twin and its _large twin are interchangeable at
 * every point of a session.  rtiow_stats reports scene_source == RTIOW_SCENE_VOLUME_GRID and the grid_* fields as after
 * rtiow_render_volume.  A scene the volume grid does not suit is refused as rtiow_render_volume refuses it, RTIOW_E_BADARG with the text
 * "<call>: the volume grid does not suit this scene (...); use <twin>", after the twin's own checks of state and arguments and before
 * anything changes -- an image of an earlier call stays readable --; it is never rendered another way.  The chunk and guide calls
 * remember nothing: a filter call that finds the guides or the layers stale renders them through the handle's scene source, so the
 * caller renders them with the _volume call after each change of camera or scene.  The two upscalers render stale guides and, with
 * use_coverage, stale layers through rtiow_render_guides_volume and rtiow_render_coverage_volume; rtiow_read_upscaled and
 * rtiow_upscaled_device_ptr serve whichever of the six upscale calls ran last.  No call selects these by itself, and
 * rtiow_set_scene_source keeps refusing RTIOW_SCENE_VOLUME_GRID.  A NULL handle: -1 before any device work.  Not available on groups. */
/* rtiow_accumulate (threads_per_block_row has no twin: chunks always run through the persistent hand-out). */
int rtiow_accumulate_volume(rtiow_handle h, int samples, float* kernel_ms);
/* rtiow_accumulate_adaptive. */
int rtiow_accumulate_adaptive_volume(rtiow_handle h, int samples, int min_samples, double rel_error, int max_samples, float* kernel_ms, int* active_pixels);
/* rtiow_accumulate_budget: RTIOW_E_STATE before a plan that is current. */
int rtiow_accumulate_budget_volume(rtiow_handle h, int samples, int min_samples, double target, int max_samples, float* kernel_ms, int* active_pixels);
/* rtiow_render_guides: what it launches, in its order and under its conditions. */
int rtiow_render_guides_volume(rtiow_handle h, float* kernel_ms);
/* rtiow_render_coverage: subsamples_per_side 2 or 4. */
int rtiow_render_coverage_volume(rtiow_handle h, int subsamples_per_side, float* kernel_ms);
/* rtiow_upscale. */
int rtiow_upscale_volume(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth,
                         int use_coverage, float* kernel_ms, uint64_t* covered_pixels);
/* rtiow_upscale_wide. */
int rtiow_upscale_wide_volume(rtiow_handle h, int factor, int source, double sigma_normal, double sigma_albedo, double sigma_depth,
                              int use_coverage, float* kernel_ms, uint64_t* covered_pixels);

/* Framebuffer: `vec3 pixel_buffer[]` (main.cu:133-134), local_rows x width x 3 T, row-major.
 * By default device memory owned by the library; rtiow_bind_framebuffer lets the caller
 * supply device memory (e.g. a torch tensor that torch.distributed will gather). */
int rtiow_bind_framebuffer(rtiow_handle h, void* device_ptr, size_t bytes);
int rtiow_framebuffer_device_ptr(rtiow_handle h, void** device_ptr, size_t* bytes);
/* D2H copy of the local rows (replaces the managed-memory read at main.cu:373). */
int rtiow_read_framebuffer(rtiow_handle h, void* host_rgb, size_t bytes);
/* The writer's quantisation done on the device (main.cu:367, 374-376: int(256 * clamp(c, 0.000, 0.999)) per channel, in T, truncated) and
 * the local rows read back as one byte per channel: local_rows x width x 3 bytes, a quarter (fp32) or an eighth (fp64) of
 * rtiow_read_framebuffer's bytes.  *nan_channels = channels holding a NaN (their level is int(NaN), undefined in the reference; its x86 build
 * prints -2147483648): when it is not 0 the bytes of those channels mean nothing -- read the T framebuffer and use the T writer
 * (rtiow_host_write_ppm), which prints what the reference prints.  The host writers for levels: rtiow_host_write_ppm_levels. */
int rtiow_read_levels(rtiow_handle h, unsigned char* host_levels, size_t bytes, uint64_t* nan_channels);

/* ---- knobs / introspection */
int rtiow_set_scene_source(rtiow_handle h, int scene_source /* RTIOW_SCENE_* */);
/* waves_per_simd: 0 = as many resident waves as fit; 1..8 caps them (PERSISTENT only). */
int rtiow_set_schedule(rtiow_handle h, int schedule /* RTIOW_SCHED_* */, int waves_per_simd);
int rtiow_get_stats(rtiow_handle h, rtiow_stats* out);
int rtiow_synchronize(rtiow_handle h);
int rtiow_stream(rtiow_handle h, void** hip_stream);   /* the hipStream_t the handle launches on */
int rtiow_device(rtiow_handle h, int* device);

/* Test hooks (device RNG states, per-pixel costs, per-wave timeline, hit_world on caller-supplied rays, the scatter step on caller-supplied hit records, ...) are NOT part of this
 * library's ABI: include/rtiow_debug.h declares them and only the test build (librtiow_hip_debug.so, -DRTIOW_DEBUG_API) exports them. */

/* ======================================================================================
 * Multi-GPU inside one process (new work: the reference is single-GPU, main.cu:81).
 *
 * A group is ngpus handles -- one per device, each with its own stream -- that render the
 * interleaved row strips of ONE image (rtiow_set_shard(rank, ngpus, strip_rows)) and exchange
 * them exactly once, after the render: every device sends its strips to device 0 over RCCL
 * (ncclCommInitAll + one ncclGroupStart/End of ncclSend/ncclRecv pairs over xGMI; librccl.so is
 * dlopen'ed on first use) or, when RCCL is unavailable, with hipMemcpyPeerAsync; device 0
 * de-interleaves the strips into the full image.  The assembled image equals the single-GPU
 * image bit for bit (RNG streams are keyed by the global pixel index).
 *
 * The calls mirror the single-handle ones phase by phase, so a host main() keeps the reference's
 * ordering (main.cu:81-400): create, set_camera, set_scene, init_rng, render, read_framebuffer.
 * rtiow_group_render's kernel_ms is the reference's render_only figure for the slowest device;
 * the exchange is NOT inside it (it belongs to the read-back, like the managed-memory read at
 * main.cu:373) and is reported separately in rtiow_group_stats.
 * ====================================================================================== */
#define RTIOW_GATHER_AUTO 0   /* RCCL if it loads and initialises, else peer copies */
#define RTIOW_GATHER_RCCL 1   /* RCCL or fail                                        */
#define RTIOW_GATHER_PEER 2   /* hipMemcpyPeerAsync per device                       */
#define RTIOW_GATHER_HOST 3   /* every strip through a host bounce buffer (blocking copies): the last resort of RTIOW_GATHER_AUTO when a
                               * transport fails AT GATHER TIME (first ncclGroupEnd / send / recv, first peer copy): the group then falls back
                               * RCCL -> peer copies -> host inside the same call, drains the devices in between, and says so in
                               * rtiow_group_transport_note / rtiow_group_stats.gather_mode.  May also be requested outright. */
#define RTIOW_GROUP_MAX_STATS 16

typedef struct rtiow_group_s* rtiow_group;

typedef struct {
    int32_t  ngpus, strip_rows;
    int32_t  gather_mode;                       /* transport of the last gather: RTIOW_GATHER_RCCL | _PEER (0: none yet) */
    int32_t  rccl_version;                      /* ncclGetVersion() when RCCL is in use, else 0 */
    double   kernel_ms[RTIOW_GROUP_MAX_STATS];  /* per device: HIP-event time of its own kernels, last render */
    double   kernel_ms_max;                     /* = what rtiow_group_render returned */
    double   gather_ms;                         /* HIP events on device 0 around exchange + de-interleave, opened when the last render finished */
    uint64_t gather_bytes;                      /* bytes that arrived on device 0 */
    double   create_ms;                         /* wall time of rtiow_group_create: contexts, streams and -- RCCL -- ncclCommInitAll
                                                 * (seconds: topology discovery); like the reference's cudaSetDevice / event creation
                                                 * (main.cu:81-92) it lies BEFORE the end-to-end timer of the executables */
    int32_t  peer_links;                        /* peer mode: ranks whose device got direct access to device 0 enabled */
    int32_t  reserved;
} rtiow_group_stats;

/* devices == NULL: devices 0..ngpus-1.  A device may be listed more than once (ranks then share
 * it and the exchange uses copies: RCCL needs distinct devices) -- used to test the N-rank logic
 * on a one-GPU box. */
/* The transport is chosen and the RCCL communicator created here (seconds: keep it out of timed
 * regions; rtiow_group_stats.create_ms); RTIOW_GATHER_RCCL fails here (RTIOW_E_STATE) when RCCL cannot serve the
 * group.  RCCL prints a version banner on stdout when a process creates its first communicator: a caller whose
 * stdout is data (the executables' CSV fragment) points fd 1 elsewhere around this call -- the library does not. */
int rtiow_group_create(int ngpus, const int* devices, int precision, int strip_rows, int gather, rtiow_group* out);
const char* rtiow_group_create_error(void);   /* text for the calling thread's last failed rtiow_group_create */
int rtiow_group_destroy(rtiow_group g);
const char* rtiow_group_last_error_string(rtiow_group g);
int rtiow_group_size(rtiow_group g);
int rtiow_group_member(rtiow_group g, int rank, rtiow_handle* out);   /* borrowed: knobs, per-device stats */
int rtiow_group_set_scene(rtiow_group g, int n, const void* center_radius, const void* albedo_fuzz,
                          const void* refraction_index, const int32_t* type, const int32_t* valid);
int rtiow_group_set_camera(rtiow_group g, const void* camera);
int rtiow_group_set_scene_source(rtiow_group g, int scene_source);
int rtiow_group_set_schedule(rtiow_group g, int schedule, int waves_per_simd);
int rtiow_group_init_rng(rtiow_group g, uint64_t seed);
int rtiow_group_render(rtiow_group g, int threads_per_block_row, float* kernel_ms);
/* The exchange alone (device 0 then holds the full image, rtiow_group_framebuffer_device_ptr). */
int rtiow_group_gather(rtiow_group g);
int rtiow_group_framebuffer_device_ptr(rtiow_group g, void** device_ptr, size_t* bytes);
/* gather + D2H of the full width*height*3 T image. */
int rtiow_group_read_framebuffer(rtiow_group g, void* host_rgb, size_t bytes);
int rtiow_group_get_stats(rtiow_group g, rtiow_group_stats* out);
/* Why RTIOW_GATHER_AUTO fell back to peer copies ("" if it did not). */
const char* rtiow_group_transport_note(rtiow_group g);
#ifdef __cplusplus
}
#endif
#endif /* RTIOW_H */
