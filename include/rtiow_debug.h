/* rtiow_debug.h -- test hooks of the HIP render library.  NOT part of the product: librtiow_hip.so exports none of these; the test build
 * lib/librtiow_hip_debug.so (the same sources compiled with -DRTIOW_DEBUG_API, raytracingincuda_amd/build.py) does, and only tests/, the
 * study scripts and the profiling scripts load it (raytracingincuda_amd.api: Renderer(..., debug=True), load_hip_library(debug=True)). */
#ifndef RTIOW_DEBUG_H
#define RTIOW_DEBUG_H
#include "rtiow.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Device RNG states after rtiow_init_rng, as
 * local_pixels x 6 uint32 {v0..v4,d}; and elementwise device arithmetic probes that the
 * parity tests compare bit-for-bit with the host (op: 0 a/b, 1 sqrt(a), 2 fma(a,b,c),
 * 3 uniform(u32 a -> T), 4 a*b+c unfused). */
int rtiow_debug_read_rng(rtiow_handle h, uint32_t* host_states, size_t count_words);
/* After a render with RTIOW_SCHED_SORTED that sorted (rtiow_stats.phases == 2) or ran in a carried order (rtiow_stats.order_reused):
 * the costs of the last ranking -- per local pixel the prepass cost (path segments of its prepass samples) and the key the sort
 * ranked it by (the mean of that cost over the pixel's neighbourhood inside its row strip, in quarter segments).  count = local pixels. */
int rtiow_debug_read_costs(rtiow_handle h, uint32_t* own, uint32_t* smoothed, size_t count);
/* The hand-out order itself: what h->order holds now, whoever wrote it last -- the ranking of a two-phase RTIOW_SCHED_SORTED render (also
 * read after the renders that reused it, and after a counting run), the ranking of an rtiow_accumulate chunk, or the active list of an
 * rtiow_accumulate_adaptive chunk.  The render kernels take their pixels from these very slots, so the tests can hold the order to its
 * invariants (tests/test_handout_order.py): a permutation with padding only where the deal leaves holes, heavy first, neighbours adjacent.
 *   info12  {kind (RTIOW_ORDER_*), total_slots, solo_slots, total_pools, pools_per_block, deal_group, lane_cap, blocks (workgroups of the
 *           launch the order was dealt for), n_active (adaptive list), W, local_rows (the frame the order indexes), 0}: always written.
 *   order   total_slots entries, slot -> (local row << 16 | column) or -1 (padding); an adaptive list: n_active pixels, then -1 up to the
 *           next multiple of 64 (total_slots; 0 when nothing was active).  NULL: not wanted.
 *   slot_of W x local_rows entries, pixel -> slot (RTIOW_ORDER_RENDER only; anything else: pass NULL).
 *   keys    W x local_rows entries, what the ranking sorted by (the rankings only; an adaptive list: pass NULL).
 * A first call with NULL buffers gives the sizes.  Waits for the stream.  RTIOW_E_STATE: nothing has written an order on this handle, or
 * the order's buffers were reallocated since; RTIOW_E_BADARG: a buffer is too small or asks for what this kind of order does not have. */
#define RTIOW_ORDER_NONE 0
#define RTIOW_ORDER_RENDER 1
#define RTIOW_ORDER_ACCUMULATE 2
#define RTIOW_ORDER_ADAPTIVE 3
int rtiow_debug_read_order(rtiow_handle h, int32_t* info12, int32_t* order, size_t order_cap, int32_t* slot_of, uint32_t* keys, size_t pixel_cap);
/* The path segments every local pixel ran in the last rtiow_accumulate chunk: what the NEXT chunk's ranking smooths into its keys
 * (rtiow_debug_read_order after that chunk).  A call of its own rather than a field of rtiow_debug_read_order: the first chunk after a
 * reset is not ranked, so there is no order to read when its costs are wanted.  RTIOW_E_STATE without such a chunk since the last reset. */
int rtiow_debug_read_chunk_costs(rtiow_handle h, uint32_t* costs, size_t count);
/* Fill the staging buffer of the staged stores (finished pixels in slot order, gathered by place_pixels_kernel) with 0xff bytes -- NaN in
 * both precisions -- on the handle's stream.  A slot the next render never hands out then shows in the image instead of keeping the bytes
 * of the render before.  RTIOW_E_STATE when the handle has no staging buffer. */
int rtiow_debug_poison_staged(rtiow_handle h);
/* Per-wave timeline of one (untimed, counting) persistent render: 8 words per wave
 * {t_start, t_pool_exhausted, t_end (100 MHz ticks), iterations alone, iterations cooperative,
 * pixels taken, 0, 0}. */
int rtiow_debug_timeline(rtiow_handle h, int threads_per_block_row, uint64_t* out_words, size_t cap_words, int* waves);
/* One (untimed, counting) persistent render: per local pixel 4 words {when a lane took it, when it finished (100 MHz ticks, low 32 bits),
 * segments it ran in the launch, wave that ran it} of the LAST launch that rendered it (the main launch of the sorted schedule). */
int rtiow_debug_pixel_times(rtiow_handle h, int threads_per_block_row, uint32_t* out_words, size_t cap_words);
int rtiow_debug_ops(rtiow_handle h, int op, size_t n, const void* a, const void* b, const void* c, void* out);
/* hit_world (hittable.h:80-98) alone, with the handle's scene and scene source, on n caller-supplied rays
 * {ox,oy,oz,dx,dy,dz} in the handle's precision: nearest root (+inf: none) and sphere index (-1: none) per ray.
 * Lets the tests compare the scene sources on rays no render produces. */
int rtiow_debug_hit_world(rtiow_handle h, int n, const void* rays, void* t_out, int32_t* index_out);
/* The scatter step alone -- everything that follows hit_world in one trip of the path loop (camera.h:88-124: sky, hit record, lambertian,
 * metal and dielectric scatter with their rejection loops) -- with the handle's scene, on n caller-supplied calls in the handle's precision,
 * one per lane: calls 64 w ... 64 w + 63 are the lanes of wave w, so the caller decides who shares a wave.  (closest, hit) are taken as
 * given, not recomputed.  form selects the statement of the step: 0 shade_step<T, false>; 1 the bounded shade_step<T, true>, called with the
 * build's rounds per trip until it stops asking for a retry; 2 (fp64 only, RTIOW_E_BADARG in fp32) shade_front, merged_rounds bounded the
 * same way and repeated while the lane is still looking, shade_back -- the rotated trip of the persistent kernels.
 *   in_real11  {ox,oy,oz, dx,dy,dz, closest, atten r,g,b, sky_uy}          in_int2  {hit (-1: miss), depth}       in_state6  {v0..v4,d}
 *   out_real12 {col r,g,b, ox,oy,oz, dx,dy,dz, atten r,g,b} afterwards     out_int4 {1: the path ended (col is its colour) / 0: it goes on,
 *              depth, trips the call took, flags (bit 0: a retry did not leave O, D, atten and depth untouched)}   out_state6 afterwards
 * rounds_per_trip (optional): the build's bound of the rejection loop per trip.  RTIOW_E_BADARG: a hit index beyond the scene. */
int rtiow_debug_scatter(rtiow_handle h, int form, int n, const void* in_real11, const int32_t* in_int2, const uint32_t* in_state6,
                        void* out_real12, int32_t* out_int4, uint32_t* out_state6, int* rounds_per_trip);
/* The 32 XORWOW subsequence-jump matrices A^(2^(67+b)) (160 x 5 words each) as the library builds
 * them: from its committed constant A^(2^67), or from_scratch != 0 from the one-step matrix A.
 * Host arithmetic only (no GPU needed).  Returns the number of matrices. */
int rtiow_debug_jump_matrices(uint32_t* out_words, size_t cap_words, int from_scratch);
/* The uniform-grid plan of RTIOW_SCENE_GRID for n spheres {cx,cy,cz,r} (doubles) around the recentring point
 * centre3, as the library builds it.  Host arithmetic only (no GPU needed).  dims4 = {nx, nz, registered
 * spheres, direct-list length}; params8 = {x0, z0, cell, slab ylo, slab yhi, Rfar, eps, Cmax}; cells (optional)
 * = nx*nz*4 sphere indices (0xffff x4: empty cell, n: pad); direct (optional) = the direct list; halfwidth
 * (optional, n entries) = registration half-width of every gridded sphere.  Returns 1 when the library would
 * use the grid for this scene, 0 when it keeps the screened loop, negative on bad arguments. */
int rtiow_debug_grid_plan(int n, const double* center_radius, const double* centre3, int32_t* dims4, double* params8,
                          uint16_t* cells, size_t cells_cap, int32_t* direct, size_t direct_cap, double* halfwidth);
/* The device grid's plan (rtiow_render_large, csrc/library/device_grid.h) for n spheres {cx,cy,cz,r} (doubles) around the recentring
 * point centre3, as the library builds it.  Host arithmetic only (no GPU needed).  dims6 = {nx, nz, registered spheres, direct-list
 * length, index entries, longest cell list}; params8 as rtiow_debug_grid_plan's; cells (optional) = nx*nz {first, count} pairs into
 * indices (optional); direct (optional) = the direct list; halfwidth (optional, n entries).  A first call with NULL buffers gives the
 * sizes.  Returns 1 when rtiow_render_large would render the scene, 0 when it would refuse, negative on bad arguments. */
int rtiow_debug_large_grid_plan(int n, const double* center_radius, const double* centre3, int32_t* dims6, double* params8,
                                uint32_t* cells, size_t cells_cap, uint32_t* indices, size_t indices_cap, int32_t* direct, size_t direct_cap, double* halfwidth);
/* rtiow_debug_hit_world through the device grid of rtiow_render_large (whatever the handle's scene source), and per ray the number of
 * cells its walk read, or -1 when its wave took the exact loop (a far, NaN or huge ray among its 64).  RTIOW_E_BADARG when the grid
 * does not suit the scene. */
int rtiow_debug_hit_world_large(rtiow_handle h, int n, const void* rays, void* t_out, int32_t* index_out, int32_t* cells_out);
/* The volume grid's plan (rtiow_render_volume, csrc/library/volume_grid.h) for n spheres {cx,cy,cz,r} (doubles) around the recentring
 * point centre3, as the library builds it.  Host arithmetic only (no GPU needed).  max_cells <= 0: the library's cap (2^20); a smaller
 * one makes the loop that widens the cells run; a larger one is refused (RTIOW_E_BADARG: a record's byte offset must stay in 32 bits).  dims8 = {nx, ny, nz, registered spheres, direct-list length, index entries, longest cell
 * list, occupied cells}; params8 = {x0, y0, z0, cell, rfar, eps, cmax, 0}; cells (optional) = nx*ny*nz {first, count} pairs, cell
 * (ix, iy, iz) at (iy nz + iz) nx + ix, into indices (optional); direct (optional) = the direct list; halfwidth (optional, n entries).
 * A first call with NULL buffers gives the sizes.  Returns 1 when rtiow_render_volume would render the scene, 0 when it would refuse,
 * negative on bad arguments. */
int rtiow_debug_volume_grid_plan(int n, const double* center_radius, const double* centre3, int64_t max_cells, int32_t* dims8, double* params8,
                                 uint32_t* cells, size_t cells_cap, uint32_t* indices, size_t indices_cap, int32_t* direct, size_t direct_cap, double* halfwidth);
/* rtiow_debug_hit_world through the volume grid of rtiow_render_volume (whatever the handle's scene source), and per ray the number of
 * cells its walk read, or -1 when its wave took the exact loop (a far, NaN or huge ray among its 64).  RTIOW_E_BADARG when the grid
 * does not suit the scene. */
int rtiow_debug_hit_world_volume(rtiow_handle h, int n, const void* rays, void* t_out, int32_t* index_out, int32_t* cells_out);

/* Test hook, host only (no GPU, no RCCL): the exchange's schedule -- the very function rtiow_group_gather runs --
 * against a recording table instead of HIP / RCCL, for n ranks on `devices` with `rows` local rows each.
 * mode = RTIOW_GATHER_RCCL, RTIOW_GATHER_PEER or RTIOW_GATHER_HOST, optionally | 0x100: with the fallback chain of RTIOW_GATHER_AUTO
 * (RCCL -> peer copies -> host-staged copies; the last record is then {12, -, the transport that carried the image}).  One record of
 * 8 int64 per call (layout: csrc/rtiow_group.hip); fail_at >= 0 makes that call fail.  Returns the number of records;
 * *schedule_rc = what the schedule returned. */
int rtiow_debug_gather_schedule(int n, const int* devices, const int* rows, int W, int precision, int mode, int fail_at,
                                int64_t* records, size_t cap_records, int* schedule_rc);


/* Instrumented builds only (-DRTIOW_PATH_STATS, scripts/path_stats_probe.py): wave-level execution counts and region clocks. */
int rtiow_debug_region_cycles(unsigned long long* out, int cap_words, int reset);
int rtiow_debug_path_stats(unsigned long long* out, int cap_words, int reset);

#ifdef __cplusplus
}
#endif
#endif /* RTIOW_DEBUG_H */
