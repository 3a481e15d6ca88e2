/*
 * lol_gpu_testing.h — fault injection, geometry switches and views of the schedule's tables for the TEST SUITE
 * (tests/test_gpu_boundary.py, tests/test_multi_device.py, tests/test_gpu_schedule.py).  Not part of the drop-in boundary: a renderer.h host never calls these, and nothing in
 * the library reads the environment for them (rounds 2-3 used getenv(): an inherited variable could change production
 * behaviour).  Each switch lives in the context it is set on and dies with it.
 */
#ifndef LOL_GPU_TESTING_H
#define LOL_GPU_TESTING_H

#include "lol_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The next `n` lol_gpu_upload_program calls on this context fail at their copy step (as a failed hipMemcpy would), after
 * every check has passed: exercises the all-or-nothing upload. */
int lol_gpu_testing_fail_uploads(lol_gpu* ctx, int n);

/* The next `n` scratch allocations of adaptive batches (lol_gpu_render_views_samples with contrast >= 0) and of blends
 * (lol_gpu_render_views_blend and lol_gpu_render_views_blend_samples with more than one camera per view) on this context fail
 * as a hipMalloc without memory would: the call returns LOL_GPU_ERR_HIP with nothing launched, and the context stays usable. */
int lol_gpu_testing_fail_view_scratch(lol_gpu* ctx, int n);

/* The next `n` FIRST runs of the scene compiler for a scene of the middle sizes (257 ... 1024 ops: out-of-line form first, inlined
 * form behind it) count as failed: exercises "the inlined form is compiled all the same" (lol_tiers.hip, apply). */
int lol_gpu_testing_fail_first_tier(lol_gpu* ctx, int n);

/* Every `stride`-th PART gets the root's band height (lol_gpu_multi_set_root_band_rows) even on ONE device, so that a
 * one-GPU box runs bands of unequal height through split, launches, exchange, assembly and host copies.  0 = off. */
int lol_gpu_multi_testing_root_stride(lol_gpu_multi* m, int stride);

/* lol_gpu_multi_render_host issues every device's copies from that device's own host thread even when there is only one
 * device (which otherwise copies inline): the code every real multi-GPU host runs, reachable on a one-GPU box. */
int lol_gpu_multi_testing_force_copier_threads(lol_gpu_multi* m, int enable);

/* The check the scene compiler applies to every code object before it may be launched (lol_gpu.hip,
 * has_return_clobbering_branch): 1 when the bytes hold a branch relaxed through s[30:31] — s_getpc_b64 s[30:31] ...
 * s_setpc_b64 s[30:31], LLVM's long-branch register bug: a function that never returns — 0 when not.  No device needed. */
int lol_gpu_testing_has_return_clobbering_branch(const void* code, size_t n_bytes);

/* What the pixels of a repeated view are dealt to waves by (lol_gpu_set_tile_order, LOL_GPU_TILES_LPT): the table its recording
 * frame — the second frame under one camera — wrote, one entry per pixel, `w` per local row of the part: the march steps plus the
 * shadow steps the pixel's lane RAN (saturating at 65535).  lol_gpu_debug reports the reference's counts, which also hold the turns
 * a stationary shadow ray left out; this is the only place the two can be told apart.  Waits for the device.  n_pixels must be that
 * frame's w x rows; LOL_GPU_ERR_ARG when the last frame went through no table or the size is another. */
int lol_gpu_testing_pixel_cost(lol_gpu* ctx, unsigned short* out, size_t n_pixels);

/* The tables of a repeated view's schedule (lol_sched.hip), for tests/test_gpu_schedule.py, which holds them to a CPU model
 * (tests/schedule_reference.py).  Tables of wave slots are passed BY LAUNCH POSITION — entry i belongs to the i-th block of the
 * launch; how the library lays them out in memory (lol_kernel.h, tile_slot) stays inside it.  No fault injection: the first two run
 * the table kernels on scratch of their own and touch no view's tables, the third only reads.
 *
 * lol_gpu_testing_deal: the lane table of a w x n_rows frame as the library would make it — its region shape, its launches:
 * rectangles when `cost` is NULL (a recording frame), else dealt by cost[n_rows][w].  lanes_out[64 * slot + lane] = column |
 * row << 16 | 1 << 31 for a lane of padding.  n_lanes must be the table's size (64 x 16 x the regions that cover the frame). */
int lol_gpu_testing_deal(lol_gpu* ctx, const unsigned short* cost, int w, int n_rows, uint32_t* lanes_out, size_t n_lanes);

/* lol_gpu_testing_sort_tiles: one sort as the library runs it between two frames (clear, count, scan, scatter).  cost[i] = the run
 * time the wave at launch position i reported, order_in[i] = the wave slot it shaded (< n_tiles); lanes (may be NULL) = a DEALT lane
 * table of n_tiles x 64 entries: a wave slot whose lane 63 is padding shaded nothing and counts 0 whatever cost[i] holds.
 * order_out[n_tiles] = the new table (0xFFFFFFFF where nothing was placed), keys_out[n_tiles] = the bucket of every launch position
 * (0 = the longest), starts_out[1024] = where every bucket begins in order_out. */
int lol_gpu_testing_sort_tiles(lol_gpu* ctx, const uint32_t* cost, const uint32_t* order_in, const uint32_t* lanes, size_t n_tiles,
                               uint32_t* order_out, uint32_t* keys_out, uint32_t* starts_out);

/* lol_gpu_testing_schedule: the tables of the view the last frame belongs to, as they stand once every queued frame has finished
 * (waits for the device; changes nothing).  frames = frames launched through the tables under this view (1 = the recording frame),
 * sorts = sorts of this set of tables since the context was created.  Every output pointer may be NULL; n_tiles / n_lanes must be
 * info's n_tiles / 64 x that where one of their tables is asked for (ask for `info` alone first).  order = the table in use,
 * order_before = the one the last sort read (meaningless before the view's first sort, like keys: the buckets that sort took the
 * launch positions of order_before for), cost = what the last frame's waves reported (a wave of padding alone reports nothing),
 * lanes = the lane table.  LOL_GPU_ERR_ARG when the last frame went out in a fixed order. */
typedef struct lol_gpu_testing_schedule_info {
	uint32_t n_tiles, frames, sorts;
	uint32_t region_w, region_h;
	uint32_t w, n_rows;
} lol_gpu_testing_schedule_info;
int lol_gpu_testing_schedule(lol_gpu* ctx, lol_gpu_testing_schedule_info* info, uint32_t* order, uint32_t* order_before, uint32_t* keys,
                             uint32_t* cost, size_t n_tiles, uint32_t* lanes, size_t n_lanes);

#ifdef __cplusplus
}
#endif
#endif /* LOL_GPU_TESTING_H */
