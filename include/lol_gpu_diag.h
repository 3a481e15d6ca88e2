/*
 * lol_gpu_diag.h — what tests, profiles and a curious maintainer ask liblol_gpu.so beside the frames: which tuning
 * switches took effect, the exhaustive proofs behind the kernel's shortcuts run one by one, the culling bounds of an
 * object, and the scene SDF and the renderer's powf on their own.  NOTHING a host needs to render: the plug-in
 * (integration/hip_renderer.c) and the other hosts include lol_gpu.h alone.  Same library, same ABI version.
 */
#ifndef LOL_GPU_DIAG_H
#define LOL_GPU_DIAG_H

#include "lol_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tuning switches in effect in this process, "NAME=value NAME=value ..." ("" when none).  The library has ten
 * LOL_GPU_* environment switches for A/B runs and debugging (INTEGRATION.md lists them) — the scene kernel's instruction scheduling
 * among them.  They are honoured ONLY in a process that also sets LOL_GPU_TUNING=1; one that is set without it is ignored and
 * reported once on stderr; every one that took effect is listed here, in lol_gpu_specialize_log() and in bench.py's
 * record, so that a number can never silently come from a shell's leftovers.  (Not fenced: LOL_GPU_CACHE_DIR, LOL_GPU_ROCTX —
 * where code objects are kept, whether frames are marked: neither changes what is computed.)  The string belongs to the library
 * and is valid until the next call of this function. */
const char* lol_gpu_tuning_switches(void);
/* Frame ranges pushed to roctx so far by this process (LOL_GPU_ROCTX=1 marks every frame launch for
 * `rocprofv3 --marker-trace`, the counterpart of the reference's -j/--jitdump aid); 0 when not asked for, -1 when asked
 * for but no roctx library could be loaded (also reported once on stderr). */
long lol_gpu_roctx_ranges(void);

/*
 * The specialised kernel may replace sqrt and the smooth-min division x/k by cheaper sequences
 * (lol_kernel.h "fast exact paths").  Each is used only after the device has run ALL 2^32 float
 * inputs through it and through the plain expression and found no difference; this call runs
 * those checks directly and returns the mismatch counts (0 = proven; ~0 = could not run).
 */
/* sqrt_mismatches[0..2] = sqrt_pm, sqrt_gs, sqrt_r2 (lol_kernel.h); div_mismatches for the divisor k */
int         lol_gpu_verify_fast_paths(lol_gpu* ctx, float k, unsigned long long sqrt_mismatches[3],
                                      unsigned long long* div_mismatches);
/* The same exhaustive run for the blend factor WITHOUT its v_div_fixup_f32 (lol_kernel.h, smin_h_fast<false>): inputs on
 * which it differs from the exact factor, or — for dlt = +-inf — fails to make the smooth minimum NaN.  0 = proven. */
int         lol_gpu_verify_smin_no_fixup(lol_gpu* ctx, float k, unsigned long long* mismatches);
/* Gamma and quantisation of a colour channel — Uint8 v = powf(c, 1 / 2.2f) * 255 (naive_renderer.c:231-232, renderer.h:17-22) —
 * through a table of 256 thresholds instead of the powf (lol_kernel.h, gamma_u8_table): used by frames only after this sweep of
 * every float in [0, 1] found no difference on the context's device (it runs at the first upload; lol_gpu_set_specialize(ctx, 3) keeps the
 * powf).  *mismatches = floats on which the two routes differ (0 = proven, ~0 = could not run); table (may be NULL): the 257
 * thresholds, T[k] = the smallest c whose channel value is >= k, T[0] = 0, T[256] = +inf. */
int         lol_gpu_verify_gamma_table(lol_gpu* ctx, unsigned long long* mismatches, float* table);

/* The bound behind the culling test (lol_gpu.h, lol_gpu_set_cull) for top-level object `root` (0-based, file order); no device needed.  Returns 1 and
 * the bounding sphere (centre, inflated radius R') when the object has one, 0 when it has none (planes, unions
 * with a plane or with smoothness <= 0, non-finite fields) and is therefore never culled. */
int         lol_gpu_cull_bounds(const lol_program* prog, uint32_t root, float c_out[3], float* r_out);
/* The tighter bound of a union of at least three primitives whose leaves split into two clusters much smaller than the
 * one enclosing sphere: value(p) >= min_j (|p - c_j| - r'_j).  Returns how many spheres out[j] = {cx, cy, cz, r'} were
 * written (0: the object is tested with its single sphere only; else 2); the specialised kernel skips such an object where
 * the tests of BOTH spheres pass. */
int         lol_gpu_cull_bounds_clusters(const lol_program* prog, uint32_t root, float out[3][4]);
/* The interpreter list of `prog` as the scene-record calls build it per record
 * (analyse_roots, plan_culling(cull), build_mops with nothing proven):
 * *n_mops, *n_tests (constants records), *n_unbounded, and for up to `cap`
 * objects in evaluation order their root id (order[]) and whether the macro-op
 * that finishes them carries MOP_TIE (tie[]).  Returns the number of objects.  No device needed; the three counts may be NULL,
 * order and tie may be NULL only with cap = 0.  LOL_GPU_ERR_ARG for no program or one beyond LOL_MAX_OPS.
 * The plan — order, tie flags, tests, unbounded objects — is the one a call builds for that record on any context.  *n_mops is the
 * length with NOTHING proven: a context whose upload proved a smoothness constant lets a smooth min of two finished sub-unions ride
 * on the record before it (MOPB_POST), so its list of the same record can be shorter than *n_mops, never longer. */
int         lol_gpu_interp_list_info(const lol_program* prog, int cull, uint32_t* n_mops, uint32_t* n_tests,
                                     uint32_t* n_unbounded, uint32_t* order, uint32_t* tie, size_t cap);
/*
 * Diagnostic: out[i] = the renderer's powf(x[i], y[i]) (device pointers, asynchronous on `stream`, NULL = the
 * context's stream).  The kernel's powf restates the algorithm of the CPU libm's powf so that colours round
 * identically on both sides (lol_kernel.h, powf_glibc); this entry point lets a test compare the two bit for bit.
 */
int         lol_gpu_powf_batch(lol_gpu* ctx, const float* x_dev, const float* y_dev, float* out_dev, size_t n,
                               void* stream);
/*
 * Diagnostic: the scene SDF alone — sdf() of naive_renderer.c:31-44, i.e. get_obj_dist over every top-level object
 * with the first strict minimum — at n arbitrary points: pts = n x {x, y, z}, dist[i] / id[i] out (device pointers,
 * asynchronous on `stream`).  Runs the SAME SDF code the frames run (the specialised module's or the interpreter's,
 * fast paths and their fallback included), so a test can hold the device's distances against known answers
 * (tests/golden/ref_sdf_points.json) without a march in between.
 */
int         lol_gpu_sdf_batch(lol_gpu* ctx, const float* pts_dev, float* dist_dev, uint32_t* id_dev, size_t n, void* stream);
/*
 * The scene module of a context whose switches before its upload were `switches`, compiled without a device: writes
 * `<out_base>.hip` (the generated source) and `<out_base>.co` (its code object for `arch`), so that every kernel's ISA can be
 * inspected.  `switches` is a mask, one bit per call that puts kernels into a module, in the order the scene compiler appends them:
 *     1  lol_gpu_set_samples > 1           lol_render_spec_aa, lol_render_spec_aa_list
 *     2  lol_gpu_set_view_batches          lol_render_spec_batch (and, up to 256 ops, lol_render_spec_batch_steps)
 *     4  lol_gpu_set_view_samples          lol_render_spec_batch_aa, lol_render_spec_batch_aa_list — and what 2 adds, which it brings
 *     8  lol_gpu_set_view_blends           lol_render_spec_batch_lin
 *    16  lol_gpu_set_view_blend_samples    lol_render_spec_batch_aa_lin
 *    32  lol_gpu_set_ray_queries           lol_trace_spec
 *    64  lol_gpu_set_shade_queries         lol_shade_spec
 * 0 writes exactly what lol_gpu_compile_offline (lol_gpu.h) writes, and a module without a switch is the module that switch never
 * existed for.  form: 0 = the form a scene of this size ends up with, 1 = the SDF as one out-of-line function, 2 = inlined — the two
 * kernels a scene of 257 ... 1024 ops gets one after the other.  assume_fast, log: as for lol_gpu_compile_offline.
 * LOL_GPU_ERR_ARG for a mask outside 0 ... 127, any other form, or no program.
 */
int         lol_gpu_compile_offline_module(const lol_program* prog, const char* arch, const char* out_base, int assume_fast,
                                           unsigned switches, int form, char* log, size_t logcap);
/* The seven entry points from before that one: each is lol_gpu_compile_offline_module for one mask, with a refusal of its own.
 * ... the module with mask (samples > 1 ? 1 : 0), form 0.  LOL_GPU_ERR_ARG for samples other than 1, 2 and 4. */
int         lol_gpu_compile_offline_samples(const lol_program* prog, const char* arch, const char* out_base, int assume_fast,
                                            int samples, char* log, size_t logcap);
/* ... the module with mask (enable ? 2 : 0) */
int         lol_gpu_compile_offline_views(const lol_program* prog, const char* arch, const char* out_base, int assume_fast,
                                          int enable, int form, char* log, size_t logcap);
/* ... the module with mask (enable ? 4 : 0) */
int         lol_gpu_compile_offline_view_samples(const lol_program* prog, const char* arch, const char* out_base, int assume_fast,
                                                 int enable, int form, char* log, size_t logcap);
/* ... the module with the mask that `enable` is in an order of its own: 1 = lol_gpu_set_view_blends, 2 = lol_gpu_set_samples > 1,
 * 4 = lol_gpu_set_view_batches, 8 = lol_gpu_set_view_samples.  LOL_GPU_ERR_ARG outside 0 ... 15. */
int         lol_gpu_compile_offline_view_blends(const lol_program* prog, const char* arch, const char* out_base, int assume_fast,
                                                int enable, int form, char* log, size_t logcap);
/* ... the module with mask (enable ? 16 : 0) and the switches of `others`, in lol_gpu_compile_offline_view_blends' order.
 * LOL_GPU_ERR_ARG for others outside 0 ... 15. */
int         lol_gpu_compile_offline_view_blend_samples(const lol_program* prog, const char* arch, const char* out_base, int assume_fast,
                                                       int enable, int others, int form, char* log, size_t logcap);
/* ... the module with mask (enable ? 32 : 0) and the switches of `others`, in that order with 16 = lol_gpu_set_view_blend_samples
 * added.  LOL_GPU_ERR_ARG for others outside 0 ... 31. */
int         lol_gpu_compile_offline_rays(const lol_program* prog, const char* arch, const char* out_base, int assume_fast,
                                         int enable, int others, int form, char* log, size_t logcap);
/* ... the module with mask (enable ? 64 : 0) and the switches of `others`, in that order with 32 = lol_gpu_set_ray_queries added.
 * LOL_GPU_ERR_ARG for others outside 0 ... 63. */
int         lol_gpu_compile_offline_shade(const lol_program* prog, const char* arch, const char* out_base, int assume_fast,
                                          int enable, int others, int form, char* log, size_t logcap);
/* The kernel the first pass of the NEXT lol_gpu_render_views_blend(..., cams_per_view, ...) of this context launches, decided by
 * the test the launch itself makes: "lol_render_spec_batch_lin" / "render_interp_batch_lin"; lol_gpu_render_views' for
 * cams_per_view = 1.  (The second pass is always the library's own blend_resolve.) */
const char* lol_gpu_view_blend_kernel_name(const lol_gpu* ctx, int cams_per_view);
/* The kernel the first pass of the NEXT lol_gpu_render_views_blend_samples(..., cams_per_view, ..., samples, ...) of this context
 * launches, decided by the test the launch itself makes: "lol_render_spec_batch_aa_lin" / "render_interp_batch_aa_lin";
 * lol_gpu_view_blend_kernel_name's for samples <= 1, lol_gpu_view_samples_kernel_name's (contrast -1) for cams_per_view <= 1. */
const char* lol_gpu_view_blend_samples_kernel_name(const lol_gpu* ctx, int cams_per_view, int samples);
/* ... and of lol_gpu_render_scene_views(..., cams_per_view, ...): "lol_render_param_batch" / "lol_render_param_batch_lin" (the structure
 * module) or "render_interp_scene_batch" / "render_interp_scene_batch_lin" (the interpreter on each record's own lists) */
const char* lol_gpu_scene_views_kernel_name(const lol_gpu* ctx, int cams_per_view);
/* The structure module of the uploaded program: 0 none (no lol_gpu_set_scene_views before the upload, specialisation off, or more than
 * 256 ops), 1 being compiled (or compiled and not yet loaded: the next batch or lol_gpu_specialize_wait loads it), 2 in use, -1 failed
 * (the interpreter's kernels render; the reason goes to stderr once). */
int         lol_gpu_scene_views_state(const lol_gpu* ctx);
/* What the last upload proved on the device for the INTERPRETER's kernels, which is also what the lists of scene views are built with:
 * the sqrt kind its kernels are instantiated with (0 plain sqrtf, 3 sqrt_r2), how many of the program's smoothness constants have a
 * proven fast blend factor, and how many of those also without v_div_fixup.  All 0 with lol_gpu_set_specialize(ctx, 0) or 3 (plain
 * arithmetic) and before any upload. */
int         lol_gpu_interp_fast_paths(const lol_gpu* ctx, int* sqrt_kind, unsigned* n_div, unsigned* n_div_no_fixup);
/* The arithmetic of the per-pixel code around the loops in the scene kernel's fast pipeline (lol_kernel.h, ShadeMath), as the last
 * upload decided it, and the two exhaustive comparisons on this device that it rests on.  In use: root_kind (0 the plain sqrtf, else
 * the lol::sqrt_fast kind) and rcp_form (0 the division, else the corrections of lol::rcp_fast) — both 0 before an upload, with plain
 * arithmetic (lol_gpu_set_specialize 0 / 3) and with LOL_GPU_SHADE_MATH=0.  Proofs ([0] the one-correction reciprocal, [1] the
 * two-correction one): on how many of the 2^32 floats shortcut and division differ (~0: not run) and the interval of bit patterns
 * around 1.0f that holds none of them (0 ... 0xFFFFFFFF: they agree everywhere). */
typedef struct lol_gpu_shade_math_info {
	int32_t  root_kind, rcp_form;
	uint32_t proof_lo[2], proof_hi[2];
	uint64_t proof_mismatches[2];
} lol_gpu_shade_math_info;
int         lol_gpu_shade_math(const lol_gpu* ctx, lol_gpu_shade_math_info* out);
/* No device needed: the structure module of `prog` — `<out_base>.hip` (source that depends on the program's structure alone: two
 * programs of one structure give the same bytes) and `<out_base>.co`. */
int         lol_gpu_compile_offline_scene_views(const lol_program* prog, const char* arch, const char* out_base, char* log, size_t logcap);
/* The kernel the NEXT lol_gpu_render_scene_views_samples(..., cams_per_view, ..., samples, ...) launches (of a blend: its first pass):
 * "lol_render_param_batch_aa" / "lol_render_param_batch_aa_lin" (a structure module made after lol_gpu_set_scene_view_samples) or
 * "render_interp_scene_batch_aa" / "render_interp_scene_batch_aa_lin"; lol_gpu_scene_views_kernel_name's for samples <= 1. */
const char* lol_gpu_scene_view_samples_kernel_name(const lol_gpu* ctx, int cams_per_view, int samples);
/* No device needed: the structure module of `prog` as lol_gpu_set_scene_view_samples asks for it, with all four kernels —
 * `<out_base>.hip` (it depends on the structure alone, and differs from lol_gpu_compile_offline_scene_views') and `<out_base>.co`. */
int         lol_gpu_compile_offline_scene_view_samples(const lol_program* prog, const char* arch, const char* out_base, char* log, size_t logcap);
/* The kernel the NEXT lol_gpu_render_views_samples(..., samples, contrast, ...) of this context launches, decided by the test the
 * launch itself makes: "lol_render_spec_batch_aa" / "render_interp_batch_aa" for contrast = -1, the refine pass's
 * "lol_render_spec_batch_aa_list" / "render_interp_batch_aa_list" for an adaptive batch, lol_gpu_render_views' for samples = 1.
 * (A scene kernel that has finished compiling takes over at the next frame, batch or lol_gpu_specialize_wait.) */
const char* lol_gpu_view_samples_kernel_name(const lol_gpu* ctx, int samples, int contrast);
/* The interpreter's instantiation for the uploaded program: *ssize = the operand-stack entries of its template argument (1, 3, 7,
 * 11 or 63), *tables_global = 1 when lights, materials and root materials are read from global memory instead of LDS (then ssize is
 * 3, 11 or 63).  The answer of the very function the interpreter's launches go through — frames, supersampled frames, refine passes
 * and every kind of batch alike.  LOL_GPU_ERR_NO_PROGRAM before an upload.  For tests. */
int         lol_gpu_interp_variant(lol_gpu* ctx, int* ssize, int* tables_global);
/* Waits for the context's last adaptive batch and gives how many pixels of all its views were refined.  LOL_GPU_ERR_ARG when no
 * adaptive batch was launched.  For tests and rate tools. */
int         lol_gpu_views_refined(lol_gpu* ctx, int64_t* n);
/*
 * Adaptive frames (lol_gpu_set_adaptive_samples): waits for the context's last adaptive frame and gives how many of its pixels
 * were refined (*n), or the time its three passes took on the device, in milliseconds between events on its stream (ms[0] the
 * plain frame, ms[1] the mask and the list, ms[2] the refined pixels).  LOL_GPU_ERR_ARG when no adaptive frame was launched.
 * For tests and rate tools; frames never need them.
 */
int         lol_gpu_adaptive_refined(lol_gpu* ctx, int64_t* n);
int         lol_gpu_adaptive_pass_ms(lol_gpu* ctx, float ms[3]);
/* The kernel the NEXT ray query of this context (lol_gpu_trace_rays, lol_gpu_trace_pixels, lol_gpu_pick) launches, decided by the
 * test the launch itself makes: "lol_trace_spec" / "trace_interp"; "" for a NULL context. */
const char* lol_gpu_trace_kernel_name(const lol_gpu* ctx);
/* The kernel the NEXT shading query of this context (lol_gpu_shade_rays, lol_gpu_shade_pixels) launches, decided by the test the
 * launch itself makes: "lol_shade_spec" / "shade_interp"; "" for a NULL context. */
const char* lol_gpu_shade_kernel_name(const lol_gpu* ctx);
/*
 * lol_gpu_kernel_key's function of a code object (lol_gpu.h says what it covers), for n bytes of one in host memory — a .co of
 * lol_gpu_compile_offline* — as 16 hex digits and a NUL in out.  A buffer that is no ELF64 little-endian file, or whose section
 * headers point outside it, gets the FNV-1a of all its bytes; no buffer is read out of bounds.  Needs no device.
 */
void        lol_gpu_code_key(const void* code, size_t n, char out[17]);

#ifdef __cplusplus
}
#endif
#endif /* LOL_GPU_DIAG_H */
