/*
 * lol_gpu.h — C ABI of the MI355X (gfx950) renderer for loltracer's per-pixel path.
 *
 * This is the drop-in boundary.  A C host that today links
 * naive_renderer.c gets the same three renderer.h entry points from
 * integration/hip_renderer.c, which is a thin adapter over the functions
 * below; INTEGRATION.md shows the binding.  Plain pointers and sizes only: no
 * C++ types, no exceptions, no torch.  Every function returns 0 on success or
 * a negative lol_gpu_status; lol_gpu_error() gives the text of the last error
 * of a context.
 *
 *   reference                                         here
 *   ------------------------------------------------  ---------------------------
 *   render_prepare()   renderer.h:25, main.c:161      lol_gpu_create + lol_gpu_upload_program
 *   render_thread() pixel loop
 *                      naive_renderer.c:207-236       lol_gpu_render_device / lol_gpu_render_host
 *   render_destroy()   renderer.h:26, main.c:213      lol_gpu_destroy
 *   row self-scheduling naive_renderer.c:216          the launch grid (+ `bands` for multi-GPU)
 *
 * There is no CPU fallback: every entry point fails with LOL_GPU_ERR_NO_DEVICE
 * when no HIP device is usable.
 */
#ifndef LOL_GPU_H
#define LOL_GPU_H

#include <stddef.h>
#include <stdint.h>
#include "lol_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Version of this binary interface.  It changes whenever an entry point changes its arguments or a structure its layout
 * (4: lol_program carries pointers + counts instead of fixed-capacity arrays; lol_gpu_render_host_end takes the surface's
 * size; lol_gpu_rows is {band, cycle, offset}.  5: lol_gpu_set_frames_in_flight / lol_gpu_next_stream; render_host_begin
 * takes up to four frames; lol_gpu_tuning_switches.  6: lol_gpu_verify_shadow_division is gone with the shortcut it
 * proved; lol::Launch carries the march's first step).  A host compiled against another version must not run: hip_renderer.c
 * and the Python mirror compare lol_gpu_abi_version() of the library they loaded with the macro they were built with.
 */
#define LOL_GPU_ABI_VERSION 6
int lol_gpu_abi_version(void);

typedef struct lol_gpu lol_gpu;      /* one renderer context = one device + one scene */

enum lol_gpu_status {
	LOL_GPU_OK              =  0,
	LOL_GPU_ERR_NO_DEVICE   = -1,
	LOL_GPU_ERR_HIP         = -2,    /* a HIP runtime call failed; see lol_gpu_error() */
	LOL_GPU_ERR_ARG         = -3,
	LOL_GPU_ERR_NO_PROGRAM  = -4,
	LOL_GPU_ERR_UNSUPPORTED = -5
};

/*
 * Which rows of the frame one call renders, and where they land.
 *
 * The frame's rows are cut into cycles of `cycle_rows` rows; inside every cycle a part owns the `band_rows` rows that
 * start at `offset_rows`.  A call renders the bands of one part and writes them compactly: local row
 * r = c * band_rows + i of the destination holds frame row c * cycle_rows + offset_rows + i (i < band_rows).
 * {band_rows = cycle_rows = h, offset_rows = 0} is the whole frame in place.  This is the multi-GPU row-tile partition
 * (SURVEY.md §8e): every rank renders its part with ONE launch and the parts are gathered.  Equal shares of n parts with
 * bands of b rows are {b, n * b, part * b}; the parts of one split may also differ in band height — how the root, which
 * also receives and un-interleaves the whole frame, gets a smaller share (lol_gpu_multi_set_root_band_rows).
 */
typedef struct lol_gpu_rows {
	int32_t band_rows;
	int32_t cycle_rows;
	int32_t offset_rows;
} lol_gpu_rows;

/*
 * How a colour becomes a pixel: SDL_MapRGB(surf->format, r, g, b) of renderer.h:17-22 for a non-palettised format
 * (SDL2, src/video/SDL_pixels.c):  (r >> Rloss) << Rshift | (g >> Gloss) << Gshift | (b >> Bloss) << Bshift | Amask.
 * The fields are SDL_PixelFormat's.  The reference stores one Uint32 per pixel whatever the format
 * (naive_renderer.c:233-235), so only 4-byte formats make sense; anything else is refused, never approximated.
 * Default (and NULL): XRGB8888 = shifts 16 / 8 / 0, no loss, Amask 0.
 */
typedef struct lol_gpu_pixel_format {
	uint8_t  r_shift, g_shift, b_shift;
	uint8_t  r_loss, g_loss, b_loss;
	uint8_t  bytes_per_pixel;     /* must be 4 */
	uint8_t  palettised;          /* must be 0 (format->palette != NULL) */
	uint32_t a_mask;
} lol_gpu_pixel_format;

/* Optional per-pixel diagnostics, all device pointers, each may be NULL.
 * Indexed by local row like the pixel destination, `w` elements per row. */
typedef struct lol_gpu_debug {
	float*    rgb;        /* 3 floats per pixel: post-gamma, pre-quantisation colour  */
	float*    hit_dist;   /* get_intersection().dist                                  */
	uint32_t* hit_id;     /* get_intersection().id                                    */
	uint32_t* steps;      /* low 16 bits: march steps; high 16 bits: shadow steps sum */
} lol_gpu_debug;

int  lol_gpu_device_count(void);
int  lol_gpu_create(int device, lol_gpu** out);
void lol_gpu_destroy(lol_gpu* ctx);
const char* lol_gpu_error(const lol_gpu* ctx);
int  lol_gpu_device(const lol_gpu* ctx);          /* the HIP device ordinal of a context */

/* Stream arguments: NULL = the context's own (non-blocking) stream; LOL_GPU_STREAM_DEFAULT = HIP's legacy
 * default stream (hipStreamLegacy, the stream a handle of 0 means to HIP itself); else a hipStream_t. */
#define LOL_GPU_STREAM_DEFAULT ((void*)1)

/* Copy the flattened scene (lol_scene_flatten) to the device.  May be called
 * again at any time (it first waits for everything queued on the device);
 * frames issued afterwards use the new program.  All or nothing: when it fails
 * (malformed program, a failed allocation or copy) the context keeps rendering
 * the scene it had.  The program is copied: the caller may free it on return.
 *
 * Returns as soon as the scene can be rendered — like the reference's
 * render_prepare (naive_renderer.c:242-244 does nothing; the JIT's takes
 * milliseconds, tracing_jit_renderer.dasc:416-434): the tables and the
 * interpreter's lists are on the device, and the scene's own kernel is being
 * compiled by hipRTC on a host thread (0.6 s for scene4, half a minute for
 * 5000 ops).  Frames render on the interpreter kernel meanwhile and switch to
 * the scene's kernel at the first frame boundary after the compiler is done —
 * same pixels on both.  lol_gpu_specialize_wait() blocks until then. */
int lol_gpu_upload_program(lol_gpu* ctx, const lol_program* prog);

/* Pixel format of every frame launched afterwards (NULL = XRGB8888).  LOL_GPU_ERR_UNSUPPORTED for palettised or
 * non-32-bit formats and shifts / losses that do not describe 8-bit channels in a 32-bit word. */
int lol_gpu_set_pixel_format(lol_gpu* ctx, const lol_gpu_pixel_format* fmt);

/* Number of local rows a part owns (for sizing destinations). */
int lol_gpu_part_rows(int h, const lol_gpu_rows* rows);

/*
 * Launch one frame (or one part of it) asynchronously.
 *   cam       per-frame camera constants (lol_frame_camera_init)
 *   w, h      frame size in pixels; max_steps = MAX_STEPS of the primary march
 *   rows      partition (NULL = whole frame)
 *   dst       DEVICE pointer to 32-bit pixels in the format of lol_gpu_set_pixel_format (default XRGB8888 =
 *             r<<16|g<<8|b), `pitch_bytes` per local row
 *   dbg       optional diagnostics (NULL in production)
 *   stream    hipStream_t to launch on, as void*; NULL = the context's own stream (see LOL_GPU_STREAM_DEFAULT)
 */
int lol_gpu_render_device(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps,
                          const lol_gpu_rows* rows, void* dst, size_t pitch_bytes,
                          const lol_gpu_debug* dbg, void* stream);

/*
 * Whole frame into a HOST surface (what render_thread does with surf->pixels,
 * naive_renderer.c:233-235): renders into the context's device framebuffer,
 * copies `h` rows of w*4 bytes honouring `pitch_bytes`, and waits.
 *
 * The surface is the host's memory: the library keeps nothing about it between calls and never registers it with the
 * device (the HIP runtime pins a copy's destination for the duration of the copy: PCIe line rate, measured), so a host
 * may free, move or resize its surface between any two frames (main.c:182-187).
 */
int lol_gpu_render_host(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps,
                        void* host_pixels, size_t pitch_bytes);

/*
 * The same with two frames in flight, for hosts that can give the next frame's camera before they consume the
 * previous frame (an orbit, a recorded path; an interactive host trades one frame of latency for it):
 *     begin(cam[0]);  for i: { begin(cam[i+1]);  end(surface);  present frame i }
 * begin() queues the frame's kernel and returns; end() copies the OLDEST queued frame into the host surface and
 * waits for that copy — which runs while the next frame's kernel does (main.c:182-194 is the loop this overlaps).
 * At most two frames may be begun and not yet ended; lol_gpu_render_host_pending() says how many are.
 *
 * The surface may change size between begin() and end() (the reference's window is resizable, main.c:157,182-187):
 * end() takes the size of the surface it is given and refuses (LOL_GPU_ERR_ARG, nothing written, frame kept) a frame
 * of another size; lol_gpu_render_host_pending_size() tells the size of the oldest queued frame beforehand and
 * lol_gpu_render_host_discard() drops every queued frame.  Frames of different sizes may be in flight together.
 *
 * The kernels of consecutive frames are queued on different streams of the context (round 5), so frame i+1's first waves
 * fill the tail of frame i's launch — the overlap the reference's sequential loop (main.c:189-194) cannot have and a host
 * with the next camera in hand can: what a MOVING camera gains from having frames in flight (the copy is hidden either
 * way).  After lol_gpu_set_frames_in_flight(ctx, n) up to n (<= 4) frames may be begun and not yet ended.
 */
int lol_gpu_render_host_begin(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps);
int lol_gpu_render_host_end(lol_gpu* ctx, void* host_pixels, size_t pitch_bytes, int w, int h);
int lol_gpu_render_host_pending(const lol_gpu* ctx);
int lol_gpu_render_host_pending_size(const lol_gpu* ctx, int* w, int* h);   /* 0 x 0 when nothing is queued */
int lol_gpu_render_host_discard(lol_gpu* ctx);

/* Wait for everything issued on the context's own stream(s). */
int lol_gpu_sync(lol_gpu* ctx);

/*
 * Frames in flight.  The reference renders frame i+1 when frame i has been shown (main.c:189-194); a frame here is ONE
 * launch that ends with its slowest waves on half-empty SIMDs, and a host whose frames are independent — an orbit, a
 * recorded path, the stripes of BASELINE.json's config 5 — loses that tail once per frame.  With n > 1 the frames launched
 * on the context's own stream (stream == NULL in lol_gpu_render_device) go to n streams of the context in turn, so up to n
 * of them run together and the next frame's first waves fill the last one's tail (+9 % scene4 at 4K, +13 % its orbit, +67 %
 * scene.lol at 1080p: profiles/r4_stream_overlap_ab.jsonl).  What the caller takes on: frames that may be in flight
 * together need destinations of their own — frame i and frame i + n share a stream, so a ring of n destinations is safe —
 * and only lol_gpu_sync() (or an event recorded on lol_gpu_next_stream() after the launch) says when a frame is there.
 * A repeated view keeps its schedule on every stream (lol_gpu_set_tile_order: one set of tables per stream).
 * n = 1 (the default) is the sequential behaviour.  Also the number of frames lol_gpu_render_host_begin accepts before an
 * _end (never fewer than two).  1 <= n <= 4.  Waits for the frames in flight before it changes the rotation.
 */
int   lol_gpu_set_frames_in_flight(lol_gpu* ctx, int n);
int   lol_gpu_frames_in_flight(const lol_gpu* ctx);
/* The hipStream_t (as void*) the NEXT frame launched with stream == NULL will be queued on: for hosts that bracket their
 * frames with events of their own. */
void* lol_gpu_next_stream(lol_gpu* ctx);

/* Raw device memory helpers so a C host needs no HIP headers. */
int lol_gpu_malloc(lol_gpu* ctx, size_t bytes, void** out);
int lol_gpu_free(lol_gpu* ctx, void* ptr);
int lol_gpu_memcpy_d2h(lol_gpu* ctx, void* host, const void* dev, size_t bytes);
/* ... and the other way, for what a host brings to a query (a list of rays or pixels): waits for the copy */
int lol_gpu_memcpy_h2d(lol_gpu* ctx, void* dev, const void* host, size_t bytes);

/*
 * Supersampling: s x s samples per pixel on an ordered grid, s in {1, 2, 4} (default 1: one ray per pixel, today's frames byte
 * for byte).  Any other s returns LOL_GPU_ERR_ARG and leaves the setting as it was (LOL_GPU_ERR_UNSUPPORTED: a library built
 * with an experimental wave patch whose sides s does not divide).  Takes effect at the next frame of
 * lol_gpu_render_device, lol_gpu_render_host and lol_gpu_render_host_begin; a frame already begun keeps the s it was begun with.
 * With s samples per axis, pixel (x, y) of a w x h frame is computed exactly so:
 *   1. sample (i, j), 0 <= i, j < s, is pixel (s x + i, s y + j) of the reference's frame of s w x s h pixels
 *      (naive_renderer.c:217-229 at view_pos = ((s x + i) + .5f) / (float)(s w) * 2 - 1, the same for y with s h): the clamped
 *      LINEAR colour get_light() returns, before gamma.  The camera is unchanged (lol_frame_camera_init with w, h: the aspect
 *      ratio of s w x s h is the same rational);
 *   2. the samples are averaged in linear space, in float32, in a fixed order: in order k = j s + i, each channel summed as a
 *      balanced binary tree ((v0 + v1) + (v2 + v3) for s = 2; the same nested four levels deep for s = 4), the sum multiplied
 *      by 1 / s^2;
 *   3. the mean goes through gamma and packing like a single sample's colour (lol_gpu_set_pixel_format).
 * Diagnostics: lol_gpu_debug.rgb is the mean after gamma; hit_dist, hit_id and steps have no single value for such a pixel, and
 * a frame that asks for them with s > 1 returns LOL_GPU_ERR_UNSUPPORTED, with nothing launched and nothing written.  Supersampled
 * frames launch in a fixed tile order (columns under LOL_GPU_TILES_COLS, rows otherwise) and neither use nor change the state of
 * LOL_GPU_TILES_LPT / _AUTO.  The scene's own kernel renders them when s > 1 was set BEFORE lol_gpu_upload_program (its module
 * then also carries lol_render_spec_aa); otherwise they render on the interpreter's render_interp_aa until the next upload —
 * same pixels either way.
 */
int         lol_gpu_set_samples(lol_gpu* ctx, int samples);
int         lol_gpu_samples(const lol_gpu* ctx);

/*
 * Adaptive supersampling: s x s samples only where the plain frame has an edge.  contrast = -1 is off (the default: frames are
 * those of lol_gpu_set_samples); 0 <= contrast <= 255 turns it on; any other value returns LOL_GPU_ERR_ARG and leaves the setting
 * as it was.  It matters only with samples > 1 (with s = 1 a frame is the plain frame whatever contrast says) and takes effect at
 * the next frame, like lol_gpu_set_samples; a frame already begun keeps the setting it was begun with.
 * For a w x h frame with s samples per axis and contrast T, pixel (x, y) is:
 *   1. P = the plain frame (what s = 1 renders), with id(x, y) = get_intersection().id (naive_renderer.c:225; 0 for an escaped ray)
 *      and c8(x, y) = the three 8-bit channels (Uint8)(c * 255) after gamma, before any pixel-format loss or shift;
 *   2. the pixel is REFINED if one of its 8 neighbours q inside the frame has id(q) != id(x, y), or |c8(q)[ch] - c8(x, y)[ch]| > T
 *      for a channel ch (neighbours outside the frame are ignored);
 *   3. a refined pixel is the s x s pixel of lol_gpu_set_samples, exactly as defined there;
 *   4. any other pixel is P's pixel, packed in the context's pixel format.
 * lol_gpu_debug.rgb is the colour after gamma of whichever of the two the pixel is; hit_dist, hit_id and steps are refused as for
 * any s > 1 frame.  A frame is three launches on its stream (the plain frame, the mask, the refined pixels) with no host wait.
 * Whole frames only: a `rows` argument that is not the whole frame returns LOL_GPU_ERR_UNSUPPORTED, nothing launched — a pixel's
 * mask reads rows another part renders.  The sample grid must fit s w <= 65536 and s h <= 32768 (else LOL_GPU_ERR_ARG).
 * lol_gpu_multi_* has no adaptive setter: multi-device adaptive frames would need halo rows, and are not built.
 */
int         lol_gpu_set_adaptive_samples(lol_gpu* ctx, int contrast);
int         lol_gpu_adaptive_samples(const lol_gpu* ctx);

/*
 * A batch of views: n_views frames of the same size, scene and settings under n_views cameras, in ONE launch.  For hosts that have
 * all their cameras in hand and want small frames — a contact sheet of an orbit, thumbnails from a ring of viewpoints, a few
 * thousand 128 x 128 views with depth and object ids — where a launch, a launch tail and a first-step evaluation per view cost
 * more than the view itself.
 * View v (0 <= v < n_views) is EXACTLY the frame lol_gpu_render_device(ctx, &cams[v], w, h, max_steps, NULL, ...) renders with one
 * sample per pixel in a fixed tile order: the same pixels in the context's pixel format, the same rgb, hit_dist, hit_id and steps
 * (lol_gpu_set_exact_skips and lol_gpu_set_miss_skip apply to every view as they do to a frame).  Row y of view v starts at
 * dst + v * view_stride_bytes + y * pitch_bytes; pitch_bytes >= 4 w and a multiple of 4; view_stride_bytes >= h * pitch_bytes and
 * a multiple of 4; bytes between rows and between views are not written.  The diagnostics of `dbg` (NULL = none), each optional,
 * are dense: element (v, y, x) at index (v * h + y) * w + x (three floats each for rgb).
 * `cams` is HOST memory and is copied before the call returns.  The call is asynchronous on `stream` like lol_gpu_render_device
 * (NULL = the context's streams in turn, lol_gpu_set_frames_in_flight): one small copy of the per-view records and one render
 * launch, no wait for any render.  Batches on different streams may be in flight together; the records go through a ring of 8
 * sets, so a host that queues batches faster than the device renders them is held 8 batches ahead of it (and a batch on one of
 * HIP's special stream handles — LOL_GPU_STREAM_DEFAULT — waits on the host for the batch that used its set 8 calls before).
 * Everything lol_gpu_render_device decides per frame from the camera is decided per view — the primary march's first step, and
 * what a camera beyond the sane range (a coordinate that is not finite, or at least 10^15 in magnitude) switches off — so a batch
 * may mix any cameras.  The views are rendered in order of v in a fixed tile order (columns under LOL_GPU_TILES_COLS, rows
 * otherwise), view v + 1's first waves filling view v's tail; a batch neither uses nor changes the state of LOL_GPU_TILES_LPT /
 * _AUTO: a plain frame after it is scheduled as if the batch had not been there.
 * Refused, with nothing launched and nothing written: n_views < 1 or > LOL_GPU_MAX_VIEWS, bad geometry, a frame of more than
 * 65535 tiles (16 x 4 pixels) along an axis, or more than 2^32 - 1 lanes in the whole launch (fewer views per call) —
 * LOL_GPU_ERR_ARG; lol_gpu_samples() > 1 — LOL_GPU_ERR_UNSUPPORTED: supersampled and adaptive batches take their samples as arguments
 * (lol_gpu_render_views_samples below); no program —
 * LOL_GPU_ERR_NO_PROGRAM.  There are no row partitions and no lol_gpu_multi_* form: a host with several devices stripes its VIEWS
 * over them, one context each.
 * Which kernel: after lol_gpu_set_view_batches(ctx, 1) BEFORE lol_gpu_upload_program the scene's own module also carries
 * lol_render_spec_batch (both kernels of a 257 ... 1024-op scene do), and batches run on it once it is ready; otherwise, and until
 * then, they run on the interpreter's render_interp_batch — same pixels either way.  A module compiled without the switch is the
 * module it was before batches existed (same code object, same lol_gpu_kernel_key).
 */
#define LOL_GPU_MAX_VIEWS 4096
int         lol_gpu_render_views(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int w, int h, int max_steps,
                                 void* dst, size_t pitch_bytes, size_t view_stride_bytes,
                                 const lol_gpu_debug* dbg, void* stream);
int         lol_gpu_set_view_batches(lol_gpu* ctx, int enable);
int         lol_gpu_view_batches(const lol_gpu* ctx);

/*
 * A supersampled batch of views: lol_gpu_render_views with s x s samples per pixel, on every pixel or edge-adaptively.  The samples
 * are ARGUMENTS of the call: it neither reads nor changes lol_gpu_set_samples / lol_gpu_set_adaptive_samples.
 * View v is EXACTLY the frame lol_gpu_render_device(ctx, &cams[v], w, h, max_steps, NULL, ...) renders on a context with
 * lol_gpu_set_samples(samples) and lol_gpu_set_adaptive_samples(contrast): the same packed pixels in the context's pixel format and
 * the same lol_gpu_debug.rgb, bit for bit.  samples in {1, 2, 4}; contrast = -1 (every pixel gets its s x s samples) or 0 ... 255
 * (only the pixels the adaptive definition refines; a view's mask reads that view's pixels alone: views are not neighbours).
 * samples == 1 is lol_gpu_render_views whatever contrast says (with all its diagnostics, and whatever lol_gpu_samples() is).
 * Addressing, `cams` (host memory, copied before the call returns), `stream`, the ring of 8 record sets, what is decided per view
 * from its camera, the fixed tile order and "neither uses nor changes LOL_GPU_TILES_LPT / _AUTO": all as lol_gpu_render_views.
 * With samples > 1 lol_gpu_debug.rgb is dense [v][y][x]; hit_dist, hit_id and steps are refused (LOL_GPU_ERR_UNSUPPORTED) as for
 * any supersampled frame.
 * A batch with contrast = -1 is one launch over the sample grids of all views.  An adaptive batch is four launches on its stream
 * with no host wait (the plain batch, every view's mask, the numbering of the lists' groups, the refined pixels) and takes its
 * scratch — 12 bytes per pixel of the batch — from a ring of 4 sets: a fifth adaptive batch in flight queues behind the first (on
 * one of HIP's special stream handles the host waits for it instead).  A scratch allocation that fails returns LOL_GPU_ERR_HIP,
 * nothing launched, and the context stays usable.
 * Refused, with nothing launched and nothing written: samples not in {1, 2, 4} or contrast outside -1 ... 255 — LOL_GPU_ERR_ARG;
 * everything lol_gpu_render_views refuses except lol_gpu_samples() > 1; a sample grid (s w x s h) of more than 65535 tiles along
 * an axis, or more than 2^32 - 1 lanes in a launch over all its samples — LOL_GPU_ERR_ARG; for adaptive batches also s w > 65536
 * or s h > 32768 — LOL_GPU_ERR_ARG — and a library whose block is not one wave — LOL_GPU_ERR_UNSUPPORTED.
 * Which kernel: after lol_gpu_set_view_samples(ctx, 1) BEFORE lol_gpu_upload_program the scene's own module also carries
 * lol_render_spec_batch_aa and lol_render_spec_batch_aa_list (both kernels of a 257 ... 1024-op scene do) and, for an adaptive
 * batch's first pass, the kernels of lol_gpu_set_view_batches; otherwise, and until that module is ready, the interpreter's
 * render_interp_batch_aa / render_interp_batch_aa_list render — same pixels either way.  A module compiled without the switch is
 * the module it was before (same code object, same lol_gpu_kernel_key).
 */
int         lol_gpu_render_views_samples(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int w, int h, int max_steps,
                                         int samples, int contrast,
                                         void* dst, size_t pitch_bytes, size_t view_stride_bytes,
                                         const lol_gpu_debug* dbg, void* stream);
int         lol_gpu_set_view_samples(lol_gpu* ctx, int enable);
int         lol_gpu_view_samples(const lol_gpu* ctx);

/*
 * Views averaged over CAMERAS: motion blur (the cameras of a frame's exposure) and depth of field (cameras on a lens).  The modes
 * above average over the pixel's area; this one averages K = cams_per_view frames of the same size under K cameras, in linear
 * light.  `cams` holds n_views * K cameras; view v uses cams[v * K + k], k = 0 ... K - 1; K in {1, 2, 4, 8, 16}.
 * Pixel (x, y) of view v:
 *   1. sample k is pixel (x, y) of the reference's w x h frame under cams[v * K + k]: the clamped LINEAR colour get_light() returns,
 *      before gamma (what lol_gpu_set_samples calls a sample);
 *   2. the K samples, in order of k, are summed per channel in binary32 as a balanced binary tree — K = 2: (v0 + v1); K = 4:
 *      (v0 + v1) + (v2 + v3); ... up to four levels deep — and the sum is multiplied by 1 / K;
 *   3. the mean goes through gamma and the context's pixel format exactly as one sample's colour does.
 * So K = 1 IS lol_gpu_render_views, with all its diagnostics, and K equal cameras give that camera's plain view bit for bit
 * (doubling and a power-of-two scale are exact on [0, 1]).  Averaging the packed 8-bit pixels of K views on the host is NOT this:
 * that mean is taken after gamma and after quantisation.
 * Addressing, `cams` (host memory, copied before the call returns), `stream`, the ring of 8 record sets, the fixed tile order and
 * "neither uses nor changes LOL_GPU_TILES_LPT / _AUTO": all as lol_gpu_render_views.  What lol_gpu_render_views decides per view
 * from its camera — the primary march's first step, what a camera beyond the sane range switches off — is decided per RECORD: a
 * group may mix sane and insane cameras.  The call neither reads nor changes lol_gpu_set_samples / lol_gpu_set_adaptive_samples.
 * With K > 1 lol_gpu_debug.rgb is the mean after gamma, dense [v][y][x]; hit_dist, hit_id and steps are refused
 * (LOL_GPU_ERR_UNSUPPORTED), as for any averaged pixel.
 * A blend with K > 1 is one copy of the n_views * K records and two launches on its stream with no host wait: every camera's linear
 * colours (the K cameras of a view are K times as many independent blocks, which is what fills the device for one or a few small
 * views), then the means.  The colours go through scratch — 16 bytes per ray, 16 * n_views * K * w * h bytes per call (12 of colour
 * and 4 of padding: one 16-byte store per lane) — from a ring of 4 sets that grow on demand and live as long as the context: a fifth
 * blend in flight queues behind the first (on one of HIP's special stream handles the host waits for it instead).  A scratch
 * allocation that fails returns LOL_GPU_ERR_HIP, nothing launched, and the context stays usable.
 * Refused with LOL_GPU_ERR_ARG, nothing launched and nothing written: K outside {1, 2, 4, 8, 16}; n_views * K > LOL_GPU_MAX_VIEWS;
 * everything lol_gpu_render_views refuses (except lol_gpu_samples() > 1), its limit of 2^32 - 1 lanes applied to all n_views * K frames.
 * Which kernel: after lol_gpu_set_view_blends(ctx, 1) BEFORE lol_gpu_upload_program the scene's own module also carries
 * lol_render_spec_batch_lin (both kernels of a 257 ... 1024-op scene do); otherwise, and until that module is ready, the
 * interpreter's render_interp_batch_lin renders — same pixels either way (lol_gpu_view_blend_kernel_name, lol_gpu_diag.h).  A
 * module compiled without the switch is the module it was before (same code object, same lol_gpu_kernel_key).
 * Supersampled blends (samples per pixel AND cameras per view): lol_gpu_render_views_blend_samples below.
 * Not built: row partitions, a lol_gpu_multi_* form (stripe the views over the devices, one context each), host surfaces, and the
 * renderer.h protocol, which has one camera per frame.
 */
#define LOL_GPU_MAX_BLEND 16
int         lol_gpu_render_views_blend(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int cams_per_view,
                                       int w, int h, int max_steps,
                                       void* dst, size_t pitch_bytes, size_t view_stride_bytes,
                                       const lol_gpu_debug* dbg, void* stream);
int         lol_gpu_set_view_blends(lol_gpu* ctx, int enable);
int         lol_gpu_view_blends(const lol_gpu* ctx);

/*
 * Supersampled blends: s x s samples under each of K cameras — a lens blur or a shutter blur whose in-focus and stationary edges
 * are as smooth as a supersampled frame's.  K = cams_per_view in {1, 2, 4, 8, 16}, s = samples in {1, 2, 4}; `cams` as for
 * lol_gpu_render_views_blend.  Pixel (x, y) of view v:
 *   1. for each k, m_k is the LINEAR mean of lol_gpu_set_samples, steps 1 - 2, under cams[v * K + k]: the s^2 samples are the pixels
 *      (s x + i, s y + j) of the reference's s w x s h frame, taken as clamped linear colours, summed in order j s + i as the
 *      balanced binary32 tree, and the sum is multiplied by 1 / s^2;
 *   2. m_0 ... m_{K - 1} are summed in order of k as the balanced binary32 tree of lol_gpu_render_views_blend, step 2, and the sum
 *      is multiplied by 1 / K;
 *   3. the result goes through gamma and the context's pixel format exactly as one sample's colour does.
 * The order of rounding is exactly this — scale by 1 / s^2 per camera first, then the tree over the cameras — and NOT one tree over
 * K s^2 leaves: the two differ on subnormal channels.
 * So s = 1 IS lol_gpu_render_views_blend (the call forwards to it: K = 1 with s = 1 keeps all diagnostics), K = 1 with s > 1 IS
 * lol_gpu_render_views_samples(..., samples, -1, ...) (the call forwards to it), and K equal cameras with s > 1 give that camera's
 * supersampled view bit for bit.
 * Addressing, the copy of `cams`, `stream`, the ring of 8 record sets, the fixed tile order and "neither reads nor changes
 * LOL_GPU_TILES_LPT / _AUTO, lol_gpu_set_samples, lol_gpu_set_adaptive_samples": all as lol_gpu_render_views_blend; what a view's
 * camera decides is decided per RECORD.  lol_gpu_debug.rgb is the mean after gamma, dense [v][y][x].
 * With K > 1 and s > 1 the call is one copy of the n_views * K records and two launches on its stream: every camera's linear means
 * — the s x s samples of a pixel are neighbouring lanes of one wave and are reduced in registers —, then the means over the cameras.
 * The scratch therefore holds one colour per PIXEL and camera, not per sample: 16 * n_views * K * w * h bytes per call, from the
 * same ring of 4 sets as lol_gpu_render_views_blend, with the same behaviour when an allocation fails (LOL_GPU_ERR_HIP, nothing
 * launched, the context stays usable).
 * Refused, nothing launched and nothing written: s outside {1, 2, 4} (LOL_GPU_ERR_ARG); everything lol_gpu_render_views_blend
 * refuses, in its order; a number of samples this build's wave patch cannot take (LOL_GPU_ERR_UNSUPPORTED, as lol_gpu_set_samples);
 * hit_dist, hit_id or steps with K > 1 or s > 1 (LOL_GPU_ERR_UNSUPPORTED); a sample grid of more than 65535 tiles along an axis, or
 * more than 2^32 - 1 lanes over all n_views * K sample grids (LOL_GPU_ERR_ARG).
 * Which kernel: after lol_gpu_set_view_blend_samples(ctx, 1) BEFORE lol_gpu_upload_program the scene's own module also carries
 * lol_render_spec_batch_aa_lin (both kernels of a 257 ... 1024-op scene do); otherwise, and until that module is ready, the
 * interpreter's render_interp_batch_aa_lin renders — same pixels either way (lol_gpu_view_blend_samples_kernel_name,
 * lol_gpu_diag.h).  The switch is its own: lol_gpu_set_view_blends and lol_gpu_set_view_samples together do not imply it, and a
 * module compiled without it is the module it was before (same code object, same lol_gpu_kernel_key).
 * Not built: an adaptive form (edge-adaptive samples under K cameras), row partitions, a lol_gpu_multi_* form, host surfaces.
 */
int         lol_gpu_render_views_blend_samples(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int cams_per_view,
                                               int w, int h, int max_steps, int samples,
                                               void* dst, size_t pitch_bytes, size_t view_stride_bytes,
                                               const lol_gpu_debug* dbg, void* stream);
int         lol_gpu_set_view_blend_samples(lol_gpu* ctx, int enable);   /* before lol_gpu_upload_program */
int         lol_gpu_view_blend_samples(const lol_gpu* ctx);

/* Name of the kernel a launch uses (for matching rocprofv3 kernel-trace rows):
 * "lol_render_spec" (scene-specialised, compiled by hipRTC at upload) or "render_interp"; with supersampling
 * (lol_gpu_set_samples) "lol_render_spec_aa" or "render_interp_aa"; for adaptive frames (lol_gpu_set_adaptive_samples) the
 * kernel of their refine pass, "lol_render_spec_aa_list" or "render_interp_aa_list".  It describes FRAMES: batches of views
 * (lol_gpu_render_views) run "lol_render_spec_batch" ("lol_render_spec_batch_steps" with lol_gpu_debug.steps) or
 * "render_interp_batch"; supersampled batches (lol_gpu_render_views_samples) what lol_gpu_view_samples_kernel_name (lol_gpu_diag.h)
 * says. */
const char* lol_gpu_kernel_name(const lol_gpu* ctx);
/* Identity of the code that kernel is: 16 hex digits.  For "lol_render_spec", FNV-1a over what the device loads of the hipRTC
 * code object: every section of the ELF file that is allocated (SHF_ALLOC) and of type PROGBITS or NOTE — the kernels' metadata
 * (.note), their descriptors (.rodata) and their instructions (.text) — in section-header order, each as its size (8 bytes,
 * little-endian) followed by its bytes.  Symbol names are not part of it: the compiler's compilation-unit id, a symbol that
 * follows the text of every header it was handed, does not rename the same instructions.  For "render_interp", FNV-1a of
 * {this library's build id (a digest of its sources and compiler flags), the uploaded macro-op lists, the square-root variant}: everything that decides which instructions the interpreter executes.  Profiles record it
 * (profiles/pmc_traffic.json) so that a counter figure is only ever quoted for the code it was measured on. */
const char* lol_gpu_kernel_key(const lol_gpu* ctx);
/* The environment: the library reads ten LOL_GPU_* switches for A/B runs and debugging (INTEGRATION.md lists them), and honours
 * them ONLY in a process that also sets LOL_GPU_TUNING=1 — a host that sets none of these runs the defaults whatever its shell
 * holds (lol_gpu_diag.h: lol_gpu_tuning_switches tells which took effect).  Not fenced: LOL_GPU_CACHE_DIR, LOL_GPU_ROCTX — where
 * code objects are kept, whether frames are marked for rocprofv3: neither changes what is computed. */

/*
 * Scene specialisation (the GPU analogue of the reference's tracing JIT, whose render_prepare
 * compiles the scene's SDF to x86 — tracing_jit_renderer.dasc:416-434).  lol_gpu_upload_program()
 * generates the scene's SDF as straight-line HIP and compiles it with hipRTC; when that is
 * disabled (set_specialize(ctx, 0) before the upload, or LOL_GPU_SPECIALIZE=0) or fails, frames
 * are rendered by the ahead-of-time interpreter kernel instead — same bits either way.
 */
/* enable: 0 = interpreter, plain arithmetic; 1 = specialise, with the proven-exact shortcuts (default);
 * 3 = specialise without them; 4 = interpreter with them; 5 = like 1, but a scene of 257 ... 1024 ops keeps its first kernel
 * (the SDF as one out-of-line function) and nothing is compiled behind it.  Takes effect at the next lol_gpu_upload_program.
 * What a host should know about the scene compiler: it runs on a thread of its own and cannot be interrupted; lol_gpu_destroy and
 * the next lol_gpu_upload_program wait for a run that is still at work — up to about 3 s for a first run, and for the SECOND run
 * of a mid-size scene (the form with the SDF inlined, 14 - 88 % faster) 2 - 18 s.  A host that would rather exit or switch
 * scenes promptly than have that kernel asks for 5. */
int         lol_gpu_set_specialize(lol_gpu* ctx, int enable);
/* The largest program (ops) the scene compiler takes on; larger scenes render on the interpreter, which reads them as data.
 * hipRTC cannot be interrupted once it runs — lol_gpu_destroy and the next upload's compile wait for it — and takes about
 * n^1.5: 5 s at 1300 ops, 41 s at 5000, minutes beyond 10,000 (fields of objects on the GPU box).  Default (and 0): 6144 ops,
 * about a minute.  A host that would rather wait for the 2x faster kernel of a huge scene raises it.  Takes effect at the next
 * lol_gpu_upload_program. */
int         lol_gpu_set_specialize_max_ops(lol_gpu* ctx, unsigned max_ops);
const char* lol_gpu_specialize_log(const lol_gpu* ctx);
/* Tiered start-up (lol_gpu_upload_program): wait for the scene compiler and switch to its kernel now (returns at once when
 * nothing is being compiled).  For tests and benchmarks that want to time or inspect one particular kernel. */
int         lol_gpu_specialize_wait(lol_gpu* ctx);
/* 0 = no scene kernel (switched off, or the scene is above the cap of lol_gpu_set_specialize_max_ops), 1 = being compiled, 3 =
 * compiled, takes over at the next frame, 2 = in use, -1 = the compiler failed (the interpreter renders; reason in
 * lol_gpu_specialize_log).  Scenes of 257 ... 1024 ops get TWO kernels, one after the other (round 5): the form with the SDF as
 * one out-of-line function, which hipRTC delivers in 0.4 - 3 s, and then the form with the SDF inlined into the three loops, 14 -
 * 88 % faster, in 3 - 18 s: 5 = the first is in use and the second being compiled, 6 = the second is compiled and takes over
 * at the next frame.  Same pixels from all of them; lol_gpu_specialize_wait waits for the last.
 * *compile_ms (may be NULL) = what the scene compiler's last finished run took. */
int         lol_gpu_specialize_state(lol_gpu* ctx, double* compile_ms);
/* (The proofs behind those shortcuts can be run one by one, and the culling bounds, the SDF and the powf asked for on
 * their own: include/lol_gpu_diag.h — nothing a frame needs.) */
/*
 * Escaped rays are shaded with material #0 (naive_renderer.c:103-112).  When that material has
 * diffuse == specular == 0, shininess >= 0 and all light intensities are finite, their colour is exactly
 * clamp(ambient_color * material.ambient) whatever the normal and shadow factors are, so a wavefront whose
 * rays ALL escaped skips the normal taps and shadow marches.  On by default when the uploaded program
 * qualifies (checked on the host); set_miss_skip(ctx, 0) turns it off.  With it on,
 * lol_gpu_debug.steps reports 0 shadow steps for the skipped pixels.
 *
 * The same switch governs the per-light form: where a surface faces away from a light (diffuse incidence
 * clamps to exactly 0) both Phong terms of that light are +-0 for any shadow factor, so that lane does not
 * march the shadow ray (needs all light intensities and material colours finite and every shininess >= 0).
 *
 * And the shadow march itself: softshadow returns maxf(res, 0) (naive_renderer.c:88-89), and once res <= 0 no later step
 * can bring the factor back above 0 — min only lowers it, and no NaN can appear when every number of the scene, its lights
 * and the camera is finite and below 10^15 (checked on the host) — so a lane's march ends there instead of going on to
 * res < -1 or t > L; a ray that grazes along just inside a surface otherwise takes all 128 steps while its wave waits
 * (C3: 5630 -> 7510 Mpixels/s).  Same pixels; lol_gpu_debug.steps counts the steps really marched.
 * lol_gpu_miss_skip_active(): bit 0 = escaped-wave skip, bit 1 = zero-incidence skip, bit 2 = settled-shadow exit.
 */
int         lol_gpu_set_miss_skip(lol_gpu* ctx, int enable);          /* all three skips on (default) or off */
/* The same, skip by skip: bit 0 = escaped waves, bit 1 = zero incidence, bit 2 = settled shadows (for tests that hold ONE
 * skip's step counts against known answers). */
int         lol_gpu_set_exact_skips(lol_gpu* ctx, unsigned mask);
int         lol_gpu_miss_skip_active(const lol_gpu* ctx);
/*
 * Exact culling of top-level objects in the specialised kernel (lol_gpu.hip, "exact culling"): sdf() is a strict-'<'
 * minimum over the objects (naive_renderer.c:31-44), so an object that a bounding sphere PROVES farther away than the
 * running minimum is not evaluated — for a whole wavefront at a time, and only then.  Same pixels, same step counts.
 * On by default; set_cull(ctx, 0) before the upload turns it off.
 */
int         lol_gpu_set_cull(lol_gpu* ctx, int enable);
/*
 * The order in which a launch hands out its tiles of 16x4 pixels.  Same pixels in every order; the time differs, because a
 * frame is one launch of blocks that differ 100x in cost and ends with its slowest waves running on half-empty SIMDs.
 *   LOL_GPU_TILES_LPT (the default): while the camera stands still, a frame is scheduled by what the frame before it cost.
 *     A frame under the same camera as the frame before it goes through tables: the pixels of every 64x16 region are dealt
 *     to the region's sixteen waves by the SDF evaluations they needed (a wave runs every loop to its slowest lane), every
 *     wave reports how long it ran, and a counting sort on the device (three small kernels on the frame's stream) hands the
 *     waves of the following frames out longest first — scheduling with costs that are exact, because nothing moved.  Only
 *     the schedule is reused: every pixel is computed from scratch in every frame, and comes out the same.  scene4 at 4K
 *     +24 % over the better of the two fixed orders, scene.lol at 1080p +40 %, the bands of an 8-way split of the 8K frame
 *     +34 % (LABNOTES.md §3.9).  A frame whose
 *     camera differs from its predecessor's is launched in the better fixed order (as LOL_GPU_TILES_AUTO finds it), with
 *     no table, cost or sort: stale costs are worse than no costs (the reference's arrow keys turn the camera 5.7 degrees
 *     a frame).  The tables live on the stream the first such frame was launched on; frames of the same geometry on
 *     other streams are launched in the fixed order.
 *   LOL_GPU_TILES_ROWS / LOL_GPU_TILES_COLS: row by row / column by column (the launch grid transposed).
 *   LOL_GPU_TILES_AUTO: the better of those two, measured: the first frames of a (scene, frame size, row partition, max_steps)
 *     are launched in both orders alternately, each between two HIP events on its launch stream (LOL_GPU_TILE_TRIALS frames
 *     per order after a few untimed ones; nothing ever waits), and the order whose typical frame is faster by more than
 *     1 % is kept — rows otherwise — until the scene, the size or the partition changes.
 * Takes effect at the next frame.  The reference has no counterpart: its thread pool claims pixels one by one
 * (naive_renderer.c:216) — which IS dynamic load balancing; this is its counterpart for a launch whose order is fixed up front.
 */
enum { LOL_GPU_TILES_ROWS = 0, LOL_GPU_TILES_COLS = 1, LOL_GPU_TILES_AUTO = 2, LOL_GPU_TILES_LPT = 3 };
#define LOL_GPU_TILE_TRIALS 16
int         lol_gpu_set_tile_order(lol_gpu* ctx, int order);
/* What the context is doing about it: mode = what was asked for; order = the order of the next frame outside a trial
 * (LOL_GPU_TILES_ROWS until AUTO has decided / until longest-first has its tables); deciding != 0 while AUTO's trials are
 * still being launched or collected, or before longest-first has sorted once; decisions = AUTO decisions / sorts so far;
 * rows_ms / cols_ms = the typical trial frame of each order behind AUTO's last decision (0 otherwise). */
typedef struct lol_gpu_tile_order_info {
	int32_t mode, order, deciding, decisions;
	float   rows_ms, cols_ms;
} lol_gpu_tile_order_info;
int         lol_gpu_tile_order(lol_gpu* ctx, lol_gpu_tile_order_info* out);
/* No device needed: writes <out_base>.hip (generated source) and <out_base>.co (code object for `arch`).
 * assume_fast != 0 generates the shortcuts without proof — for ISA inspection only, never for rendering. */
int         lol_gpu_compile_offline(const lol_program* prog, const char* arch, const char* out_base,
                                    int assume_fast, char* log, size_t logcap);

/* ------------------------------------------------------------------------------------------------
 * Several devices behind the same boundary (BASELINE.json north_star: "the image is
 * row-tile-partitioned across the 8 GPUs of one node with an RCCL gather over xGMI").
 *
 * One process, one renderer context + two HIP streams per device, one RCCL communicator per device
 * (ncclCommInitAll).  A frame's rows are cut into bands dealt round-robin over the devices — the static
 * form of the reference's row self-scheduling (naive_renderer.c:216: workers claim rows from an atomic
 * counter; every row is independent).  Device r renders part r compactly on its render stream; on its
 * exchange stream every device ncclSend()s its part to device 0 (devices[0], the root), which
 * ncclRecv()s them (one grouped call, parts may differ in size) and un-interleaves the bands into the
 * destination — the frame barrier of main.c:189-194 becomes the completion of that exchange.  Parts are
 * double-buffered, so frame i's exchange overlaps frame i+1's kernels.  RCCL is loaded (dlopen) and the
 * communicators are created by the first lol_gpu_multi_render_device: single-device users, and hosts that only ever
 * render into HOST surfaces (which need no exchange, see lol_gpu_multi_render_host), never touch it.  No CPU
 * fallback: a device listed twice fails at creation, a missing RCCL at the first frame that needs the exchange.
 */
typedef struct lol_gpu_multi lol_gpu_multi;

#define LOL_GPU_MULTI_MAX_DEVICES 16

int  lol_gpu_multi_create(const int* devices, int n_devices, lol_gpu_multi** out);
void lol_gpu_multi_destroy(lol_gpu_multi* m);
const char* lol_gpu_multi_error(const lol_gpu_multi* m);
int  lol_gpu_multi_device_count(const lol_gpu_multi* m);
/* the single-device context of device index i (to set its switches before the upload, read its logs) */
lol_gpu* lol_gpu_multi_context(lol_gpu_multi* m, int i);
/* render_prepare: the flattened scene goes to every device; the scene's kernel is compiled once, in the background
 * (lol_gpu_upload_program), and every device switches to it at its own next frame; _specialize_wait waits on all. */
int  lol_gpu_multi_upload_program(lol_gpu_multi* m, const lol_program* prog);
int  lol_gpu_multi_specialize_wait(lol_gpu_multi* m);
/* Band height used for frames of height h over n parts: the largest multiple of the 4-row wave patch <= 16
 * that gives equal parts, else the tallest one that still gives every part at least eight bands, else 4.
 * lol_gpu_multi_set_band_rows(m, b > 0) overrides. */
int  lol_gpu_choose_band_rows(int h, int n_parts);
int  lol_gpu_multi_set_band_rows(lol_gpu_multi* m, int band_rows);
/* Frame row shown by local row `local_row` of a part (the inverse of the kernel's mapping); -1 if out of range. */
int  lol_gpu_part_frame_row(int h, const lol_gpu_rows* rows, int local_row);
/*
 * One frame over all devices, asynchronously: on return the work is queued; the assembled XRGB8888 frame
 * is in `dst` (memory of the root device, `pitch_bytes` per row) once lol_gpu_multi_sync() returns.
 * Up to two frames may be in flight (double-buffered parts); give them different destinations.
 */
int  lol_gpu_multi_render_device(lol_gpu_multi* m, const lol_frame_camera* cam, int w, int h, int max_steps,
                                 void* dst, size_t pitch_bytes);
/* What render_thread does with surf->pixels: one frame over all devices into a HOST surface; waits.  No exchange is
 * needed for this: every device copies its own bands into the surface over its own PCIe link, all devices at once —
 * one host thread per device issues that device's strided copies (one per part): a copy into pageable memory occupies
 * the thread that issues it, so N threads are what makes N links run in parallel.  set_host_via_root(m, 1)
 * instead assembles on the root with the RCCL exchange and copies from there. */
int  lol_gpu_multi_render_host(lol_gpu_multi* m, const lol_frame_camera* cam, int w, int h, int max_steps,
                               void* host_pixels, size_t pitch_bytes);
int  lol_gpu_multi_set_host_via_root(lol_gpu_multi* m, int enable);
int  lol_gpu_multi_set_pixel_format(lol_gpu_multi* m, const lol_gpu_pixel_format* fmt);
int  lol_gpu_multi_set_tile_order(lol_gpu_multi* m, int order);         /* lol_gpu_set_tile_order on every device (each decides for itself under AUTO) */
int  lol_gpu_multi_set_samples(lol_gpu_multi* m, int samples);          /* lol_gpu_set_samples on every device (bands are output rows) */
/* Parts per device (default 1): the frame is cut into n * parts parts, part p belonging to device p % n, each part one
 * launch.  Finer interleaving of the rows, and the way a single-GPU machine exercises the multi-part code paths.
 * n * parts <= 64. */
int  lol_gpu_multi_set_parts_per_device(lol_gpu_multi* m, int parts);
/* The cost-weighted split: the root (devices[0]) also receives and un-interleaves the whole frame, so with an equal
 * share it finishes last.  root_band_rows > 0 makes the bands of the root's parts that tall instead of band_rows
 * (0 = like the others): its share of the rows is root_band_rows / (root_band_rows + (n - 1) * band_rows).  Still one
 * launch per part: only the geometry changes (lol_gpu_rows). */
int  lol_gpu_multi_set_root_band_rows(lol_gpu_multi* m, int root_band_rows);
/* The geometry itself, pure host logic: out[p] for p in [0, n_parts) = the lol_gpu_rows of part p when every part's
 * bands are band_rows tall except those of parts p % root_stride == 0, which are root_band_rows tall (0 = band_rows too;
 * root_stride = number of devices).  The bands tile a cycle in part order. */
int  lol_gpu_split_rows(int n_parts, int band_rows, int root_band_rows, int root_stride, lol_gpu_rows* out);
int  lol_gpu_multi_sync(lol_gpu_multi* m);
/* Memory on the root device (for destinations of lol_gpu_multi_render_device). */
int  lol_gpu_multi_malloc(lol_gpu_multi* m, size_t bytes, void** out);
int  lol_gpu_multi_free(lol_gpu_multi* m, void* ptr);
int  lol_gpu_multi_memcpy_d2h(lol_gpu_multi* m, void* host, const void* dev, size_t bytes);
/*
 * The root's assembly step on its own: `parts` holds n_parts compact parts back to back (part r starts at
 * row sum of lol_gpu_part_rows of the parts before it, w pixels per row); un-interleave them into `dst`.
 * Asynchronous on `stream` (NULL = the context's stream).  Exposed so the band logic can be checked on a
 * single device against a whole-frame render.
 */
int  lol_gpu_assemble_parts(lol_gpu* ctx, const void* parts, int n_parts, int band_rows, int w, int h,
                            void* dst, size_t pitch_bytes, void* stream);
/* The same for any split and any placement (parts gathered per rank and padded to a common size, bands of different
 * heights): part_rows[p] = the geometry of part p (the bands of all parts must tile one cycle, in order),
 * part_row0[p] = the row of `parts` (w pixels per row) where part p's compact copy starts. */
int  lol_gpu_assemble_parts_at(lol_gpu* ctx, const void* parts, const lol_gpu_rows* part_rows, const uint32_t* part_row0,
                               int n_parts, int w, int h, void* dst, size_t pitch_bytes, void* stream);

/*
 * Ray queries: what a host asks about the scene's GEOMETRY — what is under the cursor, how far is the thing the camera looks at,
 * will the camera walk through a wall, distance / object / normal for rays a torch pipeline brings itself — without a frame.
 *
 * Ray i is EXACTLY get_intersection(scene, ro_i, rd_i) (naive_renderer.c:48-69) with MAX_STEPS = max_steps, followed by
 * p = v3add(ro, v3scale(rd, dist)) (:227) and get_normal(scene, p, dist) (:228), in the reference's arithmetic: the same device code
 * the frames march with.  The normal is the reference's for escaped rays too (no miss skip applies to a query).  Nothing about a
 * ray is assumed: the direction is used as given (not normalised, may be zero), any component may be non-finite, huge, denormal or
 * -0, and each ray's answer is the reference's arithmetic on those bits, whatever the other rays of the list are.
 *
 * Queries neither use nor change the tile-order state, lol_gpu_set_samples / lol_gpu_set_adaptive_samples, the pixel format or the
 * record rings: a frame after a query is the frame it would have been.  lol_gpu_set_miss_skip / lol_gpu_set_exact_skips do not apply
 * (there is no shading); lol_gpu_set_cull applies as it does to frames: same answers either way.
 *
 * Out of scope for these entry points: shading or shadow queries (the colour along arbitrary rays is lol_gpu_shade_rays', below; the
 * shadow factor of every light is an output of lol_gpu_light_rays, further below), lol_gpu_multi_* forms, rays in host memory beyond the one-pixel
 * lol_gpu_pick, and the renderer.h protocol.
 */
typedef struct lol_gpu_hits {     /* DEVICE pointers, each may be NULL (not all four); element i belongs to ray i */
	float*    dist;               /* get_intersection().dist                               naive_renderer.c:68 */
	uint32_t* id;                 /* get_intersection().id: 1-based top-level object, 0 = escaped        :65-66 */
	uint32_t* steps;              /* iterations of the loop at :56 that ran                                     */
	float*    normal;             /* 3 floats per ray: get_normal(scene, ro + rd * dist, dist)         :114-125 */
} lol_gpu_hits;
/*
 * rays_dev: n x {ox, oy, oz, dx, dy, dz} in device memory, read only.  A NULL `normal` skips the four taps for the whole launch.
 * Asynchronous on `stream` (NULL = the context's own stream; LOL_GPU_STREAM_DEFAULT as elsewhere): one launch, no host wait, no
 * copy, no scratch.  n == 0 returns LOL_GPU_OK with nothing launched; nothing beyond element n - 1 of any output is written.
 * Refused, with nothing launched and nothing written: no context, NULL rays_dev with n > 0, NULL out or all four outputs NULL,
 * max_steps < 0, n > 2^32 - 1: LOL_GPU_ERR_ARG; no program: LOL_GPU_ERR_NO_PROGRAM.
 */
int  lol_gpu_trace_rays(lol_gpu* ctx, const float* rays_dev, size_t n, int max_steps, const lol_gpu_hits* out, void* stream);
/*
 * Ray i is the primary ray of pixel (x_i, y_i) = (xy_dev[2i], xy_dev[2i + 1]) of the w x h frame under `cam`, built as a frame
 * builds it (naive_renderer.c:218-221, :188-190).  For a pixel inside the frame `dist` and `id` ARE lol_gpu_debug.hit_dist and
 * hit_id of lol_gpu_render_device under that camera, bit for bit, and `steps` is the low 16 bits of its lol_gpu_debug.steps.
 * Coordinates are not inspected by the host: a pair outside the frame gives the ray that formula gives (the coordinates as `int`).
 * The sample rays of supersampling (lol_gpu_set_samples) are pixels (s x + i, s y + j) of the s w x s h frame under the same `cam`.
 * Refusals as for lol_gpu_trace_rays (xy_dev in the place of rays_dev), and LOL_GPU_ERR_ARG for w < 1, h < 1 or a NULL cam.
 */
int  lol_gpu_trace_pixels(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps,
                          const uint32_t* xy_dev, size_t n, const lol_gpu_hits* out, void* stream);
/*
 * The host convenience: one lol_gpu_trace_pixels of pixel (x, y) on the context's own stream, through a few dozen bytes of device
 * memory the context owns from the first pick on; copies back, WAITS, and fills HOST memory.  x, y outside the frame:
 * LOL_GPU_ERR_ARG.  It orders itself after frames already queued on the context's streams only as far as its own stream does, and
 * does not touch frames in flight.
 */
typedef struct lol_gpu_hit { float dist; uint32_t id, steps; float normal[3]; } lol_gpu_hit;
int  lol_gpu_pick(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps, int x, int y, lol_gpu_hit* out);
/*
 * Which kernel answers: after lol_gpu_set_ray_queries(ctx, 1) BEFORE lol_gpu_upload_program the scene's own module also carries
 * lol_trace_spec (both kernels of a 257 ... 1024-op scene do); otherwise, and until that module is ready, the interpreter's
 * trace_interp answers — same bits either way.  A module compiled without the switch is the module it was before the switch
 * existed: same source, same code object, same lol_gpu_kernel_key.
 */
int  lol_gpu_set_ray_queries(lol_gpu* ctx, int enable);
int  lol_gpu_ray_queries(const lol_gpu* ctx);

/*
 * Shading queries: the COLOUR the reference computes along rays the host brings itself — an equirectangular panorama or a fisheye,
 * a torch pipeline with its own camera model, the linear colour of a few pixels without a frame, one sample of a supersampled pixel.
 *
 * Ray i is EXACTLY naive_renderer.c:225-232 for one ray (ro, rd): get_intersection(scene, ro, rd) with MAX_STEPS = max_steps,
 * p = ro + rd * dist, get_normal(scene, p, dist), get_light(scene', p, n, id), v3pow(., 1 / 2.2), colorf_to_pixfmt — where scene' is
 * the uploaded scene with camera.point = ro: get_light reads the eye position from the scene (:132, :145), and a ray's eye is its
 * own origin.  For a frame ro is the camera's position, so this is no new definition.  The same device code the frames shade with.
 *
 * lol_gpu_set_miss_skip / lol_gpu_set_exact_skips and lol_gpu_set_cull apply as they do to frames: the colours are the same either
 * way, `steps` counts the steps really marched.  The pixel format (lol_gpu_set_pixel_format) and the proven gamma table are read.
 * The tile-order state, lol_gpu_set_samples / lol_gpu_set_adaptive_samples and the record rings are neither read nor written: a
 * frame after a query is the frame it would have been.
 *
 * Out of scope: a per-light shadow-factor output (lol_gpu_light_rays has it, below), normals (lol_gpu_trace_rays has them), lol_gpu_multi_* forms, rays in host
 * memory, a shading pick, and the renderer.h protocol.
 */
typedef struct lol_gpu_shades {   /* DEVICE pointers, each may be NULL (not all six); element i belongs to ray i */
	float*    rgb_linear;         /* 3 floats: what get_light() returns (naive_renderer.c:229), clamped, before gamma */
	float*    rgb;                /* 3 floats: after gamma (:231) — lol_gpu_debug.rgb of that pixel                    */
	uint32_t* pixel;              /* packed in the context's pixel format (lol_gpu_set_pixel_format), like a frame's   */
	float*    hit_dist;           /* as lol_gpu_debug                                                                  */
	uint32_t* hit_id;
	uint32_t* steps;              /* low 16 bits march steps, high 16 bits shadow steps summed over the lights         */
} lol_gpu_shades;
/*
 * rays_dev: n x {ox, oy, oz, dx, dy, dz} in device memory, read only, used as given like lol_gpu_trace_rays': not normalised, any
 * component may be zero, non-finite, huge, denormal or -0, and each ray's answer is the reference's arithmetic on those bits,
 * whatever the other rays of the list are.
 * Asynchronous on `stream` (NULL = the context's own stream; LOL_GPU_STREAM_DEFAULT as elsewhere): one launch, no host wait, no
 * copy, no scratch.  n == 0 returns LOL_GPU_OK with nothing launched; nothing beyond element n - 1 of any output is written.
 * Refused, with nothing launched and nothing written: no context, NULL rays_dev with n > 0, NULL out or all six outputs NULL,
 * max_steps < 0, n > 2^32 - 1: LOL_GPU_ERR_ARG; no program: LOL_GPU_ERR_NO_PROGRAM.
 */
int  lol_gpu_shade_rays(lol_gpu* ctx, const float* rays_dev, size_t n, int max_steps, const lol_gpu_shades* out, void* stream);
/*
 * Ray i is the primary ray of pixel (x_i, y_i) = (xy_dev[2i], xy_dev[2i + 1]) of the w x h frame under `cam`, built as
 * lol_gpu_trace_pixels builds it.  For a pixel inside the frame `pixel`, `rgb`, `hit_dist`, `hit_id` and `steps` ARE that pixel of
 * lol_gpu_render_device and its lol_gpu_debug planes under the same camera, settings and pixel format, bit for bit.  A pair
 * outside the frame gives the ray that formula gives.  The sample rays of lol_gpu_set_samples(s) are pixels (s x + i, s y + j) of
 * the s w x s h frame under the same `cam`; their `rgb_linear` are the leaves of that pixel's tree.
 * Refusals as for lol_gpu_shade_rays (xy_dev in the place of rays_dev), and LOL_GPU_ERR_ARG for w < 1, h < 1 or a NULL cam.
 */
int  lol_gpu_shade_pixels(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps,
                          const uint32_t* xy_dev, size_t n, const lol_gpu_shades* out, void* stream);
/*
 * Which kernel answers: after lol_gpu_set_shade_queries(ctx, 1) BEFORE lol_gpu_upload_program the scene's own module also carries
 * lol_shade_spec (both kernels of a 257 ... 1024-op scene do); otherwise, and until that module is ready, the interpreter's
 * shade_interp answers — same bits either way.  A module compiled without the switch is the module it was before the switch
 * existed: same source, same code object, same lol_gpu_kernel_key.
 */
int  lol_gpu_set_shade_queries(lol_gpu* ctx, int enable);
int  lol_gpu_shade_queries(const lol_gpu* ctx);

/*
 * Scene views: a batch whose every view brings its own SCENE — the frames of an animation in one launch, a moving object blurred over
 * its exposure.  The modes above vary the pixel's area, the camera and the ray; this one varies the numbers of the scene: where its
 * objects are and how large, its smoothness constants, lights, materials and ambient colour — everything but its structure.
 * `cams` and `scenes` are HOST memory and hold n_views * K entries each, K = cams_per_view in {1, 2, 4, 8, 16}; both, and the tables
 * the programs point to, are copied before the call returns.  Record r = v * K + k is one camera and one scene.
 * Record r is EXACTLY the frame that a context with this context's settings — the pixel format, lol_gpu_set_exact_skips and
 * lol_gpu_set_cull — renders under cams[r] after lol_gpu_upload_program(&scenes[r]).  With K = 1 view v IS that frame: the packed
 * pixels, rgb, hit_dist, hit_id and steps, addressed and with dense diagnostics as in lol_gpu_render_views.  With K > 1 view v is
 * lol_gpu_render_views_blend's pixel with sample k taken from record v K + k: the balanced binary32 tree over the K clamped linear
 * colours, the factor 1 / K, gamma and packing are unchanged; rgb is the mean after gamma; hit_dist, hit_id and steps are refused
 * (LOL_GPU_ERR_UNSUPPORTED) as for any blend.
 * Every scene must have the uploaded program's STRUCTURE: equal n_ops, n_lights, n_materials, n_roots and max_stack, and equal
 * ops[i].op and ops[i].id for every i.  Everything else may differ per record — every f[] of every op, lights, materials,
 * root_material, ambient_color — and nothing about the numbers is assumed: a NaN centre in one record is that record's business alone.
 * Everything an upload or a frame decides from the program or the camera is decided per record, from that record's own scene and
 * camera: the three exact skips, whether the scene is finite (which of the interpreter's two lists runs), the primary march's first
 * step, what a camera beyond the sane range switches off.  No proof runs on the device during the call: a smoothness constant the
 * upload did not prove takes the plain sminf — same bits.
 * The context's own scene, kernels, lol_gpu_kernel_key, tile-order state, sample settings and the record rings of the other batches
 * are neither read nor changed: a frame after the call is the frame it would have been.
 * Asynchronous on `stream` like lol_gpu_render_views: one copy of the records and their data (each record's macro-op lists where the
 * interpreter renders, its tables, its numbers) and, with K = 1, one launch; a blend adds lol_gpu_render_views_blend's resolve pass
 * and takes its scratch from that call's ring of 4 sets.  The records and their data go through a ring of 8 sets of their own that
 * grow on demand, under the rules of lol_gpu_render_views' ring (HIP's special stream handles included).
 * Refused, with nothing launched and nothing written: a scene whose structure differs, a NULL table that a count speaks of, a
 * root_material out of range, K outside {1, 2, 4, 8, 16} — LOL_GPU_ERR_ARG; everything lol_gpu_render_views_blend refuses, with
 * n_views * K <= LOL_GPU_MAX_VIEWS; no program — LOL_GPU_ERR_NO_PROGRAM; an allocation that fails — LOL_GPU_ERR_HIP, and the context
 * stays usable.
 * Which kernel: after lol_gpu_set_scene_views(ctx, 1) BEFORE lol_gpu_upload_program, with specialisation on and a program of at most
 * 256 ops, the scene compiler also makes the STRUCTURE MODULE behind the scene's own: the scene's SDF as straight-line code
 * specialised on the structure alone, every number read from the record (lol_render_param_batch, lol_render_param_batch_lin) —
 * objects in file order, no culling, no proven shortcut.  A code object of its own, not a switch of the scene's module: that module
 * and lol_gpu_kernel_key are what they are without the setter, and all scenes of one structure share the structure module in the
 * code-object cache.  lol_gpu_specialize_wait waits for it too.  Otherwise, until it is loaded, or if it failed, the interpreter's
 * render_interp_scene_batch / render_interp_scene_batch_lin render on each record's own lists — same bits either way
 * (lol_gpu_scene_views_kernel_name, lol_gpu_scene_views_state: lol_gpu_diag.h).  Opt-in, and not the default for a reason: on the one scene
 * measured (scene4) the interpreter with the upload's proven fast paths was the faster of the two (README.md quotes the numbers).
 * Out of scope: an adaptive form (of the supersampled and adaptive forms that batches of views have, the supersampled one is
 * lol_gpu_render_scene_views_samples below; ray and shading queries over per-record scenes are lol_gpu_trace_scene_rays' and its
 * siblings', further below), row partitions, lol_gpu_multi_* forms, host surfaces and the renderer.h protocol; and the structure module is not kept across uploads of the same structure
 * (each upload loads it anew, from the cache).
 */
int  lol_gpu_render_scene_views(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_views, int cams_per_view,
                                int w, int h, int max_steps, void* dst, size_t pitch_bytes, size_t view_stride_bytes,
                                const lol_gpu_debug* dbg, void* stream);
int  lol_gpu_set_scene_views(lol_gpu* ctx, int enable);   /* before lol_gpu_upload_program */
int  lol_gpu_scene_views(const lol_gpu* ctx);

/*
 * Supersampled scene views: lol_gpu_render_scene_views with `samples` x `samples` = s x s samples per pixel, s in {1, 2, 4} — an
 * antialiased animation in one launch, a motion-blurred object whose stationary edges are smooth as well.
 * Record r = v * K + k is one camera and one scene, as in lol_gpu_render_scene_views; K = cams_per_view in {1, 2, 4, 8, 16}.
 * Pixel (x, y) of view v:
 *  1. for each k, m_k is the linear mean of lol_gpu_set_samples' steps 1 - 2 taken on record r's OWN scene under cams[r]: the s^2
 *     samples are pixels (s x + i, s y + j) of the reference's s w x s h frame of scenes[r], as clamped linear colours, in the order
 *     j s + i, summed as the balanced binary32 tree, and the sum multiplied by 1 / s^2;
 *  2. m_0 ... m_{K-1} are summed as the tree of lol_gpu_render_views_blend, and the sum is multiplied by 1 / K;
 *  3. gamma and the context's pixel format follow, as for one sample.
 * The rounding order is that of lol_gpu_render_views_blend_samples: two trees, one after the other, not one tree over K s^2 leaves.
 * Three identities: s = 1 IS lol_gpu_render_scene_views — the call forwards to it, so K = 1 keeps all diagnostics.  With K = 1 and
 * s > 1 view v IS the frame that a context with lol_gpu_set_samples(s) renders under cams[v] after
 * lol_gpu_upload_program(&scenes[v]), bit for bit.  And when every record carries the uploaded scene the call IS
 * lol_gpu_render_views_blend_samples.
 * What carries over unchanged from lol_gpu_render_scene_views: everything an upload or a frame decides is decided per record, on the
 * host, from that record's own scene and camera — the three exact skips, which of the interpreter's lists runs, the primary march's
 * first step, what an insane camera switches off.  The first step is sdf(cam.origin) and so the same for every sample of a record.
 * No proof runs on the device.  The context's scene, kernels, lol_gpu_kernel_key, tile-order state, sample settings
 * (lol_gpu_set_samples and lol_gpu_set_adaptive_samples are not read: the samples are this argument) and the other rings are neither
 * read nor changed.
 * Resources: with K = 1 one copy of the records and one launch over the sample grids of all records.  With K > 1 the same launch
 * writes one LinearColour per PIXEL and record into the blend's scratch ring — 16 * n_views * K * w * h bytes, the ring of 4 sets
 * that lol_gpu_render_views_blend uses, a pixel's samples being reduced in registers — and the resolve pass follows.  The records go
 * through scene views' ring of 8 sets.  No new ring and no new scratch layout.
 * Diagnostics: lol_gpu_debug.rgb is the mean after gamma, dense [v][y][x]; hit_dist, hit_id and steps are refused with
 * LOL_GPU_ERR_UNSUPPORTED whenever s > 1 or K > 1.
 * Refused, with nothing launched and nothing written, and the context stays usable: s outside {1, 2, 4} — LOL_GPU_ERR_ARG, checked
 * first; then everything lol_gpu_render_scene_views refuses, in its order; a sample count this build's wave patch cannot take —
 * LOL_GPU_ERR_UNSUPPORTED (as lol_gpu_set_samples); a sample grid of more than 65535 tiles along an axis, or more than 2^32 - 1
 * lanes over all n_views * K sample grids — LOL_GPU_ERR_ARG.
 * Which kernel: after lol_gpu_set_scene_view_samples(ctx, 1) BEFORE lol_gpu_upload_program the STRUCTURE MODULE is made with two more
 * kernels, lol_render_param_batch_aa and lol_render_param_batch_aa_lin.  The setter brings lol_gpu_set_scene_views with it; it makes
 * another source of that module, hence another code object and cache entry, and without it the structure module is byte for byte
 * what it is without this call's existence.  Without the setter, until the module is loaded, or if it failed, the interpreter's
 * render_interp_scene_batch_aa / render_interp_scene_batch_aa_lin render on each record's own lists — same bits either way
 * (lol_gpu_scene_view_samples_kernel_name: lol_gpu_diag.h).
 * Out of scope: an adaptive form, row partitions, lol_gpu_multi_* forms, host surfaces and the renderer.h protocol
 * (ray and shading queries over per-record scenes are built: "Scene queries", below).
 */
int  lol_gpu_render_scene_views_samples(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_views,
                                        int cams_per_view, int w, int h, int max_steps, int samples, void* dst, size_t pitch_bytes,
                                        size_t view_stride_bytes, const lol_gpu_debug* dbg, void* stream);
int  lol_gpu_set_scene_view_samples(lol_gpu* ctx, int enable);   /* before lol_gpu_upload_program */
int  lol_gpu_scene_view_samples(const lol_gpu* ctx);

/*
 * Scene queries: ray and shading queries under each record's own SCENE — what is under the cursor in frame t of an animation, how far
 * away the moving object is in each frame (a lens that follows it), whether the camera path walks through it as it moves, the colour
 * of a probe pixel over the exposure — without an upload per frame and without rendering frames to read one pixel.
 * `scenes` (and `cams`, for the *_pixels forms) are HOST memory and hold n_scenes entries, 1 <= n_scenes <= LOL_GPU_MAX_VIEWS; both, and
 * the tables the programs point to, are copied before the call returns.  Record r is one scene and, in the pixel forms, one camera.
 * Each record answers n rays: the rays of a list in device memory (n x {ox, oy, oz, dx, dy, dz}, used as given) or the primary rays
 * of n pixels {x, y} of the w x h frame under cams[r].  list_stride == 0: one list of n elements serves every record; otherwise
 * list_stride >= n, and record r's list begins list_stride ELEMENTS (rays, or {x, y} pairs) behind record r - 1's.  The outputs are
 * dense: element (r, i) lies at index r * n + i of every output (three floats each for normal, rgb_linear and rgb); all addressing
 * is 64-bit.
 * Contract: element (r, i) is EXACTLY what lol_gpu_trace_rays, lol_gpu_trace_pixels, lol_gpu_shade_rays or lol_gpu_shade_pixels answers
 * for that ray on another context with this context's settings (lol_gpu_set_exact_skips, lol_gpu_set_cull, the pixel format) that called
 * lol_gpu_upload_program(&scenes[r]) and, for the pixel forms, asks under cams[r] — bit for bit: dist, id, normal, rgb_linear, rgb,
 * pixel, hit_dist, hit_id, and the march step count.  So each element is the reference's arithmetic on record r's own numbers, for NaN,
 * infinite, zero and unnormalised rays too, whatever the other rays and the other records hold.
 * One latitude, the one light updates have: for a LIST OF RAYS with the settled-shadow exit on (bit 2 of lol_gpu_set_exact_skips), the
 * high 16 bits of lol_gpu_shades.steps (shadow steps) are "the steps really marched", and are held equal to that other context's only
 * after lol_gpu_set_exact_skips(ctx, 0).  For pixel sources all 32 bits are equal.
 * Every scene must have the uploaded program's STRUCTURE; the test, the refusal and its text are lol_gpu_render_scene_views'.  Every
 * number may differ, and a NaN centre in one record is that record's business alone.
 * Decided per record, on the host, from that record's own scene and camera — everything an upload or a query decides: the three exact
 * skips (shading); whether the scene is finite, i.e. the scene's side of what the fast SDF and the settled exit rest on; which of the
 * record's two macro-op lists runs (lists of rays: the one every camera may use; pixels: what that record's camera allows); and, for
 * the pixel forms, the first march step sdf(cams[r].origin) on that record's scene.  No proof runs on the device: a smoothness
 * constant the upload did not prove takes the plain sminf — same bits.
 * Asynchronous on `stream` (NULL = the context's own stream; LOL_GPU_STREAM_DEFAULT as elsewhere): one copy of the records and their
 * data through scene views' ring of 8 sets, under its rules (HIP's special stream handles included), and ONE launch; no scratch, no
 * host wait.  The context's scene, kernels, lol_gpu_kernel_key, tile-order state, sample settings and other rings are neither read
 * nor changed: a frame after the call is the frame it would have been.
 * Refused, with nothing launched and nothing written, in this order:
 *  1. what the single-scene query refuses, in its order: no context, a NULL list with n > 0, NULL out or every output NULL,
 *     max_steps < 0, n > 2^32 - 1 — LOL_GPU_ERR_ARG; no program — LOL_GPU_ERR_NO_PROGRAM; w < 1 or h < 1 — LOL_GPU_ERR_ARG;
 *  2. LOL_GPU_ERR_ARG for NULL scenes, n_scenes < 1 or > LOL_GPU_MAX_VIEWS, NULL cams in a pixel form, a list_stride that is neither 0
 *     nor >= n, n_scenes * n > 2^32 - 1;
 *  3. the scene refusals of lol_gpu_render_scene_views: a missing table, another structure, a root_material out of range.
 * n == 0 returns LOL_GPU_OK with nothing launched.  An allocation that fails returns LOL_GPU_ERR_HIP, and the context stays usable.
 * Which kernel: the interpreter's trace_interp_scenes / shade_interp_scenes, always.  lol_gpu_set_scene_views, lol_gpu_set_ray_queries
 * and lol_gpu_set_shade_queries have no effect on these calls.
 * Out of scope: a structure-module form, light passes over records, lists in host memory, lol_gpu_multi_* forms, and a C pick over
 * records (the Python mirror has the convenience: Renderer.pick_scenes).
 * (Light passes over records are built since: "Scene light passes", below.)
 */
int  lol_gpu_trace_scene_rays(lol_gpu* ctx, const lol_program* scenes, int n_scenes, const float* rays_dev, size_t n, size_t list_stride,
                              int max_steps, const lol_gpu_hits* out, void* stream);
int  lol_gpu_trace_scene_pixels(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_scenes, int w, int h,
                                int max_steps, const uint32_t* xy_dev, size_t n, size_t list_stride, const lol_gpu_hits* out, void* stream);
int  lol_gpu_shade_scene_rays(lol_gpu* ctx, const lol_program* scenes, int n_scenes, const float* rays_dev, size_t n, size_t list_stride,
                              int max_steps, const lol_gpu_shades* out, void* stream);
int  lol_gpu_shade_scene_pixels(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_scenes, int w, int h,
                                int max_steps, const uint32_t* xy_dev, size_t n, size_t list_stride, const lol_gpu_shades* out, void* stream);

/*
 * Light passes and relighting: a new LOOK without a march.  The look of a scene is what a host changes most often once the rays are
 * fixed: the colour and strength of its lights, the colours of its materials, the ambient colour.  get_light (naive_renderer.c:129-175)
 * is linear in the look once three scalars per light are known, and the expensive part of a pixel — the march, the normal, the shadow
 * marches — fixes them.  Captured once (lol_gpu_light_rays, lol_gpu_light_pixels), they make any number of looks in a memory-bound
 * pass (lol_gpu_relight), each THE REFERENCE'S PIXEL FOR THE CHANGED SCENE, bit for bit: the pass executes the same binary32
 * operations in the same order.  The planes are also the per-light outputs a compositing host expects: shadow and incidence per light.
 *
 * Ray i, its march, hit point p, normal n and eye (the ray's own origin) are exactly those of lol_gpu_shade_rays /
 * lol_gpu_shade_pixels.  For each light l of the uploaded scene, in file order:
 *   shadow_l = in_shadow(scene, light_l, p)                                     naive_renderer.c:136 (:93-100, :73-90)
 *   di_l     = clamp(v3dot(n, light_dir_l), 0, 1)                               :148
 *   si_l     = di_l * powf(clamp(v3dot(reflected_dir_l, camera_dir), 0, 1),     :158-161, camera_dir from the ray's origin
 *                          material(id).shininess)
 *   steps_l  = iterations of the loop at :80 that ran for light l
 */
typedef struct lol_gpu_light_factor { float shadow, diffuse_incidence, specular_incidence; uint32_t shadow_steps; } lol_gpu_light_factor;  /* 16 bytes */

typedef struct lol_gpu_light_passes {     /* DEVICE pointers */
	lol_gpu_light_factor* factors;  /* light-major planes: light l of ray i at factors[l * light_stride + i]; 16-byte aligned */
	size_t    light_stride;         /* elements between planes; 0 = n; else >= n */
	uint32_t* hit_id;               /* as lol_gpu_shades.hit_id */
	float*    hit_dist;             /* optional */
	uint32_t* march_steps;          /* optional: low 16 bits of lol_gpu_shades.steps */
} lol_gpu_light_passes;

typedef struct lol_gpu_relit { float* rgb_linear; float* rgb; uint32_t* pixel; } lol_gpu_relit;   /* as lol_gpu_shades'; each may be NULL, not all three */
/*
 * Capture.  Every factor is the reference's value, for every ray and every light: the escaped-wave skip and the zero-incidence skip
 * are OFF for these launches, whatever lol_gpu_set_exact_skips says — a look may give material #0 a diffuse colour or a light an
 * infinite intensity, and then the values those skips leave uncomputed are no longer multiplied into +-0.  The settled-shadow exit
 * (bit 2) applies as it does to frames: it changes no factor; shadow_steps counts the steps really marched, and after
 * lol_gpu_set_exact_skips(ctx, 0) it is the reference's count.  lol_gpu_set_cull applies as it does to frames.  Rays are used as
 * given, as lol_gpu_shade_rays uses them (NaN, infinite, zero and unnormalised rays are accepted; the same per-wave test decides
 * between the fast and the exact SDF).  lol_gpu_light_pixels is lol_gpu_shade_pixels' list of pixels, or with xy_dev == NULL every
 * pixel of the frame: ray i is pixel (i % w, i / w), and n must be w * h.
 * Asynchronous on `stream` as lol_gpu_shade_rays: one launch, no copy, no scratch, no host wait; nothing of the frames' state — tile
 * order, samples, rings — is read or written.  n == 0 returns LOL_GPU_OK with nothing launched; nothing beyond element n - 1 of any
 * plane, and nothing between the planes, is written.  A scene with no lights may pass factors == NULL.
 * Which kernel: the interpreter's light_interp, always (see "Out of scope").
 *
 * Resolve.  Element i of lol_gpu_relight: with m' = look.materials[id_i ? look.root_material[id_i - 1] : 0], Id'_l, Is'_l and
 * ambient' the look's,
 *   total = 0
 *   for l in file order:  total += (Id'_l * (shadow_l * di_l)) * m'.diffuse          :150-155
 *                         total += (Is'_l * (shadow_l * si_l)) * m'.specular         :163-168
 *   total += ambient' * m'.ambient                                                   :171-172
 *   rgb_linear = v3clamp(total, 0, 1);  rgb = v3pow(., 1 / 2.2);  pixel = the context's pixel format
 * bracketed and rounded exactly as written.  `look` is HOST memory (NULL = the uploaded program: the context's own device tables are
 * read and nothing is copied) and may differ from the uploaded program in the lights' diffuse and specular intensities, the
 * materials' diffuse, specular and ambient colours, and ambient_color — any bits, NaN and infinite included.  Everything else must be
 * bitwise equal, which the host checks before anything is queued: n_ops, n_lights, n_materials, n_roots and max_stack; every
 * ops[i].op, .id and .f[]; every lights[l].point; every materials[m].shininess (as bits: a NaN shininess equals itself); every
 * root_material[].  So lol_gpu_relight(look) over planes captured from rays R IS lol_gpu_shade_rays of R on a context that uploaded
 * the look — rgb_linear, rgb and pixel, bit for bit —, over the planes of all pixels it IS lol_gpu_render_device's frame of the look,
 * and with look == NULL the capturing context's own shading query or frame.  An id in the planes beyond n_roots (no capture writes
 * one) is taken for 0.
 * The look's tables are copied before the call returns, through a ring of 8 sets of their own under the rules of lol_gpu_render_views'
 * ring (HIP's special stream handles included); an allocation that fails returns LOL_GPU_ERR_HIP with nothing launched, and the
 * context stays usable.  One copy and one launch, asynchronous on `stream`.
 *
 * Refused, with nothing launched and nothing written — LOL_GPU_ERR_ARG: no context, NULL rays_dev with n > 0, NULL out / in; NULL
 * hit_id; NULL factors while the program has lights, or factors not 16-byte aligned; light_stride neither 0 nor >= n; all three of
 * lol_gpu_relit NULL; max_steps < 0 or n > 2^32 - 1; w < 1, h < 1 or NULL cam; xy_dev == NULL with n != w * h; a look that differs
 * in anything it may not differ in, a NULL table that one of its counts speaks of, a root_material out of range.
 * LOL_GPU_ERR_NO_PROGRAM: no program uploaded.
 *
 * Out of scope: a scene-module capture kernel (a lol_light_spec would be one more module switch, and folding it into the shading
 * switch would change the code object of every module compiled with that switch: the interpreter captures, at the interpreter's
 * speed); capture in ONE launch over batches, blends or samples (lol_gpu_light_views, below, covers them with one capture launch
 * per camera, and lol_gpu_relight_views resolves them); per-record scenes; moving a light or changing a shininess (they change the
 * factors: capture again, or update the planes — "Light updates", below); lol_gpu_multi_* forms; planes in host memory; and the renderer.h protocol.
 * (Per-record scenes, and their capture in one launch, are built since: lol_gpu_light_scene_rays, lol_gpu_light_scene_pixels and
 * lol_gpu_relight_scenes, "Scene light passes", below.)
 */
int  lol_gpu_light_rays(lol_gpu* ctx, const float* rays_dev, size_t n, int max_steps, const lol_gpu_light_passes* out, void* stream);
int  lol_gpu_light_pixels(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps,
                          const uint32_t* xy_dev /* NULL: every pixel, i = y*w + x, n must be w*h */, size_t n,
                          const lol_gpu_light_passes* out, void* stream);
int  lol_gpu_relight(lol_gpu* ctx, const lol_program* look /* HOST; NULL = the uploaded program */,
                     const lol_gpu_light_passes* in, size_t n, const lol_gpu_relit* out, void* stream);

/*
 * Relit views: the AVERAGED pictures of a look without a march — the supersampled frame (lol_gpu_set_samples), the blend over K
 * cameras (lol_gpu_render_views_blend: motion blur, depth of field) and the supersampled blend (lol_gpu_render_views_blend_samples),
 * from captured light passes.  All of those average in LINEAR light, in a fixed binary32 tree, before gamma; averaging relit 8-bit
 * pixels on the host is not that (see lol_gpu_render_views_blend).  Sample (i, j) of pixel (x, y) is by contract pixel (s x + i,
 * s y + j) of the s w x s h frame under the same camera (lol_frame_camera_init gives the same bits for both sizes), so a capture of
 * every pixel of that frame holds every sample, and the camera of a blend is one more capture.
 *
 * The planes.  K = cams_per_view in {1, 2, 4, 8, 16}, s = samples in {1, 2, 4}.  LEAF (v, k, Y, X) — sample column X < s w, sample row
 * Y < s h under cams[v K + k] — is element e = ((v K + k) s h + Y) s w + X of N = n_views K s^2 w h.  The factor planes are
 * light-major over all N elements (light l of element e at factors[l * light_stride + e]; light_stride 0 = N, else >= N); hit_id,
 * hit_dist and march_steps are dense over e.
 *
 * lol_gpu_light_views is a host loop of n_views * K CAPTURE LAUNCHES and nothing else: record r = v K + k is exactly
 * lol_gpu_light_pixels(ctx, &cams[r], s w, s h, max_steps, NULL, s^2 w h, ...) into the planes r s^2 w h elements further on, with the
 * light stride of the whole; everything that call takes applies per record (the settled-shadow exit, culling, the per-camera
 * decisions).  The whole call is validated before the first launch: refused, nothing is launched; a HIP failure in the loop is
 * reported as that call reports it, with the earlier records queued.
 *
 * lol_gpu_relight_views makes pixel (x, y) of view v, bracketed and rounded exactly so:
 *   1. per leaf, c = the rgb_linear of lol_gpu_relight for its element under `look` (an id beyond n_roots is taken for 0);
 *   2. per camera k, m_k = the balanced binary32 tree over the s^2 leaves (s x + i, s y + j) in order j s + i, times 1 / s^2
 *      (s = 1: the leaf itself, unscaled);
 *   3. the balanced tree over m_0 ... m_{K-1} in order of k, times 1 / K (K = 1: m_0 itself);
 *   4. gamma and the context's pixel format, exactly as for one sample's colour.
 * Each camera's scale first, then the tree over the cameras: the order lol_gpu_render_views_blend_samples fixes.  The outputs are
 * dense over pixels, at index (v h + y) w + x: rgb_linear the mean before gamma (the render calls do not expose it), rgb the mean
 * after gamma, pixel the packed pixel; any subset, not none.  So, bit for bit: K = 1 and s = 1 is lol_gpu_relight over N elements
 * (the call forwards to it); K = 1, s > 1 over a capture of all samples is lol_gpu_render_device's frame of a context that uploaded
 * the look and has lol_gpu_set_samples(s); K > 1 is the view of lol_gpu_render_views_blend / _blend_samples on such a context; and
 * look == NULL gives the capturing context's own views.
 * The look is checked, copied and ringed exactly as lol_gpu_relight does (the same ring of 8 sets, the same refusals).  One copy and
 * ONE launch (relight_views), asynchronous on `stream`; nothing of the frames' state — tile order, samples, rings of batches and
 * blends — is read or written.
 *
 * Refused, with nothing launched and nothing written — LOL_GPU_ERR_ARG: everything lol_gpu_relight and lol_gpu_light_pixels refuse
 * (NULL cams among it); cams_per_view outside {1, 2, 4, 8, 16}; samples outside {1, 2, 4}; n_views < 1, w < 1 or h < 1;
 * N > 2^32 - 1; a light_stride neither 0 nor >= N.  LOL_GPU_ERR_NO_PROGRAM: no program uploaded.
 *
 * Out of scope: a scene-module capture kernel (as above); edge-adaptive relit supersampling; per-record scenes; lol_gpu_multi_*
 * forms; planes in host memory; pitch or stride addressing of the outputs.
 * (Per-record scenes are built since for the capture and for the resolve of single leaves: "Scene light passes", below; with equal
 * scenes that capture writes this section's planes in one launch.)
 * (Per-record scenes are built since for the averaged resolve too: "Relit scene views", below.)
 */
int  lol_gpu_light_views(lol_gpu* ctx, const lol_frame_camera* cams /* HOST */, int n_views, int cams_per_view,
                         int w, int h, int samples, int max_steps, const lol_gpu_light_passes* out, void* stream);
int  lol_gpu_relight_views(lol_gpu* ctx, const lol_program* look /* HOST; NULL = the uploaded program */,
                           const lol_gpu_light_passes* in, int n_views, int cams_per_view, int w, int h, int samples,
                           const lol_gpu_relit* out, void* stream);

/*
 * Light updates: captured planes brought to a look that MOVES LIGHTS or changes a SHININESS, without the primary march.  Those two
 * edits change the factors, so lol_gpu_relight refuses them ("capture again") — but a capture is the primary march of every ray,
 * the four normal taps and a shadow march towards every light, and almost all of it is unchanged: the march's result is in the planes
 * (hit_dist, hit_id), the hit point is p = ro + rd * dist on those bits, the normal is four SDF values at p, the factors of lights that
 * stand where they stood are in their planes, and a shininess enters specular_incidence alone.
 *
 * Definition.  The context has uploaded program U; the planes (factors light-major, hit_id, hit_dist) hold a capture of some source —
 * a list of rays, or pixels of a w x h frame under a camera — under U.  An update takes the SAME source, a HOST program `look` and two
 * masks of lights (bit l = light l):
 *   - `look` has U's geometry: equal counts, ops (opcode, id, every number) and root_material.  It may differ from U in any
 *     lights[l].point, any materials[m].shininess, and in what a look of lol_gpu_relight may differ in;
 *   - for every light l of march_lights, element i of plane l becomes the whole lol_gpu_light_factor a capture of ray i gives on a
 *     context that uploaded `look`, with the same lol_gpu_set_exact_skips: shadow, diffuse_incidence, specular_incidence and
 *     shadow_steps;
 *   - for every light l of specular_lights that is not in march_lights, the 4 bytes of specular_incidence alone become that capture's;
 *     the other 12 bytes of the element stay as they are.  For a light that did not move, where only a shininess changed: no shadow
 *     march is made;
 *   - the planes of lights in neither mask, hit_id, hit_dist and march_steps are not written.
 * The arithmetic is the capture's with its march replaced by a read: dist = hit_dist[i], id = hit_id[i] (an id above n_roots is taken
 * for 0), p = ro + rd * dist, the normal's four taps at p, the direction to the eye, and per chosen light the capture's own loop body
 * on the look's tables.  Rays that escaped (dist = +inf), NaN, infinite and zero rays go through the same expressions.  So the updated
 * planes are bit for bit a fresh capture under `look`, and lol_gpu_relight_held of them is the reference's pixel for the look's scene.
 * shadow_steps counts the steps really marched: the reference's count after lol_gpu_set_exact_skips(ctx, 0); otherwise the settled
 * shadow exit applies where it would on a context that uploaded the look (the look's light points are part of that test).
 * ONE DIFFERENCE from a capture: for a ray LIST with the settled exit on, a wave of a capture can fall back to the plain, unsettled
 * pass because of something its PRIMARY march met; an update has no primary march, and such a wave may keep the settled count in
 * shadow_steps.  The three floats are equal in every case, and for pixel sources all 16 bytes are.
 *
 * One asynchronous launch (light_update_interp: the interpreter's, always) behind one small copy of the look's tables through the
 * ring of 8 sets lol_gpu_relight uses; no host wait; nothing of the frames' state is read or written.  There is no max_steps: nothing
 * marches from the eye.  n == 0, or both masks 0, launches nothing.
 *
 * Refused, with nothing queued — LOL_GPU_ERR_ARG: everything the capture of the same source refuses; a NULL look; hit_dist == NULL;
 * a mask bit at or above n_lights (lights from the 64th on cannot be updated: capture again); a look that differs from U in a count,
 * an op, a root_material or a missing table.  LOL_GPU_ERR_NO_PROGRAM: no program uploaded.
 *
 * Resolving updated planes.  lol_gpu_relight checks a look against the UPLOADED program, and updated planes hold another one.
 * lol_gpu_relight_held and lol_gpu_relight_views_held are those resolves with that one check changed: `held` (HOST) says what the
 * planes hold; it must have U's geometry as a look of an update must, and `look` (NULL = the uploaded program) must equal `held`
 * in every light point and shininess as bits, and in everything else a look must equal U in.  held == NULL forwards to lol_gpu_relight
 * / lol_gpu_relight_views, which keep every status, text and order they have.
 *
 * Averaged pictures need no capture path of their own: record r of lol_gpu_light_views is lol_gpu_light_pixels of the s w x s h grid
 * under cams[r], r s^2 w h elements further on, so a host updates it with lol_gpu_light_update_pixels(ctx, look, &cams[r], s w, s h,
 * NULL, s^2 w h, ...) on planes offset by as many elements (light_stride that of the whole), and resolves with
 * lol_gpu_relight_views_held.
 *
 * Out of scope: a scene-module form of the update; *_views update calls; updates over per-record scenes; moving geometry;
 * lol_gpu_multi_* forms; planes in host memory; the renderer.h protocol; lights beyond the 64th.
 */
int  lol_gpu_light_update_rays(lol_gpu* ctx, const lol_program* look /* HOST, not NULL */, const float* rays_dev, size_t n,
                               uint64_t march_lights, uint64_t specular_lights, const lol_gpu_light_passes* planes, void* stream);
int  lol_gpu_light_update_pixels(lol_gpu* ctx, const lol_program* look /* HOST, not NULL */, const lol_frame_camera* cam, int w, int h,
                                 const uint32_t* xy_dev /* NULL: every pixel, n must be w*h */, size_t n,
                                 uint64_t march_lights, uint64_t specular_lights, const lol_gpu_light_passes* planes, void* stream);
int  lol_gpu_relight_held(lol_gpu* ctx, const lol_program* look /* HOST; NULL = the uploaded program */,
                          const lol_program* held /* HOST; what the planes hold; NULL = the uploaded program */,
                          const lol_gpu_light_passes* in, size_t n, const lol_gpu_relit* out, void* stream);
int  lol_gpu_relight_views_held(lol_gpu* ctx, const lol_program* look, const lol_program* held, const lol_gpu_light_passes* in,
                                int n_views, int cams_per_view, int w, int h, int samples, const lol_gpu_relit* out, void* stream);

/*
 * Scene light passes: light passes captured and relit under each record's own SCENE — an animation's capture in one call, and every
 * frame of it under a new look in one more, without an upload per frame.
 * Records and layout.  `scenes`, `looks` and `cams` are HOST memory and hold n_scenes entries, 1 <= n_scenes <= LOL_GPU_MAX_VIEWS; they
 * and the tables the programs point to are copied before the call returns.  Records, list_stride (0: one list of n elements serves
 * every record; otherwise list_stride >= n elements between the lists of two records) and the structure test are exactly those of
 * scene queries ("Scene queries", above).  Element (r, i) — ray i of record r — is element e = r * n + i of N = n_scenes * n.  The factor
 * planes are light-major over all N elements: light l of element e at factors[l * light_stride + e], light_stride 0 (= N) or >= N;
 * hit_id, hit_dist and march_steps are dense over e.  All addressing is 64-bit.  With xy_dev == NULL ray i of record r is pixel
 * (i % w, i / w) under cams[r], and n must be w * h: the leaf layout of relit views, whose record is r = v K + k and whose n is s^2 w h.
 * Capture.  Element (r, i) of lol_gpu_light_scene_rays / lol_gpu_light_scene_pixels is, bit for bit, EXACTLY what lol_gpu_light_rays /
 * lol_gpu_light_pixels writes for that ray on another context with this context's settings (lol_gpu_set_exact_skips, lol_gpu_set_cull)
 * that called lol_gpu_upload_program(&scenes[r]) and, for pixels, captures under cams[r]: all 16 bytes of every factor, hit_id,
 * hit_dist and march_steps.  So every element is the reference's arithmetic on record r's own numbers, for NaN, infinite, zero
 * and unnormalised rays too, whatever the other rays and the other records hold; a NaN centre in one record is that record's business
 * alone.  The escaped-wave skip and the zero-incidence skip are OFF for every record, as for every capture.  Decided per record, on the
 * host, from that record's own scene and camera, as for scene queries: the settled-shadow exit, whether the scene is finite, which of
 * the record's two macro-op lists runs, and the first march step.  No proof runs on the device.
 * One latitude, the one scene queries and light updates have: for a LIST OF RAYS with the settled-shadow exit on (bit 2 of
 * lol_gpu_set_exact_skips), shadow_steps is "the steps really marched", and is held equal to that other context's only after
 * lol_gpu_set_exact_skips(ctx, 0).  For pixel sources all 16 bytes are equal.
 * Relight.  looks[r] must be a look of scenes[r] in exactly lol_gpu_relight's sense, with scenes[r] in the place of the uploaded
 * program: equal counts, every ops[i].op, .id and .f[], every lights[l].point, every materials[m].shininess as bits, every
 * root_material[].  looks == NULL: the scenes' own look.  Element (r, i) of lol_gpu_relight_scenes is lol_gpu_relight's element on a
 * context that uploaded scenes[r], given looks[r] and record r's planes — rgb_linear, rgb and pixel, NaN and infinite looks included;
 * an id beyond n_roots is taken for 0; the context's gamma table and pixel format apply.  Over planes captured by the two calls above
 * it is therefore lol_gpu_shade_scene_rays / lol_gpu_shade_scene_pixels on `looks`, and over all pixels frame r of
 * lol_gpu_render_scene_views on `looks`.
 * Refused, with nothing launched and nothing written, in this order:
 *  1. what the single-scene call refuses, in its order — lol_gpu_light_rays / lol_gpu_light_pixels with n elements, lol_gpu_relight
 *     with a NULL look and n elements: no context, a NULL list of rays with n > 0, NULL out / in, max_steps < 0, n > 2^32 - 1, no
 *     program (LOL_GPU_ERR_NO_PROGRAM), the planes against n, NULL cam or bad frame geometry, xy_dev == NULL with n != w * h;
 *  2. LOL_GPU_ERR_ARG for NULL scenes, n_scenes < 1 or > LOL_GPU_MAX_VIEWS, NULL cams in the pixel form, a list_stride that is neither 0
 *     nor >= n, N > 2^32 - 1, a light_stride that is neither 0 nor >= N;
 *  3. the scene refusals of lol_gpu_render_scene_views: a missing table, another structure, a root_material out of range;
 *  4. for the relight, the first looks[r] that is not a look of scenes[r], with lol_gpu_relight's reason behind "record r" in
 *     lol_gpu_error's text.
 * n == 0 returns LOL_GPU_OK with nothing launched.  An allocation that fails returns LOL_GPU_ERR_HIP, and the context stays usable.
 * Consequence.  With scenes[r] the uploaded program for every r and `cams` the cameras of lol_gpu_light_views(n_views, K, w, h, s),
 * lol_gpu_light_scene_pixels(ctx, cams, scenes, n_views * K, s * w, s * h, max_steps, NULL, s^2 w h, 0, out, stream) writes byte for byte
 * the planes lol_gpu_light_views writes — n_views * K capture launches there, one here —, and lol_gpu_relight_views /
 * lol_gpu_relight_views_held resolve them unchanged.
 * Asynchronous on `stream` (NULL = the context's own stream; LOL_GPU_STREAM_DEFAULT as elsewhere).  A capture is one copy of the
 * records and their data through scene views' ring of 8 sets, under its rules, and ONE launch; a relight is one copy of the looks'
 * tables through lol_gpu_relight's ring of 8 sets, under its rules (HIP's special stream handles included), and ONE launch.  No scratch,
 * no host wait.  The context's scene, kernels, lol_gpu_kernel_key, tile-order state, sample settings and other rings are neither
 * read nor changed: a frame after the call is the frame it would have been.
 * Which kernel: the interpreter's light_interp_scenes and relight_rays_scenes, always.  No module switch has an effect on these calls.
 * Out of scope: an averaged resolve over records (K records per view, or s x s samples: capture here, resolve with
 * lol_gpu_relight_views where the scenes are equal); light updates over records; a structure-module or scene-module form;
 * lol_gpu_multi_* forms; planes or lists in host memory; and lol_gpu_light_views made of this call.
 * (An averaged resolve over records is built since: "Relit scene views", below.)
 */
int  lol_gpu_light_scene_rays(lol_gpu* ctx, const lol_program* scenes /* HOST */, int n_scenes, const float* rays_dev, size_t n,
                              size_t list_stride, int max_steps, const lol_gpu_light_passes* out, void* stream);
int  lol_gpu_light_scene_pixels(lol_gpu* ctx, const lol_frame_camera* cams /* HOST */, const lol_program* scenes, int n_scenes, int w, int h,
                                int max_steps, const uint32_t* xy_dev /* NULL: every pixel, n must be w*h */, size_t n, size_t list_stride,
                                const lol_gpu_light_passes* out, void* stream);
int  lol_gpu_relight_scenes(lol_gpu* ctx, const lol_program* scenes /* HOST: what the planes hold */,
                            const lol_program* looks /* HOST; NULL = the scenes themselves */, int n_scenes,
                            const lol_gpu_light_passes* in, size_t n, const lol_gpu_relit* out, void* stream);

/*
 * Relit scene views: the AVERAGED pictures of an animation under new looks without a march — s x s samples per pixel and K records
 * per view, every record under a scene and a look of its own.  What "Relit views" is to lol_gpu_relight, for planes that
 * lol_gpu_light_scene_pixels captured: lol_gpu_light_scene_pixels(ctx, cams, scenes, n_views * K, s * w, s * h, max_steps, NULL,
 * s^2 w h, 0, out, stream) writes the leaves of an antialiased or motion-blurred animation in one launch, and this call makes them
 * the frames of `looks`.
 * Layout.  K = cams_per_view in {1, 2, 4, 8, 16}, s = samples in {1, 2, 4}.  Record r = v K + k; `scenes` and `looks` are HOST memory
 * and hold n_views * K entries, copied before the call returns.  LEAF (v, k, Y, X) — sample column X < s w, sample row Y < s h of
 * record r — is element e = (r s h + Y) s w + X of N = n_views K s^2 w h: relit views' layout, and what the capture above writes.
 * The factor planes are light-major over all N elements (light l of element e at factors[l * light_stride + e]; light_stride 0 = N,
 * else >= N); hit_id is dense over e.  The outputs are dense over pixels, at index (v h + y) w + x; any subset, not none.
 * Contract.  Pixel (x, y) of view v, bracketed and rounded exactly so:
 *   1. per leaf, c = the rgb_linear of lol_gpu_relight_scenes for its element under looks[r] (an id beyond n_roots is taken for 0);
 *   2. per record k, m_k = the balanced binary32 tree over its s^2 leaves (s x + i, s y + j) in order j s + i, times 1 / s^2
 *      (s = 1: the leaf itself, unscaled);
 *   3. the balanced tree over m_0 ... m_{K-1} in order of k, times 1 / K (K = 1: m_0 itself);
 *   4. gamma and the context's pixel format, exactly as for one sample's colour.
 * Each record's scale first, then the tree over the records: the order lol_gpu_render_views_blend_samples fixes.
 * So, bit for bit: pixel and rgb are the `pixel` and `rgb` of lol_gpu_render_scene_views_samples(cams, looks, n_views, K, w, h,
 * max_steps, s), and with s = 1 those of lol_gpu_render_scene_views; with K = 1 and s = 1 the call is lol_gpu_relight_scenes with
 * n = w * h (it forwards to it, and that call's words are then the refusals' words); with every scene the uploaded program and every
 * look one look L it is lol_gpu_relight_views(L); rgb_linear is the mean before gamma, which the render calls do not expose; NaN and
 * infinite looks are included.
 * Looks.  looks[r] must be a look of scenes[r] in look_differs' sense — exactly as for lol_gpu_relight_scenes: equal counts, ops,
 * light points, shininess and root_material.  looks == NULL: the scenes' own look.  The K records of one view may carry K different
 * looks and K different scenes.
 * Refused, with nothing launched and nothing written, in this order:
 *  1. everything lol_gpu_relight_views refuses before it looks at its look: no context, NULL in / out, no output, n_views < 1 or bad
 *     frame geometry, K outside {1, 2, 4, 8, 16}, s outside {1, 2, 4}, N > 2^32 - 1, no program (LOL_GPU_ERR_NO_PROGRAM), the
 *     planes against N;
 *  2. LOL_GPU_ERR_ARG for NULL scenes or n_views * K > LOL_GPU_MAX_VIEWS;
 *  3. the scene refusals of lol_gpu_render_scene_views: a missing table, another structure, a root_material out of range;
 *  4. the first looks[r] that is no look of scenes[r], with "relight scene views: record r: " and lol_gpu_relight's reason behind it
 *     in lol_gpu_error's text.
 * Asynchronous on `stream` (NULL = the context's own stream; LOL_GPU_STREAM_DEFAULT as elsewhere).  One copy of the looks' tables
 * through lol_gpu_relight's ring of 8 sets, under its rules (HIP's special stream handles included), and ONE launch
 * (relight_views_scenes: the view in the grid's y, the look read per record).  No scratch, no host wait.  The context's scene,
 * kernels, lol_gpu_kernel_key, tile-order state, sample settings and other rings are neither read nor changed: a frame after the call
 * is the frame it would have been.  No module switch has an effect on this call.
 * Out of scope: light updates over records; an edge-adaptive relit form; a structure-module or scene-module form; lol_gpu_multi_*
 * forms; planes in host memory; pitch or stride addressing of the outputs; lol_gpu_light_views made of the scene capture; and lifting
 * the CLI's --tween-shutter refusal beside --relight (the blurred form is reached from Python: cameras_per_view = K).
 */
int  lol_gpu_relight_scene_views(lol_gpu* ctx, const lol_program* scenes /* HOST: what the planes hold; n_views * K entries */,
                                 const lol_program* looks /* HOST; NULL = the scenes themselves; n_views * K entries */,
                                 const lol_gpu_light_passes* in, int n_views, int cams_per_view, int w, int h, int samples,
                                 const lol_gpu_relit* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LOL_GPU_H */
