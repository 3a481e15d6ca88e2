/*
 * lol_kernel_batch.h — a batch of views in one launch (lol_gpu_render_views): n frames of the same size and scene under n cameras.
 *
 * The grid is a plain frame's grid (rows, or columns with FLAG_TILE_COLS) with the view as its z coordinate: blocks are handed out
 * x first, z last, so the views go in order and view v + 1's first waves fill view v's tail.  A block belongs to ONE view: it reads
 * that view's record — camera, the primary march's first step, the view's flag bits, its copy of the macro-op list — with scalar
 * loads, patches them into a copy of the launch, and shade_pixel (lol_kernel.h, unchanged) runs on that copy: blockIdx.x / .y are
 * the tile of the view's frame, so every lane shades the pixel, and every wave the 16 x 4 patch, that a frame of that camera in a
 * fixed tile order gives it.  The camera stays in SGPRs.
 *
 * launch_tail() reads the destination, the pixel format and the diagnostic pointers from the kernel-argument segment at Launch's
 * offsets, so the kernels' first argument is a lol::Launch (that of a whole frame of the batch's size: n_rows = band_rows =
 * cycle_rows = h), and the view's destination is not patched into the copy: store_pixel_view packs with pack_pixel
 * and stores at the view's address itself.  With one-wave blocks (the default 16 x 4 patch) a wave's store is
 * four whole 64-byte row segments, as store_pixel's is after its trip through LDS.
 */
#pragma once
#include "lol_kernel.h"

namespace lol {

/* What the host decides per frame, decided per view (lol_gpu.hip, lol_gpu_render_views).  18 dwords. */
struct View {
	Cam   cam;
	float first_dist;            /* FLAG_FIRST_STEP in `flags`: sdf(cam.origin) ... */
	u32   first_id;              /* ... and its object */
	u32   flags;                 /* the view's own bits of Launch::flags: VIEW_FLAGS */
	u32   ops_offset;            /* dwords from Launch::ops to the copy of the macro-op list this view's camera allows */
};
constexpr u32 VIEW_FLAGS = FLAG_SHADOW_SETTLED | FLAG_FIRST_STEP;

/* The kernels' second argument.  view_stride_px: dwords from a view's first pixel to the next view's. */
struct BatchTail { const View* views; unsigned long long view_stride_px; };
struct BatchArgs { Launch L; BatchTail B; };      /* the kernel-argument segment of a batch kernel */

/* this block's view */
__device__ __forceinline__ u32 view_of_block() { return blockIdx.z; }

/* The launch as shade_pixel sees it: the frame of view v, which must be wave-uniform (a scalar).  The record is read through the
 * constant address space, so it arrives in SGPRs like the kernel arguments it replaces. */
__device__ __forceinline__ Launch view_launch_of(const Launch& L, const View* views, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) View* view_ptr;
	view_ptr V = (view_ptr)(unsigned long long)views + v;
#else
	const View* V = views + v;
#endif
	Launch S = L;
	for (int i = 0; i < 3; i++) { S.cam.origin[i] = V->cam.origin[i]; S.cam.dir[i] = V->cam.dir[i]; S.cam.right[i] = V->cam.right[i]; S.cam.up[i] = V->cam.up[i]; }
	S.cam.width = V->cam.width; S.cam.height = V->cam.height;
	S.first_dist = V->first_dist;
	S.first_id = V->first_id;
	S.flags = (L.flags & ~VIEW_FLAGS) | (V->flags & VIEW_FLAGS);
	S.ops = L.ops + V->ops_offset;
	return S;
}
/* ... of this block's view */
__device__ __forceinline__ Launch view_launch(const Launch& L, const View* views) { return view_launch_of(L, views, view_of_block()); }

/* The view stride is needed by the last few instructions alone: read there, from the kernel-argument segment (launch_tail says why). */
__device__ __forceinline__ unsigned long long view_stride_px(const BatchTail& B0) {
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) BatchArgs* kernarg_ptr;
	kernarg_ptr A = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(A));
	return A->B.view_stride_px;
#else
	return B0.view_stride_px;
#endif
}

/* Pack the lane's colour and write it, and the diagnostics asked for, at this block's view: row y of view v starts
 * v * view_stride_px + y * pitch_px dwords into the destination; diagnostics are dense, element (v, y, x) at (v h + y) w + x.
 * `L`: the KERNEL's launch (whole frames: n_rows == h). */
__device__ __forceinline__ void store_pixel_view(const Launch& L, const BatchTail& B, const Pixel& P) {
	const LaunchTail T = launch_tail(L);
	V3 post;
	const u32 px = pack_pixel(L, T, P.rgb, post);
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	int bx, by;
	tile_of_block(L, bx, by);
	const int gx = bx * TILE_W + wave * WAVE_W + (lane % WAVE_W), gr = by * TILE_H + lane / WAVE_W;
	if (gx < L.w && gr < L.n_rows) {
		const unsigned long long v = view_of_block();
		const unsigned long long o = (v * (unsigned long long)L.h + (unsigned long long)gr) * (unsigned long long)L.w + (unsigned long long)gx;
		if (T.dbg_rgb) { T.dbg_rgb[o * 3 + 0] = post.x; T.dbg_rgb[o * 3 + 1] = post.y; T.dbg_rgb[o * 3 + 2] = post.z; }
		if (T.dbg_hit_dist) T.dbg_hit_dist[o] = P.hit.dist;
		if (T.dbg_hit_id) T.dbg_hit_id[o] = P.hit.id;
		if (T.dbg_steps) T.dbg_steps[o] = P.reported_steps();
		T.dst[v * view_stride_px(B) + (unsigned long long)gr * T.pitch_px + (unsigned long long)gx] = px;
	}
}

/* The interpreter's batch kernel: one instantiation per render_interp<SSIZE, KIND, TABLES_GLOBAL>; counts steps like it.  Always a
 * fixed tile order (lol_gpu.hip). */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void render_interp_batch(const Launch L, const BatchTail B) {
	extern __shared__ u32 lds[];
	stage_tables<TABLES_GLOBAL>(L, lds);
	const Launch S = view_launch(L, B.views);
	Interp<SSIZE, KIND> sdf{ S.ops, S.n_ops, {}, 0u };
	Pixel P = shade_pixel<Interp<SSIZE, KIND>, TABLES_GLOBAL>(S, sdf, lds);
	if (KIND != 0 && unproven(sdf)) {
		Interp<SSIZE, 0> exact{ S.ops, S.n_ops, {}, 0u };
		P = shade_pixel<Interp<SSIZE, 0>, TABLES_GLOBAL>(S, exact, lds);
	}
	store_pixel_view(L, B, P);
}

}  // namespace lol
