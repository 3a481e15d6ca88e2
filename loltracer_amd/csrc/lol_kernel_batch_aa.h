/*
 * lol_kernel_batch_aa.h — supersampled batches of views (lol_gpu_render_views_samples): n frames of the same size and scene under
 * n cameras with s x s samples per pixel, s in {2, 4}, on every pixel or on the pixels an adaptive batch refines.
 *
 * Every pixel: the grid is the SAMPLE grid's tiles (lol_kernel_aa.h) with the view as its z coordinate (lol_kernel_batch.h).  A
 * block reads its view's record with scalar loads (view_launch), scales that launch to the sample grid (sample_launch), and
 * shade_pixel (lol_kernel.h, unchanged) shades one sample per lane; the xor butterfly of store_pixel_aa reduces the s x s lanes of
 * a pixel, and the pixel's owner lane packs and stores at the view's address (store_pixel_view's addressing).
 *
 * Refined pixels (the third pass of an adaptive batch; lol_gpu.hip, render_views_adaptive): every view has a list segment of
 * its own — w h entries, counts[v] of them filled by the classify pass — and `prefix` (view_group_prefix) numbers the groups of
 * 64 / s^2 entries of all views in order of v: view v's are prefix[v] ... prefix[v + 1] - 1.  A grid-stride loop over that group
 * number: a wave looks the view of its group up (binary search, scalar loads), so a wave's entries all belong to ONE view and the
 * camera, the first step, the flags and the macro-op list stay wave-uniform; then it does what render_aa_list does for a frame,
 * through its own slot of Launch::lane_pixels.  The grid fills the device whatever the batch; list lengths stay on the device.
 */
#pragma once
#include "lol_kernel_aa.h"
#include "lol_kernel_batch.h"

namespace lol {

/* The mean of each pixel's samples (sample_mean), stored by the pixel's owner lane at this block's view (store_pixel_view's
 * addressing).  `L`: the KERNEL's launch — w, h in pixels, whole frames; `rgb`: this lane's sample, the fast SDF's exact fallback
 * already done.  Every lane of the wave must call this, all of them active. */
__device__ __forceinline__ void store_pixel_view_aa(const Launch& L, const BatchTail& B, V3 rgb) {
	const V3 c = sample_mean(L, rgb);
	const LaunchTail T = launch_tail(L);
	V3 post;
	const u32 px = pack_pixel(L, T, c, post);
	const int s = samples_of(L.flags);
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	int bx, by;
	tile_of_block(L, bx, by);
	const int sx = bx * TILE_W + wave * WAVE_W + (lane % WAVE_W), sr = by * TILE_H + lane / WAVE_W;      /* this lane's sample */
	const int gx = sx / s, gr = sr / s;                                                                   /* ... and its pixel */
	if ((sx & (s - 1)) == 0 && (sr & (s - 1)) == 0 && gx < L.w && gr < L.h) {
		const unsigned long long v = view_of_block();
		const unsigned long long o = (v * (unsigned long long)L.h + (unsigned long long)gr) * (unsigned long long)L.w + (unsigned long long)gx;
		if (T.dbg_rgb) { T.dbg_rgb[o * 3 + 0] = post.x; T.dbg_rgb[o * 3 + 1] = post.y; T.dbg_rgb[o * 3 + 2] = post.z; }
		T.dst[v * view_stride_px(B) + (unsigned long long)gr * T.pitch_px + (unsigned long long)gx] = px;
	}
}

/* The interpreter's kernel for batches with s x s samples on every pixel: one instantiation per render_interp<SSIZE, KIND,
 * TABLES_GLOBAL>, s read at run time.  No step counters; always a fixed tile order (lol_gpu.hip). */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void render_interp_batch_aa(const Launch L, const BatchTail B) {
	extern __shared__ u32 lds[];
	stage_tables<TABLES_GLOBAL>(L, lds);
	const Launch S = sample_launch(view_launch(L, B.views));
	Interp<SSIZE, KIND> sdf{ S.ops, S.n_ops, {}, 0u };
	Pixel P = shade_pixel<Interp<SSIZE, KIND>, TABLES_GLOBAL, false>(S, sdf, lds);
	if (KIND != 0 && unproven(sdf)) {
		Interp<SSIZE, 0> exact{ S.ops, S.n_ops, {}, 0u };
		P = shade_pixel<Interp<SSIZE, 0>, TABLES_GLOBAL, false>(S, exact, lds);
	}
	store_pixel_view_aa(L, B, P.rgb);
}

/* The refine kernels' third argument.  list: n_views segments of w h entries x | y << 16 (pixels of that view); counts[v]: how
 * many of view v's are filled; prefix[v]: the groups of 64 / s^2 entries before view v's, prefix[n_views]: all of them. */
struct BatchLists { const u32* list; const u32* counts; const u32* prefix; u32 n_views; };

/* The s x s pixels of the lists (the file's head says how).  `L`: the KERNEL's launch, with the lane table of render_aa_list
 * (tile_order, tile_stride, lane_pixels: a slot per block); `shade(S)` = the lane's Pixel for sample launch S of the wave's view,
 * the fast SDF's exact fallback included.  One wave per block (the host refuses adaptive batches where BLOCK != 64). */
template <bool TABLES_GLOBAL, class Shade>
__device__ __forceinline__ void render_aa_view_lists(const Launch& L, const BatchTail& B, const BatchLists& Q, Shade&& shade) {
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) u32* table_ptr;      /* wave-uniform indices: scalar loads */
#else
	typedef const u32* table_ptr;
#endif
	const table_ptr prefix = (table_ptr)(unsigned long long)Q.prefix, counts = (table_ptr)(unsigned long long)Q.counts;
	const int s = samples_of(L.flags), ss = s * s;
	const u32 per_wave = 64u / (u32)ss;
	const u32 total = prefix[Q.n_views];
	const unsigned long long segment = (unsigned long long)L.w * (unsigned long long)L.h;
	for (u32 g = blockIdx.x; g < total; g += gridDim.x) {
		/* the view of group g: the last v with prefix[v] <= g (views without a refined pixel have no group and are never found) */
		u32 v = 0, end = Q.n_views;                                   /* prefix[v] <= g < prefix[end] */
		while (end - v > 1u) {
			const u32 mid = (v + end) >> 1;
			if (prefix[mid] <= g) v = mid; else end = mid;
		}
		v = __builtin_amdgcn_readfirstlane(v);
		const u32 n = counts[v], first = (g - prefix[v]) * per_wave;      /* the view's entries; this group's first */
		const u32* list = Q.list + (unsigned long long)v * segment;
		Launch S = sample_launch(view_launch_of(L, B.views, v));
		S.flags |= FLAG_TILE_TABLE;
		/* (the lane's entry and pixel are read again after shading rather than held across it, as in render_aa_list) */
		{
			const int lane = threadIdx.x & 63, k = lane & (ss - 1);
			const u32 e = first + (u32)(lane / ss);
			const u32 px = list[e < n ? e : n - 1u];                 /* (lanes past the end shade the last entry again, store nothing) */
			const u32 slot = L.tile_order[tile_slot(blockIdx.x, L.tile_stride)];
			const_cast<u32*>(L.lane_pixels)[(unsigned long long)slot * 64u + (u32)lane] =
				(u32)(s * (int)(px & 0xFFFFu) + (k & (s - 1))) | (u32)(s * (int)(px >> 16) + k / s) << 16;
		}
		const Pixel P = shade(S);
		V3 c = P.rgb;
		for (int m = 1; m < ss; m <<= 1) c = aa_add_xor(c, m);
		c = scale(c, s == 4 ? 1.f / 16.f : 1.f / 4.f);             /* 1 / s^2 */
		const LaunchTail T = launch_tail(L);
		V3 post;
		const u32 out = pack_pixel(L, T, c, post);
		const int lane = threadIdx.x & 63, k = lane & (ss - 1);
		const u32 e = first + (u32)(lane / ss);
		if (k == 0 && e < n) {
			const u32 px = list[e];
			const unsigned long long x = px & 0xFFFFu, y = px >> 16;
			const unsigned long long o = ((unsigned long long)v * (unsigned long long)L.h + y) * (unsigned long long)L.w + x;
			if (T.dbg_rgb) { T.dbg_rgb[o * 3 + 0] = post.x; T.dbg_rgb[o * 3 + 1] = post.y; T.dbg_rgb[o * 3 + 2] = post.z; }
			T.dst[(unsigned long long)v * view_stride_px(B) + y * T.pitch_px + x] = out;
		}
	}
}

/* The interpreter's refine pass for batches: one instantiation per render_interp_batch_aa */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void render_interp_batch_aa_list(const Launch L, const BatchTail B, const BatchLists Q) {
	extern __shared__ u32 lds[];
	stage_tables<TABLES_GLOBAL>(L, lds);
	render_aa_view_lists<TABLES_GLOBAL>(L, B, Q, [&](const Launch& S) {
		Interp<SSIZE, KIND> sdf{ S.ops, S.n_ops, {}, 0u };
		Pixel P = shade_pixel<Interp<SSIZE, KIND>, TABLES_GLOBAL, false>(S, sdf, lds);
		if (KIND != 0 && unproven(sdf)) {
			Interp<SSIZE, 0> exact{ S.ops, S.n_ops, {}, 0u };
			P = shade_pixel<Interp<SSIZE, 0>, TABLES_GLOBAL, false>(S, exact, lds);
		}
		return P;
	});
}

}  // namespace lol
