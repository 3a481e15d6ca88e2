/*
 * lol_kernel_aa.h — supersampled frames (lol_gpu_set_samples): s x s samples per pixel on an ordered grid, s in {2, 4}.
 *
 * The pixel's colour is the mean of the clamped LINEAR colours of its samples, in float32, summed as a balanced binary tree over
 * k = j s + i (s = 2: (v0 + v1) + (v2 + v3); s = 4: the same four levels deep) and multiplied by 1 / s^2; then gamma and packing
 * as for one sample (include/lol_gpu.h states the contract).  Sample (i, j) of pixel (x, y) is pixel (s x + i, s y + j) of the
 * reference's frame of s w x s h pixels: a ray the reference itself traces.
 *
 * One lane per SAMPLE.  The kernel's grid covers the s w x s n_rows sample grid, and shade_pixel (lol_kernel.h) runs unchanged on
 * a Launch that describes that grid (sample_launch): a wave shades the same 16 x 4 patch of samples that a plain frame of s w x
 * s h pixels gives it, so march and shadow coherence are those of such a frame.  The s x s lanes of one pixel are neighbours in
 * the patch: i in the low bits of the lane's column (lane bits 0, 1), j in the low bits of its row (lane bits 4, 5 with 16-wide
 * patches).  An xor butterfly over those bits, lowest k bit first, IS the tree of the contract, and every lane of the group ends
 * with the same bits (float addition is commutative): a dozen VALU instructions against thousands per sample.  Then the pixel's
 * owner lane (i = j = 0) stores it.
 */
#pragma once
#include "lol_kernel.h"

namespace lol {

/* Launch::flags of a supersampled frame (the *_aa kernels alone read them).  Launch::fw / fh are then (float)(s w) / (float)(s h),
 * the sample grid's size; w, h, n_rows and the row partition stay in pixels. */
constexpr u32 FLAG_SAMPLES_2 = 256u;
constexpr u32 FLAG_SAMPLES_4 = 512u;
__device__ __forceinline__ int samples_of(u32 flags) { return (flags & FLAG_SAMPLES_4) ? 4 : (flags & FLAG_SAMPLES_2) ? 2 : 1; }
/* s samples per axis need a wave patch whose sides are multiples of s (the s x s lanes of a pixel lie in one wave).  The default
 * 16 x 4 patch takes s = 4; an experimental shape such as 32 x 2 (LOL_WAVE_W / LOL_WAVE_H) still compiles every kernel, and the host
 * refuses the numbers of samples it cannot take (lol_gpu_set_samples: LOL_GPU_ERR_UNSUPPORTED). */
__host__ __device__ constexpr bool samples_fit_wave(int s) { return WAVE_W % s == 0 && WAVE_H % s == 0; }

/* The launch as shade_pixel sees it: the sample grid as a frame of s w x s h pixels.  Local row r' = s r + j of the sample grid is
 * then frame row s frame_row(r) + j: bands, cycles and offsets scale by s, and a band of s b sample rows is b pixel rows.  Lanes
 * beyond the frame clamp to its last sample: s w and s n_rows are multiples of s, so such a lane's whole group lies beyond the
 * frame too, and nothing of it is stored — every pixel that is stored has its full set of samples. */
__device__ __forceinline__ Launch sample_launch(const Launch& L) {
	const int s = samples_of(L.flags);
	Launch S = L;
	S.w = s * L.w; S.h = s * L.h; S.n_rows = s * L.n_rows;
	S.band_rows = s * L.band_rows; S.cycle_rows = s * L.cycle_rows; S.offset_rows = s * L.offset_rows;
	return S;
}

/* one level of the tree: this lane's partial sum + the one of the lane `m` apart (same bits on both: + is commutative) */
__device__ __forceinline__ V3 aa_add_xor(V3 v, int m) {
	return { v.x + __shfl_xor(v.x, m, 64), v.y + __shfl_xor(v.y, m, 64), v.z + __shfl_xor(v.z, m, 64) };
}

/* The linear mean of the s x s samples of this lane's pixel on the sample grid's tiles: the tree over k = j s + i, lowest bit first
 * — the bits of i (lane column: xor 1, 2), then those of j (lane row: xor WAVE_W, 2 WAVE_W) — then 1 / s^2.  Every lane of the
 * pixel ends with the same bits.  Every lane of the wave must call this, all of them active.
 * (launched only with an s that samples_fit_wave: the lanes xor-paired here are then the same pixel's samples) */
__device__ __forceinline__ V3 sample_mean(const Launch& L, V3 rgb) {
	const int s = samples_of(L.flags);
	V3 c = aa_add_xor(rgb, 1);
	if (s == 4) c = aa_add_xor(c, 2);
	c = aa_add_xor(c, WAVE_W);
	if (s == 4) c = aa_add_xor(c, 2 * WAVE_W);
	return scale(c, s == 4 ? 1.f / 16.f : 1.f / 4.f);    /* 1 / s^2 */
}

/* The mean of each pixel's samples, stored by the pixel's owner lane.  `rgb` = this lane's sample (shade_pixel on sample_launch(L)),
 * the fast SDF's exact fallback already done.  Every lane of the wave must call this, all of them active. */
template <bool TABLES_GLOBAL = false>
__device__ __forceinline__ void store_pixel_aa(const Launch& L, V3 rgb) {
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
	if ((sx & (s - 1)) == 0 && (sr & (s - 1)) == 0 && gx < L.w && gr < L.n_rows) {
		const unsigned long long o = (unsigned long long)gr * L.w + gx;
		if (T.dbg_rgb) { T.dbg_rgb[o * 3 + 0] = post.x; T.dbg_rgb[o * 3 + 1] = post.y; T.dbg_rgb[o * 3 + 2] = post.z; }
		T.dst[(unsigned long long)gr * T.pitch_px + gx] = px;
	}
}

/* The interpreter's supersampling kernel: one instantiation per render_interp<SSIZE, KIND, TABLES_GLOBAL>, s read at run time
 * (wave-uniform).  No step counters; always a fixed tile order (lol_gpu.hip). */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void render_interp_aa(const Launch L) {
	extern __shared__ u32 lds[];
	stage_tables<TABLES_GLOBAL>(L, lds);
	const Launch S = sample_launch(L);
	Interp<SSIZE, KIND> sdf{ L.ops, L.n_ops, {}, 0u };
	Pixel P = shade_pixel<Interp<SSIZE, KIND>, TABLES_GLOBAL, false>(S, sdf, lds);
	if (KIND != 0 && unproven(sdf)) {
		Interp<SSIZE, 0> exact{ L.ops, L.n_ops, {}, 0u };
		P = shade_pixel<Interp<SSIZE, 0>, TABLES_GLOBAL, false>(S, exact, lds);
	}
	store_pixel_aa<TABLES_GLOBAL>(L, P.rgb);
}

/*
 * Adaptive supersampling (lol_gpu_set_adaptive_samples): the s x s pixel of a LIST of pixels, the refine pass of an adaptive frame
 * (lol_gpu.hip, render_adaptive).  `list` holds *count entries x | y << 16, whole-frame pixels, written in tile order by
 * adaptive_classify.  A grid-stride loop over the list: group g of 64 / s^2 consecutive entries goes to wave g mod (waves in the
 * grid), so a grid sized to fill the device serves any length read from device memory.
 *
 * Lane = e s^2 + k, k = j s + i: entry e of the group, sample (i, j) of its pixel.  An xor butterfly over the bits of k, lowest
 * first, is the tree of the contract (store_pixel_aa's, over other lane bits).  shade_pixel (lol_kernel.h, unchanged) finds its
 * sample through its pixel-table path (FLAG_TILE_TABLE): the wave writes the 64 sample coordinates of the group into its own slot
 * of Launch::lane_pixels, slot Launch::tile_order[tile_slot(blockIdx.x, tile_stride)] (the host makes that blockIdx.x), and
 * shade_pixel reads them back in the same lanes.  The sample grid must therefore fit that table's fields: s w <= 65536, s h <=
 * 32768 (checked by the host).  Launch::band_rows / cycle_rows / offset_rows describe the whole frame.
 *
 * `shade(S)` = the lane's Pixel for sample launch S, the fast SDF's exact fallback included: every wave reshades before anything is
 * reduced.  One wave per block (the host refuses adaptive frames where BLOCK != 64).
 */
template <bool TABLES_GLOBAL, class Shade>
__device__ __forceinline__ void render_aa_list(const Launch& L, const u32* list, const u32* count, Shade&& shade) {
	const int s = samples_of(L.flags), ss = s * s;
	const u32 per_wave = 64u / (u32)ss;
	const u32 n = __builtin_amdgcn_readfirstlane(*count);
	Launch S = sample_launch(L);
	S.flags |= FLAG_TILE_TABLE;
	/* (the lane's entry and pixel are read again after shading rather than held across it: registers are what the march needs) */
	for (u32 g = blockIdx.x; g * per_wave < n; g += gridDim.x) {
		{
			const int lane = threadIdx.x & 63, k = lane & (ss - 1);
			const u32 e = g * per_wave + (u32)(lane / ss);
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
		const u32 e = g * per_wave + (u32)(lane / ss);
		if (k == 0 && e < n) {
			const u32 px = list[e];
			const int x = (int)(px & 0xFFFFu), y = (int)(px >> 16);
			const unsigned long long o = (unsigned long long)y * L.w + x;
			if (T.dbg_rgb) { T.dbg_rgb[o * 3 + 0] = post.x; T.dbg_rgb[o * 3 + 1] = post.y; T.dbg_rgb[o * 3 + 2] = post.z; }
			T.dst[(unsigned long long)y * T.pitch_px + x] = out;
		}
	}
}

/* The interpreter's refine pass: one instantiation per render_interp_aa */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void render_interp_aa_list(const Launch L, const u32* list, const u32* count) {
	extern __shared__ u32 lds[];
	stage_tables<TABLES_GLOBAL>(L, lds);
	render_aa_list<TABLES_GLOBAL>(L, list, count, [&](const Launch& S) {
		Interp<SSIZE, KIND> sdf{ L.ops, L.n_ops, {}, 0u };
		Pixel P = shade_pixel<Interp<SSIZE, KIND>, TABLES_GLOBAL, false>(S, sdf, lds);
		if (KIND != 0 && unproven(sdf)) {
			Interp<SSIZE, 0> exact{ L.ops, L.n_ops, {}, 0u };
			P = shade_pixel<Interp<SSIZE, 0>, TABLES_GLOBAL, false>(S, exact, lds);
		}
		return P;
	});
}

}  // namespace lol
