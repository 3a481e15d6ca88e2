/*
 * lol_kernel_blend_aa.h — supersampled blends (lol_gpu_render_views_blend_samples), pass 1: the LINEAR mean of every pixel's s x s
 * samples under every camera.
 *
 * The supersampled batch kernel (lol_kernel_batch_aa.h) with z = v K + k: block z reads record z — camera k of view v — with
 * scalar loads (view_launch), scales that launch to the sample grid (sample_launch), shade_pixel (lol_kernel.h, unchanged) shades
 * one sample per lane, and the xor butterfly of store_pixel_view_aa reduces the s x s lanes of a pixel and scales by 1 / s^2
 * (view_sample_mean).  Instead of packing that mean the pixel's owner lane stores it, still linear, into the
 * call's scratch at the dense index (z, y, x) of the PIXEL grid: one LinearColour of 16 bytes (lol_kernel_blend.h), one
 * global_store_dwordx4.  Pass 2 (lol_gpu.hip, blend_resolve, unchanged) sums each pixel's K means as the balanced tree of the
 * contract, scales by 1 / K, and only then applies gamma and packs: the rounding order of include/lol_gpu.h — per camera first,
 * then over the cameras.
 *
 * The scratch is the launch's `dst`; its diagnostic pointers are null and the batch's view stride is not read.  No step counters.
 * A file of its own, like the others and for the same reason: a scene module without this kernel keeps its bytes.
 */
#pragma once
#include "lol_kernel_batch_aa.h"
#include "lol_kernel_blend.h"

namespace lol {

/* The linear mean of the s x s samples of this lane's pixel: the tree over k = j s + i, lowest bit first — the bits of i (lane
 * column: xor 1, 2), then those of j (lane row: xor WAVE_W, 2 WAVE_W) — then 1 / s^2.  Every lane of the pixel ends with the same
 * bits.  Every lane of the wave must call this, all of them active.
 * A COPY of the first lines of store_pixel_view_aa (lol_kernel_batch_aa.h), same lane bits in the same order: a change to one must
 * be made to the other.  store_pixel_view_aa does not call this, for pack_pixel's reason (lol_kernel_aa.h): moving the lines into a
 * function it could share means changing lol_kernel_batch_aa.h's text, and hipRTC's compilation-unit id follows the header text —
 * every module of lol_gpu_set_view_samples would change its code object and its kernel_key (its instructions would not).
 * tests/test_gpu_view_blend_samples.py holds the two to each other bit for bit (K equal cameras ARE the supersampled view). */
__device__ __forceinline__ V3 view_sample_mean(const Launch& L, V3 rgb) {
	const int s = samples_of(L.flags);
	V3 c = aa_add_xor(rgb, 1);
	if (s == 4) c = aa_add_xor(c, 2);
	c = aa_add_xor(c, WAVE_W);
	if (s == 4) c = aa_add_xor(c, 2 * WAVE_W);
	return scale(c, s == 4 ? 1.f / 16.f : 1.f / 4.f);    /* 1 / s^2 */
}

/* The mean of each pixel's samples (view_sample_mean), stored LINEAR by the pixel's owner lane at (z, y, x) of the scratch, z = this
 * block's record.  `L`: the KERNEL's launch — w, h in pixels, whole frames; dst = the scratch; `rgb`: this lane's sample, the fast
 * SDF's exact fallback already done.  Every lane of the wave must call this, all of them active. */
__device__ __forceinline__ void store_linear_view_aa(const Launch& L, V3 rgb) {
	const int s = samples_of(L.flags);
	const V3 c = view_sample_mean(L, rgb);
	const LaunchTail T = launch_tail(L);
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	int bx, by;
	tile_of_block(L, bx, by);
	const int sx = bx * TILE_W + wave * WAVE_W + (lane % WAVE_W), sr = by * TILE_H + lane / WAVE_W;      /* this lane's sample */
	const int gx = sx / s, gr = sr / s;                                                                   /* ... and its pixel */
	if ((sx & (s - 1)) == 0 && (sr & (s - 1)) == 0 && gx < L.w && gr < L.h) {
		const unsigned long long z = view_of_block();
		const unsigned long long o = (z * (unsigned long long)L.h + (unsigned long long)gr) * (unsigned long long)L.w + (unsigned long long)gx;
		reinterpret_cast<LinearColour*>(T.dst)[o] = LinearColour{ c.x, c.y, c.z, 0.f };
	}
}

/* The interpreter's kernel: one instantiation per render_interp<SSIZE, KIND, TABLES_GLOBAL>, s read at run time.  Always a fixed
 * tile order (lol_gpu.hip). */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void render_interp_batch_aa_lin(const Launch L, const BatchTail B) {
	extern __shared__ u32 lds[];
	if constexpr (!TABLES_GLOBAL) {
		stage_common(L, lds);
		__syncthreads();
	}
	const Launch S = sample_launch(view_launch(L, B.views));
	Interp<SSIZE, KIND> sdf{ S.ops, S.n_ops, {}, 0u };
	Pixel P = shade_pixel<Interp<SSIZE, KIND>, TABLES_GLOBAL, false>(S, sdf, lds);
	if (KIND != 0 && unproven(sdf)) {
		Interp<SSIZE, 0> exact{ S.ops, S.n_ops, {}, 0u };
		P = shade_pixel<Interp<SSIZE, 0>, TABLES_GLOBAL, false>(S, exact, lds);
	}
	store_linear_view_aa(L, P.rgb);
}

}  // namespace lol
