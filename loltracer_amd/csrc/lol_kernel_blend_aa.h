/*
 * lol_kernel_blend_aa.h — supersampled blends (lol_gpu_render_views_blend_samples), pass 1: the LINEAR mean of every pixel's s x s
 * samples under every camera.
 *
 * The supersampled batch kernel (lol_kernel_batch_aa.h) with z = v K + k: block z reads record z — camera k of view v — with
 * scalar loads (view_launch), scales that launch to the sample grid (sample_launch), shade_pixel (lol_kernel.h, unchanged) shades
 * one sample per lane, and the xor butterfly of store_pixel_view_aa reduces the s x s lanes of a pixel and scales by 1 / s^2
 * (sample_mean, lol_kernel_aa.h).  Instead of packing that mean the pixel's owner lane stores it, still linear, into the
 * call's scratch at the dense index (z, y, x) of the PIXEL grid: one LinearColour of 16 bytes (lol_kernel_blend.h), one
 * global_store_dwordx4.  Pass 2 (lol_gpu.hip, blend_resolve, unchanged) sums each pixel's K means as the balanced tree of the
 * contract, scales by 1 / K, and only then applies gamma and packs: the rounding order of include/lol_gpu.h — per camera first,
 * then over the cameras.
 *
 * The scratch is the launch's `dst`; its diagnostic pointers are null and the batch's view stride is not read.  No step counters.
 */
#pragma once
#include "lol_kernel_batch_aa.h"
#include "lol_kernel_blend.h"

namespace lol {

/* The mean of each pixel's samples (sample_mean), stored LINEAR by the pixel's owner lane at (z, y, x) of the scratch, z = this
 * block's record.  `L`: the KERNEL's launch — w, h in pixels, whole frames; dst = the scratch; `rgb`: this lane's sample, the fast
 * SDF's exact fallback already done.  Every lane of the wave must call this, all of them active. */
__device__ __forceinline__ void store_linear_view_aa(const Launch& L, V3 rgb) {
	const V3 c = sample_mean(L, rgb);
	const LaunchTail T = launch_tail(L);
	const int s = samples_of(L.flags);
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
	stage_tables<TABLES_GLOBAL>(L, lds);
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
