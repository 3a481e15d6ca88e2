/*
 * lol_kernel_blend.h — views averaged over K cameras (lol_gpu_render_views_blend), pass 1: the LINEAR colour of every ray.
 *
 * The batch kernel (lol_kernel_batch.h) with z = v K + k: block z reads record z — camera k of view v — with scalar loads
 * (view_launch), shade_pixel (lol_kernel.h, unchanged) shades the pixel of that camera's frame, and instead of packing it the lane
 * stores Pixel::rgb, the clamped colour BEFORE gamma, into the call's scratch at the dense index (z, y, x).  Pass 2 (lol_gpu.hip,
 * blend_resolve) sums each pixel's K colours as the balanced tree of the contract, scales, and only then applies gamma and packs.
 * The K cameras of a view are K times as many independent blocks: that is what fills the device for one or a few small views; no
 * partial sum lives across a march.
 *
 * The scratch is the launch's `dst` (launch_tail reads it at the end, like any destination); its diagnostic pointers are null and
 * the batch's view stride is not read.  Layout: one LinearColour of 16 bytes per ray — r, g, b and a dword of padding — so that a
 * lane's store is ONE global_store_dwordx4 and, with one-wave blocks (the 16 x 4 patch), a wave's store is four row segments of 256
 * contiguous bytes: whole 128-byte lines wherever the row starts on one (w a multiple of 8).  12 bytes interleaved would be a
 * dwordx3 per lane in segments of 192 bytes, every other one straddling a line it shares with the next tile; planar, three stores
 * per lane.  Chosen on those grounds; DESIGN.md 3.13 says what was measured of it.
 *
 * No step counters.
 */
#pragma once
#include "lol_kernel_batch.h"

namespace lol {

/* one ray's clamped linear colour in the scratch of a blend: 16 bytes, 16-byte aligned (the scratch is a hipMalloc) */
struct alignas(16) LinearColour { float r, g, b, pad; };

/* Store the lane's linear colour at (z, y, x) of the scratch, z = this block's record.  `L`: the KERNEL's launch (whole frames:
 * n_rows == h; dst = the scratch); `rgb`: the lane's colour, the fast SDF's exact fallback already done. */
__device__ __forceinline__ void store_linear_view(const Launch& L, V3 rgb) {
	const LaunchTail T = launch_tail(L);
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	int bx, by;
	tile_of_block(L, bx, by);
	const int gx = bx * TILE_W + wave * WAVE_W + (lane % WAVE_W), gr = by * TILE_H + lane / WAVE_W;
	if (gx < L.w && gr < L.n_rows) {
		const unsigned long long z = view_of_block();
		const unsigned long long o = (z * (unsigned long long)L.h + (unsigned long long)gr) * (unsigned long long)L.w + (unsigned long long)gx;
		reinterpret_cast<LinearColour*>(T.dst)[o] = LinearColour{ rgb.x, rgb.y, rgb.z, 0.f };
	}
}

/* The interpreter's kernel: one instantiation per render_interp<SSIZE, KIND, TABLES_GLOBAL>.  Always a fixed tile order (lol_gpu.hip). */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void render_interp_batch_lin(const Launch L, const BatchTail B) {
	extern __shared__ u32 lds[];
	stage_tables<TABLES_GLOBAL>(L, lds);
	const Launch S = view_launch(L, B.views);
	Interp<SSIZE, KIND> sdf{ S.ops, S.n_ops, {}, 0u };
	Pixel P = shade_pixel<Interp<SSIZE, KIND>, TABLES_GLOBAL, false>(S, sdf, lds);
	if (KIND != 0 && unproven(sdf)) {
		Interp<SSIZE, 0> exact{ S.ops, S.n_ops, {}, 0u };
		P = shade_pixel<Interp<SSIZE, 0>, TABLES_GLOBAL, false>(S, exact, lds);
	}
	store_linear_view(L, P.rgb);
}

}  // namespace lol
