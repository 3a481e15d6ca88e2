/*
 * lol_kernel_scenes_aa.h — supersampled scene views (lol_gpu_render_scene_views_samples): s x s samples per pixel, s in {2, 4}, under
 * every record's own scene.
 *
 * Two helpers joined, shade_pixel (lol_kernel.h) untouched between them: scene_launch (lol_kernel_scenes.h) patches the record's
 * camera, first step, flags, ambient colour, lists and tables into the kernel's launch, and sample_launch (lol_kernel_aa.h) scales
 * THAT launch to the sample grid.  The first step is the scene's sdf(cam.origin): it does not depend on the sample, so the record's
 * serves all of them.  The grid is the sample grid's tiles with the record in z (lol_kernel_batch_aa.h, lol_kernel_blend_aa.h);
 * one block is one record, so everything the record says is wave-uniform and arrives in SGPRs, as for one sample.
 *
 * The stores are the supersampled batches' own: store_pixel_view_aa packs the mean of a pixel's samples at the view's address (K = 1),
 * store_linear_view_aa stores it LINEAR at (z, y, x) of the blend's scratch (K > 1: blend_resolve, unchanged, then averages the K
 * means of a pixel — per record first, then over the records, the rounding order of include/lol_gpu.h).  Both read the destination,
 * the pixel format and the view stride from the kernel-argument segment at fixed offsets (launch_tail, view_stride_px), and a
 * SceneTail begins like a BatchTail, so they serve unchanged.  Both take the KERNEL's launch (w, h in pixels, the flags' sample
 * bits, which scene_launch keeps: they are none of SCENE_VIEW_FLAGS), and both need the whole wave: no lane leaves before them.
 *
 * The structure module's two kernels of this kind (lol_render_param_batch_aa, lol_render_param_batch_aa_lin) are generated text
 * (lol_codegen.hip, generate_structure_source) over the same helpers.
 */
#pragma once
#include "lol_kernel_scenes.h"
#include "lol_kernel_blend_aa.h"

namespace lol {

/* The interpreter's kernels: one instantiation each per render_interp_scene_batch<SSIZE, KIND, TABLES_GLOBAL>, s read at run time.
 * They stage the block's own tables, not the launch's.  No step counters; always a fixed tile order (lol_gpu.hip). */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void render_interp_scene_batch_aa(const Launch L, const SceneTail B) {
	extern __shared__ u32 lds[];
	const Launch R = scene_launch(L, B);
	stage_tables<TABLES_GLOBAL>(R, lds);
	const Launch S = sample_launch(R);
	Interp<SSIZE, KIND> sdf{ S.ops, S.n_ops, {}, 0u };
	Pixel P = shade_pixel<Interp<SSIZE, KIND>, TABLES_GLOBAL, false>(S, sdf, lds);
	if (KIND != 0 && unproven(sdf)) {
		Interp<SSIZE, 0> exact{ S.ops, S.n_ops, {}, 0u };
		P = shade_pixel<Interp<SSIZE, 0>, TABLES_GLOBAL, false>(S, exact, lds);
	}
	store_pixel_view_aa(L, batch_tail(B), P.rgb);
}

/* ... and pass 1 of a supersampled blend over records: the LINEAR mean of the pixel's samples into the blend's scratch */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void render_interp_scene_batch_aa_lin(const Launch L, const SceneTail B) {
	extern __shared__ u32 lds[];
	const Launch R = scene_launch(L, B);
	stage_tables<TABLES_GLOBAL>(R, lds);
	const Launch S = sample_launch(R);
	Interp<SSIZE, KIND> sdf{ S.ops, S.n_ops, {}, 0u };
	Pixel P = shade_pixel<Interp<SSIZE, KIND>, TABLES_GLOBAL, false>(S, sdf, lds);
	if (KIND != 0 && unproven(sdf)) {
		Interp<SSIZE, 0> exact{ S.ops, S.n_ops, {}, 0u };
		P = shade_pixel<Interp<SSIZE, 0>, TABLES_GLOBAL, false>(S, exact, lds);
	}
	store_linear_view_aa(L, P.rgb);
}

}  // namespace lol
