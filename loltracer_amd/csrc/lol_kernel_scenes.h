/*
 * lol_kernel_scenes.h — a batch whose every view brings its own scene (lol_gpu_render_scene_views).
 *
 * The batch kernel (lol_kernel_batch.h) with one more thing per block: block z reads record z — a camera AND a scene of the uploaded
 * program's structure — with scalar loads.  What a batch's View says of the camera, a SceneView also says of the scene: the exact
 * skips that hold for that scene, its ambient colour, its macro-op lists and how long they are (the culling plan depends on the
 * numbers, so the lists of two records differ in length), its tables (lights | materials | root_material) and its numbers (the f[]
 * of every op).  Lists, tables and numbers of all records lie in one array of dwords behind the records (`SceneTail::data`); a record
 * holds offsets into it.  One block is one record, so everything read here is wave-uniform and arrives in SGPRs.
 *
 * Two ways to evaluate the record's SDF:
 *  - the interpreter (below): Interp<SSIZE, KIND> on the record's own lists, as render_interp_batch runs it on the launch's;
 *  - the structure module (lol_codegen.hip, generate_structure_source): the scene's SDF as straight-line code whose every literal
 *    is a read K[7 i + j] of op i's number j through the constant address space — specialised on the structure alone, so one code
 *    object serves every scene of that structure.  Objects in file order with the strict-'<' rule, no culling, no fast path.
 *
 * The kernels' first argument is a lol::Launch as for any batch (launch_tail() reads the destination and the pixel format from the
 * kernel-argument segment at its offsets); the second begins like a BatchTail, so store_pixel_view / store_linear_view and
 * view_stride_px() serve unchanged.
 */
#pragma once
#include "lol_kernel_blend.h"

namespace lol {

/* What the host decides per upload and per frame, decided per record (lol_gpu.hip, lol_gpu_render_scene_views).  24 dwords. */
struct SceneView {
	Cam   cam;
	float first_dist;            /* FLAG_FIRST_STEP in `flags`: this scene's sdf(cam.origin) ... */
	u32   first_id;              /* ... and its object */
	u32   flags;                 /* the record's own bits of Launch::flags: SCENE_VIEW_FLAGS */
	u32   ops_offset;            /* dwords from SceneTail::data to the macro-op list this record's scene and camera allow */
	u32   n_mops;                /* macro-ops in that list */
	u32   tables_offset;         /* ... to the record's lights | materials | root_material */
	u32   nums_offset;           /* ... to the record's numbers: 7 per op of the program, op i's f[j] at 7 i + j */
	float ambient[3];
};
constexpr u32 SCENE_VIEW_FLAGS = VIEW_FLAGS | FLAG_MISS_SKIP | FLAG_DARK_SKIP;
constexpr u32 SCENE_VIEW_DWORDS = 24;
constexpr u32 OP_NUMBERS = 7;        /* lol_op::f */

/* The kernels' second argument: a BatchTail (same offsets: view_stride_px() reads it there) and the records' data behind it. */
struct SceneTail { const SceneView* views; unsigned long long view_stride_px; const u32* data; };
static_assert(sizeof(SceneView) == SCENE_VIEW_DWORDS * 4, "SceneView layout");
static_assert(sizeof(BatchTail) == 16 && sizeof(SceneTail) == 24, "a SceneTail begins like a BatchTail");

#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) float* param_ptr;
typedef const __attribute__((address_space(4))) SceneView* scene_view_ptr;
#else
typedef const float* param_ptr;
typedef const SceneView* scene_view_ptr;
#endif

/* this block's record, through the constant address space (view_launch_of says why) */
__device__ __forceinline__ scene_view_ptr scene_view(const SceneTail& B) {
	return (scene_view_ptr)(unsigned long long)B.views + view_of_block();
}

/* The launch as shade_pixel sees it: the frame of this block's record — its camera, first step, flags, ambient colour, lists and
 * tables patched into a copy of the kernel's launch.  The counts of lights, materials and roots are the structure's: the launch's. */
__device__ __forceinline__ Launch scene_launch(const Launch& L, const SceneTail& B) {
	const scene_view_ptr V = scene_view(B);
	Launch S = L;
	for (int i = 0; i < 3; i++) { S.cam.origin[i] = V->cam.origin[i]; S.cam.dir[i] = V->cam.dir[i]; S.cam.right[i] = V->cam.right[i]; S.cam.up[i] = V->cam.up[i]; }
	S.cam.width = V->cam.width; S.cam.height = V->cam.height;
	S.first_dist = V->first_dist;
	S.first_id = V->first_id;
	S.flags = (L.flags & ~SCENE_VIEW_FLAGS) | (V->flags & SCENE_VIEW_FLAGS);
	S.ops = B.data + V->ops_offset;
	S.n_ops = V->n_mops;
	S.lights = B.data + V->tables_offset;
	S.materials = S.lights + L.n_lights * LIGHT_DWORDS;
	S.root_material = S.materials + L.n_materials * MATERIAL_DWORDS;
	for (int i = 0; i < 3; i++) S.ambient[i] = V->ambient[i];
	return S;
}

/* the numbers of this block's record, for the structure module's SDF */
__device__ __forceinline__ param_ptr scene_numbers(const SceneTail& B) {
	return (param_ptr)(unsigned long long)B.data + scene_view(B)->nums_offset;
}

/* (store_pixel_view takes a BatchTail it reads on the host alone: the device reads the stride from the kernel-argument segment) */
__device__ __forceinline__ const BatchTail& batch_tail(const SceneTail& B) { return reinterpret_cast<const BatchTail&>(B); }

/* The interpreter's kernels: one instantiation each per render_interp_batch<SSIZE, KIND, TABLES_GLOBAL>.  They stage the block's own
 * tables, not the launch's.  Always a fixed tile order (lol_gpu.hip). */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void render_interp_scene_batch(const Launch L, const SceneTail B) {
	extern __shared__ u32 lds[];
	const Launch S = scene_launch(L, B);
	stage_tables<TABLES_GLOBAL>(S, lds);
	Interp<SSIZE, KIND> sdf{ S.ops, S.n_ops, {}, 0u };
	Pixel P = shade_pixel<Interp<SSIZE, KIND>, TABLES_GLOBAL>(S, sdf, lds);
	if (KIND != 0 && unproven(sdf)) {
		Interp<SSIZE, 0> exact{ S.ops, S.n_ops, {}, 0u };
		P = shade_pixel<Interp<SSIZE, 0>, TABLES_GLOBAL>(S, exact, lds);
	}
	store_pixel_view(L, batch_tail(B), P);
}

/* ... and pass 1 of a blend over records: the clamped LINEAR colour into the blend's scratch (lol_kernel_blend.h).  No step counters. */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void render_interp_scene_batch_lin(const Launch L, const SceneTail B) {
	extern __shared__ u32 lds[];
	const Launch S = scene_launch(L, B);
	stage_tables<TABLES_GLOBAL>(S, lds);
	Interp<SSIZE, KIND> sdf{ S.ops, S.n_ops, {}, 0u };
	Pixel P = shade_pixel<Interp<SSIZE, KIND>, TABLES_GLOBAL, false>(S, sdf, lds);
	if (KIND != 0 && unproven(sdf)) {
		Interp<SSIZE, 0> exact{ S.ops, S.n_ops, {}, 0u };
		P = shade_pixel<Interp<SSIZE, 0>, TABLES_GLOBAL, false>(S, exact, lds);
	}
	store_linear_view(L, P.rgb);
}

}  // namespace lol
