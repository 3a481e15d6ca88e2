/*
 * lol_kernel_scene_queries.h — ray and shading queries under each record's own scene (lol_gpu_trace_scene_rays,
 * lol_gpu_trace_scene_pixels, lol_gpu_shade_scene_rays, lol_gpu_shade_scene_pixels).
 *
 * The list queries (lol_kernel_rays.h, lol_kernel_shade.h) with what scene views (lol_kernel_scenes.h) add to a batch: blockIdx.y is
 * a RECORD — a scene of the uploaded program's structure and, for a list of pixels, a camera — and blockIdx.x runs over the n rays
 * that record answers.  A block reads its record with scalar loads through the constant address space, as scene_view() and
 * scene_launch() do: its macro-op list and how long it is, its tables, its ambient colour, its exact skips, its camera and first step,
 * and the two bits the host decides per record for a query (SCENE_VIEW_FINITE, SCENE_VIEW_SANE).  One block is one record, so all of
 * it is wave-uniform.  Record r's list begins list_stride elements behind record r - 1's (0: one list serves every record); its
 * answers are elements [r n, (r + 1) n) of every output.
 *
 * The per-ray bodies are trace_one and shade_ray, called.  The drivers are COPIES of trace_rays and shade_rays — the same ballots, the
 * same second pass after unproven(fast), the same from_pixels && settled rule — that differ in the index they store at and in the
 * helper that reads the outputs: ray_out(), shade_out() read the kernel-argument segment at the layouts RayQuery and ShadeArgs, so
 * a query patched in registers would be ignored by them, and a parameter for the base folded into the existing drivers is the kind of
 * fold that is not made ("Not folded").  The interpreter's kernels alone, ahead of time: no scene module
 * includes this header, and hipRTC is not handed its text.
 */
#pragma once
#include "lol_kernel_rays.h"
#include "lol_kernel_shade.h"
#include "lol_kernel_scenes.h"

namespace lol {

/* SceneView::flags, a query's alone: none of SCENE_VIEW_FLAGS, so scene_launch() masks them out and the frames never see them */
constexpr u32 SCENE_VIEW_FINITE = 1u << 30;   /* shadow_settle_ok(record's scene): RAYS_SCENE_SANE of that record (ray_query: the scene alone) */
constexpr u32 SCENE_VIEW_SANE   = 1u << 31;   /* ... and, for a list of pixels, camera_sane(record's camera): SHADE_SCENE_SANE of that record */
static_assert(((SCENE_VIEW_FINITE | SCENE_VIEW_SANE) & SCENE_VIEW_FLAGS) == 0u, "the query bits are no launch flags");

/* The kernels' last argument, by value: the records, their data (SceneTail's two) and how far apart the records' lists lie. */
struct SceneList { const SceneView* views; const u32* data; unsigned long long list_stride; };
/* the kernel-argument segments: the single-scene kernels' and the SceneList behind them */
struct SceneRayArgs { RayQuery Q; SceneList R; };
struct SceneShadeArgs { Launch L; ShadeQuery Q; SceneList R; };

__device__ __forceinline__ u32 record_of_block() { return blockIdx.y; }
/* this block's record, through the constant address space (view_launch_of says why) */
__device__ __forceinline__ scene_view_ptr scene_record(const SceneList& R) {
	return (scene_view_ptr)(unsigned long long)R.views + record_of_block();
}

/* The ray query as trace_one sees it: the launch's with this block's record patched in — its list, its scene-side bit, where its
 * rays or pixels begin and, for pixels, its camera and first step. */
__device__ __forceinline__ RayQuery scene_ray_query(const RayQuery& Q0, const SceneList& R) {
	const scene_view_ptr V = scene_record(R);
	RayQuery Q = Q0;
	const u32 vf = V->flags;
	Q.flags = (Q0.flags & ~(RAYS_SCENE_SANE | RAYS_FIRST_STEP)) | ((vf & SCENE_VIEW_FINITE) ? RAYS_SCENE_SANE : 0u);
	const unsigned long long first = R.list_stride * record_of_block();
	if (Q0.flags & RAYS_FROM_PIXELS) {
		for (int i = 0; i < 3; i++) { Q.cam.origin[i] = V->cam.origin[i]; Q.cam.dir[i] = V->cam.dir[i]; Q.cam.right[i] = V->cam.right[i]; Q.cam.up[i] = V->cam.up[i]; }
		Q.cam.width = V->cam.width; Q.cam.height = V->cam.height;
		if (vf & FLAG_FIRST_STEP) Q.flags |= RAYS_FIRST_STEP;
		Q.first_dist = V->first_dist;
		Q.first_id = V->first_id;
		Q.xy = Q0.xy + 2ull * first;
	} else {
		Q.rays = Q0.rays + 6ull * first;
	}
	Q.ops = R.data + V->ops_offset;
	Q.n_ops = V->n_mops;
	return Q;
}

/* The output pointers, read where they are needed (ray_out says why) at THIS kernel's layout, and moved to the record's first element */
__device__ __forceinline__ RayOut scene_ray_out(const RayQuery& Q0, unsigned long long base) {
	RayOut O;
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) SceneRayArgs* kernarg_ptr;
	kernarg_ptr A = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(A));                    /* opaque: these loads are not merged with the ones at kernel entry */
	O = { A->Q.out.dist, A->Q.out.id, A->Q.out.steps, A->Q.out.normal };
#else
	O = Q0.out;
#endif
	if (O.dist) O.dist += base;
	if (O.id) O.id += base;
	if (O.steps) O.steps += base;
	if (O.normal) O.normal += 3ull * base;
	return O;
}

/* trace_rays (lol_kernel_rays.h) for one record: `Q` is scene_ray_query's.  Lanes beyond n trace a copy of ray n - 1 OF THEIR OWN
 * RECORD and store nothing. */
template <class SdfFast, class SdfExact>
__device__ __forceinline__ void trace_scene_rays(SdfFast& fast, SdfExact& exact, bool have_fast, const RayQuery& Q) {
	const u32 i = blockIdx.x * 64u + threadIdx.x, j = i < Q.n ? i : Q.n - 1u;
	V3 ro, rd;
	if (Q.flags & RAYS_FROM_PIXELS) {
		const u32 x = Q.xy[2ull * j], y = Q.xy[2ull * j + 1ull];
		ro = v3(Q.cam.origin);
		rd = camera_ray(Q.cam, Q.fw, Q.fh, (int)x, (int)y);
	} else {
		const float* r = Q.rays + 6ull * j;
		ro = { r[0], r[1], r[2] };
		rd = { r[3], r[4], r[5] };
	}
	const bool first_given = (Q.flags & RAYS_FIRST_STEP) != 0u;
	const bool want_id = (Q.flags & RAYS_WANT_ID) != 0u, want_normal = (Q.flags & RAYS_WANT_NORMAL) != 0u;
	bool plain = true;
	RayHit h;
	if (have_fast && (Q.flags & RAYS_SCENE_SANE)) {
		const float lim = 1e15f;                   /* (NaN fails every comparison) */
		const u64 insane = vote(!(__builtin_fabsf(ro.x) < lim)) | vote(!(__builtin_fabsf(ro.y) < lim)) | vote(!(__builtin_fabsf(ro.z) < lim)) |
		                   vote(!(__builtin_fabsf(rd.x) < lim)) | vote(!(__builtin_fabsf(rd.y) < lim)) | vote(!(__builtin_fabsf(rd.z) < lim));
		if (insane == 0) {
			h = trace_one(fast, Q, ro, rd, first_given, want_id, want_normal);
			plain = unproven(fast);
		}
	}
	if (plain) h = trace_one(exact, Q, ro, rd, first_given, want_id, want_normal);
	const RayOut O = scene_ray_out(Q, (unsigned long long)record_of_block() * Q.n);
	if (i < Q.n) {
		if (O.dist) O.dist[i] = h.dist;
		if (O.id) O.id[i] = h.id;
		if (O.steps) O.steps[i] = h.steps;
		if (O.normal) { float* n = O.normal + 3ull * i; n[0] = h.n.x; n[1] = h.n.y; n[2] = h.n.z; }
	}
}

/* The interpreter's kernel, per stack class and root kind like trace_interp: one wave per block. */
template <int SSIZE, int KIND>
__global__ __launch_bounds__(64)
void trace_interp_scenes(const RayQuery Q0, const SceneList R) {
	const RayQuery Q = scene_ray_query(Q0, R);
	Interp<SSIZE, KIND> fast{ Q.ops, Q.n_ops, {}, 0u };
	Interp<SSIZE, 0> exact{ Q.ops, Q.n_ops, {}, 0u };
	trace_scene_rays(fast, exact, KIND != 0, Q);
}

/* The launch as shade_ray sees it: scene_launch() (lol_kernel_scenes.h) with the record in blockIdx.y.  The counts of lights,
 * materials and roots are the structure's: the launch's. */
__device__ __forceinline__ Launch scene_query_launch(const Launch& L, const SceneList& R) {
	const scene_view_ptr V = scene_record(R);
	Launch S = L;
	for (int i = 0; i < 3; i++) { S.cam.origin[i] = V->cam.origin[i]; S.cam.dir[i] = V->cam.dir[i]; S.cam.right[i] = V->cam.right[i]; S.cam.up[i] = V->cam.up[i]; }
	S.cam.width = V->cam.width; S.cam.height = V->cam.height;
	S.first_dist = V->first_dist;
	S.first_id = V->first_id;
	S.flags = (L.flags & ~SCENE_VIEW_FLAGS) | (V->flags & SCENE_VIEW_FLAGS);
	S.ops = R.data + V->ops_offset;
	S.n_ops = V->n_mops;
	S.lights = R.data + V->tables_offset;
	S.materials = S.lights + L.n_lights * LIGHT_DWORDS;
	S.root_material = S.materials + L.n_materials * MATERIAL_DWORDS;
	for (int i = 0; i < 3; i++) S.ambient[i] = V->ambient[i];
	return S;
}

/* ... and the query as fetch_ray sees it: the record's scene-side bit and where its rays or pixels begin */
__device__ __forceinline__ ShadeQuery scene_shade_query(const ShadeQuery& Q0, const SceneList& R) {
	ShadeQuery Q = Q0;
	Q.flags = (Q0.flags & ~SHADE_SCENE_SANE) | ((scene_record(R)->flags & SCENE_VIEW_SANE) ? SHADE_SCENE_SANE : 0u);
	const unsigned long long first = R.list_stride * record_of_block();
	if (Q0.flags & SHADE_FROM_PIXELS) Q.xy = Q0.xy + 2ull * first;
	else Q.rays = Q0.rays + 6ull * first;
	return Q;
}

/* The output pointers at THIS kernel's layout (shade_out says why they are read late), moved to the record's first element */
__device__ __forceinline__ ShadeOut scene_shade_out(const ShadeQuery& Q0, unsigned long long base) {
	ShadeOut O;
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) SceneShadeArgs* kernarg_ptr;
	kernarg_ptr A = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(A));                    /* opaque: these loads are not merged with the ones at kernel entry */
	O = { A->Q.out.rgb_linear, A->Q.out.rgb, A->Q.out.pixel, A->Q.out.hit_dist, A->Q.out.hit_id, A->Q.out.steps };
#else
	O = Q0.out;
#endif
	if (O.rgb_linear) O.rgb_linear += 3ull * base;
	if (O.rgb) O.rgb += 3ull * base;
	if (O.pixel) O.pixel += base;
	if (O.hit_dist) O.hit_dist += base;
	if (O.hit_id) O.hit_id += base;
	if (O.steps) O.steps += base;
	return O;
}

/* fetch_ray (lol_kernel_shade.h) with the eye as a VALUE, read before the branch.  There `L` is the kernel's argument; here it is a
 * patched copy, and with `ro = v3(L.cam.origin)` inside the branch hipcc merges the two origins' loads behind a select of their
 * ADDRESSES — a pointer into the copy, which then lives in scratch: 288 bytes per lane, 16 VGPRs more and two waves per SIMD fewer
 * in every shade_interp_scenes (profiles/r26_scene_queries_kernel_resources.json is the build with this function). */
__device__ __forceinline__ void fetch_record_ray(const Launch& L, const ShadeQuery& Q, V3 eye, u32 i, V3& ro, V3& rd) {
	u32 j = i < Q.n ? i : Q.n - 1u;
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("" : "+v"(j));
#endif
	if (Q.flags & SHADE_FROM_PIXELS) {
		const u32 x = Q.xy[2ull * j], y = Q.xy[2ull * j + 1ull];
		ro = eye;
		rd = camera_ray(L.cam, L.fw, L.fh, (int)x, (int)y);
	} else {
		const float* r = Q.rays + 6ull * j;
		ro = { r[0], r[1], r[2] };
		rd = { r[3], r[4], r[5] };
	}
}

/* shade_rays (lol_kernel_shade.h) for one record: `L` is scene_query_launch's, `Q` scene_shade_query's, the tables staged from `L`.
 * What a wave may assume is decided as there, with the record's bits in the place of the launch's.  Lanes beyond n shade a copy of
 * ray n - 1 OF THEIR OWN RECORD (fetch_record_ray, on the record's list) and store nothing. */
template <bool TABLES_GLOBAL, class SdfFast, class SdfExact>
__device__ __forceinline__ void shade_scene_rays(SdfFast& fast, SdfExact& exact, bool have_fast, const Launch& L, const ShadeQuery& Q, const u32* lds) {
	const u32 i = blockIdx.x * (u32)BLOCK + threadIdx.x;
	const bool from_pixels = (Q.flags & SHADE_FROM_PIXELS) != 0u;
	const V3 eye = v3(L.cam.origin);
	V3 ro, rd;
	fetch_record_ray(L, Q, eye, i, ro, rd);
	const bool first_given = (L.flags & FLAG_FIRST_STEP) != 0u;
	bool sane = true;
	if (!from_pixels) {
		const float lim = 1e15f;                   /* (NaN fails every comparison) */
		const u64 insane = vote(!(__builtin_fabsf(ro.x) < lim)) | vote(!(__builtin_fabsf(ro.y) < lim)) | vote(!(__builtin_fabsf(ro.z) < lim)) |
		                   vote(!(__builtin_fabsf(rd.x) < lim)) | vote(!(__builtin_fabsf(rd.y) < lim)) | vote(!(__builtin_fabsf(rd.z) < lim)) |
		                   vote(!(len2(rd) <= 0x1.00001p+0f));
		sane = insane == 0;
	}
	const bool settled = (L.flags & FLAG_SHADOW_SETTLED) != 0u && sane;
	bool plain = true;
	Pixel P;
	if (have_fast && (Q.flags & SHADE_SCENE_SANE) && sane && (!SdfFast::ASSUME_SETTLED || settled)) {
		P = shade_ray<SdfFast, TABLES_GLOBAL>(L, fast, lds, ro, rd, first_given, settled);
		plain = unproven(fast);
	}
	if (plain) {
		fetch_record_ray(L, Q, eye, i, ro, rd);
		P = shade_ray<SdfExact, TABLES_GLOBAL>(L, exact, lds, ro, rd, first_given, from_pixels && settled);
	}

	const ShadeOut O = scene_shade_out(Q, (unsigned long long)record_of_block() * Q.n);
	LaunchTail T = launch_tail(L);                 /* (the Launch is this kernel's first argument too) */
	T.dbg_rgb = O.rgb;
	V3 post = P.rgb;
	u32 px = 0u;
	if (O.rgb || O.pixel) px = pack_pixel(L, T, P.rgb, post);
	if (i < Q.n) {
		if (O.rgb_linear) { float* c = O.rgb_linear + 3ull * i; c[0] = P.rgb.x; c[1] = P.rgb.y; c[2] = P.rgb.z; }
		if (O.rgb) { float* c = O.rgb + 3ull * i; c[0] = post.x; c[1] = post.y; c[2] = post.z; }
		if (O.pixel) O.pixel[i] = px;
		if (O.hit_dist) O.hit_dist[i] = P.hit.dist;
		if (O.hit_id) O.hit_id[i] = P.hit.id;
		if (O.steps) O.steps[i] = P.reported_steps();
	}
}

/* The interpreter's kernel, per stack class, root kind and table placement like shade_interp.  It stages the block's own tables, not
 * the launch's. */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void shade_interp_scenes(const Launch L, const ShadeQuery Q0, const SceneList R) {
	extern __shared__ u32 lds[];
	const Launch S = scene_query_launch(L, R);
	const ShadeQuery Q = scene_shade_query(Q0, R);
	stage_tables<TABLES_GLOBAL>(S, lds);
	Interp<SSIZE, KIND> fast{ S.ops, S.n_ops, {}, 0u };
	Interp<SSIZE, 0> exact{ S.ops, S.n_ops, {}, 0u };
	shade_scene_rays<TABLES_GLOBAL>(fast, exact, KIND != 0, S, Q, lds);
}

}  // namespace lol
