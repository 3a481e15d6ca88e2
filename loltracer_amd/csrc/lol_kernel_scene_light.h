/*
 * lol_kernel_scene_light.h — light passes and relighting under each record's own scene (lol_gpu_light_scene_rays,
 * lol_gpu_light_scene_pixels, lol_gpu_relight_scenes).
 *
 * The capture and the resolve of lol_kernel_light.h with what scene queries (lol_kernel_scene_queries.h) add to a list query:
 * blockIdx.y is a RECORD — a scene of the uploaded program's structure and, for pixels, a camera — and blockIdx.x runs over the n
 * rays that record answers.  A block reads its record with scalar loads through the constant address space (scene_record), so all of
 * it is wave-uniform.  Element (r, i) is element e = r n + i of N = n_scenes n: the factor planes are light-major over all N elements,
 * hit_id, hit_dist and march_steps dense over e.  N <= 2^32 - 1 (the host refuses more), so e is a u32; every address is 64-bit.
 *
 * The per-ray body of the capture is light_ray, called.  It stores a factor at light_out(Q).factors[l * Q.stride + i], with the
 * pointer read from the kernel-argument segment at the layout LightArgs — which is the BEGINNING of this kernel's segment
 * (SceneLightArgs, asserted below) — so the driver hands it i = e and the launch's own factors pointer serves every record.  The
 * driver is a COPY of light_rays with shade_scene_rays' changes (the record's list, the output base, the tables staged from the
 * record, the eye read before the branch, the other three output pointers read late at this kernel's layout and indexed by e); a
 * parameter for the base folded into light_rays is the kind of fold that is not made ("Not folded").
 *
 * The resolve is relight_rays with the record in blockIdx.y: it stages look r's lights | materials | root_material, which travel
 * as a record of tables alone (LookRecord: no macro-op list, no camera — a resolve needs neither), and reads look r's ambient colour.
 *
 * The interpreter's kernels alone, ahead of time: no scene module includes this header, and hipRTC is not handed its text.
 */
#pragma once
#include <cstddef>
#include "lol_kernel_light.h"
#include "lol_kernel_scene_queries.h"

namespace lol {

/* the kernel-argument segment of light_interp_scenes: a capture's, and the SceneList behind it */
struct SceneLightArgs { Launch L; LightQuery Q; SceneList R; };
static_assert(offsetof(SceneLightArgs, Q) == offsetof(LightArgs, Q), "light_ray reads the factors pointer at LightArgs' layout");

/* The capture's query as fetch_record_light_ray sees it: the record's scene-side bit and where its rays or pixels begin */
__device__ __forceinline__ LightQuery scene_light_query(const LightQuery& Q0, const SceneList& R) {
	LightQuery Q = Q0;
	Q.flags = (Q0.flags & ~SHADE_SCENE_SANE) | ((scene_record(R)->flags & SCENE_VIEW_SANE) ? SHADE_SCENE_SANE : 0u);
	const unsigned long long first = R.list_stride * record_of_block();
	if (Q0.flags & SHADE_FROM_PIXELS) { if (!(Q0.flags & LIGHT_ALL_PIXELS)) Q.xy = Q0.xy + 2ull * first; }
	else Q.rays = Q0.rays + 6ull * first;
	return Q;
}

/* hit_id, hit_dist and march_steps at THIS kernel's layout (light_out says why they are read late), indexed by the element e of all
 * N; the factors are light_ray's own business */
__device__ __forceinline__ LightOut scene_light_out(const LightQuery& Q0) {
	LightOut O;
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) SceneLightArgs* kernarg_ptr;
	kernarg_ptr A = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(A));                    /* opaque: these loads are not merged with the ones at kernel entry */
	O = { nullptr, A->Q.out.hit_id, A->Q.out.hit_dist, A->Q.out.march_steps };
#else
	O = Q0.out;
#endif
	return O;
}

/* fetch_ray<true> (lol_kernel_shade.h) with the eye as a VALUE, read before the branch: fetch_record_ray (lol_kernel_scene_queries.h)
 * says what hipcc makes of a patched Launch otherwise.  With LIGHT_ALL_PIXELS ray j is pixel (j % w, j / w) of the record's frame. */
__device__ __forceinline__ void fetch_record_light_ray(const Launch& L, const LightQuery& Q, V3 eye, u32 i, V3& ro, V3& rd) {
	u32 j = i < Q.n ? i : Q.n - 1u;
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("" : "+v"(j));
#endif
	if (Q.flags & SHADE_FROM_PIXELS) {
		u32 x, y;
		if (Q.flags & LIGHT_ALL_PIXELS) { y = j / (u32)L.w; x = j - y * (u32)L.w; }
		else { x = Q.xy[2ull * j]; y = Q.xy[2ull * j + 1ull]; }
		ro = eye;
		rd = camera_ray(L.cam, L.fw, L.fh, (int)x, (int)y);
	} else {
		const float* r = Q.rays + 6ull * j;
		ro = { r[0], r[1], r[2] };
		rd = { r[3], r[4], r[5] };
	}
}

/* light_rays (lol_kernel_light.h) for one record: `L` is scene_query_launch's, `Q` scene_light_query's, the tables staged from `L`.
 * What a wave may assume is decided as there, with the record's bits in the place of the launch's.  Lanes beyond n capture a copy of
 * ray n - 1 OF THEIR OWN RECORD and store nothing. */
template <bool TABLES_GLOBAL, class SdfFast, class SdfExact>
__device__ __forceinline__ void light_scene_rays(SdfFast& fast, SdfExact& exact, bool have_fast, const Launch& L, const LightQuery& Q, const u32* lds) {
	const u32 i = blockIdx.x * (u32)BLOCK + threadIdx.x, first = record_of_block() * Q.n;
	const bool from_pixels = (Q.flags & SHADE_FROM_PIXELS) != 0u, store = i < Q.n;
	/* The lane's element, the ONE index that lives through the march (a lane that stores: below 2^32; any other: unused).  Opaque, so
	 * that i is not kept beside it for the rare second pass, which takes it from e again: a VGPR, and in three instantiations a wave
	 * per SIMD (profiles/r27_scene_light_kernel_resources.json). */
	u32 e = first + i;
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("" : "+v"(e));
#endif
	const V3 eye = v3(L.cam.origin);
	V3 ro, rd;
	fetch_record_light_ray(L, Q, eye, i, ro, rd);
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
	Hit hit;
	if (have_fast && (Q.flags & SHADE_SCENE_SANE) && sane && (!SdfFast::ASSUME_SETTLED || settled)) {
		hit = light_ray<SdfFast, TABLES_GLOBAL>(L, Q, fast, lds, ro, rd, first_given, settled, e, store);
		plain = unproven(fast);
	}
	if (plain) {
		fetch_record_light_ray(L, Q, eye, e - first, ro, rd);
		hit = light_ray<SdfExact, TABLES_GLOBAL>(L, Q, exact, lds, ro, rd, first_given, from_pixels && settled, e, store);
	}
	if (store) {
		const LightOut O = scene_light_out(Q);
		O.hit_id[e] = hit.id;
		if (O.hit_dist) O.hit_dist[e] = hit.dist;
		if (O.march_steps) O.march_steps[e] = hit.steps & 0xFFFFu;
	}
}

/* The interpreter's capture kernel over records, per stack class, root kind and table placement like light_interp.  It stages the
 * block's own tables, not the launch's. */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void light_interp_scenes(const Launch L, const LightQuery Q0, const SceneList R) {
	extern __shared__ u32 lds[];
	const Launch S = scene_query_launch(L, R);
	const LightQuery Q = scene_light_query(Q0, R);
	stage_tables<TABLES_GLOBAL>(S, lds);
	Interp<SSIZE, KIND> fast{ S.ops, S.n_ops, {}, 0u };
	Interp<SSIZE, 0> exact{ S.ops, S.n_ops, {}, 0u };
	light_scene_rays<TABLES_GLOBAL>(fast, exact, KIND != 0, S, Q, lds);
}

/* One look of a resolve over records: where its lights | materials | root_material lie in `data`, and its ambient colour */
struct LookRecord { u32 tables_offset; float ambient[3]; };
constexpr u32 LOOK_RECORD_DWORDS = 4;
static_assert(sizeof(LookRecord) == LOOK_RECORD_DWORDS * 4, "LookRecord layout");
/* relight_rays_scenes' last argument, by value */
struct LookList { const LookRecord* looks; const u32* data; };

/*
 * relight_rays (lol_kernel_light.h) with the record in blockIdx.y: element i of record r is element r n + i of the planes and of every
 * output, under look r.  `L`: counts, gamma table and pixel format the context's; tables and ambient colour are the record's.  `Q`:
 * the resolve's, n the elements of ONE record, stride the light stride of the whole.
 */
template <bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void relight_rays_scenes(const Launch L0, const RelightQuery Q, const LookList R) {
	extern __shared__ u32 lds[];
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) LookRecord* look_ptr;
#else
	typedef const LookRecord* look_ptr;
#endif
	const look_ptr K = (look_ptr)(unsigned long long)R.looks + record_of_block();
	/* the look's tables lie as stage_common lays them out, one behind the other: staged as one run, and no Launch is patched */
	const u32* tables = R.data + K->tables_offset;
	const V3 ambient = { K->ambient[0], K->ambient[1], K->ambient[2] };
	if constexpr (!TABLES_GLOBAL) {
		for (u32 t = threadIdx.x; t < table_dwords(L0.n_lights, L0.n_materials, L0.n_roots); t += BLOCK) lds[t] = tables[t];
		__syncthreads();
	}
	const u32* l_light = TABLES_GLOBAL ? tables : lds;
	const u32* l_mat   = l_light + L0.n_lights * LIGHT_DWORDS;
	const u32* l_rootm = l_mat + L0.n_materials * MATERIAL_DWORDS;
	const u32 i = blockIdx.x * (u32)BLOCK + threadIdx.x;
	if (i >= Q.n) return;
	const u64 e = (u64)record_of_block() * Q.n + i;

	u32 id = Q.hit_id[e];
	if (id > L0.n_roots) id = 0u;
	const u32 mid = id ? l_rootm[id - 1] : 0u;
	const float* m = reinterpret_cast<const float*>(l_mat + mid * MATERIAL_DWORDS);
	const V3 m_diff = { m[1], m[2], m[3] }, m_spec = { m[4], m[5], m[6] }, m_amb = { m[7], m[8], m[9] };

	V3 total = { 0.f, 0.f, 0.f };
	for (u32 li = 0; li < L0.n_lights; li++) {
		const u32* lp = l_light + li * LIGHT_DWORDS;
		const LightFactor f = Q.factors[(u64)li * Q.stride + e];
		V3 Id = mul(scale(lds_v3(lp + 3), f.shadow * f.di), m_diff);
		total = add(total, Id);
		V3 Is = mul(scale(lds_v3(lp + 6), f.shadow * f.si), m_spec);
		total = add(total, Is);
	}
	total = add(total, mul(ambient, m_amb));
	/* v3clamp: max(min(v, 1), 0) — NaN → 1 (vec.h:63-65) */
	const V3 c = { maxf_(minf_(total.x, 1.f), 0.f), maxf_(minf_(total.y, 1.f), 0.f), maxf_(minf_(total.z, 1.f), 0.f) };

	LaunchTail T = launch_tail(L0);                /* (the Launch is this kernel's first argument too) */
	T.dbg_rgb = Q.rgb;
	V3 post = c;
	u32 px = 0u;
	if (Q.rgb || Q.pixel) px = pack_pixel(L0, T, c, post);
	if (Q.rgb_linear) { float* o = Q.rgb_linear + 3ull * e; o[0] = c.x; o[1] = c.y; o[2] = c.z; }
	if (Q.rgb) { float* o = Q.rgb + 3ull * e; o[0] = post.x; o[1] = post.y; o[2] = post.z; }
	if (Q.pixel) Q.pixel[e] = px;
}

}  // namespace lol
