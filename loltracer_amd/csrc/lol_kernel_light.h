/*
 * lol_kernel_light.h — light passes and relighting (lol_gpu_light_rays, lol_gpu_light_pixels, lol_gpu_relight): what get_light
 * (naive_renderer.c:129-175) needs of a ray once per LIGHT, captured, and the pixel made from it again under another look.
 *
 * get_light is linear in the look — the lights' intensities, the materials' colours, the ambient colour — once three scalars per
 * light are known: the shadow factor (:136), the diffuse incidence (:148) and the specular incidence (:158-161).  The march, the
 * normal and the shadow marches fix them; light_interp captures them, one lane per RAY, and relight_rays computes
 *   total = sum over the lights, in file order, of (Id * (shadow * di)) * m.diffuse, then (Is * (shadow * si)) * m.specular
 *   total += ambient * m.ambient;  v3clamp;  v3pow(., 1 / 2.2);  colorf_to_pixfmt
 * with the bracketing of :150-172 — the expressions shade_ray writes, on the same binary32 values, so the pixel is the reference's
 * for the scene with that look, bit for bit.
 *
 * light_ray restates shade_ray's body up to the factors (the fold onto one body would move instructions of existing kernels: DESIGN.md
 * 3.16, "Not folded").  It differs in that NO skip applies — FLAG_MISS_SKIP and FLAG_DARK_SKIP rest on the uploaded look (material #0
 * dark, intensities finite), and a look may differ in exactly that; the host clears both — and in ending each light's turn with one
 * 16-byte store instead of two additions.  FLAG_SHADOW_SETTLED stays: it changes no factor (soft_shadow).
 *
 * The planes are light-major — light l of ray i at factors[l * stride + i] — so that the 64 lanes of a wave store, and relight_rays'
 * load, 1 KiB of consecutive bytes per light.
 *
 * Interpreter only: there is no scene-module form of the capture (include/lol_gpu.h, "Out of scope").
 */
#pragma once
#include "lol_kernel_shade.h"

namespace lol {

/* LightQuery::flags: SHADE_FROM_PIXELS, SHADE_SCENE_SANE and LIGHT_ALL_PIXELS of lol_kernel_shade.h */

struct alignas(16) LightFactor { float shadow, di, si; u32 shadow_steps; };      /* = lol_gpu_light_factor */
struct LightOut { LightFactor* factors; u32* hit_id; float* hit_dist; u32* march_steps; };

/* The capture kernels' second argument, by value, behind a Launch filled as a shading query's (lol_kernel_shade.h) */
struct LightQuery {
	const float* rays;           /* n x 6 floats, or unused */
	const u32*   xy;             /* SHADE_FROM_PIXELS without LIGHT_ALL_PIXELS: n x {x, y} */
	u32    n;
	u32    flags;
	u64    stride;               /* elements between the planes of two lights, >= n */
	LightOut out;                /* read late: light_out() */
};
struct LightArgs { Launch L; LightQuery Q; };      /* the kernel-argument segment of a capture kernel */

/* The output pointers, read where they are needed from the kernel-argument segment, as shade_out() does */
__device__ __forceinline__ LightOut light_out(const LightQuery& Q0) {
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) LightArgs* kernarg_ptr;
	kernarg_ptr A = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(A));                    /* opaque: these loads are not merged with the ones at kernel entry */
	return { A->Q.out.factors, A->Q.out.hit_id, A->Q.out.hit_dist, A->Q.out.march_steps };
#else
	return Q0.out;
#endif
}

/*
 * The per-ray body: shade_ray's, for the ray (ro, rd), up to the three scalars of every light.  `i` = the ray's element, `store` =
 * this lane owns one (a lane beyond n shades a copy of ray n - 1 and stores nothing).  The caller has cleared FLAG_MISS_SKIP and
 * FLAG_DARK_SKIP: every lane takes the normal's taps and marches towards every light, escaped rays included (p = ro + rd * inf for
 * them, as in the reference), and si is computed for every light.
 */
template <class Sdf, bool TABLES_GLOBAL>
__device__ __forceinline__ Hit light_ray(const Launch& L, const LightQuery& Q, Sdf& sdf, const u32* lds, V3 ro, V3 rd, bool first_given,
                                         bool settled, u32 i, bool store) {
	const u32* l_light = TABLES_GLOBAL ? L.lights : lds;
	const u32* l_mat   = TABLES_GLOBAL ? L.materials : l_light + L.n_lights * LIGHT_DWORDS;
	const u32* l_rootm = TABLES_GLOBAL ? L.root_material : l_mat + L.n_materials * MATERIAL_DWORDS;

	const Marched marched = march<true>(sdf, ro, rd, L.max_steps, first_given, L.first_dist, L.first_id);

	const V3 p = add(ro, scale(rd, marched.dist));
	bool lit;
	Hit hit = { marched.dist, 0u, marched.steps };
	const V3 n = normal_and_id(sdf, ro, rd, marched, p, false, hit.id, lit);

	/* get_material, naive_renderer.c:103-112: the shininess alone — the colours are the look's */
	const u32 mid = hit.id ? l_rootm[hit.id - 1] : 0u;
	const float shininess = reinterpret_cast<const float*>(l_mat + mid * MATERIAL_DWORDS)[0];

	const V3 camera_dir = normalize(sub(ro, p));
	for (u32 li = 0; li < L.n_lights; li++) {
		const u32* lp = l_light + li * LIGHT_DWORDS;
		V3 to_light = sub(lds_v3(lp), p);
		float light_dist = len(to_light);
		V3 light_dir = scale(to_light, 1.0f / light_dist);      /* == v3normalize(light - p) */
		const float di = clampf_(dot(n, light_dir), 0.f, 1.f);
		u32 steps = 0, skipped = 0;                             /* (turns run, turns a stationary ray left out: reported together) */
		const float shadow = soft_shadow<true>(sdf, p, light_dir, light_dist, steps, skipped, true, settled);
		V3 refl = sub(scale(n, 2.f * dot(light_dir, n)), light_dir);
		const float si = di * powf_glibc(clampf_(dot(refl, camera_dir), 0.f, 1.f), shininess);
		if (store) {
			const LightFactor f = { shadow, di, si, steps + skipped };
			light_out(Q).factors[(u64)li * Q.stride + i] = f;
		}
	}
	return hit;
}

/* The whole capture kernel, after the tables are staged: shade_rays with light_ray in the place of shade_ray — the same ballot
 * decides what a wave of a list may assume about its rays, the same second pass follows a fast SDF that left what was proven for it
 * (it stores every factor again: same lanes, same addresses, in order).  A copy of shade_rays' driver and of its ballot, not a call:
 * either fold moved all 16 light_interp (lol_kernel_shade.h, shade_rays, "Not folded"). */
template <bool TABLES_GLOBAL, class SdfFast, class SdfExact>
__device__ __forceinline__ void light_rays(SdfFast& fast, SdfExact& exact, bool have_fast, const Launch& L, const LightQuery& Q, const u32* lds) {
	const u32 i = blockIdx.x * (u32)BLOCK + threadIdx.x;
	const bool from_pixels = (Q.flags & SHADE_FROM_PIXELS) != 0u, store = i < Q.n;
	V3 ro, rd;
	fetch_ray<true>(L, Q, i, ro, rd);
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
		hit = light_ray<SdfFast, TABLES_GLOBAL>(L, Q, fast, lds, ro, rd, first_given, settled, i, store);
		plain = unproven(fast);
	}
	if (plain) {
		fetch_ray<true>(L, Q, i, ro, rd);
		hit = light_ray<SdfExact, TABLES_GLOBAL>(L, Q, exact, lds, ro, rd, first_given, from_pixels && settled, i, store);
	}
	if (store) {
		const LightOut O = light_out(Q);
		O.hit_id[i] = hit.id;
		if (O.hit_dist) O.hit_dist[i] = hit.dist;
		if (O.march_steps) O.march_steps[i] = hit.steps & 0xFFFFu;
	}
}

/* The interpreter's capture kernel (ahead of time), per stack class, root kind and table placement like shade_interp. */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void light_interp(const Launch L, const LightQuery Q) {
	extern __shared__ u32 lds[];
	stage_tables<TABLES_GLOBAL>(L, lds);
	Interp<SSIZE, KIND> fast{ L.ops, L.n_ops, {}, 0u };
	Interp<SSIZE, 0> exact{ L.ops, L.n_ops, {}, 0u };
	light_rays<TABLES_GLOBAL>(fast, exact, KIND != 0, L, Q, lds);
}

/* The resolve kernel's second argument, behind a Launch whose tables, counts and ambient colour are the LOOK's (gamma table and
 * pixel format the context's) */
struct RelightQuery {
	const LightFactor* factors;  /* light-major planes, as captured */
	u64    stride;
	const u32* hit_id;
	u32    n;
	u32    pad_;
	float* rgb_linear;           /* each may be NULL */
	float* rgb;
	u32*   pixel;
};

/*
 * relight_rays: element i of the planes under the look.  Scene-independent, no march and no SDF: per light one coalesced 16-byte load
 * and the two terms of naive_renderer.c:150-168 as shade_ray writes them, then the ambient term (:171-172), v3clamp and pack_pixel.
 * An id beyond n_roots — no capture writes one — is taken for 0, so that foreign planes cannot make the kernel read outside the tables.
 */
template <bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void relight_rays(const Launch L, const RelightQuery Q) {
	extern __shared__ u32 lds[];
	stage_tables<TABLES_GLOBAL>(L, lds);
	const u32* l_light = TABLES_GLOBAL ? L.lights : lds;
	const u32* l_mat   = TABLES_GLOBAL ? L.materials : l_light + L.n_lights * LIGHT_DWORDS;
	const u32* l_rootm = TABLES_GLOBAL ? L.root_material : l_mat + L.n_materials * MATERIAL_DWORDS;
	const u32 i = blockIdx.x * (u32)BLOCK + threadIdx.x;
	if (i >= Q.n) return;

	u32 id = Q.hit_id[i];
	if (id > L.n_roots) id = 0u;
	const u32 mid = id ? l_rootm[id - 1] : 0u;
	const float* m = reinterpret_cast<const float*>(l_mat + mid * MATERIAL_DWORDS);
	const V3 m_diff = { m[1], m[2], m[3] }, m_spec = { m[4], m[5], m[6] }, m_amb = { m[7], m[8], m[9] };

	V3 total = { 0.f, 0.f, 0.f };
	for (u32 li = 0; li < L.n_lights; li++) {
		const u32* lp = l_light + li * LIGHT_DWORDS;
		const LightFactor f = Q.factors[(u64)li * Q.stride + i];
		V3 Id = mul(scale(lds_v3(lp + 3), f.shadow * f.di), m_diff);
		total = add(total, Id);
		V3 Is = mul(scale(lds_v3(lp + 6), f.shadow * f.si), m_spec);
		total = add(total, Is);
	}
	total = add(total, mul(v3(L.ambient), m_amb));
	/* v3clamp: max(min(v, 1), 0) — NaN → 1 (vec.h:63-65) */
	const V3 c = { maxf_(minf_(total.x, 1.f), 0.f), maxf_(minf_(total.y, 1.f), 0.f), maxf_(minf_(total.z, 1.f), 0.f) };

	LaunchTail T = launch_tail(L);
	T.dbg_rgb = Q.rgb;
	V3 post = c;
	u32 px = 0u;
	if (Q.rgb || Q.pixel) px = pack_pixel(L, T, c, post);
	if (Q.rgb_linear) { float* o = Q.rgb_linear + 3ull * i; o[0] = c.x; o[1] = c.y; o[2] = c.z; }
	if (Q.rgb) { float* o = Q.rgb + 3ull * i; o[0] = post.x; o[1] = post.y; o[2] = post.z; }
	if (Q.pixel) Q.pixel[i] = px;
}

}  // namespace lol
