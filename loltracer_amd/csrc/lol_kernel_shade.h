/*
 * lol_kernel_shade.h — shading queries (lol_gpu_shade_rays, lol_gpu_shade_pixels): the colour the reference computes along a ray
 * the HOST brings — the other half of lol_kernel_rays.h, which answers geometry alone.
 *
 * One lane per RAY.  Ray i is naive_renderer.c:225-232 for (ro_i, rd_i): get_intersection, p = ro + rd * dist, get_normal,
 * get_light with the eye at ro (get_light reads the eye from the scene, :132 / :145, and a ray's eye is its own origin: for a
 * frame, the camera's position), v3pow(., 1 / 2.2), colorf_to_pixfmt — march<true>(), normal_and_id(), soft_shadow<true>(), the
 * Phong loop and pack_pixel() of lol_kernel.h on the Sdf policies the frames use.  The rays come from a list in device memory
 * (n x {ox, oy, oz, dx, dy, dz}, used as given) or are the primary rays of a list of pixels (x, y) of a w x h frame under a camera;
 * which, is a wave-uniform kernel argument.
 *
 * Blocks of lol::BLOCK threads (one wave in the default build), so that stage_common / stage_tables serve unchanged; block b owns
 * rays [b * BLOCK, (b + 1) * BLOCK).  The kernel's arguments are a Launch — the scene's half, filled by the host function that
 * fills a frame's — and a ShadeQuery behind it, as the batch kernels take a Launch and a BatchTail.
 *
 * ONE counting form (COUNT = true): `steps` is one of the six outputs, and a twin without the counters would be a second copy of
 * the whole pipeline in every module for the 1.3 % the counters cost a frame — not worth it for a query.
 *
 * shade_ray restates shade_pixel's body from the line after camera_ray onwards instead of shade_pixel being folded onto it: the
 * fold was not held against tools/code_identity.py, and a fold that moves one instruction of an existing kernel is not made
 * ("Not folded").  The two differ in where the ray comes from, in COUNT, and in `settled` being an argument (below).
 */
#pragma once
#include "lol_kernel.h"

namespace lol {

/* ShadeQuery::flags */
constexpr u32 SHADE_FROM_PIXELS = 1u;   /* the rays are the primary rays of the pixels in `xy` under Launch::cam; else the list `rays` */
constexpr u32 SHADE_SCENE_SANE = 2u;    /* the host's side of what the fast SDF rests on holds: every number of the scene finite and below
                                         * 10^15 (lol_gpu.hip, shadow_settle_ok) and, for SHADE_FROM_PIXELS, of the camera too (camera_sane) */
constexpr u32 LIGHT_ALL_PIXELS = 4u;    /* a capture's alone (lol_kernel_light.h), with SHADE_FROM_PIXELS: there is no list, ray i is pixel (i % w, i / w) of the Launch's frame */

struct ShadeOut { float* rgb_linear; float* rgb; u32* pixel; float* hit_dist; u32* hit_id; u32* steps; };   /* each may be NULL; element i belongs to ray i */

/* The kernels' second argument, by value.  Launch carries everything else: tables, ambient, FLAG_MISS_SKIP / FLAG_DARK_SKIP, pixel
 * format, gamma table, max_steps; FLAG_SHADOW_SETTLED = the host's side of it (the scene; for pixels the camera too); and for
 * SHADE_FROM_PIXELS cam, fw, fh, FLAG_FIRST_STEP and its value. */
struct ShadeQuery {
	const float* rays;           /* n x 6 floats, or unused */
	const u32*   xy;             /* SHADE_FROM_PIXELS: n x {x, y} */
	u32    n;
	u32    flags;                /* SHADE_* */
	ShadeOut out;                /* read late: shade_out() */
};
struct ShadeArgs { Launch L; ShadeQuery Q; };      /* the kernel-argument segment of a shading kernel */

/* The output pointers are needed by the last instructions of the kernel: read THERE from the kernel-argument segment, as ray_out()
 * and launch_tail() do, so that twelve SGPRs do not sit through the march and the shadow loops. */
__device__ __forceinline__ ShadeOut shade_out(const ShadeQuery& Q0) {
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) ShadeArgs* kernarg_ptr;
	kernarg_ptr A = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(A));                    /* opaque: these loads are not merged with the ones at kernel entry */
	return { A->Q.out.rgb_linear, A->Q.out.rgb, A->Q.out.pixel, A->Q.out.hit_dist, A->Q.out.hit_id, A->Q.out.steps };
#else
	return Q0.out;
#endif
}

/*
 * The per-ray body: shade_pixel (lol_kernel.h) from the line after camera_ray onwards, for the ray (ro, rd).  `lds` = lights |
 * materials | root_material as staged by stage_common, or unused with TABLES_GLOBAL.  Wave-uniform: first_given (FLAG_FIRST_STEP:
 * L.first_dist / first_id are sdf(ro)), settled (soft_shadow's: the CALLER decides what the wave may assume about its rays).
 *
 * FLAG_MISS_SKIP and FLAG_DARK_SKIP rest on the scene alone and hold for any ray, NaN and infinite components included: a shadow
 * factor is maxf(res, 0) with res <= 1, so it lies in [0, 1] whatever the march met (NaN > 0 is false: 0); the incidence is
 * clamp(., 0, 1), which maps NaN to 0; powf of a base in [0, 1] with a shininess >= 0 is finite.  So under miss_skip_ok an escaped
 * ray's light terms are finite * (+-0) = +-0 and its colour is clamp(ambient * material[0].ambient) for every p and n, and under
 * dark_skip_ok a light with incidence exactly 0 adds +-0 for every shadow factor.
 */
template <class Sdf, bool TABLES_GLOBAL>
__device__ __forceinline__ Pixel shade_ray(const Launch& L, Sdf& sdf, const u32* lds, V3 ro, V3 rd, bool first_given, bool settled) {
	const u32* l_light = TABLES_GLOBAL ? L.lights : lds;
	const u32* l_mat   = TABLES_GLOBAL ? L.materials : l_light + L.n_lights * LIGHT_DWORDS;
	const u32* l_rootm = TABLES_GLOBAL ? L.root_material : l_mat + L.n_materials * MATERIAL_DWORDS;

	const Marched marched = march<true>(sdf, ro, rd, L.max_steps, first_given, L.first_dist, L.first_id);

	const V3 p = add(ro, scale(rd, marched.dist));
	bool lit;
	Hit hit = { marched.dist, 0u, marched.steps };
	const V3 n = normal_and_id(sdf, ro, rd, marched, p, (L.flags & FLAG_MISS_SKIP) != 0u, hit.id, lit);

	/* get_material, naive_renderer.c:103-112 (per-lane table lookups) */
	u32 mid = hit.id ? l_rootm[hit.id - 1] : 0u;
	const float* m = reinterpret_cast<const float*>(l_mat + mid * MATERIAL_DWORDS);
	const float shininess = m[0];
	const V3 m_diff = { m[1], m[2], m[3] }, m_spec = { m[4], m[5], m[6] }, m_amb = { m[7], m[8], m[9] };

	/* get_light, naive_renderer.c:129-175; the skips as in shade_pixel */
	V3 total = { 0.f, 0.f, 0.f };
	u32 shadow_steps = 0, shadow_skipped = 0;
	if (lit) {
		const V3 camera_dir = normalize(sub(ro, p));
		for (u32 li = 0; li < L.n_lights; li++) {
			const u32* lp = l_light + li * LIGHT_DWORDS;
			V3 to_light = sub(lds_v3(lp), p);
			float light_dist = len(to_light);
			V3 light_dir = scale(to_light, 1.0f / light_dist);      /* == v3normalize(light - p) */
			float di = clampf_(dot(n, light_dir), 0.f, 1.f);
			bool needed = true;
			if (L.flags & FLAG_DARK_SKIP) needed = di > 0.f;
			if ((L.flags & FLAG_MISS_SKIP) && hit.id == 0u) needed = false;
			float shadow = soft_shadow<true>(sdf, p, light_dir, light_dist, shadow_steps, shadow_skipped, needed, settled);

			V3 refl = sub(scale(n, 2.f * dot(light_dir, n)), light_dir);
			V3 Id = mul(scale(lds_v3(lp + 3), shadow * di), m_diff);
			total = add(total, Id);
			float si = 0.f;
			if (!(L.flags & FLAG_DARK_SKIP) || vote(needed && shadow != 0.f) != 0)
				si = di * powf_glibc(clampf_(dot(refl, camera_dir), 0.f, 1.f), shininess);
			V3 Is = mul(scale(lds_v3(lp + 6), shadow * si), m_spec);
			total = add(total, Is);
		}
	}
	total = add(total, mul(v3(L.ambient), m_amb));
	/* v3clamp: max(min(v, 1), 0) — NaN → 1 (vec.h:63-65) */
	V3 c = { maxf_(minf_(total.x, 1.f), 0.f), maxf_(minf_(total.y, 1.f), 0.f), maxf_(minf_(total.z, 1.f), 0.f) };
	return { c, hit, shadow_steps, shadow_skipped };
}

/* Ray i of the query (a lane beyond n: ray n - 1), read or built where a pipeline begins.  A wave that shades again through the exact
 * pipeline fetches its rays AGAIN, through an index the compiler cannot see through: kept live for that rare second pass, a
 * per-lane origin and direction are six VGPRs held through the whole first one, in a kernel compiled for 64.  `Query`: a ShadeQuery or
 * a capture's LightQuery (lol_kernel_light.h); ALL_PIXELS_FORM: the capture's, the only one that compiles the LIGHT_ALL_PIXELS branch. */
template <bool ALL_PIXELS_FORM = false, class Query>
__device__ __forceinline__ void fetch_ray(const Launch& L, const Query& Q, u32 i, V3& ro, V3& rd) {
	u32 j = i < Q.n ? i : Q.n - 1u;
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("" : "+v"(j));
#endif
	if (Q.flags & SHADE_FROM_PIXELS) {
		u32 x, y;
		if (ALL_PIXELS_FORM && (Q.flags & LIGHT_ALL_PIXELS)) { y = j / (u32)L.w; x = j - y * (u32)L.w; }
		else { x = Q.xy[2ull * j]; y = Q.xy[2ull * j + 1ull]; }
		ro = v3(L.cam.origin);
		rd = camera_ray(L.cam, L.fw, L.fh, (int)x, (int)y);
	} else {
		const float* r = Q.rays + 6ull * j;
		ro = { r[0], r[1], r[2] };
		rd = { r[3], r[4], r[5] };
	}
}

/*
 * The whole kernel, after the tables are staged.  `fast` / `exact` as in the render kernels.
 *
 * What a wave may assume.  The proofs behind the fast SDF (the proven roots and blend factors, the culling bound carried along the
 * ray), behind FLAG_SHADOW_SETTLED and behind ASSUME_SETTLED of the specialised fast pipeline bound t and the points a march
 * reaches by way of a sane origin and a NORMALISED direction: what the host checks of a frame's camera.  The host never sees the
 * rays of a list, so the wave looks itself and enters the fast / settled pipeline only when
 *   - the host's scene-side flag is set (SHADE_SCENE_SANE for the fast SDF, FLAG_SHADOW_SETTLED for the settle), and
 *   - a ballot finds every lane's six components below 10^15 in magnitude (NaN fails), and
 *   - a ballot finds every lane's squared direction length <= 0x1.00001p+0: |rd| <= 1 + 2^-20, the bound the carried culling test
 *     accepts (lol_codegen.hip, ray_begin) and the regime frames run in.
 * Any other wave of a list runs the exact SDF with settled = false — the reference's own loop exits — and so does one whose fast
 * SDF left what was proven for it (unproven).  The rays of SHADE_FROM_PIXELS are a frame's: the host's camera_sane is the whole
 * test, FLAG_SHADOW_SETTLED is the frame's, and a wave that shades again does so under the launch's flag, as render_interp's does —
 * so `steps` is lol_gpu_debug.steps of that pixel, shadow steps included.
 *
 * Not folded: the ballot below stands three times — here, in light_rays and, without the length, in trace_rays — because
 * one forceinline helper for it left all 16 shade_interp and all 16 light_interp different (root kind 3: 4 bytes longer); and one
 * driver for this function and light_rays, with the per-ray body as a functor, left all 16 light_interp different (same lengths).
 */
template <bool TABLES_GLOBAL, class SdfFast, class SdfExact>
__device__ __forceinline__ void shade_rays(SdfFast& fast, SdfExact& exact, bool have_fast, const Launch& L, const ShadeQuery& Q, const u32* lds) {
	/* lanes beyond n shade a copy of ray n - 1 and store nothing: the wave stays uniform, and what its other lanes compute does not
	 * depend on the copy (every skip is exact) */
	const u32 i = blockIdx.x * (u32)BLOCK + threadIdx.x;
	const bool from_pixels = (Q.flags & SHADE_FROM_PIXELS) != 0u;
	V3 ro, rd;
	fetch_ray(L, Q, i, ro, rd);
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
		fetch_ray(L, Q, i, ro, rd);
		P = shade_ray<SdfExact, TABLES_GLOBAL>(L, exact, lds, ro, rd, first_given, from_pixels && settled);
	}

	/* gamma + packing through pack_pixel; `rgb` is the colour after gamma by powf, as lol_gpu_debug.rgb is.  Plain per-lane stores,
	 * each under its own NULL test: a list has no rows to coalesce, so nothing goes through LDS. */
	const ShadeOut O = shade_out(Q);
	LaunchTail T = launch_tail(L);
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

/* The interpreter's kernel (ahead of time), per stack class, root kind and table placement like render_interp. */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void shade_interp(const Launch L, const ShadeQuery Q) {
	extern __shared__ u32 lds[];
	stage_tables<TABLES_GLOBAL>(L, lds);
	Interp<SSIZE, KIND> fast{ L.ops, L.n_ops, {}, 0u };
	Interp<SSIZE, 0> exact{ L.ops, L.n_ops, {}, 0u };
	shade_rays<TABLES_GLOBAL>(fast, exact, KIND != 0, L, Q, lds);
}

}  // namespace lol
