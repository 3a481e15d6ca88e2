/*
 * lol_kernel_light_update.h — light updates (lol_gpu_light_update_rays, lol_gpu_light_update_pixels): the planes of a capture
 * (lol_kernel_light.h) brought to a look that moves lights or changes a shininess, without the primary march.
 *
 * What a capture's primary march found is in its planes: hit_dist and hit_id.  The hit point is p = ro + rd * dist on those very bits,
 * the normal is four SDF values at p, and what each light adds is the body of light_ray's loop at p — so light_update_ray is light_ray
 * with march<true>() replaced by two loads, and its loop taken over the lights of two masks instead of all of them:
 *   march_lights      the whole factor: soft_shadow towards the look's point, di, si, shadow_steps — one 16-byte store per lane;
 *   specular_lights   (and not in march_lights) si alone — no shadow march for the whole wave, one 4-byte store per lane at byte 8 of
 *                     the element; the other twelve bytes stay what they are.
 * The tables of the Launch — lights, materials, root_material — are the LOOK's; the macro-op lists are the context's: the geometry is
 * the uploaded program's.  hit_id, hit_dist, march_steps and the planes of lights in neither mask are not written.
 *
 * Element i is lane blockIdx.x * BLOCK + threadIdx.x, as in light_rays: the waves, and with them the ballots, are the capture's.
 * One difference is left (include/lol_gpu.h, "Light updates"): a wave of a ray LIST whose fast SDF left what was proven for it during
 * the PRIMARY march was captured by the plain pass with settled = false; here no primary march runs, the fast pass may stand, and
 * shadow_steps is then the settled count.  The three floats are equal in every case.
 *
 * Interpreter only, ahead of time only, like the capture.  Included last; its kernels are instantiated last in lol_gpu.hip.
 */
#pragma once
#include "lol_kernel_light.h"

namespace lol {

/* The update kernels' second argument, by value, behind a Launch filled as a capture's but for its tables, which are the look's.
 * The source fields are LightQuery's, in its order: fetch_ray<true> reads them from either. */
struct LightUpdateQuery {
	const float* rays;           /* n x 6 floats, or unused */
	const u32*   xy;             /* SHADE_FROM_PIXELS without LIGHT_ALL_PIXELS: n x {x, y} */
	u32    n;
	u32    flags;                /* SHADE_FROM_PIXELS, SHADE_SCENE_SANE, LIGHT_ALL_PIXELS */
	u64    march_lights;         /* bit l: light l's whole factor */
	u64    specular_lights;      /* bit l, and not in march_lights: light l's specular incidence alone */
	u64    stride;               /* elements between the planes of two lights, >= n */
	LightFactor* factors;
	const u32*   hit_id;         /* what the capture wrote */
	const float* hit_dist;
	/* (everything from march_lights on is read late: light_update_late()) */
};
struct LightUpdateArgs { Launch L; LightUpdateQuery Q; };      /* the kernel-argument segment of an update kernel */

/* Everything of the query but its source is needed for an instruction or two — the two loads at the kernel's start, a bit test per
 * light, the store behind a shadow march — so it is read THERE from the kernel-argument segment, as light_out() reads the capture's
 * pointers: none of the thirteen SGPRs sits through the taps and the shadow loops. */
struct LightUpdateLate { u32 n; u64 march_lights, specular_lights, stride; LightFactor* factors; const u32* hit_id; const float* hit_dist; };
__device__ __forceinline__ LightUpdateLate light_update_late(const LightUpdateQuery& Q0) {
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) LightUpdateArgs* kernarg_ptr;
	kernarg_ptr A = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(A));                    /* opaque: these loads are not merged with the ones at kernel entry */
	return { A->Q.n, A->Q.march_lights, A->Q.specular_lights, A->Q.stride, A->Q.factors, A->Q.hit_id, A->Q.hit_dist };
#else
	return { Q0.n, Q0.march_lights, Q0.specular_lights, Q0.stride, Q0.factors, Q0.hit_id, Q0.hit_dist };
#endif
}

/*
 * The per-ray body: light_ray's with the march read back — `dist0`, `id0`: what the capture wrote for the element, the id held to
 * n_roots (light_update_rays).  `i` = the ray's element (a lane beyond n works on a copy of element n - 1 and stores
 * nothing).  normal_and_id reads dist, id and `ask` of a Marched alone where ask is false (the interpreter keeps the id
 * in its march: Sdf::ASK_ID_ONCE is false), so prev and steps are left 0 — and kb, the bound a march keeps for its taps (lol_kernel.h,
 * bound_keep), stays at its default of -inf: no march of this Sdf object produced `p`.
 */
template <class Sdf, bool TABLES_GLOBAL>
__device__ __forceinline__ void light_update_ray(const Launch& L, const LightUpdateQuery& Q, Sdf& sdf, const u32* lds, V3 ro, V3 rd,
                                                 float dist0, u32 id0, bool settled, u32 i) {
	const u32* l_light = TABLES_GLOBAL ? L.lights : lds;
	const u32* l_mat   = TABLES_GLOBAL ? L.materials : l_light + L.n_lights * LIGHT_DWORDS;
	const u32* l_rootm = TABLES_GLOBAL ? L.root_material : l_mat + L.n_materials * MATERIAL_DWORDS;

	const Marched marched = { dist0, 0.f, 0u, id0, false };

	const V3 p = add(ro, scale(rd, marched.dist));
	bool lit;
	u32 id;
	const V3 n = normal_and_id(sdf, ro, rd, marched, p, false, id, lit);

	/* get_material, naive_renderer.c:103-112: the shininess alone, the LOOK's */
	const u32 mid = id ? l_rootm[id - 1] : 0u;
	const float shininess = reinterpret_cast<const float*>(l_mat + mid * MATERIAL_DWORDS)[0];

	const V3 camera_dir = normalize(sub(ro, p));
	/* the lights of either mask, lowest first.  The masks are kernel arguments, read again at every turn: the loop, its exit and both
	 * branches below are scalar, and what stays in registers through a shadow march is the light's number */
	for (u32 li = 0; li < 64u; li++) {
		const LightUpdateLate A = light_update_late(Q);
		const u64 rest = (A.march_lights | A.specular_lights) >> li;
		if (rest == 0) break;
		li += (u32)__builtin_ctzll(rest);
		const bool whole = (A.march_lights >> li & 1u) != 0u;
		const u32* lp = l_light + li * LIGHT_DWORDS;
		V3 to_light = sub(lds_v3(lp), p);
		float light_dist = len(to_light);
		V3 light_dir = scale(to_light, 1.0f / light_dist);      /* == v3normalize(light - p) */
		const float di = clampf_(dot(n, light_dir), 0.f, 1.f);
		u32 steps = 0, skipped = 0;                             /* (turns run, turns a stationary ray left out: reported together) */
		const float shadow = soft_shadow<true>(sdf, p, light_dir, light_dist, steps, skipped, whole, settled);      /* (specular alone: no march) */
		V3 refl = sub(scale(n, 2.f * dot(light_dir, n)), light_dir);
		const float si = di * powf_glibc(clampf_(dot(refl, camera_dir), 0.f, 1.f), shininess);
		const LightUpdateLate B = light_update_late(Q);
		if (i < B.n) {                                          /* (this lane owns an element: asked again here, not kept as a mask) */
			LightFactor* at = B.factors + ((u64)li * B.stride + i);
			if ((B.march_lights >> li & 1u) != 0u) {
				const LightFactor f = { shadow, di, si, steps + skipped };
				*at = f;
			} else {
				at->si = si;
			}
		}
	}
}

/* The whole update kernel, after the tables are staged: light_rays' driver and its ballot with light_update_ray in the place of
 * light_ray, and nothing behind the passes — no plane of the march is written.  A copy, not a call ("Not folded": lol_kernel_shade.h,
 * shade_rays; lol_kernel_light.h, light_rays).  The rule of the plain pass is the capture's: from_pixels && settled. */
template <bool TABLES_GLOBAL, class SdfFast, class SdfExact>
__device__ __forceinline__ void light_update_rays(SdfFast& fast, SdfExact& exact, bool have_fast, const Launch& L, const LightUpdateQuery& Q,
                                                  const u32* lds) {
	const u32 i = blockIdx.x * (u32)BLOCK + threadIdx.x;
	const bool from_pixels = (Q.flags & SHADE_FROM_PIXELS) != 0u;
	V3 ro, rd;
	fetch_ray<true>(L, Q, i, ro, rd);
	/* the march, read back ONCE for both passes: two VGPRs through the first pass, in a kernel that has a dozen to spare, instead of two
	 * pointers and n_roots in SGPRs through it.  An id beyond n_roots — no capture writes one — is taken for 0, as relight_rays takes it. */
	float dist0;
	u32 id0;
	{
		const u32 j = i < Q.n ? i : Q.n - 1u;
		const LightUpdateLate A = light_update_late(Q);
		id0 = A.hit_id[j];
		dist0 = A.hit_dist[j];
		if (id0 > L.n_roots) id0 = 0u;
	}
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
	if (have_fast && (Q.flags & SHADE_SCENE_SANE) && sane && (!SdfFast::ASSUME_SETTLED || settled)) {
		light_update_ray<SdfFast, TABLES_GLOBAL>(L, Q, fast, lds, ro, rd, dist0, id0, settled, i);
		plain = unproven(fast);
	}
	if (plain) {
		fetch_ray<true>(L, Q, i, ro, rd);
		light_update_ray<SdfExact, TABLES_GLOBAL>(L, Q, exact, lds, ro, rd, dist0, id0, from_pixels && settled, i);
	}
}

/* The interpreter's update kernel (ahead of time), per stack class, root kind and table placement like light_interp. */
template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void light_update_interp(const Launch L, const LightUpdateQuery Q) {
	extern __shared__ u32 lds[];
	stage_tables<TABLES_GLOBAL>(L, lds);
	Interp<SSIZE, KIND> fast{ L.ops, L.n_ops, {}, 0u };
	Interp<SSIZE, 0> exact{ L.ops, L.n_ops, {}, 0u };
	light_update_rays<TABLES_GLOBAL>(fast, exact, KIND != 0, L, Q, lds);
}

}  // namespace lol
