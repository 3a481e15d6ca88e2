/*
 * lol_kernel_rays.h — ray queries (lol_gpu_trace_rays, lol_gpu_trace_pixels, lol_gpu_pick): the first kernel that is not a frame.
 *
 * One lane per RAY.  Ray i is get_intersection(scene, ro_i, rd_i) (naive_renderer.c:48-69) followed by p = ro + rd * dist (:227) and
 * get_normal(scene, p, dist) (:114-125): march<true>() and normal_and_id() of lol_kernel.h on the Sdf policies the frames use, with
 * no miss skip — a query has no shading whose result the skip could rest on — and nothing else: no lights, no materials, no LDS, no
 * tables, no tile.  The rays come from a list in device memory (n x {ox, oy, oz, dx, dy, dz}, used as given) or are the primary
 * rays of a list of pixels (x, y) of a w x h frame under a camera; which, is a wave-uniform kernel argument.
 *
 * One wave per block, as in sdf_points: a block is done when its own 64 rays are, rays of a list differ in cost as pixels do, and
 * with neither LDS nor a barrier nothing is gained from a larger block.
 */
#pragma once
#include "lol_kernel.h"

namespace lol {

/* RayQuery::flags */
constexpr u32 RAYS_FROM_PIXELS = 1u;   /* the rays are the primary rays of the pixels in `xy` under `cam`; else the list `rays` */
constexpr u32 RAYS_SCENE_SANE = 2u;    /* the host's scene-side check holds (lol_gpu.hip, shadow_settle_ok): the fast SDF may run for waves whose rays are sane too */
constexpr u32 RAYS_FIRST_STEP = 4u;    /* RAYS_FROM_PIXELS: first_dist / first_id hold sdf(cam.origin) (lol_kernel.h, FLAG_FIRST_STEP) */
constexpr u32 RAYS_WANT_ID = 8u;       /* out.id is not NULL: an ASK_ID_ONCE scene asks for it */
constexpr u32 RAYS_WANT_NORMAL = 16u;  /* out.normal is not NULL: the four taps are taken */

struct RayOut { float* dist; u32* id; u32* steps; float* normal; };      /* each may be NULL; element i belongs to ray i */

/* Kernel argument: by value, so it arrives in SGPRs.  The ONLY argument of both kernels (trace_interp, lol_trace_spec): ray_out()
 * reads its tail from the start of the kernel-argument segment. */
struct RayQuery {
	const float* rays;           /* n x 6 floats, or unused */
	const u32*   xy;             /* RAYS_FROM_PIXELS: n x {x, y} */
	u32    n;
	i32    max_steps;
	u32    flags;                /* RAYS_* */
	float  fw, fh;               /* RAYS_FROM_PIXELS: (float)w, (float)h */
	Cam    cam;
	float  first_dist;
	u32    first_id;
	u32    n_ops;                /* the interpreter's macro-op list (trace_interp alone) */
	const u32* ops;
	RayOut out;                  /* read late: ray_out() */
};

/* The output pointers are needed by the last four instructions of the kernel: read THERE from the kernel-argument segment, as
 * launch_tail() does for the frame kernels, so that eight SGPRs do not sit through the march. */
__device__ __forceinline__ RayOut ray_out(const RayQuery& Q0) {
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) RayQuery* kernarg_ptr;
	kernarg_ptr Q = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(Q));                    /* opaque: these loads are not merged with the ones at kernel entry */
	return { Q->out.dist, Q->out.id, Q->out.steps, Q->out.normal };
#else
	return Q0.out;
#endif
}

struct RayHit { float dist; u32 id; u32 steps; V3 n; };

/* one ray through one Sdf policy.  Wave-uniform: first_given, want_id, want_normal. */
template <class Sdf>
__device__ __forceinline__ RayHit trace_one(Sdf& sdf, const RayQuery& Q, V3 ro, V3 rd, bool first_given, bool want_id, bool want_normal) {
	const Marched m = march<true>(sdf, ro, rd, Q.max_steps, first_given, Q.first_dist, Q.first_id);
	RayHit r = { m.dist, m.id, m.steps, { 0.f, 0.f, 0.f } };
	if (want_normal) {
		const V3 p = add(ro, scale(rd, m.dist));
		bool lit;
		r.n = normal_and_id(sdf, ro, rd, m, p, false, r.id, lit);
	} else if (want_id) {
		/* the id an ASK_ID_ONCE march left open (lol_kernel.h, march): normal_and_id's extra turn alone */
		if constexpr (Sdf::ASK_ID_ONCE) {
			if (vote(m.ask) != 0) {
				float s; u32 did;
				sdf.eval(add(ro, scale(rd, m.prev)), s, did);
				if (m.ask) r.id = did;
			}
		}
	}
	return r;
}

/* The whole kernel.  `fast` / `exact` as in the render kernels.  The fast SDF (the proven roots and blend factors, the culling bound
 * carried along the ray) rests on what the host checks for a frame before it sets FLAG_SHADOW_SETTLED: every number of the scene
 * AND of the camera finite and below 10^15.  The host never sees a query's rays, so the wave looks itself: a ballot over the six
 * components of its lanes' rays; one component outside that range in one lane sends the whole wave through the exact SDF, as a wave
 * does whose fast SDF left what was proven for it (unproven).  Directions longer than 1 + 2^-20 are ray_begin's own vote. */
template <class SdfFast, class SdfExact>
__device__ __forceinline__ void trace_rays(SdfFast& fast, SdfExact& exact, bool have_fast, const RayQuery& Q) {
	/* lanes beyond n trace a copy of ray n - 1 and store nothing: the wave stays uniform, and what its other lanes compute does not
	 * depend on the copy (every skip inside an SDF evaluation is exact) */
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
	const RayOut O = ray_out(Q);
	if (i < Q.n) {
		if (O.dist) O.dist[i] = h.dist;
		if (O.id) O.id[i] = h.id;
		if (O.steps) O.steps[i] = h.steps;
		if (O.normal) { float* n = O.normal + 3ull * i; n[0] = h.n.x; n[1] = h.n.y; n[2] = h.n.z; }
	}
}

/* The interpreter's kernel (ahead of time), per stack class and root kind like sdf_points_interp. */
template <int SSIZE, int KIND>
__global__ __launch_bounds__(64)
void trace_interp(const RayQuery Q) {
	Interp<SSIZE, KIND> fast{ Q.ops, Q.n_ops, {}, 0u };
	Interp<SSIZE, 0> exact{ Q.ops, Q.n_ops, {}, 0u };
	trace_rays(fast, exact, KIND != 0, Q);
}

}  // namespace lol
