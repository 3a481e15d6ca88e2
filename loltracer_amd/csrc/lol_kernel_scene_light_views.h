/*
 * lol_kernel_scene_light_views.h — relit AVERAGED pixels under each record's own look (lol_gpu_relight_scene_views): the
 * supersampled frames and the blends over K records of an animation whose every record has a scene — and so a look — of its own,
 * made from the leaves lol_gpu_light_scene_pixels captured, without a march.
 *
 * The planes are relit views' (lol_kernel_light_views.h): sample column X < s w and sample row Y < s h of record r = v K + k is
 * element e = (r s h + Y) s w + X, and pixel (x, y) of view v is
 *   1. per leaf, relight_rays_scenes' clamped linear colour under look r (relit_linear_under: the same expressions on the same
 *      binary32 values);
 *   2. per record k, the balanced tree over its s^2 leaves (s x + i, s y + j) in order j s + i, times 1 / s^2 (s = 1: the leaf);
 *   3. the balanced tree over the K records in order of k, times 1 / K (K = 1: m_0);
 *   4. pack_pixel: gamma and the context's pixel format, as for one sample.
 *
 * The kernel is relight_views with the VIEW in blockIdx.y.  One lane per sample, the xor butterfly (aa_add_xor) for a record's
 * tree, the pairwise accumulator a0 ... a3 over the records, lane (g, k) keeping the pixel of round k, one pack_pixel per pixel: all
 * as there, and said there.  What the grid's y changes:
 *   - a wave owns 64 consecutive pixels of ONE view; lanes past the view's last pixel take that pixel again and store nothing.  The
 *     walk from round to round steps through the ends of rows only, not from view to view, and the two divisions that find a lane's
 *     first pixel happen once per lane;
 *   - record r = v K + k is wave-uniform, and so is its LookRecord: it is read with scalar loads through the constant address space,
 *     as relight_rays_scenes reads its one.  The look is read per RECORD, inside the loop over the records: look r's tables and look
 *     r's ambient colour go to relit_linear_under as arguments, and no Launch is patched.
 * The K looks of a view lie one behind the other in LookList::data, look_stride(L) dwords apart (the host lays them so:
 * relight_scenes' layout).  Where all K fit (K look_stride <= TABLES_LDS_MAX_DWORDS) they are staged as ONE run of K look_stride
 * dwords behind one barrier; otherwise the TABLES_GLOBAL instantiation reads them where they lie.  The host picks by the same rule
 * (views_looks_in_lds).
 *
 * Per pixel K s^2 (4 + 16 n_lights) bytes read, at most 28 written.  No scratch, no LDS beyond the staged tables.
 * The interpreter's kernels alone, ahead of time: no scene module includes this header, and hipRTC is not handed its text.
 */
#pragma once
#include "lol_kernel_light_views.h"
#include "lol_kernel_scene_light.h"

namespace lol {

/* The resolve kernel's second argument, behind a Launch filled as relight_rays_scenes' (counts, gamma table, pixel format) and in
 * front of its LookList.  Every element index fits 32 bits: the host refuses more than 2^32 - 1 elements. */
struct RelightSceneViewsQuery {
	const LightFactor* factors;  /* light-major planes over all n_views K s^2 w h elements */
	u64    stride;
	const u32* hit_id;
	u32    w, h;                 /* of a view, in pixels */
	u32    s_log2;               /* samples per axis: 1 << s_log2, 0 ... 2 */
	u32    cams;                 /* K: 1, 2, 4, 8 or 16 */
	float* rgb_linear;           /* each may be NULL; dense over (v h + y) w + x */
	float* rgb;
	u32*   pixel;
};

/* dwords from one look's tables to the next one's in LookList::data: a look's tables on a multiple of four dwords */
__host__ __device__ inline u32 look_stride(u32 n_lights, u32 n_materials, u32 n_roots) {
	return (table_dwords(n_lights, n_materials, n_roots) + 3u) & ~3u;
}
/* whether the K looks of one view are staged: the ONE rule of kernel and host */
__host__ __device__ inline bool views_looks_in_lds(u32 cams, u32 n_lights, u32 n_materials, u32 n_roots) {
	return cams * look_stride(n_lights, n_materials, n_roots) <= TABLES_LDS_MAX_DWORDS;
}

/* relit_linear (lol_kernel_light_views.h) with the look handed in: its tables and its ambient colour, not the Launch's.  The same
 * loads, the same operations in the same order as relight_rays_scenes' element e up to v3clamp. */
__device__ __forceinline__ V3 relit_linear_under(const Launch& L, const RelightSceneViewsQuery& Q, const u32* l_light, const u32* l_mat,
                                                 const u32* l_rootm, V3 ambient, u32 e) {
	u32 id = Q.hit_id[e];
	if (id > L.n_roots) id = 0u;
	const u32 mid = id ? l_rootm[id - 1] : 0u;
	const float* m = reinterpret_cast<const float*>(l_mat + mid * MATERIAL_DWORDS);
	const V3 m_diff = { m[1], m[2], m[3] }, m_spec = { m[4], m[5], m[6] }, m_amb = { m[7], m[8], m[9] };
	V3 total = { 0.f, 0.f, 0.f };
	for (u32 li = 0; li < L.n_lights; li++) {
		const u32* lp = l_light + li * LIGHT_DWORDS;
		const LightFactor f = Q.factors[(u64)li * Q.stride + e];
		V3 Id = mul(scale(lds_v3(lp + 3), f.shadow * f.di), m_diff);
		total = add(total, Id);
		V3 Is = mul(scale(lds_v3(lp + 6), f.shadow * f.si), m_spec);
		total = add(total, Is);
	}
	total = add(total, mul(ambient, m_amb));
	return { maxf_(minf_(total.x, 1.f), 0.f), maxf_(minf_(total.y, 1.f), 0.f), maxf_(minf_(total.z, 1.f), 0.f) };
}

template <bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void relight_views_scenes(const Launch L, const RelightSceneViewsQuery Q, const LookList R) {
	extern __shared__ u32 lds[];
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) LookRecord* look_ptr;
#else
	typedef const LookRecord* look_ptr;
#endif
	const u32 view = blockIdx.y;
	const look_ptr looks = (look_ptr)(unsigned long long)R.looks + view * Q.cams;        /* the K records of this view */
	const u32 first_tables = looks[0].tables_offset;
	if constexpr (!TABLES_GLOBAL) {
		/* the K looks' tables, one behind the other: one run, and no Launch is patched */
		const u32* run = R.data + first_tables;
		const u32 n = Q.cams * look_stride(L.n_lights, L.n_materials, L.n_roots);
		for (u32 t = threadIdx.x; t < n; t += BLOCK) lds[t] = run[t];
		__syncthreads();
	}

	const u32 sl = Q.s_log2, s = 1u << sl, ss = s * s, per_round = 64u >> (2u * sl);
	const u32 lane = threadIdx.x & 63u, k = lane & (ss - 1u), i = k & (s - 1u), j = k >> sl, g = lane >> (2u * sl);
	const u32 wh = Q.w * Q.h, last = wh - 1u;
	const u32 first = ((blockIdx.x * (u32)BLOCK + threadIdx.x) >> 6) * 64u;               /* the wave's first pixel of the view */
	if (first >= wh) return;                          /* a whole wave behind the view (the block's last ones): nothing to resolve */
	const u32 sw = Q.w << sl, cam_elems = (Q.h << sl) * sw;                                  /* the sample grid of one record */
	const u32 view_base = view * Q.cams * cam_elems;

	/* this lane's pixel of round 0: row and column by division, once; the rounds walk on from it */
	u32 p = first + g;
	const u32 p0 = p < wh ? p : last;
	u32 y = p0 / Q.w, x = p0 - y * Q.w;

	V3 keep = {};
	for (u32 r = 0; r < ss; r++) {
		/* this lane's leaf under record 0 of the view */
		u32 e = view_base + ((y << sl) + j) * sw + (x << sl) + i;
		V3 a0 = {}, a1 = {}, a2 = {}, a3 = {}, c = {};
		for (u32 cam = 0; cam < Q.cams; cam++, e += cam_elems) {
			/* look v K + cam: where its tables lie, and its ambient colour (scalar loads: the record is the wave's) */
			const u32 at = looks[cam].tables_offset;
			const V3 ambient = { looks[cam].ambient[0], looks[cam].ambient[1], looks[cam].ambient[2] };
			const u32* l_light = TABLES_GLOBAL ? R.data + at : lds + (at - first_tables);
			const u32* l_mat   = l_light + L.n_lights * LIGHT_DWORDS;
			const u32* l_rootm = l_mat + L.n_materials * MATERIAL_DWORDS;
			c = relit_linear_under(L, Q, l_light, l_mat, l_rootm, ambient, e);
			if (ss >= 4u)  { c = aa_add_xor(c, 1); c = aa_add_xor(c, 2); }
			if (ss == 16u) { c = aa_add_xor(c, 4); c = aa_add_xor(c, 8); }
			if (ss > 1u) c = scale(c, ss == 16u ? 1.f / 16.f : 1.f / 4.f);            /* 1 / s^2 */
			/* the tree over the records, pairwise: a_l = the sum of the 2^l records before this one, where bit l of cam is set */
			if (cam & 1u) {
				c = add(a0, c);
				if (cam & 2u) {
					c = add(a1, c);
					if (cam & 4u) {
						c = add(a2, c);
						if (cam & 8u) c = add(a3, c); else a3 = c;
					} else a2 = c;
				} else a1 = c;
			} else a0 = c;
		}
		if (Q.cams > 1u) c = scale(c, 1.f / (float)Q.cams);           /* 1 / K: a power of two, exact */
		if (k == r) keep = c;
		/* the next round's pixel: per_round further on, through the ends of rows; past the view's end, its last pixel */
		p += per_round;
		x += per_round;
		while (x >= Q.w) { x -= Q.w; y++; }
		if (p >= wh) { x = Q.w - 1u; y = Q.h - 1u; }
	}

	/* lane (g, k) holds the pixel of round k */
	const u32 q = first + k * per_round + g;
	LaunchTail T = launch_tail(L);                 /* (the Launch is this kernel's first argument too) */
	T.dbg_rgb = Q.rgb;
	V3 post = keep;
	u32 px = 0u;
	if (Q.rgb || Q.pixel) px = pack_pixel(L, T, keep, post);
	if (q < wh) {
		const u64 at = (u64)view * wh + q;
		if (Q.rgb_linear) { float* o = Q.rgb_linear + 3ull * at; o[0] = keep.x; o[1] = keep.y; o[2] = keep.z; }
		if (Q.rgb) { float* o = Q.rgb + 3ull * at; o[0] = post.x; o[1] = post.y; o[2] = post.z; }
		if (Q.pixel) Q.pixel[at] = px;
	}
}

}  // namespace lol
