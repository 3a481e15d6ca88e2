/*
 * lol_kernel_light_views.h — relit AVERAGED pixels (lol_gpu_relight_views): the supersampled frame, the blend over K cameras and the
 * supersampled blend of a look, made from captured light passes without a march.
 *
 * The planes hold one element per LEAF: sample column X < s w and sample row Y < s h under camera k of view v is element
 *   e = ((v K + k) s h + Y) s w + X
 * — record r = v K + k is the capture of every pixel of the s w x s h frame under its camera (lol_gpu_light_views: one
 * lol_gpu_light_pixels per record).  Pixel (x, y) of view v is then
 *   1. per leaf, relight_rays' clamped linear colour under the look (relit_linear: the same expressions on the same binary32 values);
 *   2. per camera k, the balanced tree over its s^2 leaves (s x + i, s y + j) in order j s + i, times 1 / s^2 (s = 1: the leaf);
 *   3. the balanced tree over the K cameras in order of k, times 1 / K (K = 1: m_0);
 *   4. pack_pixel: gamma and the context's pixel format, as for one sample
 * which is lol_kernel_aa.h's tree, then lol_kernel_blend.h's, in the order lol_kernel_blend_aa.h fixes.
 *
 * One lane per SAMPLE, render_aa_list's mapping: lane = g s^2 + (j s + i), group g of the wave's 64 / s^2 groups, sample (i, j).  A
 * wave owns 64 consecutive pixels and takes them in s^2 ROUNDS of 64 / s^2 pixels, neighbours in x: in a round the s lanes of a
 * sample row of a pixel and the groups read consecutive elements, so per light a wave's 16-byte loads are s runs of 64 / s elements
 * (1 KiB in one run, 512 bytes in two, 256 bytes in four), and its rounds walk on through the same rows.  The xor butterfly over
 * the lane bits of the sample, lowest first (aa_add_xor), is the tree of step 2 and leaves its sum in every lane of the group.  The
 * K cameras are a loop in the lane; step 3 is a pairwise accumulator of at most four partial sums in registers — camera k is added to
 * the partial sums of the levels at which k's low bits are 1, as a binary counter carries — which performs the additions of the
 * balanced tree, each on the same two operands.  Lane (g, k) KEEPS the pixel of round k: after the last round the 64 lanes hold the
 * wave's 64 pixels, one each, and what a pixel costs once — the two divisions that find it, gamma, packing, the stores — is paid once
 * per pixel, not once per sample (with one division pair and one pack_pixel per SAMPLE the kernel was bound by its instructions and
 * 4 - 17 % slower than relight_rays over the same elements: DESIGN.md 3.22).  Pixels past the end are the last pixel again and
 * are not stored: the butterfly needs every lane of the wave.
 *
 * Per pixel K s^2 (4 + 16 n_lights) bytes read, at most 28 written.  No scratch, no LDS beyond the look's tables.
 */
#pragma once
#include "lol_kernel_light.h"

namespace lol {

/* The resolve kernel's second argument, behind a Launch filled as relight_rays'.  Every element index fits 32 bits: the host refuses
 * more than 2^32 - 1 elements. */
struct RelightViewsQuery {
	const LightFactor* factors;  /* light-major planes over all n_views K s^2 w h elements */
	u64    stride;
	const u32* hit_id;
	u32    n_pixels;             /* n_views w h */
	u32    w, h;                 /* of a view, in pixels */
	u32    s_log2;               /* samples per axis: 1 << s_log2, 0 ... 2 */
	u32    cams;                 /* K: 1, 2, 4, 8 or 16 */
	u32    last_view;            /* n_views - 1 */
	float* rgb_linear;           /* each may be NULL */
	float* rgb;
	u32*   pixel;
};

/* relight_rays' element e up to v3clamp: the same loads, the same operations in the same order */
__device__ __forceinline__ V3 relit_linear(const Launch& L, const RelightViewsQuery& Q, const u32* l_light, const u32* l_mat,
                                           const u32* l_rootm, u32 e) {
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
	total = add(total, mul(v3(L.ambient), m_amb));
	return { maxf_(minf_(total.x, 1.f), 0.f), maxf_(minf_(total.y, 1.f), 0.f), maxf_(minf_(total.z, 1.f), 0.f) };
}

template <bool TABLES_GLOBAL = false>
__global__ __launch_bounds__(BLOCK)
void relight_views(const Launch L, const RelightViewsQuery Q) {
	extern __shared__ u32 lds[];
	stage_tables<TABLES_GLOBAL>(L, lds);
	const u32* l_light = TABLES_GLOBAL ? L.lights : lds;
	const u32* l_mat   = TABLES_GLOBAL ? L.materials : l_light + L.n_lights * LIGHT_DWORDS;
	const u32* l_rootm = TABLES_GLOBAL ? L.root_material : l_mat + L.n_materials * MATERIAL_DWORDS;

	const u32 sl = Q.s_log2, s = 1u << sl, ss = s * s, per_round = 64u >> (2u * sl);
	const u32 lane = threadIdx.x & 63u, k = lane & (ss - 1u), i = k & (s - 1u), j = k >> sl, g = lane >> (2u * sl);
	const u64 first = (((u64)blockIdx.x * (u32)BLOCK + threadIdx.x) >> 6) * 64u;      /* the wave's first pixel */
	const u32 sw = Q.w << sl, cam_elems = (Q.h << sl) * sw, view_elems = Q.cams * cam_elems;      /* the sample grid of one camera; a view's leaves */
	const u32 last = Q.n_pixels - 1u;

	/* this lane's pixel of round 0: view, row and column by division, once; the rounds walk on from it */
	u64 p = first + g;
	const u32 p0 = p < Q.n_pixels ? (u32)p : last;
	const u32 wh = Q.w * Q.h, v0 = p0 / wh, in_view = p0 - v0 * wh;
	u32 y = in_view / Q.w, x = in_view - y * Q.w, view_base = v0 * view_elems;

	V3 keep = {};
	for (u32 r = 0; r < ss; r++) {
		/* this lane's leaf under camera 0 of the pixel's view */
		u32 e = view_base + ((y << sl) + j) * sw + (x << sl) + i;
		V3 a0 = {}, a1 = {}, a2 = {}, a3 = {}, c = {};
		for (u32 cam = 0; cam < Q.cams; cam++, e += cam_elems) {
			c = relit_linear(L, Q, l_light, l_mat, l_rootm, e);
			if (ss >= 4u)  { c = aa_add_xor(c, 1); c = aa_add_xor(c, 2); }
			if (ss == 16u) { c = aa_add_xor(c, 4); c = aa_add_xor(c, 8); }
			if (ss > 1u) c = scale(c, ss == 16u ? 1.f / 16.f : 1.f / 4.f);            /* 1 / s^2 */
			/* the tree over the cameras, pairwise: a_l = the sum of the 2^l cameras before this one, where bit l of cam is set */
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
		/* the next round's pixel: per_round further on, through the ends of rows and views; past the end, the last pixel */
		p += per_round;
		x += per_round;
		while (x >= Q.w) {
			x -= Q.w;
			if (++y == Q.h) { y = 0u; view_base += view_elems; }
		}
		if (p >= Q.n_pixels) { x = Q.w - 1u; y = Q.h - 1u; view_base = Q.last_view * view_elems; }
	}

	/* lane (g, k) holds the pixel of round k */
	const u64 q = first + k * per_round + g;
	LaunchTail T = launch_tail(L);
	T.dbg_rgb = Q.rgb;
	V3 post = keep;
	u32 px = 0u;
	if (Q.rgb || Q.pixel) px = pack_pixel(L, T, keep, post);
	if (q < Q.n_pixels) {
		if (Q.rgb_linear) { float* o = Q.rgb_linear + 3ull * q; o[0] = keep.x; o[1] = keep.y; o[2] = keep.z; }
		if (Q.rgb) { float* o = Q.rgb + 3ull * q; o[0] = post.x; o[1] = post.y; o[2] = post.z; }
		if (Q.pixel) Q.pixel[q] = px;
	}
}

}  // namespace lol
