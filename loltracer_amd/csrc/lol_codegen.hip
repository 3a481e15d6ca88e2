/*
 * lol_codegen.hip — from a flattened scene (lol_program) to what the kernels run: the exact-culling plan, the interpreter's
 * macro-op lists, and the scene's own kernel — generated HIP source compiled by hipRTC (the GPU counterpart of the reference's
 * tracing JIT, tracing_jit_renderer.dasc:76-216,416-434), cached in the process and on disk, refused when it shows LLVM's
 * long-branch register bug.  (Part of liblol_gpu.so; see lol_gpu_internal.h for how the library is cut.)
 */
#include "lol_gpu_internal.h"
#include "lol_code_key.h"
#include <cstdarg>
#include <stdexcept>

/* the text of the lol_kernel*.h files, embedded at build time (csrc/Makefile: lol_kernel_src.inc) for hipRTC */
#include "lol_kernel_src.inc"

#pragma GCC visibility push(hidden)
/* ------------------------------------------------- scene → HIP source (the "JIT") */

/* Appends printf-style to `s`.  It measures first, so no line is ever cut off, whatever its length: the generator's longest, the
 * saturation-culling site of SdfEmitter with its seven literals of 37 bytes, is some 620 bytes at four-digit temporaries.  The
 * compiler checks the arguments against the literal, so a site that has two forms makes two calls instead of choosing a literal.
 * (Hidden like everything here, but not static: tools/spec_source.cpp --selftest calls it.) */
void appendf(std::string& s, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void appendf(std::string& s, const char* fmt, ...) {
	va_list ap, measure;
	va_start(ap, fmt);
	va_copy(measure, ap);
	const int n = vsnprintf(nullptr, 0, fmt, measure);
	va_end(measure);
	if (n < 0) { va_end(ap); throw std::length_error("appendf"); }
	const size_t at = s.size();
	s.resize(at + (size_t)n + 1);                    /* (vsnprintf writes the terminator too) */
	vsnprintf(&s[at], (size_t)n + 1, fmt, ap);
	va_end(ap);
	s.resize(at + (size_t)n);
}

std::string fbits(float v) {
	uint32_t u;
	memcpy(&u, &v, 4);
	std::string b;
	appendf(b, "__builtin_bit_cast(float, 0x%08xu)", u);
	return b;
}

/* Which proven-exact shortcuts the generated code may use (see lol_kernel.h "fast exact paths"). */

/* ------------------------------------------------ exact culling of top-level objects
 * sdf() (naive_renderer.c:31-44) is a strict-'<' minimum over the top-level objects.  An object whose distance is
 * PROVABLY greater than the running minimum cannot change it, so its evaluation may be skipped — exactly, not
 * approximately.  The proof is a bounding sphere (C, R) per object, computed here in double precision:
 *   sphere(c, r):            value = |p-c| - r                                        → (c, max(r, 0))
 *   round box(c, b, r):      value >= |p-c| - |b| - r   (b >= 0, r >= 0)               → (c, |b| + r)
 *   smooth_union(a, b, k>0): value >= min(a, b) - k/4   (h(1-h) <= 1/4 on the clamped h) → sphere enclosing both + k/4
 *   plane, k <= 0, non-finite or absurdly large fields:                                 no bound — never skipped
 * so value(p) >= |p-C| - R in exact arithmetic.  The kernel's binary32 evaluation differs from that by a few ulps
 * of the magnitudes involved (<= 2^-19 relative to |p-C| + R, LABNOTES.md §3.6), which the test below swallows:
 *   R' = R (1 + 2^-10) + (|C|_max + 1) 2^-20, rounded up;   u = (best + R') (1 + 2^-12);
 *   skip  iff  u > 0  and  |p-C|^2 > u^2      (all in binary32; any NaN makes the comparisons false = no skip)
 * which implies |p-C| > (best + R')(1 + 2^-14), hence value(p) > best.  The decision is taken per WAVE: the
 * object is evaluated unless every lane that still cares about the result may skip it (lanes that may skip but
 * run anyway compute a value > best and change nothing).
 *
 * To have a running minimum to compare with, objects WITHOUT a bound (planes: one subtraction) are evaluated first
 * and the bounded ones after them, each group in file order.  The reference's tie rule — the FIRST object of
 * equal distance wins — is kept by comparing ids on ties wherever an object is evaluated after one that follows
 * it in the file:  t < best || (t == best && best_id > id)   (best_id = 0 only while best = +inf, where the
 * reference's inf < inf is false too). */
struct Sphere { bool ok; double c[3], r; uint32_t levels = 1; };   /* levels: nesting depth of the operations under it (a primitive is 1) */

struct RootBound {
	uint32_t first = 0, top = 0;        /* ops [first, top) compute the object, ops[top] is its LOL_OP_TOP */
	uint32_t id = 0, prims = 0;
	bool     bounded = false;
	double   c[3] = { 0, 0, 0 }, r = 0;
	uint32_t levels = 1;                /* nesting depth of its expression (sets the rounding slack of its test) */
	Sphere   sphere() const { return { bounded, { c[0], c[1], c[2] }, r, levels }; }
	std::vector<Sphere> clusters;       /* optional: two spheres that together bound the object more tightly (cluster_bounds) */
};

Sphere enclose(const Sphere& a, const Sphere& b) {
	const uint32_t levels = a.levels > b.levels ? a.levels : b.levels;
	if (!a.ok || !b.ok) return { false, { 0, 0, 0 }, 0, levels };
	const double dx = b.c[0] - a.c[0], dy = b.c[1] - a.c[1], dz = b.c[2] - a.c[2];
	const double d = sqrt(dx * dx + dy * dy + dz * dz);
	if (d + b.r <= a.r) { Sphere r = a; r.levels = levels; return r; }
	if (d + a.r <= b.r) { Sphere r = b; r.levels = levels; return r; }
	const double R = 0.5 * (d + a.r + b.r), t = d > 0 ? (R - a.r) / d : 0.0;
	return { true, { a.c[0] + dx * t, a.c[1] + dy * t, a.c[2] + dz * t }, R * (1.0 + 1e-12), levels };
}

void cluster_bounds(const lol_program& P, RootBound& R);
static bool sane(double v) { return v - v == 0.0 && fabs(v) < 1e15; }      /* finite, and of a size a bound can be made from */

std::vector<RootBound> analyse_roots(const lol_program& P) {
	std::vector<RootBound> roots;
	std::vector<Sphere> st;
	RootBound cur;
	for (uint32_t i = 0; i < P.n_ops; i++) {
		const lol_op& o = P.ops[i];
		switch (o.op) {
		case LOL_OP_SPHERE: {
			const bool ok = sane(o.f[0]) && sane(o.f[1]) && sane(o.f[2]) && sane(o.f[3]);
			st.push_back({ ok, { o.f[0], o.f[1], o.f[2] }, o.f[3] > 0 ? (double)o.f[3] : 0.0 });
			cur.prims++;
			break;
		}
		case LOL_OP_RBOX: {
			bool ok = true;
			for (int j = 0; j < 7; j++) ok = ok && sane(o.f[j]);
			ok = ok && o.f[3] >= 0 && o.f[4] >= 0 && o.f[5] >= 0 && o.f[6] >= 0;
			const double hb = sqrt((double)o.f[3] * o.f[3] + (double)o.f[4] * o.f[4] + (double)o.f[5] * o.f[5]);
			st.push_back({ ok, { o.f[0], o.f[1], o.f[2] }, hb * (1.0 + 1e-12) + o.f[6] });
			cur.prims++;
			break;
		}
		case LOL_OP_PLANE:
			st.push_back({ false, { 0, 0, 0 }, 0 });
			cur.prims++;
			break;
		case LOL_OP_SMIN: case LOL_OP_SMIN_R: {
			Sphere b = st.back(); st.pop_back();
			Sphere a = st.back(); st.pop_back();
			Sphere u = enclose(a, b);
			if (!(sane(o.f[0]) && o.f[0] > 0)) u.ok = false;
			u.r += 0.25 * (double)o.f[0];
			u.levels++;
			st.push_back(u);
			break;
		}
		case LOL_OP_TOP: {
			Sphere v = st.back(); st.pop_back();
			cur.top = i; cur.id = o.id;
			cur.bounded = v.ok && sane(v.r);
			cur.c[0] = v.c[0]; cur.c[1] = v.c[1]; cur.c[2] = v.c[2]; cur.r = v.r; cur.levels = v.levels;
			cluster_bounds(P, cur);
			roots.push_back(cur);
			cur = RootBound();
			cur.first = i + 1;
			break;
		}
		}
	}
	return roots;
}

/* Two spheres instead of one (round 3).  One sphere around a long or L-shaped union is mostly empty.  For a union tree with
 * every k > 0:  smooth_union(a, b, k) >= min(a, b) - k/4, so by induction  value(p) >= min over the LEAVES i of
 * (prim_i(p) - slack_i),  slack_i = the sum of k/4 over the unions above leaf i;  and prim_i(p) >= |p - c_i| - r_i for a sphere
 * (round box: r_i = |b| + r).  Split the leaves into two clusters and let sphere S_j enclose the spheres (c_i, r_i + slack_i) of
 * its cluster: then  value(p) >= min_j (|p - C_j| - R_j)  in exact arithmetic, and the object may be skipped where BOTH of the
 * usual tests pass (make_test: each with the rounding slack of the object's depth).  The split: along the widest axis of the
 * leaf centres, at the position that minimises R_A^3 + R_B^3; used when the larger of the two is at most 0.75 of the single
 * sphere's radius (scene4's blob: 8.6 and 7.8 against 11.1; a numpy model of C3 — tools/cull_model.py — puts the wave-evaluations
 * that may skip the blob at 35 % against 30 %). */
void cluster_bounds(const lol_program& P, RootBound& R) {
	R.clusters.clear();
	if (!R.bounded || R.prims < 3) return;
	std::vector<std::vector<Sphere>> st;
	for (uint32_t i = R.first; i < R.top; i++) {
		const lol_op& o = P.ops[i];
		if (o.op == LOL_OP_SPHERE) st.push_back({ { true, { o.f[0], o.f[1], o.f[2] }, o.f[3] > 0 ? (double)o.f[3] : 0.0, R.levels } });
		else if (o.op == LOL_OP_RBOX) {
			const double hb = sqrt((double)o.f[3] * o.f[3] + (double)o.f[4] * o.f[4] + (double)o.f[5] * o.f[5]);
			st.push_back({ { true, { o.f[0], o.f[1], o.f[2] }, hb * (1.0 + 1e-12) + o.f[6], R.levels } });
		} else if (o.op == LOL_OP_SMIN || o.op == LOL_OP_SMIN_R) {
			std::vector<Sphere> b = std::move(st.back()); st.pop_back();
			std::vector<Sphere>& a = st.back();
			a.insert(a.end(), b.begin(), b.end());
			for (Sphere& l : a) l.r += 0.25 * (double)o.f[0];          /* the slack of this union, for every leaf under it */
		} else return;                                                   /* (a plane: the object has no bound at all) */
	}
	if (st.size() != 1 || st[0].size() < 3 || st[0].size() > 4096) return;      /* (the cut search below is quadratic in the leaves) */
	std::vector<Sphere>& leaves = st[0];
	double mn[3] = { 1e300, 1e300, 1e300 }, mx[3] = { -1e300, -1e300, -1e300 };
	for (const Sphere& l : leaves) for (int a = 0; a < 3; a++) { mn[a] = fmin(mn[a], l.c[a]); mx[a] = fmax(mx[a], l.c[a]); }
	int axis = 0;
	for (int a = 1; a < 3; a++) if (mx[a] - mn[a] > mx[axis] - mn[axis]) axis = a;
	std::stable_sort(leaves.begin(), leaves.end(), [&](const Sphere& x, const Sphere& y) { return x.c[axis] < y.c[axis]; });
	auto hull = [&](size_t lo, size_t hi) { Sphere g = leaves[lo]; for (size_t k = lo + 1; k < hi; k++) g = enclose(g, leaves[k]); g.levels = R.levels; return g; };
	double best = 1e300; size_t cut = 0;
	for (size_t c = 1; c < leaves.size(); c++) {
		const Sphere a = hull(0, c), b = hull(c, leaves.size());
		const double cost = a.r * a.r * a.r + b.r * b.r * b.r;
		if (cost < best) { best = cost; cut = c; }
	}
	const Sphere a = hull(0, cut), b = hull(cut, leaves.size());
	if (!a.ok || !b.ok || !sane(a.r) || !sane(b.r)) return;
	if (fmax(a.r, b.r) > 0.75 * R.r) return;
	R.clusters = { a, b };
}

struct CullTest { float c[3]; float rm; float k; };     /* skip iff u = (best + rm)*k > 0 and |p - c|^2 > u^2 */

/* The in-kernel test's constants from a double-precision bound: centre rounded to binary32 (its rounding error is
 * covered by the |C| 2^-20 term), radius and comparison inflated by the rounding the guarded expression can
 * accumulate.  With D = |p-C|: the exact-arithmetic value is >= D - R; one smooth minimum evaluated in binary32 adds
 * at most 2^-24 (4 M + 8.5 k) to the error of its operands (it is 1-Lipschitz in them), a primitive at most
 * 2^-24 * 4 M, with M <= D + R and k <= 4 R — so the binary32 value is >= D(1 - e) - R(1 + e), e = 40 * 2^-24 * levels.
 * The test gives D > (best + R')K(1 - 2^-21); with K >= 1 + 2e + 2^-19 and R' >= R(1 + 2(K-1) + 2e) that is
 * > best in both signs of best (for best < 0 use |best| < R').  Shallow objects (levels <= 50) keep the constants
 * of the first version, K = 1 + 2^-12 and R' = R(1 + 2^-10): a chain of 500 unions gets K = 1.0024. */
CullTest make_test(const Sphere& b) {
	CullTest t;
	double cmax = 0;
	for (int j = 0; j < 3; j++) { t.c[j] = (float)b.c[j]; cmax = fmax(cmax, fabs(b.c[j])); }
	const double e = 40.0 * 0x1p-24 * (double)b.levels;
	const double K = 1.0 + fmax(0x1p-12, 2.0 * e + 0x1p-19);
	t.k = (float)K;
	if ((double)t.k < K) t.k = nextafterf(t.k, INFINITY);
	const double rho = fmax(0x1p-10, 2.0 * ((double)t.k - 1.0) + 2.0 * e);
	const double rm = b.r * (1.0 + rho) + (cmax + 1.0) * 0x1p-20;
	t.rm = nextafterf((float)rm, INFINITY);
	return t;
}

/* The culling bound carried along a ray (fast SDF, outermost run; emit_sdf).  The march and shadow loops evaluate points
 * p(t) = fl(ro + fl(rd t)) componentwise, at t that never decrease within a loop.  With e = 2^-24, eta = 2^-150 and, for one
 * test (centre C, float; radius rm; factor k), D(t) = |p(t) - C| in real arithmetic:
 *   |p(t) - (ro + rd t)| <= e |rd| t + e |p(t)| + sqrt(3) eta,   |p(t)| <= D(t) + |C|
 *   D(t) (1 + e) >= D(T) (1 - e) - |rd| ((1 + e) t - (1 - e) T) - 2 e |C| - 2 sqrt(3) eta          for t >= T >= 0.
 * The loop checks, per wave, len2(rd) <= 1 + 2^-20 in binary32, which gives |rd| <= rho = 1 + 2^-20.  The skip is allowed when
 * D(t) > (|best| + rm) k: that implies the premise of make_test's proof for best >= 0 and, for best < 0, the premise for
 * best = 0 (value > 0 > best).  Divided by k (1 + e) that is
 *   g(T) + cT T > |best| + ct t,   g(T) = (D(T)(1 - e) - 2e|C| - 2 sqrt(3) eta) / (k (1 + e)) - rm,
 *   cT = rho (1 - e) / (k (1 + e)),  ct = rho / k.
 * At a test the wave passed, D(T) >= s (1 - 2^-20) - 2^-74 for s = v_sqrt_f32(cl) (cl: the test's own binary32 squared length,
 * within (1 + e)^6 and 3 eta of D^2; v_sqrt within 4 ulps), so g(T) >= s A + B per test, and the kernel keeps
 *   lb = G - |G| 2^-20,   G = fma(T, ctt, min_j fma(s_j, A_j, B_j))
 * with ctt = cT (1 - 2^-20): the last factor and the 2^-20 in lb cover the roundings of the three fmas.  At a later t the run is
 * skipped where every lane has fl(fma(t, ctc, |best|)) < lb, ctc = ct (1 + 2^-20).  Constants are rounded towards the safe
 * side.  tests/test_cull_carry_bound.py re-derives them in rational arithmetic and checks the implication there. */
struct CarryConsts { std::vector<float> a, b; float ctt = 0.f, ctc = 0.f; };
static float f_down(double v) { v -= fabs(v) * 0x1p-40; float f = (float)v; if ((double)f > v) f = nextafterf(f, -INFINITY); return f; }
static float f_up(double v) { v += fabs(v) * 0x1p-40; float f = (float)v; if ((double)f < v) f = nextafterf(f, INFINITY); return f; }
CarryConsts carry_constants(const std::vector<CullTest>& tests) {
	const double e = 0x1p-24, rho = 1.0 + 0x1p-20;
	CarryConsts c;
	double ctt = INFINITY, ctc = 0.0;
	for (const CullTest& t : tests) {
		const double k = t.k, cn = sqrt((double)t.c[0] * t.c[0] + (double)t.c[1] * t.c[1] + (double)t.c[2] * t.c[2]) * (1.0 + 0x1p-40);
		c.a.push_back(f_down((1.0 - 0x1p-20) * (1.0 - e) / (k * (1.0 + e))));
		c.b.push_back(f_down(-(double)t.rm - (0x1p-73 + 2.0 * e * cn) / k));
		ctt = fmin(ctt, rho * (1.0 - e) / (k * (1.0 + e)) * (1.0 - 0x1p-20));
		ctc = fmax(ctc, rho / k * (1.0 + 0x1p-20));
	}
	c.ctt = f_down(ctt);
	c.ctc = f_up(ctc);
	return c;
}

/* The object's own last value as a carried bound (fast SDF, outermost run of ONE object; emit_sdf).  An object of spheres and round
 * boxes under smooth unions with k > 0 is 1-Lipschitz in real arithmetic: its primitives are, and sminf(a, b) = b + (a - b) h -
 * k h (1 - h) has the gradient h grad a + (1 - h) grad b wherever h = .5 + .5 (b - a) / k is not clamped (dS/dh = (a - b) -
 * k (1 - 2h) = 0 there) and is a or b where it is.  So with D the object's real value, (C, R) its bounding sphere (analyse_roots:
 * D(p) >= |p - C| - R), x = D(p(t)), y = D(p(T)) and the point roundings of carry_constants (|p| <= |p - C| + |C| <= D + R + |C|):
 *   x (1 + e) >= y (1 - e) - rho ((1 + e) t - (1 - e) T) - 2 e (R + |C|) - 2 sqrt(3) eta                 for t >= T >= 0.
 * The binary32 value of the plain SDF differs from D by at most et (|p - C| + Rm) <= et (D + 2 Rm), et = 40 * 2^-24 * levels
 * (make_test: a primitive 2^-24 * 4M, a smooth minimum 2^-24 (4M + 8.5k) on top of its operands' error, k <= 4R), where M bounds the
 * magnitude of every intermediate value: a leaf's is at most |p - c_i| + m_i <= |p - C| + |C - c_i| + m_i with m_i = |r_i| for a
 * sphere and |b_i| + r_i for a round box.  For radii >= 0 that is within |p - C| + R, but a sphere of NEGATIVE radius is bounded
 * with radius 0 (analyse_roots) while its value is |p - c_i| + |r_i|: so Rm = max(R, max_i (|C - c_i| + m_i)) stands for R in every
 * term below (R <= Rm keeps the point roundings' |p| <= D + R + |C| true as well).  The fast SDF's value V is the plain value or NaN,
 * or the wave shades again (lol_kernel.h, unproven).  Hence y (1 + et) >= V - 2 et Rm, and the plain value at t is >=
 * x (1 - et) - 2 et Rm.  It is > |best| — the object loses eval_dist's minimum and eval's strict '<' and its tie rule alike, for
 * either sign of best — where, with kap = (1 - et) / (1 + e),
 *   g + cT T > |best| + ct t,   g = a V - E,   a = kap (1 - e) / (1 + et),   cT = rho (1 - e) kap,   ct = rho (1 - et),
 *   E = kap (2 et Rm (1 - e) / (1 + et) + 2 e (Rm + |C|) + 2 sqrt(3) eta) + 2 et Rm.
 * After every evaluation of the object at rt = T on a ray that may carry, the kernel folds
 *   lb' = G - |G| 2^-20,   G = fma(T, ctt, fma(|V|, -dl, V) - Ef)
 * into the register of the cluster bound, lb = max(lb', lb) (a NaN V leaves lb: maxf_), with dl >= 1 - a + 4e (V (1 - dl) for
 * V >= 0, V (1 + dl) for V < 0: below a V in both signs, the two roundings of the inner expression included), Ef >= E (1 + 4e) +
 * 2^-100 and ctt = cT (1 - 2^-20); the 2^-20 in lb' covers the roundings of G and of lb' itself.  The check at a later t is the
 * cluster bound's own, fl(fma(t, ctc, |best|)) < lb, with ctc the larger of the two bounds' ct (1 + 2^-20).  Constants are rounded
 * towards the safe side; tests/test_cull_value_carry_bound.py re-derives them in rational arithmetic from the scene's tree. */
struct ValueCarryConsts { float dl = 0.f, ef = 0.f, ctt = 0.f, ctc = 0.f; };
ValueCarryConsts value_carry_constants(const lol_program& P, const RootBound& r) {
	const double e = 0x1p-24, rho = 1.0 + 0x1p-20, et = 40.0 * 0x1p-24 * (double)r.levels;
	const double cn = sqrt(r.c[0] * r.c[0] + r.c[1] * r.c[1] + r.c[2] * r.c[2]) * (1.0 + 0x1p-40);
	double R = r.r;                                                       /* Rm: the bound's radius, or what a leaf's magnitude asks for */
	for (uint32_t i = r.first; i < r.top; i++) {
		const lol_op& o = P.ops[i];
		if (o.op != LOL_OP_SPHERE && o.op != LOL_OP_RBOX) continue;
		const double dx = o.f[0] - r.c[0], dy = o.f[1] - r.c[1], dz = o.f[2] - r.c[2];
		const double m = o.op == LOL_OP_SPHERE ? fabs((double)o.f[3])
		                                       : sqrt((double)o.f[3] * o.f[3] + (double)o.f[4] * o.f[4] + (double)o.f[5] * o.f[5]) + fabs((double)o.f[6]);
		R = fmax(R, (sqrt(dx * dx + dy * dy + dz * dz) + m) * (1.0 + 0x1p-40));
	}
	R *= 1.0 + 0x1p-40;
	const double kap = (1.0 - et) / (1.0 + e), a = kap * (1.0 - e) / (1.0 + et);
	const double E = kap * (2.0 * et * R * (1.0 - e) / (1.0 + et) + 2.0 * e * (R + cn) + 0x1p-73) + 2.0 * et * R;
	ValueCarryConsts c;
	c.dl = f_up(1.0 - a + 4.0 * e);
	c.ef = f_up(E * (1.0 + 4.0 * e) + 0x1p-100);
	c.ctt = f_down(rho * (1.0 - e) * kap * (1.0 - 0x1p-20));
	c.ctc = f_up(rho * (1.0 - et) * (1.0 + 0x1p-20));
	return c;
}

/* The carried bound kept past the march (fast SDF, SdfForm::keep; DESIGN 3.3 "The bound kept past the march").  When the march's
 * loop ends, lb bounds the object along the march's ray from some T <= rt, rt the t of the lane's last evaluation: lb <= L, and
 * L - ct t > |best| at a point p(t), t >= T, is what either proof above asks for (ct = rho gam with gam = 1 - et for the value bound,
 * 1 / k_j for a cluster sphere).  The march ends at p(dist), dist = rt + (its last step), which may lie BEHIND rt; with
 * t* = rt + |dist - rt| one has t* >= |dist| and t* - T >= |dist - T| for every 0 <= T <= rt, and for ANY binary32 point q with
 * |q - p(dist)| <= d0 + nu e |q|  (|q| <= D(q) + R + |C| as above) the triangle inequality through p(dist) gives, for nu <= 3,
 *   plain value at q > |best|   where   |best| < (1 - nu e)(L - ct t*) - gam d0 - nu e B,
 * B >= (Rm + |C|)(1 + 2 et) and >= rm_j + |C_j| for every cluster sphere.  The kernel keeps, per lane,
 *   kb = fl(K1 - Ek),  K1 = fma(|K|, -2^-20, K),  K = fma(ts, -ctc, lb),  ts = fl(rt + |fl(dist - rt)|) >= t* (1 - 2 e)
 * (ctc >= ct (1 + 2^-20) makes ctc ts >= ct t*; K1 <= (L - ct t*)(1 - 2^-21); Ek >= 3 e B + 2^-100, the last for results below the
 * normal range), and the existing check fl(fma(rt, ctc, |best|)) < lb then serves the normal taps q_j = fl(p_j +- h):
 *   d0 = sqrt(3) |h|, nu = 1:      lb = fma(|h|, -c_tap, kb), rt = 0      (fma(0, ctc, |best|) is |best| exactly).
 * Each of the two roundings after K1 raises a positive result by a factor 1 + e at most, and (1 - 2^-21)(1 + e)^2 <= 1 - 2^-22 <=
 * 1 - 3 e; a result that is not positive passes no check.  -inf stays -inf and NaN stays NaN through all of it.
 * (A shadow ray q(t) = fl(ro' + fl(dir t)), ro' = fl(p + dir), has d0 = rho + rho (1 + 3 e) t + 2 sqrt(3) eta and nu = 2 + e, within
 * the same Ek and — asserted below — the same ctc; a hook that started the shadow marches from fl(kb - rho) was built on that and
 * measured: it did not separate from the taps alone and was taken out again)
 * tests/test_cull_kept_bound.py re-derives the constants in rational arithmetic and checks the implication there. */
struct KeepConsts { float ctc = 0.f, ek = 0.f, c_tap = 0.f; bool ok = false; };
KeepConsts keep_constants(const ValueCarryConsts& vc, const std::vector<CullTest>& tests, const lol_program& P, const RootBound& r) {
	const double e = 0x1p-24, rho = 1.0 + 0x1p-20, et = 40.0 * 0x1p-24 * (double)r.levels;
	const CarryConsts cc = carry_constants(tests);
	KeepConsts c;
	c.ctc = vc.ctc > cc.ctc ? vc.ctc : cc.ctc;                           /* the check's own (open_test_carried) */
	double B = 0.0, gam = 1.0 - et;
	{	/* Rm as value_carry_constants takes it */
		const double cn = sqrt(r.c[0] * r.c[0] + r.c[1] * r.c[1] + r.c[2] * r.c[2]) * (1.0 + 0x1p-40);
		double R = r.r;
		for (uint32_t i = r.first; i < r.top; i++) {
			const lol_op& o = P.ops[i];
			if (o.op != LOL_OP_SPHERE && o.op != LOL_OP_RBOX) continue;
			const double dx = o.f[0] - r.c[0], dy = o.f[1] - r.c[1], dz = o.f[2] - r.c[2];
			const double m = o.op == LOL_OP_SPHERE ? fabs((double)o.f[3])
			                                       : sqrt((double)o.f[3] * o.f[3] + (double)o.f[4] * o.f[4] + (double)o.f[5] * o.f[5]) + fabs((double)o.f[6]);
			R = fmax(R, (sqrt(dx * dx + dy * dy + dz * dz) + m) * (1.0 + 0x1p-40));
		}
		B = (R * (1.0 + 0x1p-40) + cn) * (1.0 + 2.0 * et);
	}
	for (const CullTest& t : tests) {
		const double cn = sqrt((double)t.c[0] * t.c[0] + (double)t.c[1] * t.c[1] + (double)t.c[2] * t.c[2]) * (1.0 + 0x1p-40);
		B = fmax(B, (double)t.rm + cn);
		gam = fmax(gam, 1.0 / (double)t.k);
	}
	c.ek = f_up(3.0 * e * B + 0x1p-100);
	c.c_tap = f_up(sqrt(3.0) * (1.0 + 0x1p-40));
	/* the preconditions of the argument above */
	c.ok = !tests.empty() && et < 0x1p-8 && gam <= 1.0 && (double)c.ctc >= rho * gam * (1.0 + 0x1p-21) * (1.0 + 0x1p-40)
	    && std::isfinite(c.ek) && c.ek > 0.f && (double)c.ek >= 3.0 * e * B + 0x1p-100 && (double)c.c_tap * (double)c.c_tap >= 3.0;
	return c;
}

std::vector<CullTest> cluster_tests(const RootBound& r) {
	std::vector<CullTest> t;
	for (const Sphere& c : r.clusters) t.push_back(make_test(c));
	return t;
}

/* A test guards a run of consecutive objects of the evaluation order: [begin, end) positions in `order`.  Runs nest
 * (the run of all bounded objects, inside it spatial clusters, inside those single heavy objects). */
/* `both`: when not empty the run (always a single object) is skipped where ALL of these pass — the object's two cluster
 * spheres — instead of the one test of its enclosing sphere; the interpreter keeps the one sphere (`test`). */
struct CullInterval { size_t begin, end; CullTest test; std::vector<CullTest> both; };

struct CullPlan {
	std::vector<uint32_t> order;          /* evaluation order: indices into the root list */
	size_t   n_unbounded = 0;             /* the first n_unbounded entries of `order` have no bound */
	std::vector<CullInterval> intervals;  /* outer before inner, by position */
	bool     group = false;               /* intervals[0] is the run of ALL bounded objects (what the interpreter carries) */
	CullTest group_test{};
};


/* Objects that lie together are evaluated together, behind a test of their common bounding sphere: a k-d split of
 * the bounded objects (median cut along the widest axis of their centres, down to runs of at most three) gives the
 * evaluation order, and every node of that tree gets a test — single objects too: 11 instructions against a sphere's
 * ~20 with its square root, measured faster on every scene tried (tools/flat_scene_ab.py: leaf sizes 2…8, tests from
 * 1…4 primitives up; profiles/r2_flat_scene_ab.jsonl).  A ray that is far from a whole cluster pays one test for it
 * instead of one evaluation per object — what makes a scene of hundreds of separate objects affordable. */
static void kd_build(const std::vector<RootBound>& roots, std::vector<uint32_t>& ids, size_t lo, size_t hi,
                     size_t base, bool has_predecessor, size_t leaf_max, uint32_t min_prims, CullPlan& plan) {
	const size_t count = hi - lo;
	Sphere g = roots[ids[lo]].sphere();
	uint32_t prims = roots[ids[lo]].prims;
	for (size_t k = lo + 1; k < hi; k++) {
		const RootBound& r = roots[ids[k]];
		g = enclose(g, r.sphere());
		prims += r.prims;
	}
	/* a test needs a running minimum to compare with (something evaluated before the run); a node that covers
	 * exactly what its parent covers adds nothing */
	const bool same_as_parent = !plan.intervals.empty() && plan.intervals.back().begin == base + lo && plan.intervals.back().end == base + hi;
	if ((has_predecessor || lo > 0) && prims >= min_prims && !same_as_parent)
		plan.intervals.push_back({ base + lo, base + hi, make_test(g), count == 1 ? cluster_tests(roots[ids[lo]]) : std::vector<CullTest>() });
	if (count <= leaf_max) {
		if (count > 1)                       /* inside a small run: the objects' own tests */
			for (size_t k = lo; k < hi; k++) {
				const RootBound& r = roots[ids[k]];
				if (r.prims >= min_prims && (has_predecessor || k > 0))
					plan.intervals.push_back({ base + k, base + k + 1, make_test(r.sphere()), cluster_tests(r) });
			}
		return;
	}
	double mn[3] = { 1e300, 1e300, 1e300 }, mx[3] = { -1e300, -1e300, -1e300 };
	for (size_t k = lo; k < hi; k++)
		for (int a = 0; a < 3; a++) { mn[a] = fmin(mn[a], roots[ids[k]].c[a]); mx[a] = fmax(mx[a], roots[ids[k]].c[a]); }
	int axis = 0;
	for (int a = 1; a < 3; a++) if (mx[a] - mn[a] > mx[axis] - mn[axis]) axis = a;
	const size_t mid = lo + count / 2;
	std::nth_element(ids.begin() + lo, ids.begin() + mid, ids.begin() + hi,
	                 [&](uint32_t x, uint32_t y) { return roots[x].c[axis] < roots[y].c[axis] || (roots[x].c[axis] == roots[y].c[axis] && x < y); });
	kd_build(roots, ids, lo, mid, base, has_predecessor, leaf_max, min_prims, plan);
	kd_build(roots, ids, mid, hi, base, has_predecessor, leaf_max, min_prims, plan);
}

CullPlan plan_culling(const std::vector<RootBound>& roots, bool enabled) {
	CullPlan plan;
	std::vector<uint32_t> bounded;
	if (enabled)
		for (uint32_t i = 0; i < roots.size(); i++) (roots[i].bounded ? bounded : plan.order).push_back(i);
	else
		for (uint32_t i = 0; i < roots.size(); i++) plan.order.push_back(i);
	plan.n_unbounded = plan.order.size();
	if (!enabled || bounded.empty()) return plan;
	/* LOL_GPU_CULL_CLUSTERS=0: one run of all bounded objects in scene order, no spatial clusters (for A/B runs) */
	const char* e = tuning_env("LOL_GPU_CULL_CLUSTERS");
	const size_t leaf_max = (e && atoi(e) == 0) ? (size_t)-1 : (e && atoi(e) > 1 ? (size_t)atoi(e) : 3);
	const uint32_t min_prims = 1;      /* every node of the tree gets its test (profiles/r2_flat_scene_ab.jsonl: tests from 1 ... 4 primitives up) */
	kd_build(roots, bounded, 0, bounded.size(), plan.n_unbounded, plan.n_unbounded > 0, leaf_max, min_prims, plan);
	plan.order.insert(plan.order.end(), bounded.begin(), bounded.end());
	/* outer runs before inner ones at the same position (kd_build emits parents first; keep that order stable) */
	std::stable_sort(plan.intervals.begin(), plan.intervals.end(), [](const CullInterval& a, const CullInterval& b) {
		return a.begin < b.begin || (a.begin == b.begin && a.end > b.end);
	});
	if (!plan.intervals.empty() && plan.intervals[0].begin == plan.n_unbounded && plan.intervals[0].end == plan.order.size() &&
	    plan.n_unbounded > 0) {
		plan.group = true;
		plan.group_test = plan.intervals[0].test;
	}
	return plan;
}

/* One walk of a plan for both of its consumers (build_mops and SdfEmitter): per object, in the order of evaluation, the runs that
 * open in front of it — plan.intervals[first_run, first_run + n_open), outer first —, how many runs end behind it (runs nest: they
 * are the innermost n_close of those open), and whether the tie rule applies to it. */
struct PlanStep {
	const RootBound* root = nullptr;
	size_t   first_run = 0;
	uint32_t n_open = 0, n_close = 0;
	bool     tie = false;                 /* evaluated after an object that follows it in the file: a tie goes to the lower id */
};
std::vector<PlanStep> walk_plan(const std::vector<RootBound>& roots, const CullPlan& plan) {
	std::vector<PlanStep> steps(plan.order.size());
	for (const CullInterval& iv : plan.intervals) { steps[iv.begin].n_open++; steps[iv.end - 1].n_close++; }
	size_t next_run = 0;                  /* (plan_culling sorts the runs by where they begin) */
	uint32_t max_id_seen = 0;
	for (size_t oi = 0; oi < steps.size(); oi++) {
		PlanStep& st = steps[oi];
		st.root = &roots[plan.order[oi]];
		st.first_run = next_run;
		next_run += st.n_open;
		st.tie = st.root->id < max_id_seen;
		if (st.root->id > max_id_seen) max_id_seen = st.root->id;
	}
	return steps;
}

/*
 * Post-order program → macro-ops of the interpreter (lol_kernel.h, Interp).  The accumulator is the top of the
 * post-order operand stack:
 *   primitive followed by SMIN / SMIN_R  → one macro-op: x = primitive, combined with acc at once.  In post-order
 *                                           SMIN pops b (top) then a; the primitive is the top, so x = b and the
 *                                           combine is sminf(acc, x); SMIN_R (top is a) gives sminf(x, acc);
 *   primitive otherwise                   → SET when nothing is on the stack yet, else PUSH (acc goes under);
 *   SMIN / SMIN_R after a non-primitive   → x = the popped entry under acc: SMIN has a = x, b = acc → sminf(x, acc);
 *                                           SMIN_R has a = acc, b = x → sminf(acc, x) — a POP record of its own, unless the
 *                                           record before it has a smooth min of the same, proven k: then it rides on that
 *                                           record (MOPB_POST: after the record's own combine);
 *   TOP                                   → a flag on the macro-op that produced the value (+ MOP_TIE where the
 *                                           object is evaluated after one that follows it in the file).
 * The objects come in the order of `plan` (unbounded ones first).  Every test of the plan becomes a constants
 * record in front of the first object of its run (outer runs first); the macro-op that finishes the object before
 * it gets MOPB_CULL_NEXT (the run of all bounded objects) and / or MOPB_CULL_CHAIN (inner runs), and the
 * CULLC_NEXT / CULLC_AFTER flags chain test records that follow one another directly.
 * `fast` lists the smoothness constants whose fast blend factor was proven on the device; allow_nofixup: this list may use the
 * form without v_div_fixup where that was proven too (the caller builds both lists: same records, other smooth-min bits).
 */
std::vector<uint32_t> build_mops(const lol_program& P, const FastPaths* fast, const std::vector<RootBound>& roots,
                                 const CullPlan& plan, bool allow_nofixup) {
	std::vector<uint32_t> out;
	auto fbits32 = [](float v) { uint32_t u; memcpy(&u, &v, 4); return u; };
	auto smin_fields = [&](uint32_t* m, const lol_op& sm) {
		m[9] = fbits32(sm.f[0]);
		if (fast && fast->has(sm.f[0])) {
			m[0] |= lol::MOP_FASTDIV | (allow_nofixup && fast->has_nf(sm.f[0]) ? lol::MOP_NOFIXUP : 0u);
			m[10] = fbits32(2.0f * sm.f[0]);
			m[11] = fbits32(0.5f * (1.0f / sm.f[0]));
		}
		m[0] |= lol::mop_smin_bits(m[0]);
	};
	/* (every test of the plan is kept: leaving out those of runs with few primitives was measured slower here too — a test is one
	 * turn of a scalar loop inside the rare TAIL branch) */
	/* deep: operand stacks beyond the 4-bit slot fields — slots travel in words of their own and pops are not fused (lol_kernel.h, MOP_DEEP_FROM) */
	const bool deep = interp_stack_class(P.max_stack) == lol::MOP_DEEP_SLOTS;
	const bool fuse_pops = !deep && !(tuning_env("LOL_GPU_INTERP_FUSE_POPS") && tuning_env("LOL_GPU_INTERP_FUSE_POPS")[0] == '0');     /* A/B switch */
	const std::vector<CullInterval>& ivs = plan.intervals;
	const bool group_first = plan.group && !ivs.empty() && ivs[0].begin == plan.n_unbounded && ivs[0].end == plan.order.size();
	const std::vector<PlanStep> steps = walk_plan(roots, plan);
	auto opens_at = [&](size_t pos) { return pos < steps.size() ? steps[pos].n_open : 0u; };      /* runs that begin at a position */
	std::vector<size_t> open;                        /* where the constants records of the runs now open went, outer first */
	for (size_t oi = 0; oi < steps.size(); oi++) {
		const PlanStep& st = steps[oi];
		const RootBound& R = *st.root;
		for (uint32_t n = 0; n < st.n_open; n++) {                         /* (never at oi == 0: plan_culling) */
			const CullInterval& iv = ivs[st.first_run + n];
			uint32_t c[lol::MOP_DWORDS] = { 0 };
			c[0] = (n + 1 < st.n_open ? lol::CULLC_NEXT : 0u) | (opens_at(iv.end) ? lol::CULLC_AFTER : 0u);
			for (int j = 0; j < 3; j++) c[2 + j] = fbits32(iv.test.c[j]);
			c[5] = fbits32(iv.test.rm);
			c[6] = fbits32(iv.test.k);
			open.push_back(out.size());
			out.insert(out.end(), c, c + lol::MOP_DWORDS);
		}
		int depth = 0;                                   /* post-order stack depth before the current op */
		bool emitted = false;                            /* this object has a record yet (`last` is one of its own) */
		size_t last = 0;                                 /* start of the macro-op that produced the current acc */
		for (uint32_t i = R.first; i < R.top; i++) {
			const lol_op& o = P.ops[i];
			uint32_t m[lol::MOP_DWORDS] = { 0 };
			if (o.op <= LOL_OP_PLANE) {
				const uint32_t kind = o.op == LOL_OP_SPHERE ? lol::MOP_SPHERE : o.op == LOL_OP_RBOX ? lol::MOP_RBOX : lol::MOP_PLANE;
				for (int j = 0; j < 7; j++) m[2 + j] = fbits32(o.f[j]);
				const lol_op* nx = i + 1 < R.top ? &P.ops[i + 1] : nullptr;
				if (nx && (nx->op == LOL_OP_SMIN || nx->op == LOL_OP_SMIN_R) && depth >= 1) {
					m[0] = lol::mop_header(kind, nx->op == LOL_OP_SMIN ? lol::MOP_SMIN : lol::MOP_SMIN_X);
					smin_fields(m, *nx);
					i++;                                /* the smooth min is part of this macro-op; depth unchanged */
				} else {
					m[0] = lol::mop_header(kind, depth == 0 ? lol::MOP_SET : lol::MOP_PUSH);
					if (depth > 0) {                                                       /* the accumulator goes to this slot */
						if (deep) m[9] = (uint32_t)(depth - 1);
						else m[0] |= (uint32_t)(depth - 1) << lol::MOP_SLOT_SHIFT;
					}
					depth++;
				}
			} else {                                     /* SMIN / SMIN_R on two computed operands */
				/* ... rides on the record that has just finished the second operand when that record's own smooth min has the
				 * same, proven k (the record's k words serve both; lol_kernel.h, MOPB_POST): one record less to fetch and dispatch */
				if (fuse_pops && emitted && (out[last] & lol::MOPB_SMIN) && (out[last] & lol::MOP_FASTDIV) && !(out[last] & lol::MOPB_POST) &&
				    out[last + 9] == fbits32(o.f[0])) {
					out[last] |= lol::MOPB_POST | lol::MOPB_STACK | lol::MOPB_TAIL | (o.op == LOL_OP_SMIN ? lol::MOPB_POST_YA : 0u) |
					             (uint32_t)(depth - 2) << lol::MOP_POST_SLOT_SHIFT;
					depth--;
					continue;
				}
				m[0] = lol::mop_header(lol::MOP_POP, o.op == LOL_OP_SMIN ? lol::MOP_SMIN_X : lol::MOP_SMIN);
				if (deep) m[2] = (uint32_t)(depth - 2);                                         /* the operand under the accumulator */
				else m[0] |= (uint32_t)(depth - 2) << lol::MOP_SLOT_SHIFT;
				smin_fields(m, o);
				depth--;
			}
			last = out.size();
			emitted = true;
			out.insert(out.end(), m, m + lol::MOP_DWORDS);
		}
		out[last] |= lol::MOP_TOP | lol::MOPB_TAIL | (st.tie ? lol::MOP_TIE : 0u);
		out[last + 1] = R.id;
		if (const uint32_t n_next = opens_at(oi + 1)) {
			const bool group_here = group_first && oi + 1 == plan.n_unbounded;
			if (group_here) out[last] |= lol::MOPB_CULL_NEXT;
			if (n_next > (group_here ? 1u : 0u)) out[last] |= lol::MOPB_CULL_CHAIN;
		}
		for (uint32_t n = 0; n < st.n_close; n++) {                        /* every run that ends here: how far its test jumps */
			const size_t at = open.back();
			open.pop_back();
			out[at + 1] = (uint32_t)((out.size() - at) / lol::MOP_DWORDS - 1);
		}
	}
	return out;
}

bool build_interp_lists(const lol_program& P, const FastPaths& fast, bool cull, std::vector<uint32_t>& lists, uint32_t& n_mops) {
	const std::vector<RootBound> roots = analyse_roots(P);
	const CullPlan plan = plan_culling(roots, cull);
	lists = build_mops(P, &fast, roots, plan, false);
	n_mops = (uint32_t)(lists.size() / lol::MOP_DWORDS);
	const std::vector<uint32_t> nofix = build_mops(P, &fast, roots, plan, true);
	if (nofix.size() != lists.size()) return false;
	lists.insert(lists.end(), nofix.begin(), nofix.end());
	return true;
}

/* ------------------------------------------------- the scene's SDF as HIP text (emit_sdf)
 * What form one struct takes: every decision, taken once (decide_form) before any text is written. */
struct SdfForm {
	bool out_of_line = false;       /* the body is ONE real function `<name>_fn` instead of being inlined into every loop (emit_sdf) */
	bool param = false;             /* the structure module's: every number a read K[7 i + j] instead of a literal (emit_sdf) */
	int  fsqrt = 0;                 /* the proven root of the fast SDF's primitives (FastPaths::sqrt_kind), 0: the plain one */
	bool nan_flag = false;          /* spheres may drop the range tracker (sd_sphere_fast_nr) */
	bool carry = false;             /* the culling bound of the outermost run is carried along the ray (carry_constants) */
	bool vcarry = false;            /* ... and the object's own last value is folded into it, with the constants `vc` */
	ValueCarryConsts vc;
	bool vgate = false;             /* ... only at evaluations where some lane's value of the object is not the minimum (decide_form) */
	int  keep = 0;                  /* ... and what the march leaves in lb is kept past loop_done(), a mask: 1 for the normal taps */
	KeepConsts kc;                  /*     (keep_constants) */
	bool last_id = false;           /* ID_FROM_LAST: a third body, eval_rec(), and the id decided once after the march */
	int  sat_cull_min_prims = 32;   /* operands of a smooth union from this many primitives on get a saturation test; 0: none */
	int  cooldown = 3;              /* evaluations that do not test again after a test that did not allow the skip */
};

SdfForm decide_form(const lol_program& P, const FastPaths* fast, bool out_of_line, bool param, const std::vector<RootBound>& roots,
                    const CullPlan& plan) {
	SdfForm f;
	f.out_of_line = out_of_line;
	f.param = param;
	f.fsqrt = fast ? fast->sqrt_kind : 0;
	/* spheres of radius >= 2^-20 carry no range tracker where the device has shown the fast root harmless below its proven domain
	 * (lol_kernel.h, sd_sphere_fast_nr): a NaN reaches the object's value instead, which is looked at once */
	f.nan_flag = fast && fast->sqrt_tiny_ok;
	/* In the inlined fast SDF, the culling bound carried along the ray (carry_constants): `lb` per lane, `rt` the t of the
	 * point being evaluated, `carry` whether this loop's ray may set lb (ray_begin; lol_kernel.h, march / soft_shadow).  Out of
	 * line the body keeps the plain test: its state would be per call.  By default only where the outermost run is ONE object behind
	 * its two cluster spheres: measured on one box, six alternating repetitions (profiles/r7_ab_cull_carry.txt), scene4 C3
	 * +5.5 %, orbit +2.7 %, but scene.lol's group of three objects (C2) -2.7 %: its rays keep failing the group test, and the
	 * carried check is one fma, a compare and a branch more on every test.  LOL_GPU_CULL_CARRY=0 / 1: off / on wherever inlined. */
	f.carry = fast && !out_of_line && !plan.intervals.empty();
	if (const char* e = tuning_env("LOL_GPU_CULL_CARRY")) f.carry = f.carry && atoi(e) != 0;
	else f.carry = f.carry && !plan.intervals[0].both.empty();
	/* ... and the object's own last value folded into the same lb (value_carry_constants), where the carry is on and the outermost run
	 * is ONE object: a run of several would need every object's bound per step, which is what cost scene.lol's group 2.7 % with the
	 * cluster carry.  The carried check then comes BEFORE the cool-down counter: the evaluations taken under cool-down refresh lb, and
	 * the first step at which the object has stopped winning is skipped without waiting for the counter to run out.
	 * LOL_GPU_CULL_VALUE_CARRY=0 / 1: off / on (still only for a single object behind a carried bound). */
	f.vcarry = f.carry && plan.intervals[0].end == plan.intervals[0].begin + 1 && roots[plan.order[plan.intervals[0].begin]].bounded;
	if (const char* e = tuning_env("LOL_GPU_CULL_VALUE_CARRY")) f.vcarry = f.vcarry && atoi(e) != 0;
	if (f.vcarry) f.vc = value_carry_constants(P, roots[plan.order[plan.intervals[0].begin]]);
	/* ... and that fold only at evaluations where it can matter.  In a lane where the object's value V is the minimum of the
	 * evaluation at T, V is the step the loop takes (march: dist += d; soft_shadow: t + s), so every later point of this ray has
	 * t >= fl(T + V) >= (T + V)(1 - 2^-24) — or V < 0 and the loop ends.  What the fold would leave is lb' <= ctt T + V (1 - dl) - Ef,
	 * and a later check fl(fma(t, ctc, |best|)) < lb' needs ctc t (1 - 2^-24) < lb': impossible once ctc (1 - 2^-24)^2 >= ctt and
	 * >= 1 - dl (scene4: 0.9999924 against 0.9999903 and 0.9999806).  So the fold is dead in that lane for good, and it is left
	 * out where EVERY lane in EXEC has V <= the minimum of the other objects: one compare and a scalar branch instead of four
	 * full-rate and two half-rate instructions after most evaluations (tests/tools/bound_upkeep_model.py: 71 % of the march's and
	 * 81 % of the shadow loops' evaluations of scene4's blob, none of the skips lost).  Leaving a fold out is always allowed — lb stays
	 * a bound, only an older one — so nothing here is needed for exactness: the two inequalities only say that nothing is lost.
	 * Where: the carried object is the LAST of the plan, so that `best` before its join is the minimum of all the others, and the
	 * inequalities hold for the constants written; anywhere else the fold stays unconditional.
	 * (`lhs` below: the product is taken in double, and the factor 1 - 2^-40 stands for the roundings of its three multiplications,
	 * so that the comparison errs to the side of the unconditional fold.)
	 * LOL_GPU_CULL_UPDATE_GATED=0 / 1 beside LOL_GPU_TUNING: off / on (still only where eligible). */
	if (f.vcarry) {
		const CullInterval& iv = plan.intervals[0];
		const double ctc = fmax((double)f.vc.ctc, (double)carry_constants(iv.both.empty() ? std::vector<CullTest>{ iv.test } : iv.both).ctc);
		const double lhs = ctc * (1.0 - 0x1p-24) * (1.0 - 0x1p-24) * (1.0 - 0x1p-40);
		f.vgate = iv.begin + 1 == plan.order.size() && lhs >= (double)f.vc.ctt && lhs >= 1.0 - (double)f.vc.dl;
	}
	if (const char* e = tuning_env("LOL_GPU_CULL_UPDATE_GATED")) f.vgate = f.vgate && atoi(e) != 0;
	/* ... and the bound the march ends with kept for the points the pixel evaluates next (keep_constants): loop_done() forgets lb, and
	 * the four normal taps then run the two-sphere test again — and the blob itself where the loose spheres fail — for points that lie
	 * within sqrt(3) h of the march's end.  The struct gets hooks beside ray_begin / ray_at (lol_kernel.h: bound_keep, taps_begin /
	 * taps_done) which set lb and rt so that the ONE carried check of the bodies decides; eval() and eval_dist() are the text they
	 * were.  Where the value carry is on and keep_constants' preconditions hold.  LOL_GPU_CULL_KEEP=<mask> beside LOL_GPU_TUNING: bit 1
	 * the taps; with the bit clear the source is what it was.  (Bit 2 was the start of the shadow marches while that was measured; it
	 * names nothing now and is ignored.) */
	if (f.vcarry) {
		const CullInterval& iv = plan.intervals[0];
		f.kc = keep_constants(f.vc, iv.both.empty() ? std::vector<CullTest>{ iv.test } : iv.both, P, roots[plan.order[iv.begin]]);
		f.keep = f.kc.ok ? 1 : 0;
	}
	if (const char* e = tuning_env("LOL_GPU_CULL_KEEP")) f.keep = f.keep & atoi(e);
	/* ID_FROM_LAST, for the inlined fast SDF of a scene of exactly TWO top-level objects — the scenes that keep the id in their march
	 * (ASK_ID_ONCE, SdfEmitter::head_inlined); every other scene keeps its source byte for byte.  The primary march evaluates through
	 * eval_rec(): the distance alone, like eval_dist(), plus a RECORD — each object's value at this step per lane, +inf for an object
	 * the culling skipped — and decides the id once, after the loop, from the record of the lane's own last step (lol_kernel.h, march;
	 * id_of).  Per step: one v_min_f32 per object instead of the compares and selects of the strict-'<' / lower-id rule.
	 * What it rests on: an object's value that is NaN or infinite re-shades the wave through the plain pipeline — every value
	 * recorded goes through nanacc = fma(value, 0, nanacc) (lol_kernel.h, unproven) — so the rules only have to agree for finite
	 * values, where "the lowest id among the objects at the minimum" IS what the strict '<' and the lower-id tie rule of eval()
	 * leave, in any evaluation order (-0 == +0 in both).  They differ for t = +inf alone (t < +inf is false: eval() keeps id 0) and
	 * for NaN.  A skipped object's plain value strictly loses (the tests of SdfEmitter), which is what its +inf in the record says.
	 * Measured on one box, six alternating repetitions (profiles/r19_ab_last_step_id.txt): scene4 C3 +0.9 %.
	 * LOL_GPU_LAST_STEP_ID=0 beside LOL_GPU_TUNING: off.
	 * Only for scenes of at most 32 ops (the scenes that keep 8 waves per SIMD, register_budget): eval_rec() is a third copy of the
	 * inlined body, and what it saves per step is a fixed couple of dozen cycles — 6 % of a step of scene4's 12 ops, under 1 % of a
	 * step of a hundred, for a third more code to fetch. */
	f.last_id = fast && !out_of_line && !param && P.n_roots == 2 && P.n_ops <= 32;
	if (const char* e = tuning_env("LOL_GPU_LAST_STEP_ID")) f.last_id = f.last_id && atoi(e) != 0;
	/* LOL_GPU_SAT_CULL_MIN_PRIMS: `a` operands of a smooth union with at least this many primitives get a saturation-
	 * culling test (SdfEmitter::emit_sat_culled_union); 0 = none.  Measured (tools/tree_scene_ab.py, balanced trees of spheres at
	 * 1080p, profiles/r2_tree_scene_ab.jsonl): the 17-instruction test pays from a few dozen primitives — 128 spheres
	 * 232 -> 405 Mpixels/s, 256 spheres 127 -> 166 at 32 (375 / 157 at 16); with a test on every operand scene4
	 * loses 14 %, a 32-sphere tree 30 %. */
	if (const char* e = tuning_env("LOL_GPU_SAT_CULL_MIN_PRIMS")) f.sat_cull_min_prims = atoi(e);
	/* After a test that did not allow the skip, the next `cooldown` evaluations of this SDF object do not test
	 * again (a ray that is near the object now is near it on its next steps too): the test costs 11 VALU
	 * instructions, and where it keeps failing that is pure overhead.  Never testing is always allowed — the
	 * test only ever permits a skip — so this changes no result.  `cool` lives in the Sdf struct, wave-uniform;
	 * only the outermost test keeps one. */
	f.cooldown = 3;
	return f;
}

/* An object's expression tree from its post-order ops (child `a` / `b` = the operands of sminf(a, b, k)), each node with the
 * bounding sphere of what is under it (analyse_roots' rules) for the saturation test. */
struct Node { uint32_t op; int a, b; Sphere bound; uint32_t prims; bool fon = false; };      /* fon: the fast SDF's value of this node is finite or NaN */
std::vector<Node> object_nodes(const lol_program& P, const RootBound& R, const FastPaths* fast, const SdfForm& f) {
	std::vector<Node> nodes;
	std::vector<int> st;
	for (uint32_t i = R.first; i < R.top; i++) {
		const lol_op& o = P.ops[i];
		Node n{ i, -1, -1, { false, { 0, 0, 0 }, 0, 1 }, 1 };
		if (o.op == LOL_OP_SPHERE) {
			n.fon = f.fsqrt && f.nan_flag && o.f[3] >= 0x1p-20f && std::isfinite(o.f[3]);      /* sd_sphere_fast_nr (emit_node) */
			n.bound = { sane(o.f[0]) && sane(o.f[1]) && sane(o.f[2]) && sane(o.f[3]), { o.f[0], o.f[1], o.f[2] }, o.f[3] > 0 ? (double)o.f[3] : 0.0, 1 };
		} else if (o.op == LOL_OP_RBOX) {
			bool ok = true;
			for (int j = 0; j < 7; j++) ok = ok && sane(o.f[j]);
			ok = ok && o.f[3] >= 0 && o.f[4] >= 0 && o.f[5] >= 0 && o.f[6] >= 0;
			const double hb = sqrt((double)o.f[3] * o.f[3] + (double)o.f[4] * o.f[4] + (double)o.f[5] * o.f[5]);
			n.bound = { ok, { o.f[0], o.f[1], o.f[2] }, hb * (1.0 + 1e-12) + o.f[6], 1 };
		} else if (o.op == LOL_OP_SMIN || o.op == LOL_OP_SMIN_R) {
			const int top = st.back(); st.pop_back();
			const int under = st.back(); st.pop_back();
			n.a = o.op == LOL_OP_SMIN ? under : top;
			n.b = o.op == LOL_OP_SMIN ? top : under;
			n.bound = enclose(nodes[n.a].bound, nodes[n.b].bound);
			if (!(sane(o.f[0]) && o.f[0] > 0)) n.bound.ok = false;
			n.bound.r += 0.25 * (double)o.f[0];
			n.bound.levels++;
			if (!sane(n.bound.r)) n.bound.ok = false;
			n.prims = nodes[n.a].prims + nodes[n.b].prims;
			n.fon = nodes[n.a].fon && nodes[n.b].fon && fast && fast->has(o.f[0]);
		}
		st.push_back((int)nodes.size());
		nodes.push_back(n);
	}
	return nodes;
}

/* The body is emitted once per pass where it is inlined: eval() — distance and object id — for the primary march and the normal
 * taps, and eval_dist() — the distance alone — for the shadow marches, which never look at the id.  There an object joins the running
 * minimum with ONE v_min_f32 instead of the compare(s) and selects of the strict-'<' / lower-id-wins rule: the two agree on the
 * value except for the sign of a zero (two objects at distance -0 and +0 of the same point), and a shadow march's results —
 * its factor maxf(res, 0) and its step count — are the same for s = -0 and s = +0: t + s, 50 s / t compared with 0, and
 * maxf(+-0, 0) = +0 all are (lol_kernel.h, soft_shadow).  A NaN value is dropped by either form.
 * ... and once more for an ID_FROM_LAST scene: eval_rec(), eval_dist() plus the record of each object's value (SdfForm::last_id).
 * Out of line there is the one function, which is eval(). */
enum class Pass { Eval, EvalDist, EvalRec };

/* The writer of one struct: the form, the plan's walk, the text so far, and the counters of the pass being written. */
struct SdfEmitter {
	std::string& s;
	const lol_program& P;
	const char* name;
	const FastPaths* fast;
	const std::vector<RootBound>& roots;
	const CullPlan& plan;
	const SdfForm f;
	const std::vector<PlanStep> steps;
	std::string fs;                       /* "_fast<n>": the suffix of the primitives with the proven root (run) */
	int  t = 0, n_tests = 0;             /* the next temporary and the next test of this pass: t<n>, cl<n> / sl<n> */
	bool object_has_nr = false;           /* the object being written has a value that is voted on for NaN (emit_node) */

	/* number j of op i: a literal, or the structure module's read of it */
	std::string num(uint32_t i, int j) const {
		if (!f.param) return fbits(P.ops[i].f[j]);
		std::string k;
		appendf(k, "K[%u]", (unsigned)lol::OP_NUMBERS * i + (unsigned)j);
		return k;
	}
	/* only the outermost test keeps a cool-down counter (wave-uniform state in the Sdf struct) */
	const char* cool_decl() const { return plan.intervals.empty() ? "" : "\tu32 cool[1] = {};\n"; }
	int rec_slot(size_t oi) const { return roots[plan.order[oi]].id > roots[plan.order[oi ^ 1]].id ? 1 : 0; }      /* (two objects) */

	/* ---- the struct's head */
	void head_out_of_line() {
		/* out of line the cool-down state is per call (always 0: every evaluation tests) */
		/* (amdgpu_waves_per_eu applies to kernels only: the function is scheduled with the default register budget) */
		appendf(s, "__device__ __noinline__ SdfOut %s_fn(float px, float py, float pz, u32 rg_lo, u32 rg_hi) {\n"
		        "\t\tconst V3 p = { px, py, pz };\n\t\tRange rg; rg.lo = rg_lo; rg.hi = rg_hi;\n\t\tfloat nanacc = 0.f;\n\t\tfloat best; u32 best_id;\n\t%s",
		        name, cool_decl());
	}
	void head_inlined() {
		const char* carry_decl = !f.carry ? "" :
			"\tfloat lb = -__builtin_inff(), rt = 0.f;\n\tbool carry = false;\n"
			"\t__device__ __forceinline__ void ray_begin(V3 rd) { carry = vote(!(len2(rd) <= 0x1.00001p+0f)) == 0; }\n"
			"\t__device__ __forceinline__ void ray_at(float t) { rt = t; }\n";
		/* ASSUME_SETTLED: the fast pipeline only runs under FLAG_SHADOW_SETTLED (generate_source; lol_kernel.h, soft_shadow).
		 * loop_done(): what the wave-uniform cool-down counter is after a loop that lanes leave one by one (lol_kernel.h, Interp) */
		/* ASK_ID_ONCE: the primary march evaluates the distance alone and asks for the id of its last step once (lol_kernel.h,
		 * march) — from three top-level objects on, where a v_min per object and step outweighs the one evaluation more per pixel
		 * (measured: scene.lol's four objects +3.6 %, scene4's two -0.8 %; profiles/r6_ab_id_asked_once.txt) */
		appendf(s, "struct %s {\n\tstatic constexpr bool ASSUME_SETTLED = %s;\n\tstatic constexpr bool ASK_ID_ONCE = %s;\n\tRange rg;\n\tfloat nanacc = 0.f;\n%s%s"
		        "\t__device__ __forceinline__ void loop_done() { %s%s }\n", name, fast ? "true" : "false", P.n_roots >= 3 ? "true" : "false", cool_decl(),
		        carry_decl, plan.intervals.empty() ? "" : "cool[0] = 0u;", f.carry ? " lb = -__builtin_inff(); carry = false;" : "");
		if (f.keep) keep_hooks();
		if (f.param) s += "\tparam_ptr K = nullptr;\n";
		if (f.last_id) {
			/* the record's two slots in the order of the ids: rec0 the object of the lower id, which a tie goes to */
			const uint32_t ida = roots[0].id, idb = roots[1].id;
			appendf(s, "\tstatic constexpr bool ID_FROM_LAST = true;\n"
			        "\t__device__ __forceinline__ u32 id_of(float rec0, float rec1) const { return rec0 == vmin_(rec0, rec1) ? %uu : %uu; }\n",
			        ida < idb ? ida : idb, ida < idb ? idb : ida);
		}
	}

	/* what the march leaves in lb, kept for the normal taps and the shadow rays (SdfForm::keep, keep_constants): bound_keep() is
	 * called with the march's dist before loop_done() and returns kb, -inf where nothing was carried; taps_begin() turns the carried
	 * check into |best| < kb - c_tap |h| (rt = 0; carry = false: a passed full test sets nothing, no fold runs), taps_done() forgets it */
	void keep_hooks() {
		appendf(s, "\t__device__ __forceinline__ float bound_keep(float dist) const {\n"
		        "\t\tconst float ts = rt + __builtin_fabsf(dist - rt);\n\t\tconst float kg = __builtin_fmaf(ts, -%s, lb);\n"
		        "\t\treturn __builtin_fmaf(__builtin_fabsf(kg), -0x1p-20f, kg) - %s;\n\t}\n", fbits(f.kc.ctc).c_str(), fbits(f.kc.ek).c_str());
		appendf(s, "\t__device__ __forceinline__ void taps_begin(float h, float kb) { lb = __builtin_fmaf(__builtin_fabsf(h), -%s, kb); rt = 0.f; carry = false; }\n"
		        "\t__device__ __forceinline__ void taps_done() { lb = -__builtin_inff(); }\n", fbits(f.kc.c_tap).c_str());
	}

	/* ---- one pass */
	void pass_prologue(Pass pass) {
		if (!f.out_of_line)
			s += pass == Pass::EvalRec    ? "\t__device__ __forceinline__ void eval_rec(V3 p, float& best, float& rec0, float& rec1) {\n"
			   : pass == Pass::EvalDist ? "\t__device__ __forceinline__ void eval_dist(V3 p, float& best) {\n"
			                            : "\t__device__ __forceinline__ void eval(V3 p, float& best, u32& best_id) {\n";
		s += pass == Pass::Eval ? "\t\tbest = __builtin_inff(); best_id = 0u;\n" : "\t\tbest = __builtin_inff();\n";
		if (pass != Pass::EvalRec) return;
		/* an object behind a test that lets the wave skip it is recorded as +inf: it strictly loses */
		for (size_t oi = 0; oi < plan.order.size(); oi++)
			for (const CullInterval& iv : plan.intervals)
				if (iv.begin <= oi && oi < iv.end) {
					appendf(s, "\t\trec%d = __builtin_inff();\n", rec_slot(oi));
					break;
				}
	}
	void emit_pass(Pass pass) {
		pass_prologue(pass);
		t = 0;
		n_tests = 0;
		for (size_t oi = 0; oi < steps.size(); oi++) emit_object(pass, oi);
		if (!f.out_of_line) s += "\t}\n";
	}
	void emit_object(Pass pass, size_t oi) {
		const PlanStep& st = steps[oi];
		for (uint32_t n = 0; n < st.n_open; n++) {                            /* outer runs first */
			const size_t run = st.first_run + n;
			if (run != 0) open_test_plain(plan.intervals[run]);
			else if (f.carry) open_test_carried(plan.intervals[run]);
			else open_test_cooldown(plan.intervals[run]);
		}
		const std::vector<Node> nodes = object_nodes(P, *st.root, fast, f);
		object_has_nr = false;
		const int d = emit_node(nodes, (int)nodes.size() - 1);
		const bool rec = pass == Pass::EvalRec;
		/* a NaN from a sphere without range tracker reaches the object's value: 0 * NaN (or inf) = NaN (... and every value the record takes) */
		if (object_has_nr || rec) appendf(s, "\t\tnanacc = __builtin_fmaf(t%d, 0.f, nanacc);\n", d);
		if (rec) appendf(s, "\t\trec%d = t%d;\n", rec_slot(oi), d);
		const bool folds = f.vcarry && oi == plan.intervals[0].begin;
		if (folds && f.vgate) value_carry_gate(d);
		join_minimum(pass, st, d);
		if (folds) value_carry_update(d);
		for (uint32_t n = 0; n < st.n_close; n++) s += "\t\t} }\n";           /* every run that ends here */
	}

	/* ---- the tests in front of a run.  One test = one bounding sphere; a run guarded by several (an object's two cluster spheres)
	 * is skipped where ALL pass.  This writes their declarations into `decl` and the votes that say "some lane needs the run" into
	 * `votes`, and returns the number of the first. */
	static std::vector<CullTest> tests_of(const CullInterval& iv) { return iv.both.empty() ? std::vector<CullTest>{ iv.test } : iv.both; }
	int declare_tests(const std::vector<CullTest>& tests, std::string& decl, std::string& votes) {
		const int k0 = n_tests;
		for (const CullTest& ct : tests) {
			const int k = n_tests++;
			appendf(decl,
			        "\t\t  const float cx%d = p.x - %s, cy%d = p.y - %s, cz%d = p.z - %s;\n"
			        "\t\t  const float cl%d = (cx%d * cx%d + cy%d * cy%d) + cz%d * cz%d;\n"
			        "\t\t  const float cu%d = (best + %s) * %s;\n",
			        k, fbits(ct.c[0]).c_str(), k, fbits(ct.c[1]).c_str(), k, fbits(ct.c[2]).c_str(),
			        k, k, k, k, k, k, k, k, fbits(ct.rm).c_str(), fbits(ct.k).c_str());
			appendf(votes, "%svote(!(cl%d > cu%d * cu%d)) | vote(!(cu%d > 0.f))", votes.empty() ? "" : " | ", k, k, k, k);
		}
		return k0;
	}
	/* an inner run: tested at every evaluation */
	void open_test_plain(const CullInterval& iv) {
		std::string decl, votes;
		declare_tests(tests_of(iv), decl, votes);
		s += "\t\t{\n" + decl + "\t\t  if (((" + votes + ")) != 0) {\n";
	}
	/* the outermost run: tested unless the cool-down counter runs (SdfForm::cooldown) */
	void open_test_cooldown(const CullInterval& iv) {
		std::string decl, votes;
		const int k0 = declare_tests(tests_of(iv), decl, votes);
		appendf(s, "\t\t{ bool need%d = true;\n\t\t  if (cool[0] == 0u) {\n", k0);
		s += decl;
		appendf(s, "\t\t  need%d = ((", k0);
		s += votes;
		appendf(s, ")) != 0;\n\t\t  if (need%d) cool[0] = %du;\n\t\t  } else cool[0]--;\n\t\t  if (need%d) {\n", k0, f.cooldown, k0);
	}
	/* the outermost run of a struct that carries its bound: the carried bound first (one fma and one compare); where a lane fails it,
	 * the full test — which, passed by the whole wave on a ray that may carry, sets lb anew (one v_sqrt per sphere).  A failed full
	 * test leaves lb as it is: still a bound, only an older one.  With the value carry the carried check comes before the counter
	 * (SdfForm::vcarry) and the new bound joins lb by maxf_. */
	void open_test_carried(const CullInterval& iv) {
		const std::vector<CullTest> tests = tests_of(iv);
		std::string decl, votes;
		const int k0 = declare_tests(tests, decl, votes);
		const CarryConsts cc = carry_constants(tests);
		const float ctc = f.vcarry && f.vc.ctc > cc.ctc ? f.vc.ctc : cc.ctc;      /* one left-hand side for both bounds: the more conservative */
		if (f.vcarry)
			appendf(s, "\t\t{ bool need%d = true;\n\t\t  {\n"
			        "\t\t  if (vote(!(__builtin_fmaf(rt, %s, __builtin_fabsf(best)) < lb)) == 0) need%d = false; else if (cool[0] == 0u) {\n",
			        k0, fbits(ctc).c_str(), k0);
		else
			appendf(s, "\t\t{ bool need%d = true;\n\t\t  if (cool[0] == 0u) {\n"
			        "\t\t  if (vote(!(__builtin_fmaf(rt, %s, __builtin_fabsf(best)) < lb)) == 0) need%d = false; else {\n",
			        k0, fbits(ctc).c_str(), k0);
		s += decl;
		appendf(s, "\t\t  need%d = ((", k0);
		s += votes;
		appendf(s, ")) != 0;\n\t\t  if (need%d) cool[0] = %du;\n\t\t  else if (carry) {\n", k0, f.cooldown);
		for (size_t j = 0; j < tests.size(); j++) {
			if (j) appendf(s, "\t\t    lm = vmin_(__builtin_fmaf(__builtin_amdgcn_sqrtf(cl%d), %s, %s), lm);\n",
			               k0 + (int)j, fbits(cc.a[j]).c_str(), fbits(cc.b[j]).c_str());
			else   appendf(s, "\t\t    float lm = __builtin_fmaf(__builtin_amdgcn_sqrtf(cl%d), %s, %s);\n",
			               k0 + (int)j, fbits(cc.a[j]).c_str(), fbits(cc.b[j]).c_str());
		}
		if (f.vcarry)
			appendf(s, "\t\t    const float lg = __builtin_fmaf(rt, %s, lm);\n\t\t    lb = maxf_(__builtin_fmaf(__builtin_fabsf(lg), -0x1p-20f, lg), lb);\n"
			        "\t\t  }\n\t\t  } else cool[0]--; }\n\t\t  if (need%d) {\n", fbits(cc.ctt).c_str(), k0);
		else
			appendf(s, "\t\t    const float lg = __builtin_fmaf(rt, %s, lm);\n\t\t    lb = __builtin_fmaf(__builtin_fabsf(lg), -0x1p-20f, lg);\n"
			        "\t\t  }\n\t\t  } } else cool[0]--;\n\t\t  if (need%d) {\n", fbits(cc.ctt).c_str(), k0);
	}

	/* ---- an object's expression: one SSA temporary per node, returned by number */
	/* what the call of one smooth minimum is written with: k, 2k, 1/(2k) and the saturation threshold as text, "<false>" where the
	 * form without v_div_fixup is proven, and whether the call takes the threshold */
	struct SminText { std::string k, k2, hrk, ks; const char* fx; bool sat_arith; };
	int emit_node(const std::vector<Node>& nodes, int ni) {
		const Node& n = nodes[ni];
		const lol_op& o = P.ops[n.op];
		switch (o.op) {
		case LOL_OP_SPHERE:
			if (n.fon) {                                       /* sd_sphere_fast_nr: no range tracker (SdfForm::nan_flag) */
				appendf(s, "\t\tconst float t%d = sd_sphere_fast_nr<%d>(p, %s, %s, %s, %s);\n", t, f.fsqrt,
				        fbits(o.f[0]).c_str(), fbits(o.f[1]).c_str(), fbits(o.f[2]).c_str(), fbits(o.f[3]).c_str());
				object_has_nr = true;
			} else
				appendf(s, "\t\tconst float t%d = sd_sphere%s(p, %s, %s, %s, %s%s);\n", t, fs.c_str(),
				        num(n.op, 0).c_str(), num(n.op, 1).c_str(), num(n.op, 2).c_str(), num(n.op, 3).c_str(), f.fsqrt ? ", rg" : "");
			return t++;
		case LOL_OP_RBOX:
			appendf(s, "\t\tconst float t%d = sd_round_box%s(p, %s, %s, %s, %s, %s, %s, %s%s);\n", t, fs.c_str(),
			        num(n.op, 0).c_str(), num(n.op, 1).c_str(), num(n.op, 2).c_str(), num(n.op, 3).c_str(),
			        num(n.op, 4).c_str(), num(n.op, 5).c_str(), num(n.op, 6).c_str(), f.fsqrt ? ", rg" : "");
			return t++;
		case LOL_OP_PLANE:
			appendf(s, "\t\tconst float t%d = p.y - %s;\n", t, num(n.op, 0).c_str());
			return t++;
		default: break;
		}
		/* LOL_OP_SMIN / LOL_OP_SMIN_R */
		const float ks = smooth_sat_threshold(o.f[0]);
		const bool proven = fast && fast->has(o.f[0]);
		/* without v_div_fixup where that is proven too; such an object's value is then voted on for NaN (an infinite
		 * operand difference — lol_kernel.h, smin_h_fast) like one with spheres that carry no range tracker */
		const char* fx = proven && fast->has_nf(o.f[0]) ? "<false>" : "";
		if (fx[0]) object_has_nr = true;
		/* (sat_arith) the arithmetic shortcut only where the SDF is inlined: in the out-of-line function its four-way branching
		 * costs more than it saves (504-op chain: 100 -> 42 Mpixels/s) */
		const SminText m{ num(n.op, 0), fbits(2.0f * o.f[0]), fbits(0.5f * (1.0f / o.f[0])), fbits(ks), fx, !f.out_of_line && ks > 0.f };
		if (proven && ks > 0.f && f.sat_cull_min_prims > 0 && nodes[n.a].bound.ok && nodes[n.a].prims >= (uint32_t)f.sat_cull_min_prims)
			return emit_sat_culled_union(nodes, n, m);
		/* operands in program order (a flattened chain keeps its deep operand first and its operand stack shallow) */
		const bool a_first = o.op == LOL_OP_SMIN;
		const int first = emit_node(nodes, a_first ? n.a : n.b), second = emit_node(nodes, a_first ? n.b : n.a);
		const int a = a_first ? first : second, b = a_first ? second : first;
		if (proven && m.sat_arith)
			appendf(s, "\t\tconst float t%d = sminf_fastdiv_sat%s%s(t%d, t%d, %s, %s, %s, %s);\n", t,
			        nodes[n.a].fon && nodes[n.b].fon ? "2" : "", fx, a, b, m.k.c_str(), m.k2.c_str(), m.hrk.c_str(), m.ks.c_str());
		else if (proven)
			appendf(s, "\t\tconst float t%d = sminf_fastdiv%s(t%d, t%d, %s, %s, %s);\n", t, fx, a, b, m.k.c_str(), m.k2.c_str(), m.hrk.c_str());
		else
			appendf(s, "\t\tconst float t%d = sminf_(t%d, t%d, %s);\n", t, a, b, m.k.c_str());
		return t++;
	}
	/* Saturation culling inside a smooth union (fast struct only, proven k > 0): sminf(a, b, k) is EXACTLY
	 * b - dlt*0.f = b + 0.f when dlt = b - a <= -ks (sminf_fastdiv_sat), so operand `a` need not be evaluated
	 * where it is provably that much greater than b.  b is evaluated first; with sb = fl(b + ks) the bounding-
	 * sphere test of the top-level culling (best := sb) gives a > sb for the binary32 value of `a`, hence
	 * dlt = fl(b - a) <= fl(b - sb) =: sw by the monotonicity of rounding, and sw <= -ks is checked directly;
	 * |p - C|^2 < 2^120 keeps every primitive of `a` (all within R < 10^15 of C) finite, so dlt is finite and
	 * dlt*0.f = -0.  A NaN or infinite b fails the comparisons.  Per wave, like every other skip. */
	int emit_sat_culled_union(const std::vector<Node>& nodes, const Node& n, const SminText& m) {
		const int b = emit_node(nodes, n.b);
		const CullTest ct = make_test(nodes[n.a].bound);
		const int r = t++, q = n_tests++;
		appendf(s,
		        "\t\tfloat t%d;\n"
		        "\t\t{ const float sb%d = t%d + %s, sw%d = t%d - sb%d;\n"
		        "\t\t  const float sx%d = p.x - %s, sy%d = p.y - %s, sz%d = p.z - %s;\n"
		        "\t\t  const float sl%d = (sx%d * sx%d + sy%d * sy%d) + sz%d * sz%d;\n"
		        "\t\t  const float su%d = (sb%d + %s) * %s;\n"
		        "\t\t  if ((vote(!(sl%d > su%d * su%d)) | vote(!(su%d > 0.f)) | vote(!(sw%d <= -%s)) | vote(!(sl%d < 0x1p120f))) != 0) {\n",
		        r, q, b, m.ks.c_str(), q, b, q,
		        q, fbits(ct.c[0]).c_str(), q, fbits(ct.c[1]).c_str(), q, fbits(ct.c[2]).c_str(),
		        q, q, q, q, q, q, q,
		        q, q, fbits(ct.rm).c_str(), fbits(ct.k).c_str(),
		        q, q, q, q, q, m.ks.c_str(), q);
		const int a = emit_node(nodes, n.a);
		if (m.sat_arith)
			appendf(s, "\t\t  t%d = sminf_fastdiv_sat%s(t%d, t%d, %s, %s, %s, %s);\n\t\t  } else t%d = t%d + 0.f;\n\t\t}\n",
			        r, m.fx, a, b, m.k.c_str(), m.k2.c_str(), m.hrk.c_str(), m.ks.c_str(), r, b);
		else
			appendf(s, "\t\t  t%d = sminf_fastdiv%s(t%d, t%d, %s, %s, %s);\n\t\t  } else t%d = t%d + 0.f;\n\t\t}\n",
			        r, m.fx, a, b, m.k.c_str(), m.k2.c_str(), m.hrk.c_str(), r, b);
		return r;
	}

	/* ---- how the object's value t<d> joins the running minimum */
	void join_minimum(Pass pass, const PlanStep& st, int d) {
		const uint32_t id = st.root->id;
		if (pass != Pass::Eval)
			appendf(s, "\t\tbest = vmin_(t%d, best);\n", d);
		else if (st.tie)                  /* evaluated after an object that follows it in the file: ties go to the lower id */
			appendf(s, "\t\tif (t%d < best || (t%d == best && best_id > %uu)) { best = t%d; best_id = %uu; }\n", d, d, id, d, id);
		else
			appendf(s, "\t\tif (t%d < best) { best = t%d; best_id = %uu; }\n", d, d, id);
	}
	/* (SdfForm::vgate) before the join, where `best` is still the minimum of the other objects: from here to the end of the run's block
	 * `carry` is a local that shadows the member — "this ray may carry AND some lane's value of the object is not its minimum" —
	 * and the fold below, the only thing in that block that reads it, is written as it always was */
	void value_carry_gate(int d) {
		appendf(s, "\t\tconst bool carry = this->carry && vote(t%d > best) != 0;\n", d);
	}
	/* the value just computed bounds the object further along the ray (value_carry_constants) */
	void value_carry_update(int d) {
		appendf(s, "\t\tif (carry) {\n\t\t  const float vg = __builtin_fmaf(rt, %s, __builtin_fmaf(__builtin_fabsf(t%d), -%s, t%d) - %s);\n"
		        "\t\t  lb = maxf_(__builtin_fmaf(__builtin_fabsf(vg), -0x1p-20f, vg), lb);\n%s\t\t}\n",
		        fbits(f.vc.ctt).c_str(), d, fbits(f.vc.dl).c_str(), d, fbits(f.vc.ef).c_str(),
		        f.vgate ? "\t\t  asm volatile(\"\");\n" : "");      /* (gated: keep the branch, or the fold comes back as a select) */
	}

	/* ---- what closes the struct */
	void epilogue() {
		if (f.out_of_line) {
			s += "\t\treturn { best, best_id, rg.lo, rg.hi, nanacc };\n}\n";
			appendf(s, "struct %s {\n\tstatic constexpr bool ASSUME_SETTLED = %s;\n\tstatic constexpr bool ASK_ID_ONCE = false;\n\tRange rg;\n\tfloat nanacc = 0.f;\n"
			        "\t__device__ __forceinline__ void loop_done() {}\n"
			        "\t__device__ __forceinline__ void eval(V3 p, float& best, u32& best_id) {\n"
			        "\t\tconst SdfOut o = %s_fn(p.x, p.y, p.z, rg.lo, rg.hi);\n"
			        "\t\tbest = o.best; best_id = o.id; rg.lo = o.lo; rg.hi = o.hi; nanacc += o.nanacc;\n\t}\n"
			        "\t__device__ __forceinline__ void eval_dist(V3 p, float& best) { u32 unused; eval(p, best, unused); }\n", name, fast ? "true" : "false", name);
		}
		/* the arithmetic of the shading around the loops that the device has proven for the fast pipeline (lol_kernel.h, ShadeMath); a
		 * struct without it — the plain SDF, LOL_GPU_SHADE_MATH=0 — is the text it was */
		if (fast && fast->shade_root) appendf(s, "\tstruct Shade { static constexpr int ROOT = %d, RCP = %d; };\n", fast->shade_root, fast->shade_rcp);
		s += "};\n";
	}

	/* the passes in the order in which they stand in the struct: eval_rec() first where there is one, then eval(), then eval_dist() */
	void run() {
		if (f.fsqrt) appendf(fs, "_fast<%d>", f.fsqrt);
		if (f.out_of_line) head_out_of_line(); else head_inlined();
		if (f.last_id) emit_pass(Pass::EvalRec);
		emit_pass(Pass::Eval);
		if (!f.out_of_line) emit_pass(Pass::EvalDist);
		epilogue();
	}
};

/* Emits one `struct <name>` with eval(): one SSA temporary per op, same operation order WITHIN every top-level object
 * as the post-order program; the objects themselves in the order of `plan` (file order when culling is off).
 * out_of_line: the body becomes ONE real function (`<name>_fn`, __noinline__) that the march, normal and shadow
 * loops call, instead of being inlined into each of them — for large scenes, whose straight-line SDF would
 * otherwise be replicated six times (three loops x fast / exact) and outgrow the instruction cache.
 * `param` (the structure module, generate_structure_source: fast == nullptr, an empty plan, inlined): every number of the scene is
 * not a literal but a read K[7 i + j] of op i's f[j] through the member pointer K — the source then depends on the structure alone. */
void emit_sdf(std::string& s, const lol_program& P, const char* name, const FastPaths* fast, bool out_of_line,
              const std::vector<RootBound>& roots, const CullPlan& plan, bool param = false) {
	SdfEmitter em{ s, P, name, fast, roots, plan, decide_form(P, fast, out_of_line, param, roots, plan), walk_plan(roots, plan) };
	em.run();
}
bool spec_out_of_line(const lol_program& P, int form) {
	if (form == SPEC_OUT_OF_LINE) return true;
	if (form == SPEC_INLINE) return false;
	uint32_t limit = LOL_SPEC_INLINE_MAX_OPS;
	if (const char* e = tuning_env("LOL_GPU_SPEC_INLINE_MAX")) limit = (uint32_t)strtoul(e, nullptr, 10);
	return P.n_ops > limit;
}

/* Register budget, as the attribute of every kernel of a scene's modules.  The SDF of one object is a long dependent chain (every
 * smooth min waits for the one below it) fed by independent primitives, and the kernel is compiled with the max-ILP scheduling
 * strategy (compile_source): the more registers a wave may use, the more primitives it keeps in flight.  Measured on
 * MI355X (profiles/r2_large_scene_ab.jsonl): with max-ILP, scene4 (12 ops) is fastest when 8 waves per SIMD are
 * kept (64 VGPRs: 4640 vs 4530 Mpixels/s unconstrained), a 44-op chain at >= 6, chains of 142+ ops at >= 4
 * (128 VGPRs: 427 vs 400 Mpixels/s at 8). */
static std::string register_budget(const lol_program& P) {
	const int waves_lo = P.n_ops <= 32 ? 8 : P.n_ops <= 96 ? 6 : 4, waves_hi = 8;
	return " __attribute__((amdgpu_waves_per_eu(" + std::to_string(waves_lo) + ", " + std::to_string(waves_hi) + ")))";
}

std::string generate_source(const lol_program& P, const FastPaths* fast, bool cull, int form = SPEC_BY_SIZE, ModuleKernels carries = {}) {
	std::string s;
	const FamilyRow* K = KERNEL_FAMILIES;
	const bool ool = spec_out_of_line(P, form);
	const std::vector<RootBound> roots = analyse_roots(P);
	const CullPlan plan = plan_culling(roots, cull);
	/* the header of a switch's block (MODULE_SWITCHES) */
	auto include = [](ModuleSwitch sw) { return std::string("#include \"") + MODULE_SWITCHES[sw].header + "\"\n"; };
	s += include(SWITCH_NONE);
	s += "namespace lol {\n";
	const std::string occupancy = register_budget(P);
	if (ool) s += "struct SdfOut { float best; u32 id; u32 lo, hi; float nanacc; };\n";
	emit_sdf(s, P, "SpecSdfExact", nullptr, ool, roots, plan);
	const bool any_fast = fast && (fast->sqrt_kind || !fast->div_ok.empty());
	if (any_fast) emit_sdf(s, P, "SpecSdfFast", fast, ool, roots, plan);
	s += "}  // namespace lol\n";
	/* where lights / materials are read from is a property of the scene too (lol_kernel.h, TABLES_LDS_MAX_DWORDS) */
	const bool tables_global = !lol::tables_in_lds(P.n_lights, P.n_materials, P.n_roots);
	const std::string tg = tables_global ? "true" : "false";
	/* The pipeline once as a template on COUNT (lol_kernel.h, march: the per-lane step counters), and as one or two kernels:
	 *   lol_render_spec_steps  counts steps: frames with diagnostics (lol_gpu_debug::steps) and the one frame of a view that records
	 *                          what its pixels cost (lol_gpu.hip, "pixels dealt by cost");
	 *   lol_render_spec        does not (+1.3 % on C3): every other frame.
	 * A scene above LOL_SPEC_TWO_KERNELS_MAX_OPS gets the counting kernel alone, under the name lol_render_spec: a second copy of
	 * its pipeline would nearly double what the compiler takes for it. */
	const bool two = P.n_ops <= LOL_SPEC_TWO_KERNELS_MAX_OPS;
	/* what every kernel begins with: lights, materials and root materials staged in LDS, where the scene keeps them there */
	const std::string stage = tables_global ? "" : "\tlol::stage_common(L, lds);\n\t__syncthreads();\n";
	/* P = the lane's pixel or sample of launch `of`: shaded with the fast SDF, and again with the exact one where the wave left what
	 * was proven.  The fast pipeline takes FLAG_SHADOW_SETTLED for granted (lol_kernel.h, soft_shadow): a launch without it — `flags`
	 * names the one that says; for a batch the VIEW's, so that a camera beyond the sane range in the middle of a batch takes the plain
	 * pipeline — is the plain pipeline's.  `in`: indentation; `count`: shade_pixel's COUNT; `decl`: how a scene without a fast SDF
	 * declares P in the statement that shades it, or "": on a line of its own first, as the fast form always does. */
	auto shade = [&](const std::string& in, const std::string& flags, const std::string& of, const std::string& count, const std::string& decl) {
		const std::string args = tg + ", " + count + ">(" + of + ", ";
		std::string b;
		if (any_fast || decl.empty()) b += in + "lol::Pixel P;\n";
		if (any_fast) {
			b += in + "bool plain = !(" + flags + ".flags & lol::FLAG_SHADOW_SETTLED);\n";
			b += in + "if (!plain) {\n";
			b += in + "\tlol::SpecSdfFast fast;\n";
			b += in + "\tP = lol::shade_pixel<lol::SpecSdfFast, " + args + "fast, lds);\n";
			b += in + "\tplain = lol::unproven(fast);\n";
			b += in + "}\n";
			b += in + "if (plain) {\n";
			b += in + "\tlol::SpecSdfExact exact;\n";
			b += in + "\tP = lol::shade_pixel<lol::SpecSdfExact, " + args + "exact, lds);\n";
			b += in + "}\n";
		} else {
			b += in + "lol::SpecSdfExact exact;\n";
			b += in + (decl.empty() ? "P = " : decl) + "lol::shade_pixel<lol::SpecSdfExact, " + args + "exact, lds);\n";
		}
		return b;
	};
	s += "template <bool COUNT> __device__ __forceinline__ void lol_spec_body(const lol::Launch& L, lol::u32* lds) {\n" + stage;
	s += "\tif (!lol::start_tile_clock<" + tg + ">(L, lds)) return;\n";
	s += shade("\t", "L", "L", "COUNT", "lol::Pixel P = ");
	s += "\tlol::store_pixel<" + tg + ">(L, P, lds);\n";
	s += "}\n";
	const std::string head = "extern \"C\" __global__ __launch_bounds__(lol::BLOCK)" + occupancy + " void ";
	const std::string tail = "(const lol::Launch L) {\n\textern __shared__ lol::u32 lds[];\n\tlol_spec_body<";
	if (two) s += head + K[FAM_FRAME].counting + tail + "true>(L, lds);\n}\n";
	s += head + K[FAM_FRAME].symbol + tail + (two ? "false" : "true") + ">(L, lds);\n}\n";
	/* the SDF alone at arbitrary points (lol_gpu_sdf_batch) */
	s += "extern \"C\" __global__ __launch_bounds__(64) void lol_sdf_spec(const float* pts, float* dist, lol::u32* id, lol::u32 n) {\n";
	s += "\tlol::SpecSdfExact exact;\n";
	if (any_fast) s += "\tlol::SpecSdfFast fast;\n\tlol::sdf_points(fast, exact, true, pts, dist, id, n);\n";
	else          s += "\tlol::sdf_points(exact, exact, false, pts, dist, id, n);\n";
	s += "}\n";
	/* Supersampling (lol_gpu_set_samples before the upload): the same pipeline with one lane per sample and the mean of each pixel's
	 * samples stored (lol_kernel.h, store_pixel_aa), s read at run time.  Appended, so that a module without it is the same source
	 * — and the same code object and kernel_key — as before supersampling existed.  No step counters: hit_dist, hit_id and steps
	 * have no single value for a pixel of several samples (lol_gpu_render_device refuses them). */
	if (carries.carries(SWITCH_AA)) {
		s += include(SWITCH_AA);
		s += head + K[FAM_FRAME_AA].symbol + "(const lol::Launch L) {\n\textern __shared__ lol::u32 lds[];\n" + stage;
		s += "\tconst lol::Launch S = lol::sample_launch(L);\n";
		s += shade("\t", "L", "S", "false", "");
		s += "\tlol::store_pixel_aa<" + tg + ">(L, P.rgb);\n";
		s += "}\n";
		/* the refine pass of adaptive frames (lol_gpu_set_adaptive_samples): the same pixel for a list of pixels */
		s += head + K[FAM_FRAME_AA_LIST].symbol + "(const lol::Launch L, const lol::u32* list, const lol::u32* count) {\n";
		s += "\textern __shared__ lol::u32 lds[];\n" + stage;
		s += "\tlol::render_aa_list<" + tg + ">(L, list, count, [&](const lol::Launch& S) {\n";
		s += shade("\t\t", "L", "S", "false", "");
		s += "\t\treturn P;\n";
		s += "\t});\n";
		s += "}\n";
	}
	/* Batches of views (lol_gpu_set_view_batches before the upload): the same pipeline on the launch of the block's view
	 * (lol_kernel_batch.h), stored at that view's address.  Appended after everything else, for the reason above.  With and without
	 * the step counters like the frame kernel: a batch with lol_gpu_debug::steps runs the counting twin. */
	if (carries.carries(SWITCH_BATCH)) {
		s += include(SWITCH_BATCH);
		s += "template <bool COUNT> __device__ __forceinline__ void lol_spec_batch_body(const lol::Launch& L, const lol::BatchTail& B, lol::u32* lds) {\n" + stage;
		s += "\tconst lol::Launch S = lol::view_launch(L, B.views);\n";
		s += shade("\t", "S", "S", "COUNT", "const lol::Pixel P = ");
		s += "\tlol::store_pixel_view(L, B, P);\n";
		s += "}\n";
		const std::string btail = "(const lol::Launch L, const lol::BatchTail B) {\n\textern __shared__ lol::u32 lds[];\n\tlol_spec_batch_body<";
		if (two) s += head + K[FAM_BATCH].counting + btail + "true>(L, B, lds);\n}\n";
		s += head + K[FAM_BATCH].symbol + btail + (two ? "false" : "true") + ">(L, B, lds);\n}\n";
	}
	/* Supersampled batches (lol_gpu_set_view_samples before the upload; the batch kernels above come with it: the first pass of an
	 * adaptive batch is theirs): the pipeline on the sample grid of the block's view, every pixel's samples reduced before the
	 * store (lol_kernel_batch_aa.h), and the same for the per-view lists of an adaptive batch.  Appended after everything else,
	 * for the reason above.  No step counters. */
	if (carries.carries(SWITCH_BATCH_AA)) {
		s += include(SWITCH_BATCH_AA);
		s += head + K[FAM_BATCH_AA].symbol + "(const lol::Launch L, const lol::BatchTail B) {\n\textern __shared__ lol::u32 lds[];\n" + stage;
		s += "\tconst lol::Launch S = lol::sample_launch(lol::view_launch(L, B.views));\n";
		s += shade("\t", "S", "S", "false", "");
		s += "\tlol::store_pixel_view_aa(L, B, P.rgb);\n";
		s += "}\n";
		s += head + K[FAM_BATCH_AA_LIST].symbol + "(const lol::Launch L, const lol::BatchTail B, const lol::BatchLists Q) {\n";
		s += "\textern __shared__ lol::u32 lds[];\n" + stage;
		s += "\tlol::render_aa_view_lists<" + tg + ">(L, B, Q, [&](const lol::Launch& S) {\n";
		s += shade("\t\t", "S", "S", "false", "");
		s += "\t\treturn P;\n";
		s += "\t});\n";
		s += "}\n";
	}
	/* Views averaged over K cameras (lol_gpu_set_view_blends before the upload): the batch pipeline on the launch of the block's
	 * record, the clamped LINEAR colour stored into the blend's scratch instead of a packed pixel (lol_kernel_blend.h).  Appended
	 * after everything else, for the reason above.  No step counters. */
	if (carries.carries(SWITCH_BATCH_BLEND)) {
		s += include(SWITCH_BATCH_BLEND);
		s += head + K[FAM_BATCH_LIN].symbol + "(const lol::Launch L, const lol::BatchTail B) {\n\textern __shared__ lol::u32 lds[];\n" + stage;
		s += "\tconst lol::Launch S = lol::view_launch(L, B.views);\n";
		s += shade("\t", "S", "S", "false", "");
		s += "\tlol::store_linear_view(L, P.rgb);\n";
		s += "}\n";
	}
	/* Supersampled blends (lol_gpu_set_view_blend_samples before the upload, a switch of its own): lol_render_spec_batch_aa's
	 * pipeline on the sample grid of the block's record, every pixel's samples reduced to their LINEAR mean and that stored into
	 * the blend's scratch (lol_kernel_blend_aa.h).  Appended after everything else, for the reason above.  No step counters. */
	if (carries.carries(SWITCH_BATCH_BLEND_AA)) {
		s += include(SWITCH_BATCH_BLEND_AA);
		s += head + K[FAM_BATCH_AA_LIN].symbol + "(const lol::Launch L, const lol::BatchTail B) {\n\textern __shared__ lol::u32 lds[];\n" + stage;
		s += "\tconst lol::Launch S = lol::sample_launch(lol::view_launch(L, B.views));\n";
		s += shade("\t", "S", "S", "false", "");
		s += "\tlol::store_linear_view_aa(L, P.rgb);\n";
		s += "}\n";
	}
	/* Ray queries (lol_gpu_set_ray_queries before the upload): get_intersection and get_normal for a list of rays or of pixels, one
	 * lane per ray, one wave per block (lol_kernel_rays.h) — no Launch, no LDS, no tables.  Appended after everything else, for the
	 * reason above.  The name does not begin with lol_render_spec: it is no frame. */
	if (carries.carries(SWITCH_RAYS)) {
		s += include(SWITCH_RAYS);
		s += "extern \"C\" __global__ __launch_bounds__(64)" + occupancy + " void lol_trace_spec(const lol::RayQuery Q) {\n";
		s += "\tlol::SpecSdfExact exact;\n";
		if (any_fast) s += "\tlol::SpecSdfFast fast;\n\tlol::trace_rays(fast, exact, true, Q);\n";
		else          s += "\tlol::trace_rays(exact, exact, false, Q);\n";
		s += "}\n";
	}
	/* Shading queries (lol_gpu_set_shade_queries before the upload): the frames' pipeline for a list of rays or of pixels, one lane per
	 * ray (lol_kernel_shade.h) — a Launch for the scene's half and a ShadeQuery behind it; which SDF and which shadow loop a wave may
	 * run is decided in shade_rays.  One counting form.  Appended after everything else, for the reason above. */
	if (carries.carries(SWITCH_SHADE)) {
		s += include(SWITCH_SHADE);
		s += head + "lol_shade_spec(const lol::Launch L, const lol::ShadeQuery Q) {\n\textern __shared__ lol::u32 lds[];\n" + stage;
		s += "\tlol::SpecSdfExact exact;\n";
		if (any_fast) s += "\tlol::SpecSdfFast fast;\n\tlol::shade_rays<" + tg + ">(fast, exact, true, L, Q, lds);\n";
		else          s += "\tlol::shade_rays<" + tg + ">(exact, exact, false, L, Q, lds);\n";
		s += "}\n";
	}
	return s;
}

using lol_key::fnv64;
static std::string hex16(unsigned long long h) {
	std::string b;
	appendf(b, "%016llx", h);
	return b;
}
std::string fnv_hex(const void* data, size_t n) { return hex16(fnv64(data, n)); }
/* the key of a code object: what the device loads of it (lol_code_key.h) */
std::string code_key_hex(const void* code, size_t n) { return hex16(lol_key::code_key(code, n)); }

/* Process-wide cache of compiled kernels: hosts (and the tests) upload the same scene many times. */
std::mutex g_cache_mutex;
std::unordered_map<std::string, std::vector<char>> g_code_cache;

/* ... and a cache on disk, so that the N ranks of a multi-GPU run (and the next run of the same host) do not each
 * pay the 0.3 - 1 s hipRTC compile of the same scene.  One file per key under LOL_GPU_CACHE_DIR (default
 * $XDG_CACHE_HOME/lol_gpu or $HOME/.cache/lol_gpu; set it to the empty string to switch the disk cache off): the
 * file holds the full key in front of the code object and is only used when that key matches byte for byte, so a
 * hash collision or a stale file can never hand out the wrong kernel; writes go through a temporary name + rename.
 * Any I/O failure simply means "not cached". */
std::string disk_cache_path(const std::string& key) {
	const char* e = getenv("LOL_GPU_CACHE_DIR");
	std::string dir;
	if (e) { if (!e[0]) return ""; dir = e; }
	else if (const char* x = getenv("XDG_CACHE_HOME")) { if (!x[0]) return ""; dir = std::string(x) + "/lol_gpu"; }
	else if (const char* h = getenv("HOME")) { if (!h[0]) return ""; dir = std::string(h) + "/.cache/lol_gpu"; }
	else return "";
	for (size_t i = 1; i <= dir.size(); i++)              /* mkdir -p */
		if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0700);
	unsigned long long h = 0xcbf29ce484222325ull;         /* FNV-1a of the key names the file */
	for (unsigned char c : key) { h ^= c; h *= 0x100000001b3ull; }
	appendf(dir, "/%016llx.co", h);
	return dir;
}

/* GPU code is only ever loaded from a file this user wrote: the file and its directory must belong to the effective
 * user and must not be writable by group or others (a shared LOL_GPU_CACHE_DIR / XDG_CACHE_HOME would otherwise let
 * another user plant kernels), and the code object must match the checksum stored next to it. */
bool private_to_user(const struct stat& st) { return st.st_uid == geteuid() && !(st.st_mode & (S_IWGRP | S_IWOTH)); }

bool disk_cache_load(const std::string& key, std::vector<char>& code) {
	const std::string path = disk_cache_path(key);
	if (path.empty()) return false;
	struct stat dir_st, file_st;
	const std::string dir = path.substr(0, path.rfind('/'));
	if (stat(dir.c_str(), &dir_st) != 0 || !S_ISDIR(dir_st.st_mode) || !private_to_user(dir_st)) return false;
	FILE* f = fopen(path.c_str(), "rb");
	if (!f) return false;
	bool ok = false;
	unsigned long long klen = 0, clen = 0, sum = 0;
	if (fstat(fileno(f), &file_st) == 0 && S_ISREG(file_st.st_mode) && private_to_user(file_st) &&
	    fread(&klen, 8, 1, f) == 1 && fread(&clen, 8, 1, f) == 1 && fread(&sum, 8, 1, f) == 1 &&
	    klen == key.size() && clen > 0 && clen < (1ull << 28)) {
		std::string k(klen, 0);
		code.resize(clen);
		ok = fread(&k[0], 1, klen, f) == klen && k == key && fread(code.data(), 1, clen, f) == clen && fnv64(code.data(), clen) == sum;
	}
	fclose(f);
	return ok;
}

void disk_cache_store(const std::string& key, const std::vector<char>& code) {
	const std::string path = disk_cache_path(key);
	if (path.empty()) return;
	std::string t = path;
	appendf(t, ".%ld.tmp", (long)getpid());
	FILE* f = fopen(t.c_str(), "wb");
	if (!f) return;
	(void)fchmod(fileno(f), 0600);
	const unsigned long long klen = key.size(), clen = code.size(), sum = fnv64(code.data(), code.size());
	const bool ok = fwrite(&klen, 8, 1, f) == 1 && fwrite(&clen, 8, 1, f) == 1 && fwrite(&sum, 8, 1, f) == 1 &&
	                fwrite(key.data(), 1, klen, f) == klen && fwrite(code.data(), 1, clen, f) == clen;
	if (fclose(f) != 0 || !ok || rename(t.c_str(), path.c_str()) != 0) (void)remove(t.c_str());
}

/* The long-branch bug described in compile_spec, as it looks in the code: a relaxed branch that goes through s[30:31], the
 * register pair a function RETURNS through —
 *     s_getpc_b64 s[30:31];  s_add_u32 s30, s30, <lit>;  s_addc_u32 s31, s31, <lit>;  s_setpc_b64 s[30:31]
 * (a call is s_getpc into some OTHER pair + s_swappc_b64 s[30:31], <pair>; a return is a bare s_setpc_b64 s[30:31] with no
 * s_getpc of that pair before it).  Recognised by instruction fields, not by four literal words (round-4 review): SOP1
 * s_getpc_b64 with SDST = s30, followed within a few instructions by SOP1 s_setpc_b64 with SSRC0 = s30 and no s_swappc_b64
 * in between — whatever arithmetic (add / sub, literal in either source position, a scavenged temporary, s_nop padding)
 * sits between the two.  The words are read with memcpy at EVERY byte offset: no assumption about where the buffer or the
 * text section inside the ELF begins, and nothing that can make the check pass by default.  A false alarm — constants that
 * happen to spell the two instructions eight dwords apart — only costs the scene its own kernel (the interpreter renders). */
bool has_return_clobbering_branch(const void* data, size_t n_bytes) {
	constexpr uint32_t SOP1 = 0xBE800000u, SOP1_MASK = 0xFF800000u;         /* [31:23] = 0b1_0111_1101 */
	constexpr uint32_t OP_GETPC = 28, OP_SETPC = 29, OP_SWAPPC = 30;        /* SOP1 opcodes (GFX9 / gfx950 encoding), bits [15:8] */
	constexpr uint32_t RETURN_PAIR = 30;                                    /* s[30:31] */
	constexpr size_t WINDOW = 12;                                           /* dwords after the s_getpc in which the s_setpc counts */
	const unsigned char* b = static_cast<const unsigned char*>(data);
	auto word = [&](size_t at) { uint32_t w; memcpy(&w, b + at, 4); return w; };
	for (size_t at = 0; at + 8 <= n_bytes; at++) {
		const uint32_t w = word(at);
		if ((w & SOP1_MASK) != SOP1 || ((w >> 8) & 0xFF) != OP_GETPC || ((w >> 16) & 0x7F) != RETURN_PAIR) continue;
		for (size_t k = 1; k <= WINDOW && at + 4 * k + 4 <= n_bytes; k++) {
			const uint32_t v = word(at + 4 * k);
			if ((v & SOP1_MASK) != SOP1) continue;
			const uint32_t op = (v >> 8) & 0xFF;
			if (op == OP_SWAPPC) break;                                     /* a call: the pair is being written as a link register */
			if (op == OP_SETPC && (v & 0xFF) == RETURN_PAIR) return true;
		}
	}
	return false;
}
bool has_return_clobbering_branch(const std::vector<char>& code) { return has_return_clobbering_branch(code.data(), code.size()); }

/* `src` → code object.  out_of_line: the source holds an out-of-line SDF function (what the refusal after dropped options is about).
 * structure: the source is a structure module's (generate_structure_source), which is handed lol_kernel_scenes.h as well (1), and
 * with the supersampled kernels lol_kernel_scenes_aa.h too (2) — a scene module, and a structure module without them, is handed
 * exactly the headers it always was, so what the compiler makes of it and where the disk cache keeps it do not change. */
static bool compile_source(const std::string& src, bool out_of_line, int structure, const std::string& arch, std::vector<char>& code,
                           std::string& log) {
	int rtc_major = 0, rtc_minor = 0;
	(void)hiprtcVersion(&rtc_major, &rtc_minor);
	/* the option list first: it is part of the cache key (a changed flag — -ffp-contract above all — must never be served
	 * a code object compiled under the old one) */
	std::string arch_opt = "--offload-arch=" + arch;
	/* -ffp-contract=off: no FMA contraction (the reference has none); the rest are hipcc's defaults made explicit */
	/* -fno-slp-vectorize: the SLP pass pairs scalar f32 ops into v_pk_*_f32, which issue at half the
	 * rate of two scalar ops on gfx950 (tools/valu_rate.hip); measured +10 % Mpixels/s without it. */
	/* -amdgpu-sched-strategy=max-ilp: schedule for instruction-level parallelism within a wave rather than for
	 * occupancy.  The default strategy serialises the independent primitives of a long smooth-union chain to save
	 * registers; with max-ILP the same instructions run 1.4x faster on 142 - 1024-op scenes and 2 - 5 % faster on the
	 * example scenes (generate_source sets the matching register budget).  Scheduling only: same instructions, same bits.
	 * An LLVM that does not know an -mllvm option ends the PROCESS from its option parser, so the option is only
	 * passed to hipRTC versions it was verified on (hiprtcVersion >= 9.0 = ROCm 7.x); LOL_GPU_SCHED=default leaves it out. */
	std::vector<const char*> opts = { arch_opt.c_str(), "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
	                                  "-fno-slp-vectorize" };
	const char* sched = tuning_env("LOL_GPU_SCHED");
	if (rtc_major >= 9 && !(sched && !strcmp(sched, "default"))) {
		opts.push_back("-mllvm"); opts.push_back("-amdgpu-sched-strategy=max-ilp");
		/* ... and no post-RA scheduling pass: it re-orders the ILP-friendly schedule after register allocation and
		 * costs 10 % on C3 (4650 -> 5150 Mpixels/s without it, same box and call; nothing on the large scenes) */
		opts.push_back("-mllvm"); opts.push_back("-enable-post-misched=0");
		/* ... and SimplifyCFG may turn small two-sided branches into selects more readily (default threshold 2): the per-lane
		 * `if (alive) { ... }` updates around the SDF become straight-line code for the ILP scheduler.  Sweep of 3 ... 64 on one
		 * box (tools/rtc_flag_sweep.sh phi): from 4 upwards C2 +1.5 ... 2.5 %, C3 +0.2 %, the large scenes +-3 %; same bits. */
		opts.push_back("-mllvm"); opts.push_back("-phi-node-folding-threshold=8");
		/* ... and NO register reserved ahead of time for long branches.  An out-of-line SDF function of more than 128 KB (about
		 * 800 ops: a field of 600 objects) has forward branches beyond s_cbranch's 16-bit reach; LLVM's AMDGPU backend then
		 * reserves "an unused" SGPR pair for the s_getpc / s_add / s_setpc sequence before register allocation — and in a leaf
		 * function picks s[30:31], the RETURN ADDRESS: the function jumps, and at its end "returns" to the branch target for
		 * ever (found in round 4 when scenes lost their 1024-op capacity: the kernel never finished; ROCm 7.0 and 7.2 alike).
		 * With the factor 0 no register is reserved and the branch relaxation scavenges a dead one at the branch, correctly.
		 * has_return_clobbering_branch() below refuses any code object that still shows the pattern. */
		opts.push_back("-mllvm"); opts.push_back("-amdgpu-long-branch-factor=0");
	}
	/* ... and so is the compiler: which libhiprtc this process has loaded.  A Python host gets the one torch ships, a C host the
	 * system's, a process under rocprofv3 yet another mix — the same source came out as three different code objects — and one
	 * compiler's output must not be handed to a process that would have compiled something else.
	 * LOL_GPU_CACHE_ANY_COMPILER=1 leaves the compiler out of the key: a profiling aid (tools/final_profile.sh lets a plain run
	 * compile the kernels, and the runs under the profiler load exactly those). */
	std::string compiler = "?";
	{
		Dl_info info;
		if (dladdr(reinterpret_cast<void*>(&hiprtcCompileProgram), &info) && info.dli_fname) compiler = info.dli_fname;
		compiler = std::to_string(rtc_major) + "." + std::to_string(rtc_minor) + " " + compiler;
		const char* any = tuning_env("LOL_GPU_CACHE_ANY_COMPILER");
		if (any && any[0] == '1') compiler = "*";         /* its version too: torch's hipRTC and the system's differ in it */
	}
	std::string key = "lol_gpu/4|hiprtc " + compiler + "|";
	for (const char* o : opts) { key += o; key += ' '; }
	key += "|" + src;
	{
		std::lock_guard<std::mutex> lock(g_cache_mutex);
		auto it = g_code_cache.find(key);
		if (it != g_code_cache.end()) { code = it->second; log.clear(); return true; }
	}
	/* on disk the pipeline source (the kernel headers, embedded in this library) is part of the key: another build of the
	 * library must not pick up this one's kernels */
	static const char* const hdr_src[8] = { LOL_KERNEL_H_TEXT, LOL_KERNEL_AA_H_TEXT, LOL_KERNEL_BATCH_H_TEXT, LOL_KERNEL_BATCH_AA_H_TEXT,
	                                        LOL_KERNEL_BLEND_H_TEXT, LOL_KERNEL_BLEND_AA_H_TEXT, LOL_KERNEL_RAYS_H_TEXT, LOL_KERNEL_SHADE_H_TEXT };
	static const char* const hdr_name[8] = { "lol_kernel.h", "lol_kernel_aa.h", "lol_kernel_batch.h", "lol_kernel_batch_aa.h",
	                                         "lol_kernel_blend.h", "lol_kernel_blend_aa.h", "lol_kernel_rays.h", "lol_kernel_shade.h" };
	constexpr int n_hdr = 8;                            /* every module is handed all of them: what it does not #include is never parsed */
	static const std::string all_headers = [] { std::string t; for (const char* h : hdr_src) { t += '|'; t += h; } return t; }();
	const char* use_src[n_hdr + 2];
	const char* use_name[n_hdr + 2];
	for (int i = 0; i < n_hdr; i++) { use_src[i] = hdr_src[i]; use_name[i] = hdr_name[i]; }
	use_src[n_hdr] = LOL_KERNEL_SCENES_H_TEXT; use_name[n_hdr] = "lol_kernel_scenes.h";
	use_src[n_hdr + 1] = LOL_KERNEL_SCENES_AA_H_TEXT; use_name[n_hdr + 1] = "lol_kernel_scenes_aa.h";
	const int n_use = n_hdr + structure;
	const std::string disk_key = key + all_headers + (structure ? std::string("|") + LOL_KERNEL_SCENES_H_TEXT : std::string()) +
	                             (structure > 1 ? std::string("|") + LOL_KERNEL_SCENES_AA_H_TEXT : std::string());
	if (disk_cache_load(disk_key, code)) {
		std::lock_guard<std::mutex> lock(g_cache_mutex);
		g_code_cache[key] = code;
		log = "(code object from the disk cache)";
		return true;
	}
	hiprtcProgram prog = nullptr;
	if (hiprtcCreateProgram(&prog, src.c_str(), "lol_render_spec.hip", n_use, use_src, use_name) != HIPRTC_SUCCESS) {
		log = "hiprtcCreateProgram failed";
		return false;
	}
	bool options_dropped = false;
	hiprtcResult r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
	if (r != HIPRTC_SUCCESS) {
		/* a hipRTC that does not know the scheduling option must not cost the specialisation: once more without it */
		std::vector<const char*> plain;
		for (size_t i = 0; i < opts.size(); i++) {
			if (!strcmp(opts[i], "-mllvm") && i + 1 < opts.size() &&
			    (!strcmp(opts[i + 1], "-amdgpu-sched-strategy=max-ilp") || !strcmp(opts[i + 1], "-enable-post-misched=0") ||
			     !strcmp(opts[i + 1], "-phi-node-folding-threshold=8") || !strcmp(opts[i + 1], "-amdgpu-long-branch-factor=0"))) { i++; continue; }
			plain.push_back(opts[i]);
		}
		if (plain.size() != opts.size()) {
			/* what comes out now was NOT compiled under the options the key lists: it serves this process (the retry would
			 * give the same again) but never goes to disk under that key */
			options_dropped = true;
			hiprtcDestroyProgram(&prog);
			prog = nullptr;
			if (hiprtcCreateProgram(&prog, src.c_str(), "lol_render_spec.hip", n_use, use_src, use_name) != HIPRTC_SUCCESS) {
				log = "hiprtcCreateProgram failed";
				return false;
			}
			r = hiprtcCompileProgram(prog, (int)plain.size(), plain.data());
		}
	}
	size_t log_size = 0;
	hiprtcGetProgramLogSize(prog, &log_size);
	log.clear();
	if (log_size > 1) { log.resize(log_size); hiprtcGetProgramLog(prog, &log[0]); }
	if (r != HIPRTC_SUCCESS) {
		log = std::string("hipRTC: ") + hiprtcGetErrorString(r) + "\n" + log;
		hiprtcDestroyProgram(&prog);
		return false;
	}
	size_t code_size = 0;
	hiprtcGetCodeSize(prog, &code_size);
	code.resize(code_size);
	hiprtcGetCode(prog, code.data());
	hiprtcDestroyProgram(&prog);
	if (has_return_clobbering_branch(code)) {
		/* a kernel that would never finish is worse than no kernel: the interpreter renders this scene */
		log = "the compiler relaxed a long branch through s[30:31], the return address of a function (LLVM AMDGPU long-branch "
		      "register bug; see compile_spec): code object refused";
		code.clear();
		return false;
	}
	if (options_dropped && out_of_line) {
		/* The retry above also dropped -amdgpu-long-branch-factor=0, the option that KEEPS the compiler from that bug, and an
		 * out-of-line SDF is where it bites (a function beyond s_cbranch's reach).  The pattern check would be all that is left
		 * between this code object and a launch that never ends: not enough — the interpreter renders this scene. */
		log = "this hipRTC refused the -mllvm options (among them the workaround for LLVM's long-branch register bug) and the scene's "
		      "SDF is out of line: code object refused";
		code.clear();
		return false;
	}
	{
		std::lock_guard<std::mutex> lock(g_cache_mutex);
		g_code_cache[key] = code;
	}
	if (!options_dropped) disk_cache_store(disk_key, code);
	return true;
}

/* hipRTC: generated source + lol_kernel.h → code object for `arch`.  Needs no device. */
bool compile_spec(const lol_program& P, const FastPaths* fast, const std::string& arch, std::vector<char>& code,
                  std::string& log, std::string* src_out, bool cull, int form, ModuleKernels carries) {
	std::string src = generate_source(P, fast, cull, form, carries);
	if (src_out) *src_out = src;
	if (const char* dump = tuning_env("LOL_GPU_DUMP_SPEC_SOURCE"))       /* debugging aid: the source as really generated on this device */
		if (FILE* f = fopen(dump, "w")) { fputs(src.c_str(), f); fclose(f); }
	return compile_source(src, spec_out_of_line(P, form), 0, arch, code, log);
}

/* The structure module (lol_kernel_scenes.h; lol_gpu_render_scene_views): the scene's SDF emitted ONCE — no fast form, no culling plan,
 * inlined, objects in file order —, every number a read K[7 i + j] through a member pointer in the constant address space, so the numbers
 * arrive by scalar loads and feed the VALU as SGPR operands while the SDF stays straight-line code.  Nothing of the text depends on a
 * number of `P`: all scenes of one structure share the source, the code object and its place in the disk cache.  Two kernels:
 * lol_render_param_batch (counts steps: it serves a batch with or without lol_gpu_debug::steps) and lol_render_param_batch_lin.
 * `samples` (lol_gpu_set_scene_view_samples): two more, lol_render_param_batch_aa and lol_render_param_batch_aa_lin — the same body
 * with sample_launch applied to the record's launch and the supersampled batches' stores (lol_kernel_scenes_aa.h), the same
 * ParamSdf, register budget and LDS.  Without it the text is what it was before those existed, byte for byte. */
std::string generate_structure_source(const lol_program& P, bool samples) {
	std::string s = samples ? "#include \"lol_kernel_scenes_aa.h\"\nnamespace lol {\n" : "#include \"lol_kernel_scenes.h\"\nnamespace lol {\n";
	const std::vector<RootBound> roots = analyse_roots(P);
	const CullPlan plan = plan_culling(roots, false);        /* file order, no test */
	const std::string occupancy = register_budget(P);
	emit_sdf(s, P, "ParamSdf", nullptr, false, roots, plan, true);
	s += "}  // namespace lol\n";
	const bool tables_global = !lol::tables_in_lds(P.n_lights, P.n_materials, P.n_roots);
	const std::string tg = tables_global ? "true" : "false";
	s += "template <bool LIN> __device__ __forceinline__ void lol_param_body(const lol::Launch& L, const lol::SceneTail& B, lol::u32* lds) {\n";
	s += "\tconst lol::Launch S = lol::scene_launch(L, B);\n";
	if (!tables_global) s += "\tlol::stage_common(S, lds);\n\t__syncthreads();\n";
	s += "\tlol::ParamSdf sdf;\n\tsdf.K = lol::scene_numbers(B);\n";
	s += "\tconst lol::Pixel P = lol::shade_pixel<lol::ParamSdf, " + tg + ", !LIN>(S, sdf, lds);\n";
	s += "\tif constexpr (LIN) lol::store_linear_view(L, P.rgb);\n\telse lol::store_pixel_view(L, lol::batch_tail(B), P);\n}\n";
	const std::string head = "extern \"C\" __global__ __launch_bounds__(lol::BLOCK)" + occupancy + " void ";
	const std::string tail = "(const lol::Launch L, const lol::SceneTail B) {\n\textern __shared__ lol::u32 lds[];\n\tlol_param_body<";
	s += head + "lol_render_param_batch" + tail + "false>(L, B, lds);\n}\n";
	s += head + "lol_render_param_batch_lin" + tail + "true>(L, B, lds);\n}\n";
	if (!samples) return s;
	/* (every lane reaches the store: the butterfly of sample_mean needs the whole wave) */
	s += "template <bool LIN> __device__ __forceinline__ void lol_param_body_aa(const lol::Launch& L, const lol::SceneTail& B, lol::u32* lds) {\n";
	s += "\tconst lol::Launch R = lol::scene_launch(L, B);\n";
	if (!tables_global) s += "\tlol::stage_common(R, lds);\n\t__syncthreads();\n";
	s += "\tconst lol::Launch S = lol::sample_launch(R);\n";
	s += "\tlol::ParamSdf sdf;\n\tsdf.K = lol::scene_numbers(B);\n";
	s += "\tconst lol::Pixel P = lol::shade_pixel<lol::ParamSdf, " + tg + ", false>(S, sdf, lds);\n";
	s += "\tif constexpr (LIN) lol::store_linear_view_aa(L, P.rgb);\n\telse lol::store_pixel_view_aa(L, lol::batch_tail(B), P.rgb);\n}\n";
	const std::string tail_aa = "(const lol::Launch L, const lol::SceneTail B) {\n\textern __shared__ lol::u32 lds[];\n\tlol_param_body_aa<";
	s += head + "lol_render_param_batch_aa" + tail_aa + "false>(L, B, lds);\n}\n";
	s += head + "lol_render_param_batch_aa_lin" + tail_aa + "true>(L, B, lds);\n}\n";
	return s;
}

bool compile_structure(const lol_program& P, const std::string& arch, std::vector<char>& code, std::string& log, std::string* src_out, bool samples) {
	const std::string src = generate_structure_source(P, samples);
	if (src_out) *src_out = src;
	return compile_source(src, false, samples ? 2 : 1, arch, code, log);
}

/* What the offline entry points share: `compile(code, log, src)` runs under g_rtc_mutex on the large-stack thread, like every run of
 * the scene compiler (BigStackThread); the log is copied out; `<out_base>.hip` is written whether or not the compile succeeded,
 * `<out_base>.co` when it did. */
template <class Compile>
static int compile_offline(const char* out_base, char* log, size_t logcap, Compile compile) {
	std::vector<char> code;
	std::string lg, src;
	bool ok = false;
	{
		BigStackThread th;
		auto work = [&]() {
			try { std::lock_guard<std::mutex> rtc(g_rtc_mutex); ok = compile(code, lg, src); }
			catch (...) { ok = false; lg = "the scene compiler ran out of memory"; }
		};
		bool started = false;
		try { started = th.start(work); } catch (...) { started = false; }
		if (started) th.join(); else work();
	}
	if (log && logcap) snprintf(log, logcap, "%s", lg.c_str());
	if (out_base && out_base[0]) {
		std::string base = out_base;
		if (FILE* f = fopen((base + ".hip").c_str(), "w")) { fputs(src.c_str(), f); fclose(f); }
		if (ok) if (FILE* f = fopen((base + ".co").c_str(), "wb")) { fwrite(code.data(), 1, code.size(), f); fclose(f); }
	}
	return ok ? LOL_GPU_OK : LOL_GPU_ERR_UNSUPPORTED;
}

#pragma GCC visibility pop

extern "C" {

/* Host-only view of the bound behind the culling test of top-level object `root` (0-based, file order):
 * 1 = bounded (centre and inflated radius R' out), 0 = no bound (never culled), < 0 = bad argument. */
int lol_gpu_cull_bounds(const lol_program* prog, uint32_t root, float c_out[3], float* r_out) {
	if (!prog || !c_out || !r_out || root >= prog->n_roots || prog->n_ops > LOL_MAX_OPS) return LOL_GPU_ERR_ARG;
	const std::vector<RootBound> roots = analyse_roots(*prog);
	if (root >= roots.size()) return LOL_GPU_ERR_ARG;
	const RootBound& R = roots[root];
	if (!R.bounded) return 0;
	const CullTest t = make_test(R.sphere());
	c_out[0] = t.c[0]; c_out[1] = t.c[1]; c_out[2] = t.c[2];
	*r_out = t.rm;
	return 1;
}

/* ... and the tighter two-sphere bound, where the object has one (cluster_bounds): value(p) >= min_j (|p - c_j| - r_j) with the
 * inflated radii the kernel tests with.  Returns the number of spheres written to out[j] = {cx, cy, cz, r'} (0 or 2). */
int lol_gpu_cull_bounds_clusters(const lol_program* prog, uint32_t root, float out[3][4]) {
	if (!prog || !out || root >= prog->n_roots || prog->n_ops > LOL_MAX_OPS) return LOL_GPU_ERR_ARG;
	const std::vector<RootBound> roots = analyse_roots(*prog);
	if (root >= roots.size()) return LOL_GPU_ERR_ARG;
	int n = 0;
	for (const Sphere& c : roots[root].clusters) {
		if (n == 3) break;
		const CullTest t = make_test(c);
		out[n][0] = t.c[0]; out[n][1] = t.c[1]; out[n][2] = t.c[2]; out[n][3] = t.rm;
		n++;
	}
	return n;
}

/* Host-only view of the interpreter list the scene-record calls build for `prog` (build_interp_lists with no proven fast path):
 * its length, its test records, the objects without a bound, and per object in evaluation order its id and whether the record that
 * finishes it carries MOP_TIE — read back from the list itself, not from the plan.  Returns the number of objects. */
int lol_gpu_interp_list_info(const lol_program* prog, int cull, uint32_t* n_mops, uint32_t* n_tests, uint32_t* n_unbounded,
                             uint32_t* order, uint32_t* tie, size_t cap) {
	if (!prog || prog->n_ops > LOL_MAX_OPS || (cap && (!order || !tie))) return LOL_GPU_ERR_ARG;
	const std::vector<RootBound> roots = analyse_roots(*prog);
	const CullPlan plan = plan_culling(roots, cull != 0);
	const std::vector<uint32_t> list = build_mops(*prog, nullptr, roots, plan, false);
	if (n_mops) *n_mops = (uint32_t)(list.size() / lol::MOP_DWORDS);
	if (n_tests) *n_tests = (uint32_t)plan.intervals.size();
	if (n_unbounded) *n_unbounded = (uint32_t)plan.n_unbounded;
	const std::vector<PlanStep> steps = walk_plan(roots, plan);
	size_t at = 0, n = 0;
	for (const PlanStep& st : steps) {
		at += (size_t)st.n_open * lol::MOP_DWORDS;                       /* the constants records in front of the object */
		while (at < list.size() && !(list[at] & lol::MOP_TOP)) at += lol::MOP_DWORDS;
		if (at >= list.size()) return LOL_GPU_ERR_UNSUPPORTED;
		if (n < cap) { order[n] = list[at + 1]; tie[n] = (list[at] & lol::MOP_TIE) ? 1u : 0u; }
		n++;
		at += lol::MOP_DWORDS;
	}
	return (int)n;
}

void lol_gpu_code_key(const void* code, size_t n, char out[17]) {
	if (!out) return;
	snprintf(out, 17, "%s", code ? code_key_hex(code, n).c_str() : "");
}

int lol_gpu_testing_has_return_clobbering_branch(const void* code, size_t n_bytes) {
	if (!code) return LOL_GPU_ERR_ARG;
	return has_return_clobbering_branch(code, n_bytes) ? 1 : 0;
}

/* Offline use (tests, ISA inspection; needs no device): compile the scene module with the switches of mask `switches` for `arch` and
 * write `<out_base>.hip` (generated source) and `<out_base>.co` (code object); lol_gpu_diag.h */
int lol_gpu_compile_offline_module(const lol_program* prog, const char* arch, const char* out_base, int assume_fast, unsigned switches,
                                   int form, char* log, size_t logcap) {
	if (!prog || !arch || switches > ALL_SWITCHES) return LOL_GPU_ERR_ARG;
	if (form != SPEC_BY_SIZE && form != SPEC_OUT_OF_LINE && form != SPEC_INLINE) return LOL_GPU_ERR_ARG;
	const ModuleKernels carries = { switches };
	FastPaths fast;
	if (assume_fast) {                 /* ISA inspection only: pretend every shortcut was proven */
		fast.sqrt_kind = assume_fast >= 1 && assume_fast <= 3 ? 4 - assume_fast : 3;   /* 1 → sqrt_r2, 2 → sqrt_gs, 3 → sqrt_pm */
		fast.sqrt_tiny_ok = true;
		/* (the shading's arithmetic as an MI355X proves it: the one-correction reciprocal) */
		if (shade_math_wanted()) { fast.shade_root = fast.sqrt_kind; fast.shade_rcp = 1; }
		for (uint32_t i = 0; i < prog->n_ops; i++)
			if ((prog->ops[i].op == LOL_OP_SMIN || prog->ops[i].op == LOL_OP_SMIN_R) && !fast.has(prog->ops[i].f[0]))
				{ fast.div_ok.push_back(prog->ops[i].f[0]); fast.div_nf_ok.push_back(prog->ops[i].f[0]); }
	}
	return compile_offline(out_base, log, logcap, [&](std::vector<char>& code, std::string& lg, std::string& src) {
		return compile_spec(*prog, &fast, arch, code, lg, &src, culling_enabled(1), form, carries);
	});
}

/* ... and the structure module of `prog` (lol_gpu_set_scene_views; `samples`: lol_gpu_set_scene_view_samples): `<out_base>.hip` and
 * `<out_base>.co`; lol_gpu_diag.h */
static int compile_offline_structure(const lol_program* prog, const char* arch, const char* out_base, char* log, size_t logcap, bool samples) {
	if (!prog || !arch || prog->n_ops > LOL_MAX_OPS || (prog->n_ops && !prog->ops)) return LOL_GPU_ERR_ARG;
	return compile_offline(out_base, log, logcap, [&](std::vector<char>& code, std::string& lg, std::string& src) {
		return compile_structure(*prog, arch, code, lg, &src, samples);
	});
}
int lol_gpu_compile_offline_scene_views(const lol_program* prog, const char* arch, const char* out_base, char* log, size_t logcap) {
	return compile_offline_structure(prog, arch, out_base, log, logcap, false);
}
int lol_gpu_compile_offline_scene_view_samples(const lol_program* prog, const char* arch, const char* out_base, char* log, size_t logcap) {
	return compile_offline_structure(prog, arch, out_base, log, logcap, true);
}

/* The entry points from before that one, each the module of a mask (lol_gpu_diag.h).  Their `others` is a mask in an order of its
 * own, the one in which the switches came to be. */
static unsigned on(int enable, ModuleSwitch sw) { return enable ? switch_bit(sw) : 0u; }
static unsigned switches_of(int others) {
	return on(others & 1, SWITCH_BATCH_BLEND) | on(others & 2, SWITCH_AA) | on(others & 4, SWITCH_BATCH) | on(others & 8, SWITCH_BATCH_AA) |
	       on(others & 16, SWITCH_BATCH_BLEND_AA) | on(others & 32, SWITCH_RAYS);
}

int lol_gpu_compile_offline(const lol_program* prog, const char* arch, const char* out_base, int assume_fast,
                            char* log, size_t logcap) {
	return lol_gpu_compile_offline_module(prog, arch, out_base, assume_fast, 0, SPEC_BY_SIZE, log, logcap);
}

int lol_gpu_compile_offline_samples(const lol_program* prog, const char* arch, const char* out_base, int assume_fast, int samples,
                                    char* log, size_t logcap) {
	if (samples != 1 && samples != 2 && samples != 4) return LOL_GPU_ERR_ARG;
	return lol_gpu_compile_offline_module(prog, arch, out_base, assume_fast, on(samples > 1, SWITCH_AA), SPEC_BY_SIZE, log, logcap);
}

int lol_gpu_compile_offline_views(const lol_program* prog, const char* arch, const char* out_base, int assume_fast, int enable, int form,
                                  char* log, size_t logcap) {
	return lol_gpu_compile_offline_module(prog, arch, out_base, assume_fast, on(enable, SWITCH_BATCH), form, log, logcap);
}

int lol_gpu_compile_offline_view_samples(const lol_program* prog, const char* arch, const char* out_base, int assume_fast, int enable,
                                         int form, char* log, size_t logcap) {
	return lol_gpu_compile_offline_module(prog, arch, out_base, assume_fast, on(enable, SWITCH_BATCH_AA), form, log, logcap);
}

/* (`enable` is the mask here: bit 0 is the switch itself) */
int lol_gpu_compile_offline_view_blends(const lol_program* prog, const char* arch, const char* out_base, int assume_fast, int enable,
                                        int form, char* log, size_t logcap) {
	if (enable < 0 || enable > 15) return LOL_GPU_ERR_ARG;
	return lol_gpu_compile_offline_module(prog, arch, out_base, assume_fast, switches_of(enable), form, log, logcap);
}

int lol_gpu_compile_offline_view_blend_samples(const lol_program* prog, const char* arch, const char* out_base, int assume_fast, int enable,
                                               int others, int form, char* log, size_t logcap) {
	if (others < 0 || others > 15) return LOL_GPU_ERR_ARG;
	return lol_gpu_compile_offline_module(prog, arch, out_base, assume_fast, switches_of(others) | on(enable, SWITCH_BATCH_BLEND_AA), form, log, logcap);
}

int lol_gpu_compile_offline_rays(const lol_program* prog, const char* arch, const char* out_base, int assume_fast, int enable,
                                 int others, int form, char* log, size_t logcap) {
	if (others < 0 || others > 31) return LOL_GPU_ERR_ARG;
	return lol_gpu_compile_offline_module(prog, arch, out_base, assume_fast, switches_of(others) | on(enable, SWITCH_RAYS), form, log, logcap);
}

int lol_gpu_compile_offline_shade(const lol_program* prog, const char* arch, const char* out_base, int assume_fast, int enable,
                                  int others, int form, char* log, size_t logcap) {
	if (others < 0 || others > 63) return LOL_GPU_ERR_ARG;
	return lol_gpu_compile_offline_module(prog, arch, out_base, assume_fast, switches_of(others) | on(enable, SWITCH_SHADE), form, log, logcap);
}

}  // extern "C"
