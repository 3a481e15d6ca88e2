/*
 * lol_gpu.hip — C ABI (include/lol_gpu.h) over the gfx950 render kernels (lol_kernel.h).
 *
 * Host side of the drop-in: context = {device, stream, device copy of the
 * flattened scene, the scene-specialised kernel, a device framebuffer for the
 * host-surface path}.  No CPU rendering path exists here; without a HIP device
 * every call fails.
 *
 * Two kernels render the same bits:
 *  - render_interp<STACK>   compiled ahead of time; interprets the scene's macro-op list, fetched with
 *    wave-uniform scalar loads (lol_kernel.h, Interp);
 *  - lol_render_spec        compiled by hipRTC in lol_gpu_upload_program() from
 *    lol_kernel.h + a generated SpecSdf::eval() — the scene's SDF as straight-line
 *    code with immediates (the GPU analogue of tracing_jit_renderer.dasc:76-216,
 *    whose render_prepare JIT-compiles the scene the same way).  Used when the
 *    compile succeeds (LOL_GPU_SPECIALIZE=0 or lol_gpu_set_specialize(ctx,0)
 *    keep the interpreter).
 */
#include "lol_gpu_internal.h"

/* LOL_BUILD_ID: a digest of this library's sources and compiler flags (csrc/Makefile: lol_build_id.inc) — the identity
 * of the ahead-of-time kernels (lol_gpu_kernel_key) */
#include "lol_build_id.inc"

/*
 * Tuning switches.  Two dozen LOL_GPU_* environment variables select code paths and compiler options for A/B runs (the list:
 * INTEGRATION.md) — LOL_GPU_RTC_FLAGS appends arbitrary options to the hot kernel's compile, and "-ffp-contract=fast"
 * inherited from some shell would silently end parity with the reference.  So they are read ONLY in a process that also has
 * LOL_GPU_TUNING=1 set, every one that was read and found is recorded (lol_gpu_tuning_switches(), the scene compiler's log,
 * bench.py's `config.env`), and one that is set without LOL_GPU_TUNING=1 is reported once on stderr and ignored.  Not fenced,
 * because they change where things are kept or what is traced, never what is computed: LOL_GPU_CACHE_DIR, LOL_GPU_ROCTX.
 */
static std::mutex g_tuning_mutex;
static std::vector<std::pair<std::string, std::string>> g_tuning_seen;      /* switches that took effect: name, value */
static std::vector<std::string> g_tuning_ignored;                           /* set, but LOL_GPU_TUNING=1 was not */
static std::string g_tuning_text;

__attribute__((visibility("hidden"))) const char* lol_gpu_internal_tuning_env(const char* name) {
	const char* v = getenv(name);
	if (!v) return nullptr;
	const char* on = getenv("LOL_GPU_TUNING");
	/* (called from entry points of the C ABI, some of which hold no try block of their own: a switch that cannot be RECORDED —
	 * no memory for its name — is not honoured, and nothing is thrown) */
	try {
		std::lock_guard<std::mutex> lock(g_tuning_mutex);
		if (!(on && on[0] == '1' && !on[1])) {
			if (std::find(g_tuning_ignored.begin(), g_tuning_ignored.end(), name) == g_tuning_ignored.end()) {
				g_tuning_ignored.push_back(name);
				fprintf(stderr, "lol_gpu: %s is set but LOL_GPU_TUNING=1 is not: ignored (tuning switches are for A/B runs)\n", name);
			}
			return nullptr;
		}
		for (auto& e : g_tuning_seen) if (e.first == name) { e.second = v; return v; }
		g_tuning_seen.emplace_back(name, v);
		return v;
	} catch (...) { return nullptr; }
}

extern "C" const char* lol_gpu_tuning_switches(void) {
	try {
		std::lock_guard<std::mutex> lock(g_tuning_mutex);
		g_tuning_text.clear();
		for (const auto& e : g_tuning_seen) { if (!g_tuning_text.empty()) g_tuning_text += ' '; g_tuning_text += e.first + "=" + e.second; }
		return g_tuning_text.c_str();
	} catch (...) { return "(out of memory)"; }
}

#pragma GCC visibility push(hidden)
int fail(lol_gpu* ctx, int status, const char* what, hipError_t e) {
	if (ctx) {
		if (e != hipSuccess) snprintf(ctx->err, sizeof ctx->err, "%s: %s", what, hipGetErrorString(e));
		else snprintf(ctx->err, sizeof ctx->err, "%s", what);
	}
	return status;
}
std::mutex g_rtc_mutex;
#pragma GCC visibility pop

namespace {

/* No exception crosses the C boundary: `body()`, or — where it throws — the failure of a call that was preparing `what` in host memory
 * (the analysis of a scene, the records of a call: whatever the body had queued or committed before stays as it is) */
template <class Body>
int guarded(lol_gpu* ctx, const char* what, Body&& body) {
	auto failed = [&](const char* how) {
		char text[128];
		snprintf(text, sizeof text, "%s while preparing %s", how, what);
		return fail(ctx, LOL_GPU_ERR_HIP, text);           /* (fail copies the text) */
	};
	try { return body(); }
	catch (const std::bad_alloc&) { return failed("out of host memory"); }
	catch (...) { return failed("unexpected failure"); }
}

/* the interpreter's kernel of a family (lol_gpu_internal.h, KERNEL_FAMILIES) for one stack class, sqrt kind and table placement: its
 * address, for hipLaunchKernel */
template <int SSIZE, int KIND, bool TABLES_GLOBAL>
const void* interp_kernel(KernelFamily f) {
	switch (f) {
	case FAM_FRAME:         return reinterpret_cast<const void*>(&lol::render_interp<SSIZE, KIND, TABLES_GLOBAL>);
	case FAM_FRAME_AA:      return reinterpret_cast<const void*>(&lol::render_interp_aa<SSIZE, KIND, TABLES_GLOBAL>);
	case FAM_FRAME_AA_LIST: return reinterpret_cast<const void*>(&lol::render_interp_aa_list<SSIZE, KIND, TABLES_GLOBAL>);
	case FAM_BATCH:         return reinterpret_cast<const void*>(&lol::render_interp_batch<SSIZE, KIND, TABLES_GLOBAL>);
	case FAM_BATCH_AA:      return reinterpret_cast<const void*>(&lol::render_interp_batch_aa<SSIZE, KIND, TABLES_GLOBAL>);
	case FAM_BATCH_AA_LIST: return reinterpret_cast<const void*>(&lol::render_interp_batch_aa_list<SSIZE, KIND, TABLES_GLOBAL>);
	case FAM_BATCH_LIN:     return reinterpret_cast<const void*>(&lol::render_interp_batch_lin<SSIZE, KIND, TABLES_GLOBAL>);
	case FAM_BATCH_AA_LIN:  return reinterpret_cast<const void*>(&lol::render_interp_batch_aa_lin<SSIZE, KIND, TABLES_GLOBAL>);
	default:                return nullptr;
	}
}

/* Conditions under which an escaped ray's colour is exactly clamp(ambient * materials[0].ambient), so
 * that waves of escaped rays may skip normal + lights (lol_kernel.h, FLAG_MISS_SKIP): material #0 has
 * diffuse == specular == 0 (either sign), shininess >= 0 and not NaN (powf(c in [0,1], s >= 0) is finite),
 * and every light intensity is finite (finite * 0 = 0, never NaN). */
bool miss_skip_ok(const lol_program& P) {
	if (P.n_materials == 0) return false;
	const lol_material& m = P.materials[0];
	const float z[6] = { m.diffuse.x, m.diffuse.y, m.diffuse.z, m.specular.x, m.specular.y, m.specular.z };
	for (float v : z) if (!(v == 0.0f)) return false;
	if (!(m.shininess >= 0.0f)) return false;
	for (uint32_t i = 0; i < P.n_lights; i++) {
		const lol_light& l = P.lights[i];
		const float f[6] = { l.diffuse_intensity.x, l.diffuse_intensity.y, l.diffuse_intensity.z,
		                     l.specular_intensity.x, l.specular_intensity.y, l.specular_intensity.z };
		for (float v : f) if (!(v - v == 0.0f)) return false;      /* inf or NaN */
	}
	return true;
}

/* Conditions for FLAG_DARK_SKIP (lol_kernel.h): with diffuse incidence exactly 0 a light contributes
 * I * (shadow * 0) * colour and I * (shadow * (0 * powf(c, shininess))) * colour, which is +-0 for any shadow in
 * [0, 1] provided I and the colours are finite and powf is finite (c in [0, 1], shininess >= 0). */
bool dark_skip_ok(const lol_program& P) {
	auto finite = [](float v) { return v - v == 0.0f; };
	for (uint32_t i = 0; i < P.n_lights; i++) {
		const lol_light& l = P.lights[i];
		const float f[6] = { l.diffuse_intensity.x, l.diffuse_intensity.y, l.diffuse_intensity.z,
		                     l.specular_intensity.x, l.specular_intensity.y, l.specular_intensity.z };
		for (float v : f) if (!finite(v)) return false;
	}
	for (uint32_t i = 0; i < P.n_materials; i++) {
		const lol_material& m = P.materials[i];
		const float f[6] = { m.diffuse.x, m.diffuse.y, m.diffuse.z, m.specular.x, m.specular.y, m.specular.z };
		for (float v : f) if (!finite(v)) return false;
		if (!(m.shininess >= 0.0f)) return false;
	}
	return true;
}

/* Conditions for FLAG_SHADOW_SETTLED (lol_kernel.h, soft_shadow): nothing a shadow march can compute overflows or turns
 * NaN, so that a factor that has reached 0 stays there.  Every number of the scene finite and below 10^15 in magnitude
 * (positions, radii, box sizes, smoothness, light positions).  What bounds the march is its own `t > L` exit, not the
 * step count: t starts at 0 and stays in [0, L] up to the step that ends the march — a step with s < 0 either ends it
 * (res = 50 s / t < -1) or has |s| <= t / 50 and leaves t positive — with L = |light - p| and |p| <= |camera| + 100 + one
 * step of the primary march, all below 10^16; the last step adds one SDF value at such a point.  So every coordinate
 * stays below 10^17 and every squared length below 10^35 < FLT_MAX.  The camera is checked per frame (launch). */
bool shadow_settle_ok(const lol_program& P) {
	auto sane = [](float v) { return v - v == 0.0f && fabsf(v) < 1e15f; };
	for (uint32_t i = 0; i < P.n_ops; i++) {
		const lol_op& o = P.ops[i];
		const int nf = o.op == LOL_OP_SPHERE ? 4 : o.op == LOL_OP_RBOX ? 7 : (o.op == LOL_OP_PLANE || o.op == LOL_OP_SMIN || o.op == LOL_OP_SMIN_R) ? 1 : 0;
		for (int j = 0; j < nf; j++) if (!sane(o.f[j])) return false;
	}
	for (uint32_t i = 0; i < P.n_lights; i++)
		if (!sane(P.lights[i].point.x) || !sane(P.lights[i].point.y) || !sane(P.lights[i].point.z)) return false;
	return true;
}
bool camera_sane(const lol_frame_camera& c) {
	const float* f = reinterpret_cast<const float*>(&c);
	for (size_t i = 0; i < sizeof c / 4; i++) if (!(f[i] - f[i] == 0.0f && fabsf(f[i]) < 1e15f)) return false;
	return true;
}

/* ---------------------------------------------------------------- the primary march's first step, once per camera position
 * Step 0 of get_intersection (naive_renderer.c:56-57) evaluates sdf(ro + rd * 0): the camera's position, the same point for
 * every pixel of the frame.  Like the camera basis of get_camera_ray (naive_renderer.c:183-186, computed once per frame in
 * lol_frame_camera_init) it is a per-frame constant, hoisted: the value is computed HERE, once per camera position, in the
 * reference's own arithmetic — sdf() / get_obj_dist() / sdSphere / sdRoundBox / sminf (naive_renderer.c:11-44, sdf.h:8-22,
 * float.h:6-33) over the post-order program of lol_scene.h, objects in file order, first strict minimum — and handed to the
 * kernels as two launch arguments (lol_kernel.h, FLAG_FIRST_STEP / march).  Every operation is an IEEE binary32 +, -, *, /,
 * sqrt or comparison, correctly rounded here as on the device (this file is compiled with -ffp-contract=off; no libm call), so
 * the value IS what every lane's first step would have computed.  Not used (the kernels take the step themselves) unless:
 * the camera is sane (camera_sane: then every ray direction that is finite makes ro + rd * 0 = ro, see march), no component of
 * the origin is a negative zero, max_steps >= 1, and the value lies in [0.001, 100] — a march that ends on its first step, or
 * goes on with a NaN, is left to the loop.  tests/test_gpu_parity.py compares every pixel's distance, id and step count
 * (this step included) with the oracle's either way.  host_sdf's `d < best` is the reference's tie rule (the first object in file
 * order wins among equals) only because lol_scene_flatten emits the LOL_OP_TOP records with strictly ascending ids, in file order:
 * it checks that itself, and tests/test_scene_shapes.py and tests/test_gpu_hostile.py hold it and the ties to the oracle. */
inline float h_minf(float a, float b) { return a < b ? a : b; }      /* MINSS: b on NaN / equal (float.h:6) */
inline float h_maxf(float a, float b) { return a > b ? a : b; }
inline float h_len3(float x, float y, float z) { return __builtin_sqrtf((x * x + y * y) + z * z); }      /* DPPS 0x71 (vec.h:52-56): (x² + y²) + (z² + 0) */
bool host_sdf(const lol_program& P, const float p[3], std::vector<float>& st, float* dist_out, uint32_t* id_out) {
	if (st.size() < (size_t)P.max_stack + 1) st.resize((size_t)P.max_stack + 1);
	size_t sp = 0;
	float best = __builtin_inff();
	uint32_t best_id = 0;
	for (uint32_t i = 0; i < P.n_ops; i++) {
		const lol_op& o = P.ops[i];
		switch (o.op) {
		case LOL_OP_SPHERE:
			if (sp >= st.size()) return false;
			st[sp++] = h_len3(p[0] - o.f[0], p[1] - o.f[1], p[2] - o.f[2]) - o.f[3];
			break;
		case LOL_OP_RBOX: {
			if (sp >= st.size()) return false;
			const float qx = __builtin_fabsf(p[0] - o.f[0]) - o.f[3], qy = __builtin_fabsf(p[1] - o.f[1]) - o.f[4], qz = __builtin_fabsf(p[2] - o.f[2]) - o.f[5];
			st[sp++] = h_len3(h_maxf(qx, 0.f), h_maxf(qy, 0.f), h_maxf(qz, 0.f)) + h_minf(h_maxf(qx, h_maxf(qy, qz)), 0.f) - o.f[6];
			break;
		}
		case LOL_OP_PLANE:
			if (sp >= st.size()) return false;
			st[sp++] = p[1] - o.f[0];
			break;
		case LOL_OP_SMIN: case LOL_OP_SMIN_R: {
			if (sp < 2) return false;
			const float top = st[--sp], under = st[--sp];
			const float a = o.op == LOL_OP_SMIN ? under : top, b = o.op == LOL_OP_SMIN ? top : under, k = o.f[0];
			const float h = h_minf(h_maxf(.5f + .5f * (b - a) / k, 0.f), 1.f);
			st[sp++] = (b + (a - b) * h) - k * h * (1.f - h);
			break;
		}
		case LOL_OP_TOP: {
			if (sp < 1) return false;
			const float d = st[--sp];
			if (d < best) { best = d; best_id = o.id; }
			break;
		}
		default: return false;
		}
	}
	*dist_out = best;
	*id_out = best_id;
	return true;
}
/* may a frame of `cam` take its first step on the host at all: what is decided before the SDF is asked */
bool first_step_possible(const lol_frame_camera& cam, int max_steps) {
	if (max_steps < 1 || !camera_sane(cam)) return false;
	uint32_t bits[3];
	memcpy(bits, &cam.origin, sizeof bits);
	for (uint32_t b : bits) if (b == 0x80000000u) return false;
	return true;
}
/* FLAG_FIRST_STEP for a frame of `cam` over program `P`?  *dist and *id: the SDF at the camera's position (NaN where host_sdf
 * could not say, or threw), written whenever the camera allows the question. */
constexpr float FIRST_STEP_MIN = 0.001f, FIRST_STEP_MAX = 100.f;      /* the reference's EPSILON and MAX_DIST */
bool program_first_step(const lol_program& P, const lol_frame_camera& cam, int max_steps, std::vector<float>& stack, float* dist, uint32_t* id) {
	if (!first_step_possible(cam, max_steps)) return false;
	const float origin[3] = { cam.origin.x, cam.origin.y, cam.origin.z };
	bool ok = false;
	*dist = 0.f; *id = 0;
	try { ok = host_sdf(P, origin, stack, dist, id); } catch (...) { ok = false; }
	if (!ok) *dist = __builtin_nanf("");
	return *dist >= FIRST_STEP_MIN && *dist <= FIRST_STEP_MAX;
}
/* ... over the uploaded program: the answer, ctx->first_dist and first_id are kept while the camera stays where it is (what the
 * camera rules out by itself never reaches the cache) */
bool first_step(lol_gpu* ctx, const lol_frame_camera& cam, int max_steps) {
	if (!first_step_possible(cam, max_steps)) return false;
	if (ctx->first_gen != ctx->generation || memcmp(ctx->first_origin, &cam.origin, sizeof ctx->first_origin) != 0) {
		ctx->first_taken = program_first_step(ctx->h_prog, cam, max_steps, ctx->first_stack, &ctx->first_dist, &ctx->first_id);
		ctx->first_gen = ctx->generation;
		memcpy(ctx->first_origin, &cam.origin, sizeof ctx->first_origin);
	}
	return ctx->first_taken;
}
/* What a record — a frame's Launch, a lol::View, a lol::SceneView — owes to its camera: FLAG_SHADOW_SETTLED (`settle`: the scene
 * qualifies and the host wants it), FLAG_FIRST_STEP with its value (`first`: program_first_step's answer, `dist` and `id` with it).
 * True: the record runs the second copy of the macro-op list, the one without v_div_fixup (`finite`: shadow_settle_ok(scene)). */
template <class Record>
bool camera_fields(Record& R, const lol_frame_camera& cam, bool finite, bool settle, bool first, float dist, uint32_t id) {
	const bool sane = camera_sane(cam);
	if (settle && sane) R.flags |= lol::FLAG_SHADOW_SETTLED;
	if (first) { R.flags |= lol::FLAG_FIRST_STEP; R.first_dist = dist; R.first_id = id; }
	return finite && sane;
}

/* ---- optional roctx ranges (LOL_GPU_ROCTX=1): one range per frame launch, visible to `rocprofv3 --marker-trace`.
 * The counterpart of the reference's perf/jitdump aid (jitdump.c) on this side; resolved with dlopen so the library
 * is only needed when asked for. */
struct Roctx {
	int  (*push)(const char*) = nullptr;
	int  (*pop)() = nullptr;
	std::atomic<long> ranges{0};        /* ranges pushed so far (lol_gpu_roctx_ranges) */
	bool asked = false;                 /* LOL_GPU_ROCTX=1 was set */
	std::once_flag once;
	void init() { std::call_once(once, [this] { resolve(); }); }      /* frames may be launched from several host threads */
	void resolve() {
		const char* e = getenv("LOL_GPU_ROCTX");
		if (!e || e[0] != '1') return;
		asked = true;
		for (const char* name : { "librocprofiler-sdk-roctx.so", "libroctx64.so", "/opt/rocm/lib/librocprofiler-sdk-roctx.so", "/opt/rocm/lib/libroctx64.so" }) {
			if (void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
				push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
				pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
				if (push && pop) return;
				push = nullptr; pop = nullptr;
			}
		}
		/* asked for and not there: say so once instead of silently tracing nothing */
		fprintf(stderr, "lol_gpu: LOL_GPU_ROCTX=1 but no roctx library could be loaded (%s): frames are not marked\n", dlerror());
	}
} g_roctx;

/* the scene kernel that runs family `f`, or nullptr: the interpreter does — there is no module yet, or it was compiled without that
 * family (a switch set after the upload).  Same pixels either way. */
const SceneKernel* family_kernel(const lol_gpu* ctx, KernelFamily f) {
	const SceneKernel* k = scene_kernel(ctx);
	return k && k->fn[f] ? k : nullptr;
}
const char* family_name(const lol_gpu* ctx, KernelFamily f) { return family_kernel(ctx, f) ? KERNEL_FAMILIES[f].symbol : KERNEL_FAMILIES[f].interp; }
/* the family of a frame under the context's current settings (of an adaptive frame: its refine pass) */
KernelFamily frame_family(const lol_gpu* ctx) { return ctx->samples == 1 ? FAM_FRAME : ctx->adaptive >= 0 ? FAM_FRAME_AA_LIST : FAM_FRAME_AA; }
const char* kernel_name(const lol_gpu* ctx) { return family_name(ctx, frame_family(ctx)); }

/* The interpreter's instantiation for the program's stack class and table placement — THE ladder, for every kernel the interpreter
 * has (launch_family, the list queries, lol_gpu_sdf_batch): launch(InterpVariant) is called with the two as compile-time constants. */
template <int SSIZE, bool TABLES_GLOBAL = false> struct InterpVariant {
	static constexpr int ssize = SSIZE;
	static constexpr bool tables_global = TABLES_GLOBAL;
};
/* which rung: the stack class the program needs (lol_gpu_internal.h, interp_stack_class) on the LDS ladder; with large tables, read
 * from global memory (lol_kernel.h, TABLES_LDS_MAX_DWORDS), the next of three stack classes.  interp_dispatch launches what this
 * says and lol_gpu_interp_variant (lol_gpu_diag.h) reports it: one choice, made here. */
struct InterpRung { int ssize; bool tables_global; };
InterpRung interp_rung(const lol_program& P) {
	const int cls = interp_stack_class(P.max_stack);
	if (lol::tables_in_lds(P.n_lights, P.n_materials, P.n_roots)) return { cls, false };
	return { cls <= 3 ? 3 : cls <= lol::MOP_DEEP_FROM - 1 ? lol::MOP_DEEP_FROM - 1 : lol::MOP_DEEP_SLOTS, true };
}
/* the five stack classes with the tables in LDS — and ALL the rungs of a kernel that reads no table (the SDF alone, a ray query):
 * lol_gpu_sdf_batch and ray_query come here directly */
template <class Launcher>
hipError_t stack_class_dispatch(int ssize, Launcher&& launch) {
	switch (ssize) {
	case 1:  return launch(InterpVariant<1>());
	case 3:  return launch(InterpVariant<3>());
	case 7:  return launch(InterpVariant<7>());
	case lol::MOP_DEEP_FROM - 1: return launch(InterpVariant<lol::MOP_DEEP_FROM - 1>());
	case lol::MOP_DEEP_SLOTS:    return launch(InterpVariant<lol::MOP_DEEP_SLOTS>());
	}
	return hipErrorInvalidValue;           /* a class without an instantiation: never a silent substitute */
}
template <class Launcher>
hipError_t interp_dispatch(const lol_gpu* ctx, Launcher&& launch) {
	const InterpRung r = interp_rung(ctx->h_prog);
	if (!r.tables_global) return stack_class_dispatch(r.ssize, launch);
	switch (r.ssize) {
	case 3:  return launch(InterpVariant<3, true>());
	case lol::MOP_DEEP_FROM - 1: return launch(InterpVariant<lol::MOP_DEEP_FROM - 1, true>());
	case lol::MOP_DEEP_SLOTS:    return launch(InterpVariant<lol::MOP_DEEP_SLOTS, true>());
	}
	return hipErrorInvalidValue;           /* a rung without an instantiation: never a silent substitute */
}
/* ... and THE launch of an interpreter's kernel that reads the tables: the instantiation for the program's rung and the root kind the
 * upload proved, a block of lol::BLOCK lanes.  `kernel_of(variant, kind)`: the address of the caller's kernel for an InterpVariant and
 * a std::integral_constant of the kind — the caller names the kernel, so its instantiations stand where the caller stands. */
template <class KernelOf>
hipError_t launch_interp(const lol_gpu* ctx, dim3 grid, void** args, unsigned lds, hipStream_t s, KernelOf&& kernel_of) {
	const int kind = ctx->interp_sqrt_kind;
	return interp_dispatch(ctx, [&](auto v) {
		const void* k = kind == 3 ? kernel_of(v, std::integral_constant<int, 3>()) : kernel_of(v, std::integral_constant<int, 0>());
		return hipLaunchKernel(k, grid, dim3(lol::BLOCK), args, lds, s);
	});
}

/* ONE launch of a kernel of family `f`: the scene module's where the module carries the family, else the interpreter's instantiation
 * for the program's rung (interp_dispatch: a rung without one is an error, never a substitute).  `args`: the addresses of the
 * kernel's arguments — (L), (L, list, count), (L, B) or (L, B, Q), the same for both kernels of a family, so one array serves
 * hipModuleLaunchKernel and hipLaunchKernel.  `counts`: somebody reads the per-lane step counters — a module compiles them into the
 * family's counting twin alone (generate_source); the interpreter's kernels always count, the supersampling families never. */
hipError_t launch_family(const lol_gpu* ctx, KernelFamily f, bool counts, void** args, dim3 grid, hipStream_t s) {
	/* dynamic LDS, of frames and batches alike: the scene's tables and a dword per lane of the block (lol_kernel.h, common_lds_dwords) */
	const lol_program& P = ctx->h_prog;
	const unsigned lds = lol::common_lds_dwords(P.n_lights, P.n_materials, P.n_roots) * 4u;
	if (const SceneKernel* k = family_kernel(ctx, f))
		return hipModuleLaunchKernel(counts ? k->counting[f] : k->fn[f], grid.x, grid.y, grid.z, lol::BLOCK, 1, 1, lds, s, args, nullptr);
	return launch_interp(ctx, grid, args, lds, s, [f](auto v, auto kind) {
		return interp_kernel<decltype(v)::ssize, decltype(kind)::value, decltype(v)::tables_global>(f);
	});
}

/* lights | materials | root_material of `P` as one run of lol::table_dwords dwords at `dst`: how an upload lays a program's tables
 * out, and what every copy of a scene's or a look's tables to the device holds */
void pack_tables(uint32_t* dst, const lol_program& P) {
	if (P.n_lights) memcpy(dst, P.lights, (size_t)P.n_lights * sizeof(lol_light));
	dst += (size_t)P.n_lights * lol::LIGHT_DWORDS;
	memcpy(dst, P.materials, (size_t)P.n_materials * sizeof(lol_material));
	dst += (size_t)P.n_materials * lol::MATERIAL_DWORDS;
	if (P.n_roots) memcpy(dst, P.root_material, (size_t)P.n_roots * 4);
}
/* ... and its inverse: the three tables of a launch whose counts are set, from such a run on the device */
void launch_tables(lol::Launch& L, const uint32_t* packed) {
	L.lights        = packed;
	L.materials     = L.lights + (size_t)L.n_lights * lol::LIGHT_DWORDS;
	L.root_material = L.materials + (size_t)L.n_materials * lol::MATERIAL_DWORDS;
}

/*
 * Adaptive frames (lol_gpu_set_adaptive_samples), pass 2: classify and compact.  One lane per pixel, a 16 x 4 tile per wave, tiles
 * row by row.  A pixel is refined when one of its (up to 8) neighbours inside the frame has another object id, or differs from it
 * by more than `contrast` in one of the 8-bit channels of the plain frame (`xrgb`, XRGB8888).  An unrefined pixel is the plain
 * pixel: written here, in the surface's format.  A refined one is appended to `list` (x | y << 16): one ballot and one atomic add
 * per wave, so a wave's pixels stay together in tile order — the refine pass's waves take consecutive entries.  Which wave gets
 * which part of the list depends on the order of the atomics; no pixel's value does.
 */
constexpr int CLASSIFY_W = 16, CLASSIFY_H = 4;
__device__ __forceinline__ void classify_tile(const uint32_t* xrgb, const uint32_t* ids, int w, int h, int contrast,
                                              uint32_t* dst, uint32_t pitch_px, uint32_t fmt_shift, uint32_t fmt_loss,
                                              uint32_t fmt_amask, uint32_t* list, uint32_t* count) {
	const int lane = threadIdx.x;
	const int x = blockIdx.x * CLASSIFY_W + lane % CLASSIFY_W, y = blockIdx.y * CLASSIFY_H + lane / CLASSIFY_W;
	const bool in = x < w && y < h;
	bool refined = false;
	uint32_t c = 0;
	if (in) {
		const size_t o = (size_t)y * w + x;
		c = xrgb[o];
		const uint32_t id = ids[o];
		for (int dy = -1; dy <= 1; dy++) {
			for (int dx = -1; dx <= 1; dx++) {
				const int qx = x + dx, qy = y + dy;
				if ((dx == 0 && dy == 0) || qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
				const size_t q = (size_t)qy * w + qx;
				const uint32_t cq = xrgb[q];
				bool differs = ids[q] != id;
				for (int sh = 0; sh <= 16; sh += 8)
					differs |= abs((int)(c >> sh & 0xFFu) - (int)(cq >> sh & 0xFFu)) > contrast;
				refined |= differs;
			}
		}
	}
	if (in && !refined) {                    /* SDL_MapRGB's packing of the plain pixel's 8-bit channels (store_pixel) */
		const uint32_t r8 = c >> 16 & 0xFFu, g8 = c >> 8 & 0xFFu, b8 = c & 0xFFu;
		dst[(size_t)y * pitch_px + x] = (r8 >> (fmt_loss & 0xFFu)) << (fmt_shift & 0xFFu) | (g8 >> (fmt_loss >> 8 & 0xFFu)) << (fmt_shift >> 8 & 0xFFu) |
		                                (b8 >> (fmt_loss >> 16 & 0xFFu)) << (fmt_shift >> 16 & 0xFFu) | fmt_amask;
	}
	const unsigned long long m = __ballot(refined);
	if (!m) return;
	uint32_t base = 0;
	if (lane == 0) base = atomicAdd(count, (uint32_t)__popcll(m));
	base = __shfl(base, 0, 64);
	if (refined) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)x | (uint32_t)y << 16;
}
__global__ __launch_bounds__(64) void adaptive_classify(const uint32_t* xrgb, const uint32_t* ids, int w, int h, int contrast,
                                                        uint32_t* dst, uint32_t pitch_px, uint32_t fmt_shift, uint32_t fmt_loss,
                                                        uint32_t fmt_amask, uint32_t* list, uint32_t* count) {
	classify_tile(xrgb, ids, w, h, contrast, dst, pitch_px, fmt_shift, fmt_loss, fmt_amask, list, count);
}

/*
 * Adaptive batches (lol_gpu_render_views_samples), pass 2: the same for every view of a batch, the view in the grid's z.  The plain
 * batch is dense (view v's pixels and ids at v w h); a view's mask reads that view's pixels alone — classify_tile's frame is the
 * view, so neighbours outside it are ignored —, its unrefined pixels go to the view's address in `dst`, and its refined ones to
 * a list segment of its own (w h entries at v w h) with a count of its own.
 */
__global__ __launch_bounds__(64) void adaptive_classify_views(const uint32_t* xrgb, const uint32_t* ids, int w, int h, int contrast,
                                                              uint32_t* dst, uint32_t pitch_px, unsigned long long view_stride_px,
                                                              uint32_t fmt_shift, uint32_t fmt_loss, uint32_t fmt_amask,
                                                              uint32_t* lists, uint32_t* counts) {
	const unsigned long long v = blockIdx.z, o = v * (unsigned long long)w * (unsigned long long)h;
	classify_tile(xrgb + o, ids + o, w, h, contrast, dst + v * view_stride_px, pitch_px, fmt_shift, fmt_loss, fmt_amask, lists + o, counts + v);
}

/* ... and between pass 2 and 3: the lists' lengths into the numbering of their groups of `per_wave` entries (lol_kernel_batch_aa.h,
 * render_aa_view_lists): prefix[v] = the groups of the views before v, prefix[n_views] = all of them.  One wave: lane l sums
 * the views [l c, (l + 1) c), c = ceil(n_views / 64), and a scan over the lanes gives each its start. */
__global__ __launch_bounds__(64) void view_group_prefix(const uint32_t* counts, uint32_t n_views, uint32_t per_wave, uint32_t* prefix) {
	const uint32_t lane = threadIdx.x, chunk = (n_views + 63u) / 64u;
	const uint32_t v0 = min(lane * chunk, n_views), v1 = min(v0 + chunk, n_views);
	uint32_t sum = 0;
	for (uint32_t v = v0; v < v1; v++) sum += (counts[v] + per_wave - 1u) / per_wave;
	uint32_t upto = sum;                                   /* inclusive scan over the lanes */
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t below = __shfl_up(upto, d, 64);
		if (lane >= (uint32_t)d) upto += below;
	}
	uint32_t run = upto - sum;
	for (uint32_t v = v0; v < v1; v++) { prefix[v] = run; run += (counts[v] + per_wave - 1u) / per_wave; }
	if (lane == 63u) prefix[n_views] = upto;
}

/*
 * Views averaged over K cameras (lol_gpu_render_views_blend), pass 2: one lane per output pixel, a 16 x 4 tile per wave, the view in
 * the grid's z.  `lin`: pass 1's linear colours, dense [v K + k][y][x] (lol_kernel_blend.h).  The pixel's K colours are summed per
 * channel in binary32 as a balanced binary tree in order of k — (c0 + c1) + (c2 + c3) ... — and the sum is multiplied by 1 / K; the
 * mean goes through gamma and the pixel format as one sample's colour does (pack_pixel), to the view's address, and after gamma
 * to the dense diagnostic.  Bytes between rows and between views are not written.
 */
struct BlendOut {
	uint32_t* dst; uint32_t pitch_px; unsigned long long view_stride_px;
	uint32_t fmt_shift, fmt_loss, fmt_amask, flags;       /* flags: FLAG_GAMMA_TABLE or 0 */
	float* dbg_rgb; const float* gamma_table;
};
template <int K>
__global__ __launch_bounds__(64) void blend_resolve(const lol::LinearColour* lin, int w, int h, const BlendOut O) {
	const int lane = threadIdx.x;
	const int x = blockIdx.x * CLASSIFY_W + lane % CLASSIFY_W, y = blockIdx.y * CLASSIFY_H + lane / CLASSIFY_W;
	if (x >= w || y >= h) return;
	const unsigned long long v = blockIdx.z, frame = (unsigned long long)w * (unsigned long long)h;
	const unsigned long long at = (unsigned long long)y * (unsigned long long)w + (unsigned long long)x;
	lol::V3 c[K];                            /* (K is a template argument: every loop below unrolls, c[] stays in registers) */
#pragma unroll
	for (int k = 0; k < K; k++) {
		const lol::LinearColour e = lin[(v * K + k) * frame + at];
		c[k] = { e.r, e.g, e.b };
	}
#pragma unroll
	for (int m = 1; m < K; m <<= 1)
#pragma unroll
		for (int i = 0; i < K; i += 2 * m) c[i] = { c[i].x + c[i + m].x, c[i].y + c[i + m].y, c[i].z + c[i + m].z };
	const float inv = 1.f / (float)K;
	const lol::V3 mean = { c[0].x * inv, c[0].y * inv, c[0].z * inv };
	lol::Launch L{};
	L.flags = O.flags;
	const lol::LaunchTail T = { O.dst, O.pitch_px, O.fmt_shift, O.fmt_loss, O.fmt_amask, O.dbg_rgb, nullptr, nullptr, nullptr, O.gamma_table };
	lol::V3 post;
	const uint32_t px = lol::pack_pixel(L, T, mean, post);
	const unsigned long long o = v * frame + at;
	if (O.dbg_rgb) { O.dbg_rgb[o * 3 + 0] = post.x; O.dbg_rgb[o * 3 + 1] = post.y; O.dbg_rgb[o * 3 + 2] = post.z; }
	O.dst[v * O.view_stride_px + (unsigned long long)y * O.pitch_px + (unsigned long long)x] = px;
}

/* not by hipStreamWaitEvent on HIP's special handles (the legacy default stream, the per-thread one): this HIP's hipStreamWaitEvent
 * dereferences the handle it is given and crashes (lol_sched.hip says the same) — there the host waits for the event */
int wait_on_stream(lol_gpu* ctx, hipStream_t s, hipEvent_t ev) {
	const bool special = s == hipStreamLegacy || s == hipStreamPerThread || s == nullptr;
	if (!special) LOL_HIP(ctx, hipStreamWaitEvent(s, ev, 0));
	else LOL_HIP(ctx, hipEventSynchronize(ev));
	return LOL_GPU_OK;
}

/*
 * The protocol of the context's rings of per-call device sets (lol_gpu_internal.h, RingSet), written once: take, copy, done, free.
 */
void ring_release(RingSet& S) {
	if (S.d_buf) (void)hipFree(S.d_buf);
	if (S.h_buf) (void)hipHostFree(S.h_buf);
	S.d_buf = nullptr; S.h_buf = nullptr; S.bytes = 0; S.used = false;
}
/* take: `S`, the ring's next set, is this call's, of at least `need` bytes, for work queued on `s`.  Its events are created on first
 * use.  Where it must grow — to `grow_to` bytes — the host waits for the set's last user and the buffers are replaced; an allocation
 * that fails leaves the set empty and the thread's last error cleared (the host's next HIP call must not trip over it), and `what`
 * in the context's error.  Then the waits: for `copied` on the host — the pinned half is the host's to write once the set's last
 * COPY has run (a ring's length of calls ago: a host that queues faster than the device renders is held that far ahead of it here)
 * —, for `done` on `s`: the device half is this call's once the set's last LAUNCH has finished, whatever stream it ran on.
 * `inject`: lol_gpu_testing_fail_view_scratch's counter, for the rings it is about. */
enum RingKind : unsigned { RING_SCRATCH = 0, RING_PINNED = 1, RING_TIMED = 2 };
int ensure_event(lol_gpu* ctx, hipEvent_t* ev, bool timed = false) {
	if (!*ev) LOL_HIP(ctx, hipEventCreateWithFlags(ev, timed ? hipEventDefault : hipEventDisableTiming));
	return LOL_GPU_OK;
}
int ring_take(lol_gpu* ctx, RingSet& S, size_t need, size_t grow_to, unsigned kind, hipStream_t s, int* inject, const char* what) {
	const bool pinned = kind & RING_PINNED;
	LOL_TRY(ensure_event(ctx, &S.done, kind & RING_TIMED));
	if (pinned) LOL_TRY(ensure_event(ctx, &S.copied));
	if (need > S.bytes) {
		if (S.used) LOL_HIP(ctx, hipEventSynchronize(S.done));
		ring_release(S);
		const bool injected = inject && *inject > 0;
		if (injected) --*inject;
		hipError_t me = injected ? hipErrorOutOfMemory : hipMalloc(reinterpret_cast<void**>(&S.d_buf), grow_to);
		if (me == hipSuccess && pinned) me = hipHostMalloc(reinterpret_cast<void**>(&S.h_buf), grow_to, hipHostMallocDefault);
		if (me != hipSuccess) {
			ring_release(S);
			(void)hipGetLastError();
			return fail(ctx, LOL_GPU_ERR_HIP, what, me);
		}
		S.bytes = grow_to;
	}
	if (S.used && pinned) LOL_HIP(ctx, hipEventSynchronize(S.copied));
	/* (an event recorded on one of HIP's special handles is waited for on the host too, whatever `s` is: a stream's
	 * hipStreamWaitEvent for an event last recorded on the legacy default stream crashed in this HIP — the GPU suite found it) */
	if (S.used && S.done_special) LOL_HIP(ctx, hipEventSynchronize(S.done));
	else if (S.used) LOL_TRY(wait_on_stream(ctx, s, S.done));
	return LOL_GPU_OK;
}
/* copy: the first `bytes` of the pinned half to the device on `s`, and `copied` behind them */
hipError_t ring_copy(RingSet& S, size_t bytes, hipStream_t s) {
	const hipError_t e = hipMemcpyAsync(S.d_buf, S.h_buf, bytes, hipMemcpyHostToDevice, s);
	const hipError_t e2 = hipEventRecord(S.copied, s);
	return e != hipSuccess ? e : e2;
}
/* done: `done` behind the last thing the call queued on `s` through `S` (and through `also`, the set of a second ring the same call
 * took).  `e`: what that last thing returned, `what` it was.  Called on EVERY path once anything has been queued — behind a failed
 * launch, a failed copy — because the work before it is queued, and the set's next user must find it behind the event it waits for. */
int ring_done(lol_gpu* ctx, RingSet& S, hipStream_t s, hipError_t e, const char* what, RingSet* also = nullptr) {
	const bool special = s == hipStreamLegacy || s == hipStreamPerThread || s == nullptr;
	hipError_t e2 = hipEventRecord(S.done, s);
	S.used = true;
	S.done_special = special;
	if (also) {
		const hipError_t e3 = hipEventRecord(also->done, s);
		also->used = true;
		also->done_special = special;
		if (e2 == hipSuccess) e2 = e3;
	}
	if (e != hipSuccess) return fail(ctx, LOL_GPU_ERR_HIP, what, e);
	if (e2 != hipSuccess) return fail(ctx, LOL_GPU_ERR_HIP, "hipEventRecord (behind a call's last launch)", e2);
	return LOL_GPU_OK;
}
/* free: at the end of the context, its streams drained */
template <class Set, int N>
void ring_free(Ring<Set, N>& ring) {
	for (RingSet& S : ring.sets) {
		ring_release(S);
		if (S.copied) (void)hipEventDestroy(S.copied);
		if (S.done) (void)hipEventDestroy(S.done);
	}
}

}  // namespace

extern "C" {

int lol_gpu_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

int lol_gpu_create(int device, lol_gpu** out) {
	if (!out) return LOL_GPU_ERR_ARG;
	*out = nullptr;
	int n = lol_gpu_device_count();
	if (n <= 0 || device < 0 || device >= n) return LOL_GPU_ERR_NO_DEVICE;
	lol_gpu* ctx = new (std::nothrow) lol_gpu;
	if (!ctx) return LOL_GPU_ERR_HIP;
	ctx->device = device;
	hipError_t e = hipSetDevice(device);
	if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
	ctx->frame_streams[0] = ctx->stream;
	/* (the device tables are sized by the first upload) */
	if (e != hipSuccess) {
		fprintf(stderr, "lol_gpu_create: %s\n", hipGetErrorString(e));
		lol_gpu_destroy(ctx);
		return LOL_GPU_ERR_HIP;
	}
	*out = ctx;
	return LOL_GPU_OK;
}


void lol_gpu_destroy(lol_gpu* ctx) {
	if (!ctx) return;
	if (ctx->device >= 0) (void)hipSetDevice(ctx->device);
	for (int i = lol_gpu::MAX_FRAME_STREAMS - 1; i >= 0; i--) {      /* ([0] is ctx->stream) */
		hipStream_t fs = i ? ctx->frame_streams[i] : ctx->stream;
		if (fs) { (void)hipStreamSynchronize(fs); (void)hipStreamDestroy(fs); }
	}
	for (int i = 0; i < 2; i++) {
		if (ctx->d_tables[i]) (void)hipFree(ctx->d_tables[i]);
		if (ctx->d_mops[i]) (void)hipFree(ctx->d_mops[i]);
	}
	if (ctx->d_frame) (void)hipFree(ctx->d_frame);
	if (ctx->copy_stream) { (void)hipStreamSynchronize(ctx->copy_stream); (void)hipStreamDestroy(ctx->copy_stream); }
	for (int i = 0; i < lol_gpu::PIPE_SLOTS; i++) {
		if (ctx->d_pipe[i]) (void)hipFree(ctx->d_pipe[i]);
		if (ctx->pipe_rendered[i]) (void)hipEventDestroy(ctx->pipe_rendered[i]);
		if (ctx->pipe_copied[i]) (void)hipEventDestroy(ctx->pipe_copied[i]);
	}

	ring_free(ctx->view_records);
	ring_free(ctx->scene_view_records);
	ring_free(ctx->adaptive_batches);
	ring_free(ctx->blends);
	ring_free(ctx->looks);
	ring_free(ctx->adaptive_frames);
	for (lol_gpu::AdaptiveFrameSet& S : ctx->adaptive_frames.sets)
		for (hipEvent_t ev : S.ev) if (ev) (void)hipEventDestroy(ev);
	if (ctx->d_adaptive_order) (void)hipFree(ctx->d_adaptive_order);
	if (ctx->d_bad) (void)hipFree(ctx->d_bad);
	if (ctx->d_gamma) (void)hipFree(ctx->d_gamma);
	if (ctx->d_pick) (void)hipFree(ctx->d_pick);
	if (ctx->tiles.have_events) for (hipEvent_t e : ctx->tiles.ev) (void)hipEventDestroy(e);
	lpt_release(ctx);
	delete ctx;                              /* ~SpecTiers: a compiler run still going is waited for, the scene kernels unloaded */
}

const char* lol_gpu_error(const lol_gpu* ctx) { return ctx ? ctx->err : "null context"; }

int lol_gpu_device(const lol_gpu* ctx) { return ctx ? ctx->device : -1; }

/* which of the wanted skips the uploaded program (and the environment) allows */
static void resolve_skips(lol_gpu* ctx) {
	const unsigned want = ctx->want_skips;
	ctx->miss_skip = (want & 1u) && miss_skip_ok(ctx->h_prog);
	ctx->dark_skip = (want & 2u) && dark_skip_ok(ctx->h_prog);
	ctx->shadow_settle = (want & 4u) && shadow_settle_ok(ctx->h_prog);
}

int lol_gpu_set_exact_skips(lol_gpu* ctx, unsigned mask) {
	if (!ctx || mask > 7u) return LOL_GPU_ERR_ARG;
	ctx->want_skips = mask;
	if (ctx->have_prog) resolve_skips(ctx);
	return LOL_GPU_OK;
}

int lol_gpu_set_miss_skip(lol_gpu* ctx, int enable) { return lol_gpu_set_exact_skips(ctx, enable ? 7u : 0u); }
int lol_gpu_set_cull(lol_gpu* ctx, int enable) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	ctx->want_cull = enable ? 1 : 0;          /* takes effect at the next lol_gpu_upload_program */
	return LOL_GPU_OK;
}

/* bit 0: escaped-wave skip active; bit 1: zero-incidence shadow skip active */
int lol_gpu_miss_skip_active(const lol_gpu* ctx) {
	return ctx ? (ctx->miss_skip ? 1 : 0) | (ctx->dark_skip ? 2 : 0) | (ctx->shadow_settle ? 4 : 0) : 0;
}
static int upload_program(lol_gpu* ctx, const lol_program* prog);

/* No exception crosses the C boundary: programs may have 2^20 ops, and the analysis of a scene (culling plan, the interpreter's
 * lists, the tables) allocates as it goes — a std::bad_alloc anywhere in it is an upload that failed, with the scene the
 * context had still rendering (every step before the commit works on the side). */
int lol_gpu_upload_program(lol_gpu* ctx, const lol_program* prog) {
	return guarded(ctx, "the scene", [&] { return upload_program(ctx, prog); });
}

static int upload_program(lol_gpu* ctx, const lol_program* prog) {
	if (!ctx || !prog) return LOL_GPU_ERR_ARG;
	/* sanity caps (lol_scene.h): counts beyond them are corruption, not scenes; every table a count speaks of must be there */
	if (prog->n_ops > LOL_MAX_OPS || prog->n_lights > LOL_MAX_LIGHTS || prog->n_materials > LOL_MAX_MATERIALS ||
	    prog->n_roots > LOL_MAX_OPS || prog->max_stack > LOL_MAX_STACK || prog->n_materials == 0)
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "program exceeds the sanity caps of lol_scene.h (or has no material)");
	if ((prog->n_ops && !prog->ops) || (prog->n_lights && !prog->lights) || !prog->materials || (prog->n_roots && !prog->root_material))
		return fail(ctx, LOL_GPU_ERR_ARG, "malformed program: a table is missing");
	/* validate what the kernel indexes with: stack discipline and material indices */
	int depth = 0;
	for (uint32_t i = 0; i < prog->n_ops; i++) {
		switch (prog->ops[i].op) {
		case LOL_OP_SPHERE: case LOL_OP_RBOX: case LOL_OP_PLANE: depth++; break;
		case LOL_OP_SMIN: case LOL_OP_SMIN_R:
			if (depth < 2) return fail(ctx, LOL_GPU_ERR_ARG, "malformed program: smin underflow");
			depth--; break;
		case LOL_OP_TOP:
			if (depth != 1 || prog->ops[i].id == 0 || prog->ops[i].id > prog->n_roots)
				return fail(ctx, LOL_GPU_ERR_ARG, "malformed program: bad top");
			depth = 0; break;
		default: return fail(ctx, LOL_GPU_ERR_ARG, "malformed program: unknown opcode");
		}
		if (depth > (int)prog->max_stack) return fail(ctx, LOL_GPU_ERR_ARG, "malformed program: max_stack too small");
	}
	if (depth != 0) return fail(ctx, LOL_GPU_ERR_ARG, "malformed program: dangling operands");
	for (uint32_t i = 0; i < prog->n_roots; i++)
		if (prog->root_material[i] >= prog->n_materials)
			return fail(ctx, LOL_GPU_ERR_ARG, "material index out of range");

	LOL_HIP(ctx, hipSetDevice(ctx->device));
	/* frames already queued — on the context's stream or on a caller's — still read the old tables and code
	 * object: drain the whole device before replacing them */
	LOL_HIP(ctx, hipDeviceSynchronize());
	/* Everything that can fail happens on the side: the tables for both kernels and the interpreter's macro-op list
	 * (smooth unions whose blend factor is proven on this device carry {k, 2k, .5/k}; the proven sqrt is selected by
	 * instantiation at launch) go to the table set no frame reads.  Only then is the context switched over, so a
	 * rejected program leaves the previous scene rendering (the reference asserts instead: scene.c:284-292). */
	FastPaths fast = prove_fast_paths(ctx, *prog);
	/* Two lists of the same records: the second one takes the blend factors without v_div_fixup where the device proved
	 * them.  That proof covers every FINITE difference of operands; the launch picks the second list only when nothing an
	 * evaluation computes can be infinite (finite_scene, and a sane camera for that frame), the SDF of arbitrary points
	 * (lol_gpu_sdf_batch) never does.  (The specialised kernel looks at NaN per object instead; here that costs more than
	 * the fixup saves.) */
	std::vector<uint32_t> mops;
	uint32_t n_mops = 0;
	if (!build_interp_lists(*prog, fast, culling_enabled(ctx->want_cull), mops, n_mops))
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "interpreter lists differ in length");      /* (same records by construction) */
	const int next = ctx->cur ^ 1;
	const bool injected = ctx->fail_uploads > 0;      /* lol_gpu_testing_fail_uploads (tests/test_gpu_boundary.py) */
	if (injected) ctx->fail_uploads--;
	/* lights | materials | root_material as one array of dwords, in the set no frame reads; grown when this scene needs more */
	std::vector<uint32_t> tables(lol::table_dwords(prog->n_lights, prog->n_materials, prog->n_roots));
	pack_tables(tables.data(), *prog);
	auto fit = [&](uint32_t*& buf, size_t& cap, size_t need) -> hipError_t {
		if (need <= cap) return hipSuccess;
		uint32_t* nb = nullptr;
		const size_t want = need + need / 2 + 256;
		const hipError_t me = hipMalloc(reinterpret_cast<void**>(&nb), want * 4);
		if (me != hipSuccess) return me;
		if (buf) (void)hipFree(buf);                  /* (the device is idle and no frame reads this set) */
		buf = nb; cap = want;
		return hipSuccess;
	};
	hipError_t e = injected ? hipErrorOutOfMemory : fit(ctx->d_tables[next], ctx->tables_cap[next], tables.size());
	if (e == hipSuccess) e = fit(ctx->d_mops[next], ctx->mops_cap[next], mops.size());
	if (e == hipSuccess) e = hipMemcpy(ctx->d_tables[next], tables.data(), tables.size() * 4, hipMemcpyHostToDevice);
	if (e == hipSuccess && !mops.empty())
		e = hipMemcpy(ctx->d_mops[next], mops.data(), mops.size() * 4, hipMemcpyHostToDevice);
	if (e != hipSuccess) return fail(ctx, LOL_GPU_ERR_HIP, "upload of the scene tables", e);
	const int interp_sqrt_kind = fast.sqrt_kind == 3 ? 3 : 0;
	std::string interp_key, interp_aa_key;
	{
		/* what render_interp executes = this build's code (lol_kernel.h AND this file: record layout, flags) + the lists */
		std::string id = std::string(LOL_BUILD_ID) + "|" + fnv_hex(mops.data(), mops.size() * 4) + "|" + std::to_string(interp_sqrt_kind) +
		                 (fast.gamma_ok ? "|gamma" : "");
		interp_key = fnv_hex(id.data(), id.size());
		id += "|render_interp_aa";
		interp_aa_key = fnv_hex(id.data(), id.size());
	}
	FastPaths fast_kept = fast;                       /* (may throw: before the commit) */
	ctx->h_own.assign(*prog);                         /* the last fallible step (host memory; all or nothing itself): the old scene is intact until here */
	/* commit (nothing below allocates on the way to the new scene being in place) */
	ctx->generation++;
	ctx->cur = next;
	ctx->have_prog = true;
	ctx->n_mops = n_mops;
	ctx->finite_scene = shadow_settle_ok(*prog);
	ctx->interp_sqrt_kind = interp_sqrt_kind;
	ctx->gamma_table = fast.gamma_ok;
	ctx->interp_key.swap(interp_key);
	ctx->interp_aa_key.swap(interp_aa_key);
	ctx->fast = std::move(fast_kept);
	resolve_skips(ctx);
	/* the scene compiler starts on its own thread; the new scene renders on the interpreter until its kernel is there
	 * (a failed specialisation is not an error either: the interpreter goes on rendering) */
	try { start_specialise(ctx, fast); }
	catch (...) {}                                    /* (no memory for a compiler run: the interpreter renders the scene) */
	return LOL_GPU_OK;
}

int lol_gpu_part_rows(int h, const lol_gpu_rows* rows) {
	if (h <= 0) return 0;
	if (!rows) return h;
	if (rows->band_rows <= 0 || rows->cycle_rows < rows->band_rows || rows->offset_rows < 0 ||
	    rows->offset_rows > rows->cycle_rows - rows->band_rows)
		return -1;
	long n = 0;
	for (long y0 = rows->offset_rows; y0 < h; y0 += rows->cycle_rows) {
		long y1 = y0 + rows->band_rows;
		if (y1 > h) y1 = h;
		n += y1 - y0;
	}
	return (int)n;
}

static int ensure_refine_grid(lol_gpu* ctx) {
	if (!ctx->adaptive_blocks) {
		/* the refine grid: enough one-wave blocks to fill the device (8 waves per SIMD, 4 SIMDs per CU), each with a slot of its own
		 * in the lane table; the order table maps block b to slot b */
		int cus = 0;
		LOL_HIP(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
		const uint32_t blocks = (uint32_t)std::max(1, cus) * 32u, stride = (blocks + 7u) / 8u;
		std::vector<uint32_t> order;
		try { order.assign((size_t)stride * 8u, 0u); } catch (...) { return fail(ctx, LOL_GPU_ERR_HIP, "out of host memory"); }
		for (uint32_t b = 0; b < blocks; b++) order[(b & 7u) * stride + (b >> 3)] = b;      /* (lol_kernel.h, tile_slot) */
		if (!ctx->d_adaptive_order) LOL_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_adaptive_order), order.size() * 4));
		LOL_HIP(ctx, hipMemcpy(ctx->d_adaptive_order, order.data(), order.size() * 4, hipMemcpyHostToDevice));
		ctx->adaptive_blocks = blocks; ctx->adaptive_stride = stride;
	}
	return LOL_GPU_OK;
}

/* The part of a launch that is the context's whoever brings the scene — the uploaded program, or the records of a call, which have
 * its structure: the tables' counts (alone: a capture over records, which packs no pixel), the gamma table, the surface's pixel format */
static void launch_counts(const lol_gpu* ctx, lol::Launch& L) {
	const lol_program& P = ctx->h_prog;
	L.n_lights = P.n_lights; L.n_materials = P.n_materials; L.n_roots = P.n_roots;
}
static void context_launch_fields(const lol_gpu* ctx, lol::Launch& L) {
	launch_counts(ctx, L);
	if (ctx->gamma_table) { L.flags |= lol::FLAG_GAMMA_TABLE; L.gamma_table = ctx->d_gamma; }
	L.fmt_shift = ctx->fmt_shift; L.fmt_loss = ctx->fmt_loss; L.fmt_amask = ctx->fmt_amask;
}

/* The part of a launch that is the uploaded scene's and the context's: program and tables, ambient, the exact skips that hold for
 * every camera, context_launch_fields' part, the diagnostics' buffers.  What depends on the camera (which copy of the
 * macro-op list, FLAG_SHADOW_SETTLED, the first step) is the caller's: per frame, or per view of a batch. */
static void scene_launch_fields(const lol_gpu* ctx, const lol_gpu_debug* dbg, lol::Launch& L) {
	const lol_program& P = ctx->h_prog;
	L.flags = (ctx->miss_skip ? lol::FLAG_MISS_SKIP : 0u) | (ctx->dark_skip ? lol::FLAG_DARK_SKIP : 0u);
	context_launch_fields(ctx, L);
	L.n_ops = ctx->n_mops;
	L.ops   = ctx->d_mops[ctx->cur];
	launch_tables(L, ctx->d_tables[ctx->cur]);
	L.ambient[0] = P.ambient_color.x; L.ambient[1] = P.ambient_color.y; L.ambient[2] = P.ambient_color.z;
	if (dbg) {
		L.dbg_rgb = dbg->rgb; L.dbg_hit_dist = dbg->hit_dist;
		L.dbg_hit_id = dbg->hit_id; L.dbg_steps = dbg->steps;
	}
}

/* Pass 1 of an adaptive frame or batch, from `A`, the launch of the whole supersampled one: one sample per pixel, whole frames,
 * dense XRGB8888 into `xrgb` and the object ids into `ids` (the diagnostic colour straight into the caller's buffer) */
static lol::Launch plain_pass_of(const lol::Launch& A, uint32_t* xrgb, uint32_t* ids, const lol_gpu_debug* dbg) {
	lol::Launch L = A;
	L.fw = (float)A.w; L.fh = (float)A.h;
	L.flags &= ~(lol::FLAG_SAMPLES_2 | lol::FLAG_SAMPLES_4);
	L.n_rows = A.h; L.band_rows = A.h; L.cycle_rows = A.h; L.offset_rows = 0;
	L.dst = xrgb; L.pitch_px = (uint32_t)A.w;
	L.fmt_shift = 16u | 8u << 8; L.fmt_loss = 0; L.fmt_amask = 0;
	L.dbg_rgb = dbg ? dbg->rgb : nullptr; L.dbg_hit_dist = nullptr; L.dbg_hit_id = ids; L.dbg_steps = nullptr;
	return L;
}

/*
 * An adaptive frame (lol_gpu_set_adaptive_samples): three launches on `s`, no host wait between them.  `A` = the launch of the
 * whole supersampled frame (lol_gpu_render_device).
 *  1. the plain frame P into the scratch set: XRGB8888 pixels and object ids, by the non-counting kernel (the diagnostic colour
 *     straight into the caller's buffer), in a fixed tile order — the longest-first tables and AUTO's trials are left alone;
 *  2. adaptive_classify: the mask; unrefined pixels go to `dst`, refined ones to the list;
 *  3. the refine pass (lol_kernel_aa.h, render_aa_list) over the list, on a grid that fills the device — the list's length stays
 *     on the device.
 * Scratch: the next set of the ring, after the frame that used it last (hipStreamWaitEvent: frames on other streams, frames in
 * flight); the host waits for that frame only where the set has to grow, or where this frame goes to one of HIP's special stream
 * handles and that frame has not finished.
 */
static int render_adaptive(lol_gpu* ctx, const lol::Launch& A, const lol_gpu_debug* dbg, hipStream_t s) {
	const int w = A.w, h = A.h, ss = ctx->samples;
	const size_t px = (size_t)w * h;
	LOL_TRY(ensure_refine_grid(ctx));
	const uint32_t per_wave = 64u / (uint32_t)(ss * ss);
	const uint32_t blocks = (uint32_t)std::min<size_t>(ctx->adaptive_blocks, (px + per_wave - 1) / per_wave);
	lol_gpu::AdaptiveFrameSet& S = ctx->adaptive_frames.next();
	for (hipEvent_t& ev : S.ev) LOL_TRY(ensure_event(ctx, &ev, true));
	const size_t need = (3 * px + 64 + (size_t)ctx->adaptive_blocks * 64) * 4;
	LOL_TRY(ring_take(ctx, S, need, need, RING_TIMED, s, nullptr, "scratch of an adaptive frame"));
	uint32_t* xrgb = S.d_buf;
	uint32_t* ids = xrgb + px;
	uint32_t* list = ids + px;
	uint32_t* count = list + px;
	uint32_t* lanes = count + 64;
	/* from here on things are queued on `s`: whatever fails, the rest is skipped and the set's `done` recorded behind what is there */
	const char* what = "hipEventRecord (adaptive frame)";
	hipError_t e = hipEventRecord(S.ev[0], s);
	if (e == hipSuccess) { what = "hipMemsetAsync (adaptive frame)"; e = hipMemsetAsync(count, 0, 4, s); }

	/* 1. the plain frame */
	if (e == hipSuccess) {
		lol::Launch L = plain_pass_of(A, xrgb, ids, dbg);
		dim3 grid((w + lol::TILE_W - 1) / lol::TILE_W, (h + lol::TILE_H - 1) / lol::TILE_H);
		if (ctx->tiles.mode == LOL_GPU_TILES_COLS) {
			L.flags |= lol::FLAG_TILE_COLS;
			const unsigned t = grid.x; grid.x = grid.y; grid.y = t;
		}
		what = "kernel launch (adaptive frame, plain pass)";
		void* args[] = { &L };
		e = launch_family(ctx, FAM_FRAME, false, args, grid, s);
	}
	if (e == hipSuccess) { what = "hipEventRecord (adaptive frame)"; e = hipEventRecord(S.ev[1], s); }
	/* 2. classify and compact */
	if (e == hipSuccess) {
		what = "kernel launch (adaptive frame, classify pass)";
		hipLaunchKernelGGL(adaptive_classify, dim3((w + CLASSIFY_W - 1) / CLASSIFY_W, (h + CLASSIFY_H - 1) / CLASSIFY_H), dim3(64), 0, s,
		                   xrgb, ids, w, h, ctx->adaptive, A.dst, A.pitch_px, A.fmt_shift, A.fmt_loss, A.fmt_amask, list, count);
		e = hipGetLastError();
	}
	if (e == hipSuccess) { what = "hipEventRecord (adaptive frame)"; e = hipEventRecord(S.ev[2], s); }
	/* 3. the s x s pixels of the list */
	if (e == hipSuccess) {
		lol::Launch R = A;
		R.n_rows = h; R.band_rows = h; R.cycle_rows = h; R.offset_rows = 0;
		R.tile_order = ctx->d_adaptive_order; R.tile_stride = ctx->adaptive_stride; R.lane_pixels = lanes;
		what = "kernel launch (adaptive frame, refine pass)";
		void* args[] = { &R, &list, &count };
		e = launch_family(ctx, FAM_FRAME_AA_LIST, false, args, dim3(blocks), s);
	}
	S.d_count = count;
	ctx->adaptive_last = &S;
	return ring_done(ctx, S, s, e, what);
}

int lol_gpu_render_device(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps,
                          const lol_gpu_rows* rows, void* dst, size_t pitch_bytes,
                          const lol_gpu_debug* dbg, void* stream) {
	if (!ctx || !cam || !dst) return LOL_GPU_ERR_ARG;
	if (!ctx->have_prog) return fail(ctx, LOL_GPU_ERR_NO_PROGRAM, "no scene program uploaded");
	if (w <= 0 || h <= 0 || max_steps < 0 || pitch_bytes % 4 || pitch_bytes < (size_t)w * 4)
		return fail(ctx, LOL_GPU_ERR_ARG, "bad frame geometry");
	lol_gpu_rows whole = { h, h, 0 };
	const lol_gpu_rows* R = rows ? rows : &whole;
	int n_rows = lol_gpu_part_rows(h, R);
	if (n_rows < 0) return fail(ctx, LOL_GPU_ERR_ARG, "bad row partition");
	/* supersampling (lol_gpu_set_samples): s x s samples per pixel, one lane each — the kernel's grid covers the s w x s n_rows
	 * samples, and a pixel of several samples has no single hit distance, object or step count */
	const int ss = ctx->samples;
	const bool aa = ss > 1;
	if (aa && dbg && (dbg->hit_dist || dbg->hit_id || dbg->steps))
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "hit_dist, hit_id and steps have no single value for a supersampled pixel (lol_gpu_set_samples)");
	if (aa && ((long long)ss * w > (1 << 24) || (long long)ss * h > (1 << 24) ||
	           ((long long)ss * n_rows + lol::TILE_H - 1) / lol::TILE_H > 65535 || ((long long)ss * w + lol::TILE_W - 1) / lol::TILE_W > 65535))
		return fail(ctx, LOL_GPU_ERR_ARG, "frame too large for its samples per pixel");
	/* adaptive supersampling (lol_gpu_set_adaptive_samples): a pixel's mask reads its neighbours' rows, so whole frames only; the
	 * refine pass finds its samples through shade_pixel's pixel table (lol_kernel_aa.h, render_aa_list): 16-bit columns, 15-bit rows */
	const bool adaptive = aa && ctx->adaptive >= 0;
	if (adaptive && n_rows != h)
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "adaptive frames are whole frames: a row partition needs halo rows (lol_gpu_set_adaptive_samples)");
	if (adaptive && ((long long)ss * w > 65536 || (long long)ss * h > 32768))
		return fail(ctx, LOL_GPU_ERR_ARG, "frame too large for adaptive supersampling (s w <= 65536, s h <= 32768)");
	if (n_rows == 0) return LOL_GPU_OK;
	/* h need not be a multiple of cycle_rows: a part's band in the last, partial cycle is cut or absent, and it is the
	 * part's last, so every part's local rows stay dense (lol_gpu_part_frame_row is the mapping) */

	lol::Launch L;
	memset(&L, 0, sizeof L);
	memcpy(&L.cam, cam, sizeof L.cam);
	L.fw = (float)(ss * w); L.fh = (float)(ss * h);      /* AA: the size of the sample grid (the camera's aspect ratio is the same rational) */
	L.w = w; L.h = h; L.max_steps = max_steps;
	L.n_rows = n_rows;
	L.band_rows = R->band_rows; L.cycle_rows = R->cycle_rows; L.offset_rows = R->offset_rows;
	scene_launch_fields(ctx, dbg, L);
	const bool first = first_step(ctx, *cam, max_steps);
	if (camera_fields(L, *cam, ctx->finite_scene, ctx->shadow_settle, first, ctx->first_dist, ctx->first_id)) L.ops += (size_t)ctx->n_mops * lol::MOP_DWORDS;
	if (aa) L.flags |= ss == 4 ? lol::FLAG_SAMPLES_4 : lol::FLAG_SAMPLES_2;
	L.dst = static_cast<uint32_t*>(dst);
	L.pitch_px = (uint32_t)(pitch_bytes / 4);

	/* LOL_GPU_STREAM_DEFAULT == hipStreamLegacy; NULL = the context's own stream(s), in turn (lol_gpu_set_frames_in_flight) */
	hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->frame_streams[ctx->frame_rr++ % (unsigned)ctx->n_frame_streams];
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	finish_specialise(ctx, false);           /* the frame boundary at which a finished scene kernel takes over */
	const int tile_w = lol::TILE_W, tile_h = lol::TILE_H;      /* both kernels: one 16 x 4 wave per block (lol_kernel.h) */
	const int block = tile_w * tile_h;
	dim3 grid((ss * w + tile_w - 1) / tile_w, (ss * n_rows + tile_h - 1) / tile_h);
	if (adaptive) return render_adaptive(ctx, L, dbg, s);
	int trial = -1;
	bool table = false;
	if (aa) {
		/* Supersampled frames go in a fixed order — columns where the host asked for them, rows otherwise — and leave the longest-first
		 * tables and AUTO's trials alone: a plain frame after them is scheduled as if they had not been there. */
		if (ctx->tiles.mode == LOL_GPU_TILES_COLS) {
			L.flags |= lol::FLAG_TILE_COLS;
			const unsigned t = grid.x; grid.x = grid.y; grid.y = t;
		}
	} else if (ctx->tiles.mode == LOL_GPU_TILES_LPT) {
		FrameTables F;
		if ((table = lpt_table_for_frame(ctx, cam, w, h, max_steps, R, n_rows, block, s, &F))) {
			L.flags |= lol::FLAG_TILE_TABLE;
			L.tile_order = F.order;
			L.tile_cost = F.cost;
			L.tile_stride = (F.n_waves + 7u) >> 3;
			L.lane_pixels = F.lanes;
			L.pixel_cost = F.pixel_cost;
			grid = dim3(F.n_waves, 1);
		}
	}
	if (!table && !aa) ctx->lpt_last_set = -1;
	/* (longest-first without a table — the camera moves, or another stream —: the better of the two fixed orders, like AUTO) */
	if (!table && !aa && tile_order_for_frame(ctx, w, h, max_steps, R, dbg != nullptr, &trial) == LOL_GPU_TILES_COLS) {
		L.flags |= lol::FLAG_TILE_COLS;
		const unsigned t = grid.x; grid.x = grid.y; grid.y = t;      /* (both stay far below the 65535 blocks a grid may have in y) */
	}
	if (trial >= 0) LOL_HIP(ctx, hipEventRecord(ctx->tiles.ev[2 * trial], s));
	g_roctx.init();
	if (g_roctx.push) {
		char label[96];
		snprintf(label, sizeof label, "lol frame %dx%d rows=%d band=%d@%d/%d %s", w, h, n_rows, R->band_rows, R->offset_rows, R->cycle_rows, kernel_name(ctx));
		g_roctx.push(label);
		g_roctx.ranges++;
	}
	void* args[] = { &L };
	const hipError_t e = launch_family(ctx, aa ? FAM_FRAME_AA : FAM_FRAME, (dbg && dbg->steps) || L.pixel_cost, args, grid, s);
	if (g_roctx.pop) g_roctx.pop();
	if (e != hipSuccess) return fail(ctx, LOL_GPU_ERR_HIP, "kernel launch", e);
	if (table) lpt_frame_queued(ctx, s);
	if (trial >= 0) LOL_HIP(ctx, hipEventRecord(ctx->tiles.ev[2 * trial + 1], s));
	return LOL_GPU_OK;
}

/*
 * A batch of views: ONE render launch whose grid has the view as its z coordinate (lol_kernel_batch.h), behind one copy of the view
 * records on the same stream.  Everything lol_gpu_render_device decides per frame from the camera is decided here per view and
 * goes into the view's record: which copy of the macro-op list, FLAG_SHADOW_SETTLED (camera_sane), FLAG_FIRST_STEP and its value
 * (first_step).  Fixed tile order; the longest-first tables, AUTO's trials and what they remember of the last frame are neither
 * read nor written.  Records: the next set of their ring (lol_gpu_internal.h, lol_gpu::view_records).
 *
 * The pieces, shared by lol_gpu_render_views and lol_gpu_render_views_samples: what both refuse (batch_refused), the launch of a
 * whole frame of the batch's size with one sample per pixel (batch_launch), the view records queued on the batch's stream
 * (queue_view_records) and the event behind the batch's last launch (ring_done).
 */
static int batch_refused(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int w, int h, int max_steps, const void* dst, size_t pitch_bytes,
                         size_t view_stride_bytes) {
	if (!ctx || !cams || !dst) return LOL_GPU_ERR_ARG;
	if (!ctx->have_prog) return fail(ctx, LOL_GPU_ERR_NO_PROGRAM, "no scene program uploaded");
	if (n_views < 1 || n_views > LOL_GPU_MAX_VIEWS) return fail(ctx, LOL_GPU_ERR_ARG, "a batch holds 1 ... LOL_GPU_MAX_VIEWS views");
	if (w <= 0 || h <= 0 || max_steps < 0 || pitch_bytes % 4 || pitch_bytes < (size_t)w * 4 ||
	    view_stride_bytes % 4 || view_stride_bytes / pitch_bytes < (size_t)h)
		return fail(ctx, LOL_GPU_ERR_ARG, "bad batch geometry");
	return LOL_GPU_OK;
}

/* the grid of a batch over a grid of gw x gh pixels or samples per view (transposed under LOL_GPU_TILES_COLS: batch_launch sets the
 * flag), or false: a grid has at most 65535 blocks in y and z, and HIP takes at most 2^32 - 1 threads per launch */
static bool batch_grid(const lol_gpu* ctx, long long gw, long long gh, int n_views, dim3* grid) {
	const long long tx = (gw + lol::TILE_W - 1) / lol::TILE_W, ty = (gh + lol::TILE_H - 1) / lol::TILE_H;
	if (tx > 65535 || ty > 65535 || (unsigned long long)tx * (unsigned long long)ty * (unsigned)n_views * (unsigned)lol::BLOCK > 0xFFFFFFFFull) return false;
	const bool cols = ctx->tiles.mode == LOL_GPU_TILES_COLS;
	*grid = dim3((unsigned)(cols ? ty : tx), (unsigned)(cols ? tx : ty), (unsigned)n_views);
	return true;
}

static void batch_launch(const lol_gpu* ctx, int w, int h, int max_steps, void* dst, size_t pitch_bytes, const lol_gpu_debug* dbg, lol::Launch& L) {
	memset(&L, 0, sizeof L);
	L.fw = (float)w; L.fh = (float)h;
	L.w = w; L.h = h; L.max_steps = max_steps;
	L.n_rows = h; L.band_rows = h; L.cycle_rows = h; L.offset_rows = 0;
	scene_launch_fields(ctx, dbg, L);                        /* (ops: + View::ops_offset) */
	if (ctx->tiles.mode == LOL_GPU_TILES_COLS) L.flags |= lol::FLAG_TILE_COLS;
	L.dst = static_cast<uint32_t*>(dst);
	L.pitch_px = (uint32_t)(pitch_bytes / 4);
}

/* LOL_GPU_STREAM_DEFAULT == hipStreamLegacy; NULL = the context's own stream(s), in turn.  Makes the context's device current and
 * takes a finished scene kernel over: the frame boundary. */
static int batch_stream(lol_gpu* ctx, void* stream, hipStream_t* s) {
	*s = stream ? static_cast<hipStream_t>(stream) : ctx->frame_streams[ctx->frame_rr++ % (unsigned)ctx->n_frame_streams];
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	finish_specialise(ctx, false);
	return LOL_GPU_OK;
}

/* the view records of a batch: the next set of the ring filled — everything a frame decides from its camera, per record — and its
 * copy to the device queued on `s`.  The batch's last launch goes to ring_done with the set. */
static int queue_view_records(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int max_steps, hipStream_t s, RingSet** out) {
	RingSet& S = ctx->view_records.next();
	const size_t bytes = (size_t)n_views * sizeof(lol::View);
	LOL_TRY(ring_take(ctx, S, bytes, std::max<size_t>(64, (size_t)n_views) * sizeof(lol::View), RING_PINNED, s, nullptr, "records of a batch of views"));
	lol::View* views = reinterpret_cast<lol::View*>(S.h_buf);
	for (int v = 0; v < n_views; v++) {
		lol::View& V = views[v];
		memcpy(&V.cam, &cams[v], sizeof V.cam);
		V.flags = 0u; V.first_dist = 0.f; V.first_id = 0u;
		const bool first = first_step(ctx, cams[v], max_steps);
		V.ops_offset = camera_fields(V, cams[v], ctx->finite_scene, ctx->shadow_settle, first, ctx->first_dist, ctx->first_id)
		               ? ctx->n_mops * (uint32_t)lol::MOP_DWORDS : 0u;
	}
	*out = &S;
	const hipError_t e = ring_copy(S, bytes, s);
	return e == hipSuccess ? LOL_GPU_OK : ring_done(ctx, S, s, e, "copy of the records of a batch of views");
}
static const lol::View* device_views(const RingSet* S) { return reinterpret_cast<const lol::View*>(S->d_buf); }

static void batch_range(const char* what, int n_views, int w, int h) {
	g_roctx.init();
	if (g_roctx.push) {
		char label[96];
		snprintf(label, sizeof label, "lol %s %d x %dx%d", what, n_views, w, h);
		g_roctx.push(label);
		g_roctx.ranges++;
	}
}

/* lol_gpu_render_views without its look at lol_gpu_set_samples */
static int render_views_plain(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int w, int h, int max_steps,
                              void* dst, size_t pitch_bytes, size_t view_stride_bytes, const lol_gpu_debug* dbg, void* stream) {
	dim3 grid;
	if (!batch_grid(ctx, w, h, n_views, &grid))
		return fail(ctx, LOL_GPU_ERR_ARG, "batch too large for one launch: fewer views per call");
	lol::Launch L;
	batch_launch(ctx, w, h, max_steps, dst, pitch_bytes, dbg, L);
	hipStream_t s;
	LOL_TRY(batch_stream(ctx, stream, &s));
	RingSet* S = nullptr;
	LOL_TRY(queue_view_records(ctx, cams, n_views, max_steps, s, &S));
	lol::BatchTail B = { device_views(S), (unsigned long long)(view_stride_bytes / 4) };
	batch_range("batch", n_views, w, h);
	void* args[] = { &L, &B };
	const hipError_t e = launch_family(ctx, FAM_BATCH, dbg && dbg->steps, args, grid, s);
	if (g_roctx.pop) g_roctx.pop();
	return ring_done(ctx, *S, s, e, "kernel launch (batch of views)");
}

int lol_gpu_render_views(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int w, int h, int max_steps,
                         void* dst, size_t pitch_bytes, size_t view_stride_bytes, const lol_gpu_debug* dbg, void* stream) {
	LOL_TRY(batch_refused(ctx, cams, n_views, w, h, max_steps, dst, pitch_bytes, view_stride_bytes));
	if (ctx->samples > 1)
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "batches of views are one sample per pixel (lol_gpu_set_samples): lol_gpu_render_views_samples");
	return render_views_plain(ctx, cams, n_views, w, h, max_steps, dst, pitch_bytes, view_stride_bytes, dbg, stream);
}

/*
 * An adaptive batch: what render_adaptive does for a frame, for every view of a batch — four launches on `s` behind the copy of
 * the view records, no host wait between them.  `A` = the launch of the whole supersampled batch.
 *  1. the plain batch P into the scratch set, dense: XRGB8888 pixels and object ids (the diagnostic colour straight into the
 *     caller's buffer), by the batch kernel as lol_gpu_render_views runs it;
 *  2. adaptive_classify_views: every view's mask from its own pixels; unrefined pixels go to `dst`, refined ones to the view's list;
 *  3. view_group_prefix: the lists' lengths into the numbering of their groups;
 *  4. the refine pass (lol_kernel_batch_aa.h, render_aa_view_lists) on a grid that fills the device.
 * Scratch: the next set of a ring of its own (lol_gpu_internal.h, lol_gpu::adaptive_batches), under the rings' protocol (ring_take).
 */
static int render_views_adaptive(lol_gpu* ctx, const lol::Launch& A, const lol_frame_camera* cams, int n_views, int samples, int contrast,
                                 size_t view_stride_bytes, const lol_gpu_debug* dbg, hipStream_t s) {
	const int w = A.w, h = A.h;
	const size_t px = (size_t)w * h, all = px * (size_t)n_views;
	LOL_TRY(ensure_refine_grid(ctx));
	const uint32_t per_wave = 64u / (uint32_t)(samples * samples);
	/* (every view's list ends with a group that may be partly filled: at most n_views groups more than the entries need) */
	const uint32_t blocks = (uint32_t)std::min<size_t>(ctx->adaptive_blocks, (px + per_wave - 1) / per_wave * (size_t)n_views);
	lol_gpu::AdaptiveBatchSet& S = ctx->adaptive_batches.next();
	const size_t need = (3 * all + 2 * ((size_t)n_views + 1) + (size_t)ctx->adaptive_blocks * 64) * 4;
	LOL_TRY(ring_take(ctx, S, need, need, RING_SCRATCH, s, &ctx->fail_view_scratch, "scratch of an adaptive batch"));
	uint32_t* xrgb = S.d_buf;
	uint32_t* ids = xrgb + all;
	uint32_t* lists = ids + all;
	uint32_t* counts = lists + all;
	uint32_t* prefix = counts + n_views + 1;
	uint32_t* lanes = prefix + n_views + 1;
	RingSet* V = nullptr;
	LOL_TRY(queue_view_records(ctx, cams, n_views, A.max_steps, s, &V));
	const char* what = "hipMemsetAsync (adaptive batch)";
	hipError_t e = hipMemsetAsync(counts, 0, ((size_t)n_views + 1) * 4, s);

	/* 1. the plain batch */
	if (e == hipSuccess) {
		lol::Launch L = plain_pass_of(A, xrgb, ids, dbg);
		lol::BatchTail B = { device_views(V), (unsigned long long)px };
		dim3 grid;
		(void)batch_grid(ctx, w, h, n_views, &grid);      /* (a part of the sample grid the caller has checked) */
		what = "kernel launch (adaptive batch, plain pass)";
		void* args[] = { &L, &B };
		e = launch_family(ctx, FAM_BATCH, false, args, grid, s);
	}
	/* 2. classify and compact, view by view */
	if (e == hipSuccess) {
		what = "kernel launch (adaptive batch, classify pass)";
		hipLaunchKernelGGL(adaptive_classify_views, dim3((w + CLASSIFY_W - 1) / CLASSIFY_W, (h + CLASSIFY_H - 1) / CLASSIFY_H, n_views), dim3(64), 0, s,
		                   xrgb, ids, w, h, contrast, A.dst, A.pitch_px, (unsigned long long)(view_stride_bytes / 4), A.fmt_shift, A.fmt_loss,
		                   A.fmt_amask, lists, counts);
		e = hipGetLastError();
	}
	/* 3. the groups' numbering */
	if (e == hipSuccess) {
		what = "kernel launch (adaptive batch, group prefix)";
		hipLaunchKernelGGL(view_group_prefix, dim3(1), dim3(64), 0, s, counts, (uint32_t)n_views, per_wave, prefix);
		e = hipGetLastError();
	}
	/* 4. the s x s pixels of the lists */
	if (e == hipSuccess) {
		lol::Launch R = A;
		R.flags &= ~lol::FLAG_TILE_COLS;                  /* (a one-dimensional grid) */
		R.tile_order = ctx->d_adaptive_order; R.tile_stride = ctx->adaptive_stride; R.lane_pixels = lanes;
		lol::BatchTail B = { device_views(V), (unsigned long long)(view_stride_bytes / 4) };
		lol::BatchLists Q = { lists, counts, prefix, (uint32_t)n_views };
		what = "kernel launch (adaptive batch, refine pass)";
		void* args[] = { &R, &B, &Q };
		e = launch_family(ctx, FAM_BATCH_AA_LIST, false, args, dim3(blocks), s);
	}
	S.d_counts = counts; S.n_views = n_views;
	ctx->view_adaptive_last = &S;
	return ring_done(ctx, S, s, e, what, V);
}

/*
 * A supersampled batch of views: lol_gpu_render_views with s x s samples per pixel — on every pixel (contrast -1: ONE launch over
 * the sample grids of all views, lol_kernel_batch_aa.h) or on the pixels the adaptive definition refines (render_views_adaptive).
 * The samples are arguments: lol_gpu_set_samples / lol_gpu_set_adaptive_samples are neither read nor changed.
 */
int lol_gpu_render_views_samples(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int w, int h, int max_steps,
                                 int samples, int contrast, void* dst, size_t pitch_bytes, size_t view_stride_bytes,
                                 const lol_gpu_debug* dbg, void* stream) {
	if (!ctx || !cams || !dst) return LOL_GPU_ERR_ARG;
	if (samples != 1 && samples != 2 && samples != 4) return fail(ctx, LOL_GPU_ERR_ARG, "samples per axis must be 1, 2 or 4");
	if (contrast < -1 || contrast > 255) return fail(ctx, LOL_GPU_ERR_ARG, "adaptive contrast must be -1 (off) or 0 ... 255");
	LOL_TRY(batch_refused(ctx, cams, n_views, w, h, max_steps, dst, pitch_bytes, view_stride_bytes));
	if (samples == 1) return render_views_plain(ctx, cams, n_views, w, h, max_steps, dst, pitch_bytes, view_stride_bytes, dbg, stream);
	const bool adaptive = contrast >= 0;
	if (!lol::samples_fit_wave(samples))
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "this build's wave patch (LOL_WAVE_W x LOL_WAVE_H) does not divide into that many samples per axis");
	if (adaptive && lol::BLOCK != 64)
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "adaptive batches need one-wave blocks (this build's LOL_WAVES_X is not 1)");
	if (dbg && (dbg->hit_dist || dbg->hit_id || dbg->steps))
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "hit_dist, hit_id and steps have no single value for a supersampled pixel");
	/* the launch is counted in SAMPLES: the grid of the kernel that shades every pixel's (an adaptive batch shades a part of it) */
	dim3 grid;
	if (!batch_grid(ctx, (long long)samples * w, (long long)samples * h, n_views, &grid))
		return fail(ctx, LOL_GPU_ERR_ARG, "batch too large for one launch in samples: fewer views per call");
	/* ... and the refine pass finds its samples through shade_pixel's pixel table (lol_kernel_aa.h, render_aa_list) */
	if (adaptive && ((long long)samples * w > 65536 || (long long)samples * h > 32768))
		return fail(ctx, LOL_GPU_ERR_ARG, "views too large for adaptive supersampling (s w <= 65536, s h <= 32768)");

	lol::Launch L;
	batch_launch(ctx, w, h, max_steps, dst, pitch_bytes, dbg, L);
	L.fw = (float)(samples * w); L.fh = (float)(samples * h);      /* the size of the sample grid */
	L.flags |= samples == 4 ? lol::FLAG_SAMPLES_4 : lol::FLAG_SAMPLES_2;
	hipStream_t s;
	LOL_TRY(batch_stream(ctx, stream, &s));
	if (adaptive) return render_views_adaptive(ctx, L, cams, n_views, samples, contrast, view_stride_bytes, dbg, s);
	RingSet* S = nullptr;
	LOL_TRY(queue_view_records(ctx, cams, n_views, max_steps, s, &S));
	lol::BatchTail B = { device_views(S), (unsigned long long)(view_stride_bytes / 4) };
	batch_range("supersampled batch", n_views, w, h);
	void* args[] = { &L, &B };
	const hipError_t e = launch_family(ctx, FAM_BATCH_AA, false, args, grid, s);
	if (g_roctx.pop) g_roctx.pop();
	return ring_done(ctx, *S, s, e, "kernel launch (supersampled batch of views)");
}

/* what lol_gpu_render_views_blend refuses before it looks at anything else, in its order (everything lol_gpu_render_views refuses
 * first: no program before any word about K) */
static int blend_refused(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int K, int w, int h, int max_steps, const void* dst,
                         size_t pitch_bytes, size_t view_stride_bytes) {
	LOL_TRY(batch_refused(ctx, cams, n_views, w, h, max_steps, dst, pitch_bytes, view_stride_bytes));
	if (K != 1 && K != 2 && K != 4 && K != 8 && K != 16) return fail(ctx, LOL_GPU_ERR_ARG, "cameras per view must be 1, 2, 4, 8 or 16");
	if ((long long)n_views * K > LOL_GPU_MAX_VIEWS) return fail(ctx, LOL_GPU_ERR_ARG, "a blend holds at most LOL_GPU_MAX_VIEWS cameras in all");
	return LOL_GPU_OK;
}

/*
 * Views averaged over K cameras: two launches on `s` behind ONE copy of the n K records, no host wait between them.
 *  1. the linear-colour batch kernel (lol_kernel_blend.h) over z = v K + k, into the scratch set: everything a batch decides per
 *     view is decided per RECORD (queue_view_records), so a group may mix sane and insane cameras;
 *  2. blend_resolve: each pixel's tree over its K colours, gamma, packing, the stores.
 * Scratch: the next set of a ring of its own (lol_gpu_internal.h, lol_gpu::blends), under the rings' protocol (ring_take).  Fixed
 * tile order, like any batch.
 * K > 1 here, and `samples` x `samples` samples per pixel: with samples > 1 pass 1 is the supersampled linear kernel
 * (lol_kernel_blend_aa.h) over the SAMPLE grids, on the launch of lol_gpu_render_views_samples.  It reduces a pixel's samples in
 * registers before it stores, so the scratch holds one LinearColour per PIXEL and record either way: the ring and the resolve pass
 * are the same for both.
 */
/* pass 2 of a blend (blend_resolve) behind pass 1's launch `L`, whose scratch `lin` holds the linear colours [v K + k][y][x] */
static hipError_t launch_blend_resolve(const lol_gpu* ctx, const lol::Launch& L, const uint32_t* scratch, int n_views, int K, int w, int h, void* dst,
                                       size_t pitch_bytes, size_t view_stride_bytes, const lol_gpu_debug* dbg, hipStream_t s) {
	const BlendOut O = { static_cast<uint32_t*>(dst), (uint32_t)(pitch_bytes / 4), (unsigned long long)(view_stride_bytes / 4),
	                     ctx->fmt_shift, ctx->fmt_loss, ctx->fmt_amask, L.flags & lol::FLAG_GAMMA_TABLE,
	                     dbg ? dbg->rgb : nullptr, L.gamma_table };
	const lol::LinearColour* lin = reinterpret_cast<const lol::LinearColour*>(scratch);
	const dim3 rgrid((w + CLASSIFY_W - 1) / CLASSIFY_W, (h + CLASSIFY_H - 1) / CLASSIFY_H, n_views);
	switch (K) {
	case 2:  hipLaunchKernelGGL(blend_resolve<2>, rgrid, dim3(64), 0, s, lin, w, h, O); break;
	case 4:  hipLaunchKernelGGL(blend_resolve<4>, rgrid, dim3(64), 0, s, lin, w, h, O); break;
	case 8:  hipLaunchKernelGGL(blend_resolve<8>, rgrid, dim3(64), 0, s, lin, w, h, O); break;
	default: hipLaunchKernelGGL(blend_resolve<16>, rgrid, dim3(64), 0, s, lin, w, h, O); break;
	}
	return hipGetLastError();
}

static int render_blend(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int K, int w, int h, int max_steps, int samples,
                        void* dst, size_t pitch_bytes, size_t view_stride_bytes, const lol_gpu_debug* dbg, void* stream) {
	if (samples > 1 && !lol::samples_fit_wave(samples))
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "this build's wave patch (LOL_WAVE_W x LOL_WAVE_H) does not divide into that many samples per axis");
	if (dbg && (dbg->hit_dist || dbg->hit_id || dbg->steps))
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "hit_dist, hit_id and steps have no single value for a pixel averaged over cameras");
	const int n_rays = n_views * K;
	dim3 grid;
	if (!batch_grid(ctx, (long long)samples * w, (long long)samples * h, n_rays, &grid))
		return fail(ctx, LOL_GPU_ERR_ARG, samples > 1 ? "blend too large for one launch in samples over all its cameras: fewer views per call"
		                                              : "blend too large for one launch over all its cameras: fewer views per call");
	hipStream_t s;
	LOL_TRY(batch_stream(ctx, stream, &s));
	RingSet& S = ctx->blends.next();
	const size_t need = (size_t)n_rays * (size_t)w * (size_t)h * sizeof(lol::LinearColour);
	LOL_TRY(ring_take(ctx, S, need, need, RING_SCRATCH, s, &ctx->fail_view_scratch, "scratch of a blend of views"));
	RingSet* V = nullptr;
	LOL_TRY(queue_view_records(ctx, cams, n_rays, max_steps, s, &V));
	batch_range(samples > 1 ? "supersampled blend" : "blend", n_rays, w, h);
	/* 1. the linear colours: the launch's destination is the scratch (no diagnostics: they are the resolve's) */
	lol::Launch L;
	batch_launch(ctx, w, h, max_steps, S.d_buf, (size_t)w * 4, nullptr, L);
	if (samples > 1) {
		L.fw = (float)(samples * w); L.fh = (float)(samples * h);      /* the size of the sample grid */
		L.flags |= samples == 4 ? lol::FLAG_SAMPLES_4 : lol::FLAG_SAMPLES_2;
	}
	lol::BatchTail B = { device_views(V), 0ull };
	const char* what = "kernel launch (blend of views, linear pass)";
	void* args[] = { &L, &B };
	hipError_t e = launch_family(ctx, samples > 1 ? FAM_BATCH_AA_LIN : FAM_BATCH_LIN, false, args, grid, s);
	/* 2. the means */
	if (e == hipSuccess) {
		what = "kernel launch (blend of views, resolve pass)";
		e = launch_blend_resolve(ctx, L, S.d_buf, n_views, K, w, h, dst, pitch_bytes, view_stride_bytes, dbg, s);
	}
	if (g_roctx.pop) g_roctx.pop();
	return ring_done(ctx, S, s, e, what, V);
}

int lol_gpu_render_views_blend(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int cams_per_view, int w, int h, int max_steps,
                               void* dst, size_t pitch_bytes, size_t view_stride_bytes, const lol_gpu_debug* dbg, void* stream) {
	LOL_TRY(blend_refused(ctx, cams, n_views, cams_per_view, w, h, max_steps, dst, pitch_bytes, view_stride_bytes));
	if (cams_per_view == 1) return render_views_plain(ctx, cams, n_views, w, h, max_steps, dst, pitch_bytes, view_stride_bytes, dbg, stream);
	return render_blend(ctx, cams, n_views, cams_per_view, w, h, max_steps, 1, dst, pitch_bytes, view_stride_bytes, dbg, stream);
}

/*
 * A supersampled blend: s x s samples under each of K cameras.  s = 1 IS lol_gpu_render_views_blend — the same two functions behind
 * the same refusals, render_views_plain for K = 1 (all diagnostics) and render_blend with one sample — and K = 1 IS
 * lol_gpu_render_views_samples without a contrast, which is called.  Otherwise render_blend with the supersampled linear kernel in
 * pass 1: 1 / s^2 per camera there, the tree over the cameras in blend_resolve.
 */
int lol_gpu_render_views_blend_samples(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int cams_per_view, int w, int h,
                                       int max_steps, int samples, void* dst, size_t pitch_bytes, size_t view_stride_bytes,
                                       const lol_gpu_debug* dbg, void* stream) {
	if (!ctx || !cams || !dst) return LOL_GPU_ERR_ARG;
	if (samples != 1 && samples != 2 && samples != 4) return fail(ctx, LOL_GPU_ERR_ARG, "samples per axis must be 1, 2 or 4");
	LOL_TRY(blend_refused(ctx, cams, n_views, cams_per_view, w, h, max_steps, dst, pitch_bytes, view_stride_bytes));
	/* s = 1: what lol_gpu_render_views_blend does behind the refusals just made */
	if (samples == 1 && cams_per_view == 1)
		return render_views_plain(ctx, cams, n_views, w, h, max_steps, dst, pitch_bytes, view_stride_bytes, dbg, stream);
	/* K = 1: the supersampled batch (its own refusals — the wave patch, the diagnostics, the grid in samples — are still to be made) */
	if (cams_per_view == 1)
		return lol_gpu_render_views_samples(ctx, cams, n_views, w, h, max_steps, samples, -1, dst, pitch_bytes, view_stride_bytes, dbg, stream);
	return render_blend(ctx, cams, n_views, cams_per_view, w, h, max_steps, samples, dst, pitch_bytes, view_stride_bytes, dbg, stream);
}

const char* lol_gpu_view_blend_samples_kernel_name(const lol_gpu* ctx, int cams_per_view, int samples) {
	if (!ctx) return "";
	if (samples <= 1) return lol_gpu_view_blend_kernel_name(ctx, cams_per_view);
	if (cams_per_view <= 1) return lol_gpu_view_samples_kernel_name(ctx, samples, -1);
	return family_name(ctx, FAM_BATCH_AA_LIN);
}

const char* lol_gpu_view_blend_kernel_name(const lol_gpu* ctx, int cams_per_view) {
	if (!ctx) return "";
	return family_name(ctx, cams_per_view <= 1 ? FAM_BATCH : FAM_BATCH_LIN);
}

const char* lol_gpu_view_samples_kernel_name(const lol_gpu* ctx, int samples, int contrast) {
	if (!ctx) return "";
	return family_name(ctx, samples <= 1 ? FAM_BATCH : contrast >= 0 ? FAM_BATCH_AA_LIST : FAM_BATCH_AA);
}

int lol_gpu_interp_variant(lol_gpu* ctx, int* ssize, int* tables_global) {
	if (!ctx || !ssize || !tables_global) return LOL_GPU_ERR_ARG;
	if (!ctx->have_prog) return fail(ctx, LOL_GPU_ERR_NO_PROGRAM, "no scene program uploaded");
	const InterpRung r = interp_rung(ctx->h_prog);
	*ssize = r.ssize;
	*tables_global = r.tables_global ? 1 : 0;
	return LOL_GPU_OK;
}

int lol_gpu_views_refined(lol_gpu* ctx, int64_t* n) {
	if (!ctx || !n) return LOL_GPU_ERR_ARG;
	/* (`used`: the set's `done` is behind that batch, and its buffer has not been replaced since) */
	if (!ctx->view_adaptive_last || !ctx->view_adaptive_last->used) return fail(ctx, LOL_GPU_ERR_ARG, "no adaptive batch has been launched");
	lol_gpu::AdaptiveBatchSet& S = *ctx->view_adaptive_last;
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	LOL_HIP(ctx, hipEventSynchronize(S.done));
	std::vector<uint32_t> c;
	try { c.resize((size_t)S.n_views); } catch (...) { return fail(ctx, LOL_GPU_ERR_HIP, "out of host memory"); }
	LOL_HIP(ctx, hipMemcpy(c.data(), S.d_counts, c.size() * 4, hipMemcpyDeviceToHost));
	*n = 0;
	for (uint32_t v : c) *n += v;
	return LOL_GPU_OK;
}

int lol_gpu_testing_fail_view_scratch(lol_gpu* ctx, int n) {
	if (!ctx || n < 0) return LOL_GPU_ERR_ARG;
	ctx->fail_view_scratch = n;
	return LOL_GPU_OK;
}

int lol_gpu_set_pixel_format(lol_gpu* ctx, const lol_gpu_pixel_format* fmt) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	static const lol_gpu_pixel_format xrgb8888 = { 16, 8, 0, 0, 0, 0, 4, 0, 0 };
	const lol_gpu_pixel_format& f = fmt ? *fmt : xrgb8888;
	/* the reference stores a Uint32 per pixel whatever the format says (naive_renderer.c:233-235): 4-byte formats only,
	 * and SDL_MapRGB's shift formula only describes non-palettised ones */
	if (f.palettised) return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "palettised surfaces are not supported");
	if (f.bytes_per_pixel != 4) return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "only 32-bit surfaces are supported");
	if (f.r_shift > 31 || f.g_shift > 31 || f.b_shift > 31 || f.r_loss > 8 || f.g_loss > 8 || f.b_loss > 8)
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "pixel format shifts / losses out of range");
	ctx->fmt_shift = (uint32_t)f.r_shift | (uint32_t)f.g_shift << 8 | (uint32_t)f.b_shift << 16;
	ctx->fmt_loss = (uint32_t)f.r_loss | (uint32_t)f.g_loss << 8 | (uint32_t)f.b_loss << 16;
	ctx->fmt_amask = f.a_mask;
	return LOL_GPU_OK;
}

/* the context's second, third ... frame stream, created when first wanted */
static int ensure_frame_streams(lol_gpu* ctx, int n) {
	for (int i = 1; i < n && i < lol_gpu::MAX_FRAME_STREAMS; i++)
		if (!ctx->frame_streams[i]) LOL_HIP(ctx, hipStreamCreateWithFlags(&ctx->frame_streams[i], hipStreamNonBlocking));
	return LOL_GPU_OK;
}

static int ensure_copy_stream(lol_gpu* ctx) {
	if (ctx->copy_stream) return LOL_GPU_OK;
	LOL_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
	for (int i = 0; i < lol_gpu::PIPE_SLOTS; i++) {
		LOL_HIP(ctx, hipEventCreateWithFlags(&ctx->pipe_rendered[i], hipEventDisableTiming));
		LOL_HIP(ctx, hipEventCreateWithFlags(&ctx->pipe_copied[i], hipEventDisableTiming));
	}
	return LOL_GPU_OK;
}

/*
 * The surface is memory the HOST owns (SDL's window surface, main.c:182): nothing about it is remembered between
 * calls, and it is never registered with the device by this library — the HIP runtime pins the pages of a copy's
 * destination for the duration of that copy by itself and reaches PCIe line rate that way (56 GB/s into plain malloc'd
 * memory on MI355X, the same as into hipHostRegister'd memory: tools/d2h_bench.hip, profiles/r3_d2h_routes.jsonl).
 * So one frame costs kernel + copy here (C3: 1.09 + 0.59 + 0.1 ms); a host that can give the next camera early hides the
 * copy completely with lol_gpu_render_host_begin / _end below.  Two ways to hide it inside ONE call were built in round 3,
 * measured and removed (profiles/r3_host_surface_routes.md):
 *  - the surface registered once by address (hipHostRegister) and the kernel storing straight into it: +27 % per frame,
 *    but a host that unmaps and re-maps its surface at the same address behind the library's back — what SDL may do to a
 *    window surface on a resize — left the device writing into pages that were gone: the runtime aborted the process;
 *  - the frame as row chunks, chunk i copied while chunk i+1 renders: no gain — a copy into unregistered memory costs
 *    ~0.1 ms of pinning per call and did not run under the following kernels (4 chunks 3840 vs 3880 Mpixels/s, 8: 3020).
 */
int lol_gpu_render_host(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps,
                        void* host_pixels, size_t pitch_bytes) {
	if (!ctx || !host_pixels) return LOL_GPU_ERR_ARG;
	if (w <= 0 || h <= 0 || pitch_bytes < (size_t)w * 4) return fail(ctx, LOL_GPU_ERR_ARG, "bad frame geometry");
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	size_t need = (size_t)w * h * 4;
	if (need > ctx->frame_bytes) {          /* the surface may be resized between frames (main.c:182-187) */
		if (ctx->d_frame) { LOL_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->d_frame); }
		ctx->d_frame = nullptr; ctx->frame_bytes = 0;
		LOL_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_frame), need));
		ctx->frame_bytes = need;
	}
	LOL_TRY(lol_gpu_render_device(ctx, cam, w, h, max_steps, nullptr, ctx->d_frame, (size_t)w * 4, nullptr, ctx->stream));
	LOL_HIP(ctx, hipMemcpy2DAsync(host_pixels, pitch_bytes, ctx->d_frame, (size_t)w * 4, (size_t)w * 4, h,
	                              hipMemcpyDeviceToHost, ctx->stream));
	LOL_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return LOL_GPU_OK;
}

/*
 * The host-surface path with frames in flight: begin() queues frame i+1's kernel while end() copies frame i
 * into the host's surface, so the 33 MB device-to-host copy of a 4K frame (0.6 ms at PCIe Gen5 rates) runs under
 * the next frame's kernel instead of after its own.  Copies go to a stream of their own, one device framebuffer per
 * frame in flight.
 *
 * Round 5: and the KERNELS of consecutive frames go to different streams.  A frame is one launch that ends with its slowest
 * waves on half-empty SIMDs (LABNOTES.md §3.9); the reference's loop cannot start frame i+1 before frame i has been shown
 * (main.c:189-194), but a host that has handed over the next camera already can: frame i+1's first waves fill frame i's
 * tail (tools/stream_overlap_ab.py: +9 % C3, +13 % the orbit, +67 % scene.lol at 1080p).  That is what helps a camera that
 * MOVES, whose frames cannot be scheduled by their predecessors' costs; a camera that stands still keeps its schedule as
 * well — one set of tables per stream (lpt_table_for_frame).  Frames in flight: two by default, up to PIPE_SLOTS after
 * lol_gpu_set_frames_in_flight(ctx, n).  What keeps a framebuffer safe is events, not stream order: a slot's kernel
 * waits for the copy that last read the slot, a slot's copy for the kernel that wrote it.
 */
int lol_gpu_render_host_begin(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps) {
	if (!ctx || !cam) return LOL_GPU_ERR_ARG;
	if (w <= 0 || h <= 0) return fail(ctx, LOL_GPU_ERR_ARG, "bad frame geometry");
	const unsigned depth = (unsigned)std::max(2, ctx->n_frame_streams);
	if (ctx->pipe_begun - ctx->pipe_ended >= depth)
		return fail(ctx, LOL_GPU_ERR_ARG, depth == 2 ? "two frames already in flight: call lol_gpu_render_host_end first"
		                                             : "every frame slot is in flight (lol_gpu_set_frames_in_flight): call lol_gpu_render_host_end first");
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	LOL_TRY(ensure_copy_stream(ctx));
	LOL_TRY(ensure_frame_streams(ctx, (int)depth));
	const int slot = (int)(ctx->pipe_begun % lol_gpu::PIPE_SLOTS);
	/* Which stream.  A frame whose view is NEW goes to the next stream of the rotation: it runs in a fixed tile order, its launch
	 * has a long tail, and the frame after it fills that tail (the orbit through the C host: 9170 -> 11,000 Mpixels/s).  A frame
	 * under the SAME view as the frame before it follows that frame on its stream: such frames are scheduled by their
	 * predecessor's costs and have no tail to fill, and two of them side by side finish together — after which nothing is
	 * queued while the host waits in _end() for the first one's copy (measured: 1.03 ms per frame on two streams against 0.83
	 * on one, profiles/r5_frames_in_flight.md). */
	const int geom[3] = { w, h, max_steps };
	const bool same_view = ctx->pipe_last_stream && memcmp(geom, ctx->pipe_last_geom, sizeof geom) == 0 && memcmp(cam, &ctx->pipe_last_cam, sizeof *cam) == 0;
	hipStream_t ks = same_view ? ctx->pipe_last_stream : ctx->frame_streams[ctx->pipe_rr++ % depth];
	const size_t need = (size_t)w * h * 4;
	if (need > ctx->pipe_bytes[slot]) {
		/* the surface grew (main.c:182-187).  This slot's last frame was ended PIPE_SLOTS calls ago; its copy may still run, and
		 * so may the kernel of a frame that was discarded: wait for both, then replace this slot's framebuffer only — the
		 * frames queued in the OTHER slots stay valid */
		LOL_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
		if (ctx->pipe_stream[slot]) LOL_HIP(ctx, hipStreamSynchronize(ctx->pipe_stream[slot]));
		if (ctx->d_pipe[slot]) (void)hipFree(ctx->d_pipe[slot]);
		ctx->d_pipe[slot] = nullptr;
		ctx->pipe_bytes[slot] = 0;
		LOL_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_pipe[slot]), need));
		ctx->pipe_bytes[slot] = need;
	}
	/* the copy that last read this framebuffer must be done before the kernel overwrites it — and so must the kernel that
	 * last wrote it, where that one ran on another stream (a frame that was discarded; a changed number of streams) */
	LOL_HIP(ctx, hipStreamWaitEvent(ks, ctx->pipe_copied[slot], 0));
	if (ctx->pipe_stream[slot] && ctx->pipe_stream[slot] != ks) LOL_HIP(ctx, hipStreamWaitEvent(ks, ctx->pipe_rendered[slot], 0));
	LOL_TRY(lol_gpu_render_device(ctx, cam, w, h, max_steps, nullptr, ctx->d_pipe[slot], (size_t)w * 4, nullptr, ks));
	LOL_HIP(ctx, hipEventRecord(ctx->pipe_rendered[slot], ks));
	ctx->pipe_stream[slot] = ks;
	ctx->pipe_last_stream = ks;
	ctx->pipe_last_cam = *cam;
	memcpy(ctx->pipe_last_geom, geom, sizeof geom);
	ctx->pipe_w[slot] = w; ctx->pipe_h[slot] = h;
	ctx->pipe_begun++;
	return LOL_GPU_OK;
}

int lol_gpu_render_host_end(lol_gpu* ctx, void* host_pixels, size_t pitch_bytes, int w, int h) {
	if (!ctx || !host_pixels) return LOL_GPU_ERR_ARG;
	if (ctx->pipe_begun == ctx->pipe_ended) return fail(ctx, LOL_GPU_ERR_ARG, "no frame in flight");
	const int slot = (int)(ctx->pipe_ended % lol_gpu::PIPE_SLOTS);
	/* the surface's size, as the caller sees it NOW, decides what may be written: a frame queued before a resize
	 * is never copied into a surface of another size (it stays queued: discard it, or end it into a fitting one) */
	if (w != ctx->pipe_w[slot] || h != ctx->pipe_h[slot])
		return fail(ctx, LOL_GPU_ERR_ARG, "the queued frame's size differs from the surface's: lol_gpu_render_host_discard");
	if (pitch_bytes < (size_t)w * 4) return fail(ctx, LOL_GPU_ERR_ARG, "bad frame geometry");
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	LOL_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->pipe_rendered[slot], 0));
	LOL_HIP(ctx, hipMemcpy2DAsync(host_pixels, pitch_bytes, ctx->d_pipe[slot], (size_t)w * 4, (size_t)w * 4, h,
	                              hipMemcpyDeviceToHost, ctx->copy_stream));
	LOL_HIP(ctx, hipEventRecord(ctx->pipe_copied[slot], ctx->copy_stream));
	ctx->pipe_ended++;
	LOL_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
	return LOL_GPU_OK;
}

int lol_gpu_render_host_pending(const lol_gpu* ctx) { return ctx ? (int)(ctx->pipe_begun - ctx->pipe_ended) : 0; }

int lol_gpu_render_host_pending_size(const lol_gpu* ctx, int* w, int* h) {
	if (!ctx || !w || !h) return LOL_GPU_ERR_ARG;
	const bool any = ctx->pipe_begun != ctx->pipe_ended;
	const int slot = (int)(ctx->pipe_ended % lol_gpu::PIPE_SLOTS);
	*w = any ? ctx->pipe_w[slot] : 0;
	*h = any ? ctx->pipe_h[slot] : 0;
	return LOL_GPU_OK;
}

int lol_gpu_render_host_discard(lol_gpu* ctx) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	/* the kernels still run to completion into their own framebuffers; nothing of them reaches a surface */
	ctx->pipe_ended = ctx->pipe_begun;
	return LOL_GPU_OK;
}

/* every stream of the context's own: frames in flight may be on any of them */
static int sync_own_streams(lol_gpu* ctx) {
	for (hipStream_t fs : ctx->frame_streams) if (fs) LOL_HIP(ctx, hipStreamSynchronize(fs));
	return LOL_GPU_OK;
}

int lol_gpu_sync(lol_gpu* ctx) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	return sync_own_streams(ctx);
}

int lol_gpu_set_frames_in_flight(lol_gpu* ctx, int n) {
	if (!ctx || n < 1 || n > lol_gpu::MAX_FRAME_STREAMS) return LOL_GPU_ERR_ARG;
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	LOL_TRY(ensure_frame_streams(ctx, n));
	/* a frame queued on a stream that is about to fall out of the rotation stays ordered before whatever comes next */
	LOL_TRY(sync_own_streams(ctx));
	ctx->n_frame_streams = n;
	ctx->frame_rr = 0;
	return LOL_GPU_OK;
}

int lol_gpu_frames_in_flight(const lol_gpu* ctx) { return ctx ? ctx->n_frame_streams : 0; }

void* lol_gpu_next_stream(lol_gpu* ctx) {
	return ctx ? static_cast<void*>(ctx->frame_streams[ctx->frame_rr % (unsigned)ctx->n_frame_streams]) : nullptr;
}

int lol_gpu_malloc(lol_gpu* ctx, size_t bytes, void** out) {
	if (!ctx || !out) return LOL_GPU_ERR_ARG;
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	LOL_HIP(ctx, hipMalloc(out, bytes));
	return LOL_GPU_OK;
}

int lol_gpu_free(lol_gpu* ctx, void* ptr) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	LOL_HIP(ctx, hipFree(ptr));
	return LOL_GPU_OK;
}

int lol_gpu_memcpy_d2h(lol_gpu* ctx, void* host, const void* dev, size_t bytes) {
	if (!ctx || !host || !dev) return LOL_GPU_ERR_ARG;
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	LOL_TRY(sync_own_streams(ctx));
	LOL_HIP(ctx, hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
	return LOL_GPU_OK;
}
int lol_gpu_memcpy_h2d(lol_gpu* ctx, void* dev, const void* host, size_t bytes) {
	if (!ctx || !host || !dev) return LOL_GPU_ERR_ARG;
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	LOL_HIP(ctx, hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
	return LOL_GPU_OK;
}

const char* lol_gpu_kernel_name(const lol_gpu* ctx) { return ctx ? kernel_name(ctx) : ""; }

int lol_gpu_set_samples(lol_gpu* ctx, int samples) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	if (samples != 1 && samples != 2 && samples != 4) return fail(ctx, LOL_GPU_ERR_ARG, "samples per axis must be 1, 2 or 4");
	if (!lol::samples_fit_wave(samples))
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "this build's wave patch (LOL_WAVE_W x LOL_WAVE_H) does not divide into that many samples per axis");
	ctx->samples = samples;                 /* the next frame's; a frame already queued keeps its own */
	return LOL_GPU_OK;
}

int lol_gpu_samples(const lol_gpu* ctx) { return ctx ? ctx->samples : LOL_GPU_ERR_ARG; }

/* The module switches beside it (lol_gpu_internal.h, MODULE_SWITCHES): each takes effect at the next lol_gpu_upload_program */
static int set_module_switch(lol_gpu* ctx, ModuleSwitch sw, int enable) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	ctx->module_switches = enable ? ctx->module_switches | switch_bit(sw) : ctx->module_switches & ~switch_bit(sw);
	return LOL_GPU_OK;
}
static int module_switch(const lol_gpu* ctx, ModuleSwitch sw) { return ctx ? (ctx->module_switches & switch_bit(sw)) != 0 : LOL_GPU_ERR_ARG; }
int lol_gpu_set_view_batches(lol_gpu* ctx, int enable)       { return set_module_switch(ctx, SWITCH_BATCH, enable); }
int lol_gpu_set_view_samples(lol_gpu* ctx, int enable)       { return set_module_switch(ctx, SWITCH_BATCH_AA, enable); }
int lol_gpu_set_view_blends(lol_gpu* ctx, int enable)        { return set_module_switch(ctx, SWITCH_BATCH_BLEND, enable); }
int lol_gpu_set_view_blend_samples(lol_gpu* ctx, int enable) { return set_module_switch(ctx, SWITCH_BATCH_BLEND_AA, enable); }
int lol_gpu_set_ray_queries(lol_gpu* ctx, int enable)        { return set_module_switch(ctx, SWITCH_RAYS, enable); }
int lol_gpu_set_shade_queries(lol_gpu* ctx, int enable)      { return set_module_switch(ctx, SWITCH_SHADE, enable); }
int lol_gpu_view_batches(const lol_gpu* ctx)       { return module_switch(ctx, SWITCH_BATCH); }
int lol_gpu_view_samples(const lol_gpu* ctx)       { return module_switch(ctx, SWITCH_BATCH_AA); }
int lol_gpu_view_blends(const lol_gpu* ctx)        { return module_switch(ctx, SWITCH_BATCH_BLEND); }
int lol_gpu_view_blend_samples(const lol_gpu* ctx) { return module_switch(ctx, SWITCH_BATCH_BLEND_AA); }
int lol_gpu_ray_queries(const lol_gpu* ctx)        { return module_switch(ctx, SWITCH_RAYS); }
int lol_gpu_shade_queries(const lol_gpu* ctx)      { return module_switch(ctx, SWITCH_SHADE); }

int lol_gpu_set_adaptive_samples(lol_gpu* ctx, int contrast) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	if (contrast < -1 || contrast > 255) return fail(ctx, LOL_GPU_ERR_ARG, "adaptive contrast must be -1 (off) or 0 ... 255");
	if (contrast >= 0 && lol::BLOCK != 64)
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "adaptive frames need one-wave blocks (this build's LOL_WAVES_X is not 1)");
	ctx->adaptive = contrast;               /* the next frame's; a frame already queued keeps its own */
	return LOL_GPU_OK;
}

int lol_gpu_adaptive_samples(const lol_gpu* ctx) { return ctx ? ctx->adaptive : LOL_GPU_ERR_ARG; }

/* the set of the context's last adaptive frame, waited for */
static int last_adaptive_set(lol_gpu* ctx, lol_gpu::AdaptiveFrameSet** out) {
	if (!ctx->adaptive_last || !ctx->adaptive_last->used) return fail(ctx, LOL_GPU_ERR_ARG, "no adaptive frame has been launched");
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	LOL_HIP(ctx, hipEventSynchronize(ctx->adaptive_last->done));
	*out = ctx->adaptive_last;
	return LOL_GPU_OK;
}

int lol_gpu_adaptive_refined(lol_gpu* ctx, int64_t* n) {
	if (!ctx || !n) return LOL_GPU_ERR_ARG;
	lol_gpu::AdaptiveFrameSet* S = nullptr;
	LOL_TRY(last_adaptive_set(ctx, &S));
	uint32_t c = 0;
	LOL_HIP(ctx, hipMemcpy(&c, S->d_count, 4, hipMemcpyDeviceToHost));
	*n = c;
	return LOL_GPU_OK;
}

int lol_gpu_adaptive_pass_ms(lol_gpu* ctx, float ms[3]) {
	if (!ctx || !ms) return LOL_GPU_ERR_ARG;
	lol_gpu::AdaptiveFrameSet* S = nullptr;
	LOL_TRY(last_adaptive_set(ctx, &S));
	for (int i = 0; i < 3; i++) LOL_HIP(ctx, hipEventElapsedTime(&ms[i], S->ev[i], i < 2 ? S->ev[i + 1] : S->done));
	return LOL_GPU_OK;
}

long lol_gpu_roctx_ranges(void) {
	g_roctx.init();
	return g_roctx.asked && !g_roctx.push ? -1 : g_roctx.ranges.load();
}

const char* lol_gpu_kernel_key(const lol_gpu* ctx) {
	if (!ctx) return "";
	const SceneKernel* k = family_kernel(ctx, frame_family(ctx));
	return k ? k->key.c_str() : ctx->samples > 1 ? ctx->interp_aa_key.c_str() : ctx->interp_key.c_str();
}

int lol_gpu_abi_version(void) { return LOL_GPU_ABI_VERSION; }

int lol_gpu_testing_fail_uploads(lol_gpu* ctx, int n) {
	if (!ctx || n < 0) return LOL_GPU_ERR_ARG;
	ctx->fail_uploads = n;
	return LOL_GPU_OK;
}
int lol_gpu_sdf_batch(lol_gpu* ctx, const float* pts_dev, float* dist_dev, uint32_t* id_dev, size_t n, void* stream) {
	if (!ctx || !pts_dev || !dist_dev || !id_dev || n > 0xFFFFFFFFu) return LOL_GPU_ERR_ARG;
	if (!ctx->have_prog) return fail(ctx, LOL_GPU_ERR_NO_PROGRAM, "no scene program uploaded");
	if (n == 0) return LOL_GPU_OK;
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
	uint32_t n32 = (uint32_t)n;
	hipError_t e;
	finish_specialise(ctx, false);
	if (const SceneKernel* k = scene_kernel(ctx)) {
		void* args[] = { &pts_dev, &dist_dev, &id_dev, &n32 };
		e = hipModuleLaunchKernel(k->sdf, (n32 + 63) / 64, 1, 1, 64, 1, 1, 0, s, args, nullptr);
	} else {
		/* per stack class and root kind; the SDF alone reads no lights or materials, so where the tables lie (interp_rung) does not matter */
		const int kind = ctx->interp_sqrt_kind;
		e = stack_class_dispatch(interp_stack_class(ctx->h_prog.max_stack), [&](auto v) {
			constexpr int ssize = decltype(v)::ssize;
			const dim3 grid((n32 + 63) / 64);
			const uint32_t* mops = ctx->d_mops[ctx->cur];
			if (kind == 3) hipLaunchKernelGGL((lol::sdf_points_interp<ssize, 3>), grid, dim3(64), 0, s, mops, ctx->n_mops, pts_dev, dist_dev, id_dev, n32);
			else           hipLaunchKernelGGL((lol::sdf_points_interp<ssize, 0>), grid, dim3(64), 0, s, mops, ctx->n_mops, pts_dev, dist_dev, id_dev, n32);
			return hipGetLastError();
		});
	}
	if (e != hipSuccess) return fail(ctx, LOL_GPU_ERR_HIP, "sdf kernel launch", e);
	return LOL_GPU_OK;
}

}  // extern "C"

/*
 * List queries: ray queries, shading queries and light passes (include/lol_gpu.h; the kernels: lol_kernel_rays.h, lol_kernel_shade.h,
 * lol_kernel_light.h).  Each call is ONE launch over a list of n elements on the caller's stream: no host wait, no copy, no scratch,
 * and nothing of the context changes but — for a list of pixels — the cached first step of the camera's position (first_step: a
 * function of that position alone, whoever asks).  The tile-order state, the samples and the record rings are neither read nor
 * written.  What the families share stands here once:
 *   QuerySource         where a call's elements come from, and the name its family's refusals carry
 *   source_refused      every refusal of a *_rays or *_pixels call, in the order a host sees them
 *   launch_on_stream    the call's device, its stream, the launch and the launch's error
 *   source_fields       the source's half of a Launch and a query: the list, its length, a frame's size
 *   launch_scene_query  the scene's half of a shading query's or a capture's launch: the Launch, what rests on the camera, the tables' LDS
 *   record_query        a list query under each record's own scene: the trace, shade and capture forms are its three callers, further down
 * and, further up and further down, what they share with the frames and with the families whose records bring their own scene:
 *   guarded               the C boundary's guard against exceptions, for the calls that prepare something in host memory
 *   launch_interp         the interpreter's instantiation for the program's rung and root kind, launched
 *   pack_tables           a program's three tables as an upload lays them out (launch_tables: a Launch's three pointers into them)
 *   context_launch_fields the context's part of every Launch: the tables' counts, the gamma table, the pixel format
 *   look_differs          the walk over a program that says what a look, or a held program, may not differ in
 *   record_resolve        a resolve under each record's own look: both resolves over records are its callers
 */
struct QuerySource {
	const char*     who;             /* "ray query", "shading query", "light passes": what the family's refusals begin with */
	const float*    rays;            /* a list of rays, or ... */
	const uint32_t* xy;              /* ... (`pixels`) of pixels of the w x h frame under `cam` */
	bool            pixels;
	const lol_frame_camera* cam;
	int             w, h;
	size_t          n;
	int             max_steps;
	void*           stream;
	bool            list_optional;   /* a capture's: no list is every pixel of the frame, n = w h */
};
static QuerySource rays_source(const char* who, const float* rays, size_t n, int max_steps, void* stream) {
	return { who, rays, nullptr, false, nullptr, 0, 0, n, max_steps, stream, false };
}
static QuerySource pixels_source(const char* who, const lol_frame_camera* cam, int w, int h, const uint32_t* xy, size_t n, int max_steps,
                                 void* stream, bool list_optional = false) {
	return { who, nullptr, xy, true, cam, w, h, n, max_steps, stream, list_optional };
}

/* what the planes of a capture or of a relight are refused for, once the program is known to be there */
static int passes_refused(lol_gpu* ctx, const lol_gpu_light_passes* p, size_t n) {
	if (!p->hit_id) return fail(ctx, LOL_GPU_ERR_ARG, "light passes: no hit_id plane");
	if (ctx->h_prog.n_lights && !p->factors) return fail(ctx, LOL_GPU_ERR_ARG, "light passes: no factors, and the program has lights");
	if (reinterpret_cast<uintptr_t>(p->factors) & 15u) return fail(ctx, LOL_GPU_ERR_ARG, "light passes: factors must be 16-byte aligned");
	if (p->light_stride != 0 && p->light_stride < n) return fail(ctx, LOL_GPU_ERR_ARG, "light passes: light_stride is neither 0 nor at least n");
	return LOL_GPU_OK;
}

/* LOL_GPU_ERR_ARG in the family's words: "<who>: <why>" */
static int source_refuse(lol_gpu* ctx, const QuerySource& src, const char* why) {
	char text[128];
	snprintf(text, sizeof text, "%s: %s", src.who, why);
	return fail(ctx, LOL_GPU_ERR_ARG, text);           /* (fail copies the text) */
}
/* The refusals of a list query, in THE order (tests/test_gpu_rays.py, test_refusals, and its three siblings pin it): a bad argument
 * beats a missing program, and a missing program the camera and the frame's geometry — which are asked for with n = 0 too.
 * `no_output`: the family's own test of its outputs; `planes`: a capture's, held to passes_refused where the parent held them. */
static int source_refused(lol_gpu* ctx, const QuerySource& src, bool no_output, const lol_gpu_light_passes* planes = nullptr) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	auto refuse = [&](const char* why) { return source_refuse(ctx, src, why); };
	if (!(src.pixels ? (const void*)src.xy : (const void*)src.rays) && !src.list_optional && src.n > 0) return refuse("no list");
	if (no_output) return refuse("no output");
	if (src.max_steps < 0 || src.n > 0xFFFFFFFFu) return refuse("max_steps < 0 or more than 2^32 - 1 rays");
	if (!ctx->have_prog) return fail(ctx, LOL_GPU_ERR_NO_PROGRAM, "no scene program uploaded");
	if (planes) LOL_TRY(passes_refused(ctx, planes, src.n));
	if (!src.pixels) return LOL_GPU_OK;
	if (!src.cam || src.w < 1 || src.h < 1) return refuse("no camera or bad frame geometry");
	if (!src.xy && src.list_optional && src.n != (size_t)src.w * (size_t)src.h) return refuse("no list of pixels, and n is not w * h");
	return LOL_GPU_OK;
}

/* `launch(s)` on the context's device and the call's stream; `what` names the launch where it fails */
template <class Launch>
static int launch_on_stream(lol_gpu* ctx, void* stream, const char* what, Launch&& launch) {
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
	const hipError_t e = launch(s);
	if (e != hipSuccess) return fail(ctx, LOL_GPU_ERR_HIP, what, e);
	return LOL_GPU_OK;
}

/* dynamic LDS of the kernels that stage the scene's tables and nothing else (lol_kernel.h, tables_in_lds): no output tile */
static unsigned tables_lds_bytes(const lol_program& P) {
	return lol::tables_in_lds(P.n_lights, P.n_materials, P.n_roots) ? lol::table_dwords(P.n_lights, P.n_materials, P.n_roots) * 4u : 0u;
}

/* The source's half of a shading query, a capture or an update — `Q` a ShadeQuery, LightQuery or LightUpdateQuery — and of its Launch:
 * the list and its length; for pixels the frame's size and SHADE_FROM_PIXELS, with LIGHT_ALL_PIXELS where there is no list (only a
 * capture or an update gets here without one: source_refused).  The camera is not set here: it is the call's, or each record's own. */
template <class Query>
static void source_fields(const QuerySource& src, lol::Launch& L, Query& Q) {
	Q.rays = src.rays;
	Q.xy = src.xy;
	Q.n = (uint32_t)src.n;
	if (src.pixels) {
		Q.flags |= lol::SHADE_FROM_PIXELS | (src.xy ? 0u : lol::LIGHT_ALL_PIXELS);
		L.fw = (float)src.w; L.fh = (float)src.h;
		L.w = src.w; L.h = src.h;
	}
}

/* ---- ray queries.  A RayQuery carries its own camera: no Launch, no tables, a wave per block. */
/* the scene kernel that answers queries, or nullptr: trace_interp does — the test the launch makes and lol_gpu_trace_kernel_name reports */
static const SceneKernel* trace_kernel(const lol_gpu* ctx) {
	const SceneKernel* k = scene_kernel(ctx);
	return k && k->trace ? k : nullptr;
}

static int ray_query(lol_gpu* ctx, const QuerySource& src, const lol_gpu_hits* out) {
	LOL_TRY(source_refused(ctx, src, !out || (!out->dist && !out->id && !out->steps && !out->normal)));
	if (src.n == 0) return LOL_GPU_OK;
	lol::RayQuery Q;
	memset(&Q, 0, sizeof Q);
	Q.rays = src.rays;
	Q.xy = src.xy;
	Q.n = (uint32_t)src.n;
	Q.max_steps = src.max_steps;
	if (src.pixels) {
		Q.flags = lol::RAYS_FROM_PIXELS;
		memcpy(&Q.cam, src.cam, sizeof Q.cam);
		Q.fw = (float)src.w; Q.fh = (float)src.h;
		if (first_step(ctx, *src.cam, src.max_steps)) { Q.flags |= lol::RAYS_FIRST_STEP; Q.first_dist = ctx->first_dist; Q.first_id = ctx->first_id; }
	}
	/* the scene's side of what the fast SDF rests on (shadow_settle_ok, whatever lol_gpu_set_exact_skips says: no shadow is cast);
	 * the rays' side is the kernel's own ballot */
	if (ctx->finite_scene) Q.flags |= lol::RAYS_SCENE_SANE;
	if (out->id) Q.flags |= lol::RAYS_WANT_ID;
	if (out->normal) Q.flags |= lol::RAYS_WANT_NORMAL;
	Q.out = { out->dist, out->id, out->steps, out->normal };
	return launch_on_stream(ctx, src.stream, "ray query launch", [&](hipStream_t s) {
		finish_specialise(ctx, false);           /* a scene kernel that has finished compiling takes over here, as at a frame boundary */
		const dim3 grid((Q.n + 63u) / 64u);
		if (const SceneKernel* k = trace_kernel(ctx)) {
			void* args[] = { &Q };
			return hipModuleLaunchKernel(k->trace, grid.x, 1, 1, 64, 1, 1, 0, s, args, nullptr);
		}
		/* the list every camera may use (with v_div_fixup: upload_program), as lol_gpu_sdf_batch; per stack class and root kind, as there */
		Q.ops = ctx->d_mops[ctx->cur];
		Q.n_ops = ctx->n_mops;
		const int kind = ctx->interp_sqrt_kind;
		return stack_class_dispatch(interp_stack_class(ctx->h_prog.max_stack), [&](auto v) {
			constexpr int ssize = decltype(v)::ssize;
			if (kind == 3) hipLaunchKernelGGL((lol::trace_interp<ssize, 3>), grid, dim3(64), 0, s, Q);
			else           hipLaunchKernelGGL((lol::trace_interp<ssize, 0>), grid, dim3(64), 0, s, Q);
			return hipGetLastError();
		});
	});
}

/* ---- shading queries.  The scene's half of the launch is a frame's (scene_launch_fields: tables, ambient, the skips that hold for
 * every camera, the gamma table, the pixel format). */
/* the scene kernel that answers shading queries, or nullptr: shade_interp does — the test the launch makes and lol_gpu_shade_kernel_name reports */
static const SceneKernel* shade_kernel(const lol_gpu* ctx) {
	const SceneKernel* k = scene_kernel(ctx);
	return k && k->shade ? k : nullptr;
}
/* ... at a launch: a scene kernel that has finished compiling takes over here, as at a frame boundary */
static hipFunction_t shade_module_fn(lol_gpu* ctx) {
	finish_specialise(ctx, false);
	const SceneKernel* k = shade_kernel(ctx);
	return k ? k->shade : nullptr;
}

/* The scene's half of a shading query or a capture, and the launch; nothing for n = 0.  `Q`: zeroed but for the family's own fields;
 * its source is filled in here.  `clear_look_skips`: a capture's — every factor of every ray, so the two skips that rest on the
 * uploaded look are off, whatever the context's switches say.  `module_fn`: the scene module's kernel at this launch, where the family
 * has one (a capture has none: light_interp always, and no tier takes over at a capture).  `interp_kernel(variant, kind)`: the
 * interpreter's instantiation. */
template <class Query, class InterpKernel>
static int launch_scene_query(lol_gpu* ctx, const QuerySource& src, Query& Q, bool clear_look_skips, hipFunction_t (*module_fn)(lol_gpu*),
                              const char* what, InterpKernel&& interp_kernel) {
	if (src.n == 0) return LOL_GPU_OK;
	lol::Launch L;
	memset(&L, 0, sizeof L);
	L.max_steps = src.max_steps;
	/* the macro-op list every camera may use (with v_div_fixup: upload_program), as ray_query: scene_launch_fields' */
	scene_launch_fields(ctx, nullptr, L);
	if (clear_look_skips) L.flags &= ~(lol::FLAG_MISS_SKIP | lol::FLAG_DARK_SKIP);
	/* the host's side of what the fast SDF and the settled shadow loop rest on: the scene (shadow_settle_ok) and, where the rays are a
	 * camera's, the camera, as lol_gpu_render_device; the side of a list's rays is the kernel's own ballot (shade_rays, light_rays) */
	const bool sane = !src.pixels || camera_sane(*src.cam);
	if (ctx->finite_scene && sane) Q.flags |= lol::SHADE_SCENE_SANE;
	if (ctx->shadow_settle && sane) L.flags |= lol::FLAG_SHADOW_SETTLED;
	source_fields(src, L, Q);
	if (src.pixels) {
		memcpy(&L.cam, src.cam, sizeof L.cam);
		if (first_step(ctx, *src.cam, src.max_steps)) { L.flags |= lol::FLAG_FIRST_STEP; L.first_dist = ctx->first_dist; L.first_id = ctx->first_id; }
	}
	return launch_on_stream(ctx, src.stream, what, [&](hipStream_t s) {
		const hipFunction_t fn = module_fn ? module_fn(ctx) : nullptr;
		const unsigned lds = tables_lds_bytes(ctx->h_prog);
		const dim3 grid((unsigned)(((unsigned long long)Q.n + lol::BLOCK - 1) / lol::BLOCK));
		void* args[] = { &L, &Q };
		if (fn) return hipModuleLaunchKernel(fn, grid.x, 1, 1, lol::BLOCK, 1, 1, lds, s, args, nullptr);
		return launch_interp(ctx, grid, args, lds, s, interp_kernel);
	});
}

/* (scene views' records, their ring and the refusal of their scenes stand with scene views, further down) */
static int build_scene_records(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n, int max_steps, bool lists,
                               std::vector<lol::SceneView>& views, std::vector<uint32_t>& data);
static int queue_scene_records(lol_gpu* ctx, const std::vector<lol::SceneView>& views, const std::vector<uint32_t>& data, hipStream_t s, RingSet** out);
static int scenes_refused(lol_gpu* ctx, const lol_program* scenes, int n);

/* THE host path of a list query under each record's own scene, for its three forms — trace, shade, capture (`planes`: its planes, and
 * what makes it one).  In the order a host sees (include/lol_gpu.h numbers the refusals the same way):
 *  1. the single-scene query's refusals (source_refused); a NULL `cams` is 2.'s, so the camera source_refused looks at is there;
 *  2. the records and their lists, and a capture's planes over all of them;
 *  3. the scenes, as lol_gpu_render_scene_views refuses them; then nothing for n = 0.
 * Then the call's device and stream, scene views' records (every factor of every ray at a capture, as at every capture: a look may
 * differ from the record in exactly what the two skips rest on, so they are cleared on EVERY record) through scene views' ring, the
 * family's `launch(R, s)` — its query, its grid with the record in y, its kernel — and the ring's event behind it, `what` its name. */
template <class Launcher>
static int record_query(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_scenes, QuerySource src, size_t list_stride,
                        bool no_output, const lol_gpu_light_passes* planes, const char* what, Launcher&& launch) {
	static const lol_frame_camera no_cam = {};
	if (src.pixels && !cams) src.cam = &no_cam;
	LOL_TRY(source_refused(ctx, src, no_output, planes));
	auto refuse = [&](const char* why) { return source_refuse(ctx, src, why); };
	if (!scenes) return refuse("no scenes");
	if (n_scenes < 1 || n_scenes > LOL_GPU_MAX_VIEWS) return refuse("the number of scenes is not in 1 ... LOL_GPU_MAX_VIEWS");
	if (src.pixels && !cams) return refuse("no cameras");
	if (list_stride != 0 && list_stride < src.n) return refuse("list_stride is neither 0 nor at least n");
	const unsigned long long N = (unsigned long long)n_scenes * (unsigned long long)src.n;
	if (N > 0xFFFFFFFFull) return refuse("more than 2^32 - 1 rays over all scenes");
	if (planes && planes->light_stride != 0 && planes->light_stride < N) return refuse("light_stride is neither 0 nor at least n_scenes * n");
	LOL_TRY(scenes_refused(ctx, scenes, n_scenes));
	if (src.n == 0) return LOL_GPU_OK;

	LOL_HIP(ctx, hipSetDevice(ctx->device));
	hipStream_t s = src.stream ? static_cast<hipStream_t>(src.stream) : ctx->stream;
	std::vector<lol::SceneView> views;
	std::vector<uint32_t> data;
	LOL_TRY(build_scene_records(ctx, src.pixels ? cams : nullptr, scenes, n_scenes, src.max_steps, true, views, data));
	if (planes) for (lol::SceneView& V : views) V.flags &= ~(lol::FLAG_MISS_SKIP | lol::FLAG_DARK_SKIP);
	RingSet* S = nullptr;
	LOL_TRY(queue_scene_records(ctx, views, data, s, &S));
	lol::SceneList R = { reinterpret_cast<const lol::SceneView*>(S->d_buf), S->d_buf + views.size() * lol::SCENE_VIEW_DWORDS,
	                     (unsigned long long)list_stride };
	return ring_done(ctx, *S, s, launch(R, s), what);
}
/* the grid of such a launch: a block per `block` elements of the list in x, the record in y */
static dim3 record_grid(size_t n, unsigned block, int n_scenes) { return dim3((unsigned)((n + block - 1) / block), (unsigned)n_scenes); }

static int shade_query(lol_gpu* ctx, const QuerySource& src, const lol_gpu_shades* out) {
	LOL_TRY(source_refused(ctx, src, !out || (!out->rgb_linear && !out->rgb && !out->pixel && !out->hit_dist && !out->hit_id && !out->steps)));
	lol::ShadeQuery Q = {};
	Q.out = { out->rgb_linear, out->rgb, out->pixel, out->hit_dist, out->hit_id, out->steps };
	return launch_scene_query(ctx, src, Q, false, shade_module_fn, "shading query launch", [](auto v, auto kind) {
		return reinterpret_cast<const void*>(&lol::shade_interp<decltype(v)::ssize, decltype(kind)::value, decltype(v)::tables_global>);
	});
}

extern "C" {

int lol_gpu_trace_rays(lol_gpu* ctx, const float* rays_dev, size_t n, int max_steps, const lol_gpu_hits* out, void* stream) {
	return ray_query(ctx, rays_source("ray query", rays_dev, n, max_steps, stream), out);
}

int lol_gpu_trace_pixels(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps,
                         const uint32_t* xy_dev, size_t n, const lol_gpu_hits* out, void* stream) {
	return ray_query(ctx, pixels_source("ray query", cam, w, h, xy_dev, n, max_steps, stream), out);
}

int lol_gpu_pick(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps, int x, int y, lol_gpu_hit* out) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	if (!cam || !out || w < 1 || h < 1 || max_steps < 0) return fail(ctx, LOL_GPU_ERR_ARG, "pick: no camera, no output or bad frame geometry");
	if (x < 0 || y < 0 || x >= w || y >= h) return fail(ctx, LOL_GPU_ERR_ARG, "pick: the pixel lies outside the frame");
	if (!ctx->have_prog) return fail(ctx, LOL_GPU_ERR_NO_PROGRAM, "no scene program uploaded");
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	/* xy [2] | dist | id | steps | normal [3]: eight dwords, the context's from the first pick on */
	if (!ctx->d_pick) LOL_HIP(ctx, hipMalloc(&ctx->d_pick, 8 * 4));
	uint32_t* d = static_cast<uint32_t*>(ctx->d_pick);
	uint32_t host[8] = { (uint32_t)x, (uint32_t)y, 0, 0, 0, 0, 0, 0 };
	LOL_HIP(ctx, hipMemcpyAsync(d, host, 2 * 4, hipMemcpyHostToDevice, ctx->stream));
	const lol_gpu_hits hits = { reinterpret_cast<float*>(d + 2), d + 3, d + 4, reinterpret_cast<float*>(d + 5) };
	LOL_TRY(lol_gpu_trace_pixels(ctx, cam, w, h, max_steps, d, 1, &hits, ctx->stream));
	LOL_HIP(ctx, hipMemcpyAsync(host, d, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
	LOL_HIP(ctx, hipStreamSynchronize(ctx->stream));
	memcpy(&out->dist, &host[2], 4);
	out->id = host[3];
	out->steps = host[4];
	memcpy(out->normal, &host[5], 3 * 4);
	return LOL_GPU_OK;
}

const char* lol_gpu_trace_kernel_name(const lol_gpu* ctx) {
	if (!ctx) return "";
	return trace_kernel(ctx) ? "lol_trace_spec" : "trace_interp";
}

int lol_gpu_shade_rays(lol_gpu* ctx, const float* rays_dev, size_t n, int max_steps, const lol_gpu_shades* out, void* stream) {
	return shade_query(ctx, rays_source("shading query", rays_dev, n, max_steps, stream), out);
}

int lol_gpu_shade_pixels(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps,
                         const uint32_t* xy_dev, size_t n, const lol_gpu_shades* out, void* stream) {
	return shade_query(ctx, pixels_source("shading query", cam, w, h, xy_dev, n, max_steps, stream), out);
}

const char* lol_gpu_shade_kernel_name(const lol_gpu* ctx) {
	if (!ctx) return "";
	return shade_kernel(ctx) ? "lol_shade_spec" : "shade_interp";
}
}  // extern "C"

/*
 * Scene views (lol_gpu_render_scene_views): a batch whose every record brings a camera AND a scene of the uploaded program's
 * structure (lol_kernel_scenes.h).  Everything an upload decides from the program and a frame from the camera is decided here per
 * record, from that record's own scene and camera, on the host: the three exact skips, finite_scene (which of its two lists the
 * record runs), the primary march's first step (program_first_step on that scene), what an insane camera switches off.  No device
 * proof runs: the lists are built with what the upload proved (lol_gpu::fast), and a smoothness constant it did not prove takes the
 * plain sminf.  One copy — the records and, behind them, every record's lists, tables and numbers — from a ring of sets of their own
 * (lol_gpu::scene_view_records), and with K = 1 one launch; a blend adds the resolve pass and scratch ring of lol_gpu_render_views_blend.
 * The context's scene, kernels, keys, tile-order state, sample settings and view-record ring are neither read nor changed.
 */
static bool same_structure(const lol_program& A, const lol_program& B) {
	if (A.n_ops != B.n_ops || A.n_lights != B.n_lights || A.n_materials != B.n_materials || A.n_roots != B.n_roots || A.max_stack != B.max_stack)
		return false;
	for (uint32_t i = 0; i < A.n_ops; i++)
		if (A.ops[i].op != B.ops[i].op || A.ops[i].id != B.ops[i].id) return false;
	return true;
}

/* the address of the interpreter's scene-view kernel for one stack class, sqrt kind and table placement; `aa`: the supersampled ones
 * (lol_kernel_scenes_aa.h) */
template <int SSIZE, int KIND, bool TABLES_GLOBAL>
static const void* scene_interp_kernel(bool lin, bool aa) {
	if (aa) return lin ? reinterpret_cast<const void*>(&lol::render_interp_scene_batch_aa_lin<SSIZE, KIND, TABLES_GLOBAL>)
	                   : reinterpret_cast<const void*>(&lol::render_interp_scene_batch_aa<SSIZE, KIND, TABLES_GLOBAL>);
	return lin ? reinterpret_cast<const void*>(&lol::render_interp_scene_batch_lin<SSIZE, KIND, TABLES_GLOBAL>)
	           : reinterpret_cast<const void*>(&lol::render_interp_scene_batch<SSIZE, KIND, TABLES_GLOBAL>);
}

/* the structure module's kernel for a call, or nullptr: the interpreter renders it.  A module made without
 * lol_gpu_set_scene_view_samples has no supersampled kernels: those calls then go to the interpreter's. */
static hipFunction_t structure_kernel(const lol_gpu* ctx, bool lin, bool aa) {
	const StructureKernel& k = ctx->tiers.structure;
	if (!k) return nullptr;
	return aa ? (lin ? k.aa_lin : k.batch_aa) : (lin ? k.lin : k.batch);
}

/* ONE launch over the records: the structure module's kernel where it is loaded, else the interpreter's instantiation for the
 * program's rung (the structure's: every record has it).  `args`: (L, B) for all four of either form. */
static hipError_t launch_scene_views(const lol_gpu* ctx, bool lin, bool aa, void** args, dim3 grid, hipStream_t s) {
	const lol_program& P = ctx->h_prog;
	const unsigned lds = lol::common_lds_dwords(P.n_lights, P.n_materials, P.n_roots) * 4u;
	if (const hipFunction_t f = structure_kernel(ctx, lin, aa))
		return hipModuleLaunchKernel(f, grid.x, grid.y, grid.z, lol::BLOCK, 1, 1, lds, s, args, nullptr);
	return launch_interp(ctx, grid, args, lds, s, [lin, aa](auto v, auto kind) {
		return scene_interp_kernel<decltype(v)::ssize, decltype(kind)::value, decltype(v)::tables_global>(lin, aa);
	});
}

/* the records of a call and their data, on the host: SceneView r and, in `data`, what its offsets point to (each part on a multiple
 * of four dwords: the macro-op records want 16 bytes).  `lists`: the interpreter renders, so every record needs its pair of lists.
 * `cams` == nullptr: the records of a query over lists of RAYS — no camera, no first step, and the list every camera may use. */
static int build_scene_records(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n, int max_steps, bool lists,
                               std::vector<lol::SceneView>& views, std::vector<uint32_t>& data) {
	views.resize((size_t)n);
	data.clear();
	std::vector<float> stack;
	std::vector<uint32_t> mops;
	auto align = [&]() { data.resize((data.size() + 3u) & ~(size_t)3u, 0u); };
	const bool cull = culling_enabled(ctx->want_cull);
	for (int r = 0; r < n; r++) {
		const lol_program& P = scenes[r];
		lol::SceneView& V = views[(size_t)r];
		memset(&V, 0, sizeof V);
		const bool finite = shadow_settle_ok(P);
		const unsigned want = ctx->want_skips;
		V.flags = ((want & 1u) && miss_skip_ok(P) ? lol::FLAG_MISS_SKIP : 0u) | ((want & 2u) && dark_skip_ok(P) ? lol::FLAG_DARK_SKIP : 0u);
		bool second_list = false;
		if (cams) {
			const lol_frame_camera& cam = cams[r];
			memcpy(&V.cam, &cam, sizeof V.cam);
			float d = 0.f; uint32_t id = 0;
			const bool first = program_first_step(P, cam, max_steps, stack, &d, &id);      /* (on this record's scene: nothing is kept) */
			second_list = camera_fields(V, cam, finite, (want & 4u) && finite, first, d, id);
		} else if ((want & 4u) && finite) {
			V.flags |= lol::FLAG_SHADOW_SETTLED;      /* the scene's side of it; the rays' side is the kernel's ballot, as for any list of rays */
		}
		/* a query's two bits (lol_kernel_scene_queries.h): what ray_query and launch_scene_query decide from the uploaded scene and the
		 * call's camera, from this record's.  None of SCENE_VIEW_FLAGS: the frames' kernels mask them out. */
		if (finite) V.flags |= lol::SCENE_VIEW_FINITE;
		if (finite && (!cams || camera_sane(cams[r]))) V.flags |= lol::SCENE_VIEW_SANE;
		V.ambient[0] = P.ambient_color.x; V.ambient[1] = P.ambient_color.y; V.ambient[2] = P.ambient_color.z;
		if (lists) {
			uint32_t n_mops = 0;
			if (!build_interp_lists(P, ctx->fast, cull, mops, n_mops)) return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "interpreter lists differ in length");
			align();
			V.n_mops = n_mops;
			V.ops_offset = (uint32_t)data.size() + (second_list ? n_mops * (uint32_t)lol::MOP_DWORDS : 0u);
			data.insert(data.end(), mops.begin(), mops.end());
		}
		align();
		V.tables_offset = (uint32_t)data.size();
		data.resize(data.size() + lol::table_dwords(P.n_lights, P.n_materials, P.n_roots));
		pack_tables(data.data() + V.tables_offset, P);
		align();
		V.nums_offset = (uint32_t)data.size();
		data.resize(data.size() + (size_t)P.n_ops * lol::OP_NUMBERS);
		for (uint32_t i = 0; i < P.n_ops; i++) memcpy(data.data() + V.nums_offset + (size_t)i * lol::OP_NUMBERS, P.ops[i].f, sizeof P.ops[i].f);
		if (data.size() > 0x7FFFFFFFu) return fail(ctx, LOL_GPU_ERR_ARG, "the scenes of one call hold more than 2^31 dwords: fewer views per call");
	}
	align();
	return LOL_GPU_OK;
}

/* the next set of the ring filled with the records and their data, and its copy to the device queued on `s` (queue_view_records) */
static int queue_scene_records(lol_gpu* ctx, const std::vector<lol::SceneView>& views, const std::vector<uint32_t>& data, hipStream_t s, RingSet** out) {
	RingSet& S = ctx->scene_view_records.next();
	const size_t head = views.size() * lol::SCENE_VIEW_DWORDS, need = head + data.size();
	LOL_TRY(ring_take(ctx, S, need * 4, std::max<size_t>(4096, need + need / 2) * 4, RING_PINNED, s, nullptr, "records of a batch of scene views"));
	memcpy(S.h_buf, views.data(), head * 4);
	if (!data.empty()) memcpy(S.h_buf + head, data.data(), data.size() * 4);
	*out = &S;
	const hipError_t e = ring_copy(S, need * 4, s);
	return e == hipSuccess ? LOL_GPU_OK : ring_done(ctx, S, s, e, "copy of the records of a batch of scene views");
}

/* what the scenes of the records are refused for, once the program is known to be there: a missing table, another structure, a
 * material that is not there */
static int scenes_refused(lol_gpu* ctx, const lol_program* scenes, int n) {
	const lol_program& U = ctx->h_prog;
	for (int r = 0; r < n; r++) {
		const lol_program& P = scenes[r];
		if ((P.n_ops && !P.ops) || (P.n_lights && !P.lights) || !P.materials || (P.n_roots && !P.root_material))
			return fail(ctx, LOL_GPU_ERR_ARG, "malformed scene of a view: a table is missing");
		if (P.n_ops != U.n_ops || !same_structure(U, P))
			return fail(ctx, LOL_GPU_ERR_ARG, "a view's scene has not the uploaded program's structure (counts, opcodes, ids)");
		for (uint32_t i = 0; i < P.n_roots; i++)
			if (P.root_material[i] >= P.n_materials) return fail(ctx, LOL_GPU_ERR_ARG, "material index out of range in a view's scene");
	}
	return LOL_GPU_OK;
}

/* `samples` x `samples` samples per pixel (lol_gpu_render_scene_views_samples; 1: lol_gpu_render_scene_views).  Nothing in the records
 * depends on it: with samples > 1 the launch is the one of lol_gpu_render_views_samples — counted in samples, the sample grid's size
 * in fw / fh, the sample bits in the flags — and the kernels are the supersampled ones, which reduce a pixel's samples in registers:
 * the destination, the scratch (one LinearColour per PIXEL and record) and the resolve pass are those of one sample. */
static int render_scene_views(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_views, int K, int w, int h,
                              int max_steps, int samples, void* dst, size_t pitch_bytes, size_t view_stride_bytes, const lol_gpu_debug* dbg,
                              void* stream) {
	if (!ctx || !cams || !scenes || !dst) return LOL_GPU_ERR_ARG;
	if (samples != 1 && samples != 2 && samples != 4) return fail(ctx, LOL_GPU_ERR_ARG, "samples per axis must be 1, 2 or 4");
	LOL_TRY(blend_refused(ctx, cams, n_views, K, w, h, max_steps, dst, pitch_bytes, view_stride_bytes));
	const int n = n_views * K;
	LOL_TRY(scenes_refused(ctx, scenes, n));
	const bool aa = samples > 1;
	if (aa && !lol::samples_fit_wave(samples))
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, "this build's wave patch (LOL_WAVE_W x LOL_WAVE_H) does not divide into that many samples per axis");
	if ((K > 1 || aa) && dbg && (dbg->hit_dist || dbg->hit_id || dbg->steps))
		return fail(ctx, LOL_GPU_ERR_UNSUPPORTED, aa ? "hit_dist, hit_id and steps have no single value for a supersampled pixel"
		                                             : "hit_dist, hit_id and steps have no single value for a pixel averaged over scenes");
	dim3 grid;
	if (!batch_grid(ctx, (long long)samples * w, (long long)samples * h, n, &grid))
		return fail(ctx, LOL_GPU_ERR_ARG, aa ? "batch too large for one launch in samples over all its records: fewer views per call"
		                                     : "batch too large for one launch over all its records: fewer views per call");
	hipStream_t s;
	LOL_TRY(batch_stream(ctx, stream, &s));              /* (the frame boundary: a structure module that has finished is loaded here) */
	std::vector<lol::SceneView> views;
	std::vector<uint32_t> data;
	LOL_TRY(build_scene_records(ctx, cams, scenes, n, max_steps, !structure_kernel(ctx, K > 1, aa), views, data));
	RingSet* scratch = nullptr;
	if (K > 1) {
		scratch = &ctx->blends.next();
		const size_t need = (size_t)n * (size_t)w * (size_t)h * sizeof(lol::LinearColour);
		LOL_TRY(ring_take(ctx, *scratch, need, need, RING_SCRATCH, s, &ctx->fail_view_scratch, "scratch of a blend of scene views"));
	}
	RingSet* S = nullptr;
	LOL_TRY(queue_scene_records(ctx, views, data, s, &S));
	batch_range(aa ? (K > 1 ? "supersampled blend of scene views" : "supersampled scene views") : K > 1 ? "blend of scene views" : "scene views", n, w, h);
	lol::Launch L;
	if (K > 1) batch_launch(ctx, w, h, max_steps, scratch->d_buf, (size_t)w * 4, nullptr, L);
	else       batch_launch(ctx, w, h, max_steps, dst, pitch_bytes, dbg, L);
	if (aa) {
		L.fw = (float)(samples * w); L.fh = (float)(samples * h);      /* the size of the sample grid */
		L.flags |= samples == 4 ? lol::FLAG_SAMPLES_4 : lol::FLAG_SAMPLES_2;
	}
	lol::SceneTail B = { reinterpret_cast<const lol::SceneView*>(S->d_buf), K > 1 ? 0ull : (unsigned long long)(view_stride_bytes / 4),
	                     S->d_buf + views.size() * lol::SCENE_VIEW_DWORDS };
	void* args[] = { &L, &B };
	const char* what = aa ? "kernel launch (supersampled scene views)" : "kernel launch (scene views)";
	hipError_t e = launch_scene_views(ctx, K > 1, aa, args, grid, s);
	if (e == hipSuccess && K > 1) {
		what = aa ? "kernel launch (supersampled blend of scene views, resolve pass)" : "kernel launch (blend of scene views, resolve pass)";
		e = launch_blend_resolve(ctx, L, scratch->d_buf, n_views, K, w, h, dst, pitch_bytes, view_stride_bytes, dbg, s);
	}
	if (g_roctx.pop) g_roctx.pop();
	return ring_done(ctx, *S, s, e, what, scratch);
}

extern "C" {

int lol_gpu_render_scene_views(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_views, int cams_per_view,
                               int w, int h, int max_steps, void* dst, size_t pitch_bytes, size_t view_stride_bytes,
                               const lol_gpu_debug* dbg, void* stream) {
	return guarded(ctx, "the scenes of a batch", [&] {
		return render_scene_views(ctx, cams, scenes, n_views, cams_per_view, w, h, max_steps, 1, dst, pitch_bytes, view_stride_bytes, dbg, stream);
	});
}

/* s = 1 IS lol_gpu_render_scene_views: the call forwards to it behind the one refusal that comes first */
int lol_gpu_render_scene_views_samples(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_views, int cams_per_view,
                                       int w, int h, int max_steps, int samples, void* dst, size_t pitch_bytes, size_t view_stride_bytes,
                                       const lol_gpu_debug* dbg, void* stream) {
	if (!ctx || !cams || !scenes || !dst) return LOL_GPU_ERR_ARG;
	if (samples != 1 && samples != 2 && samples != 4) return fail(ctx, LOL_GPU_ERR_ARG, "samples per axis must be 1, 2 or 4");
	if (samples == 1)
		return lol_gpu_render_scene_views(ctx, cams, scenes, n_views, cams_per_view, w, h, max_steps, dst, pitch_bytes, view_stride_bytes, dbg, stream);
	return guarded(ctx, "the scenes of a batch", [&] {
		return render_scene_views(ctx, cams, scenes, n_views, cams_per_view, w, h, max_steps, samples, dst, pitch_bytes, view_stride_bytes, dbg, stream);
	});
}

int lol_gpu_set_scene_view_samples(lol_gpu* ctx, int enable) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	ctx->want_scene_view_samples = enable ? 1 : 0;      /* takes effect at the next lol_gpu_upload_program; brings lol_gpu_set_scene_views */
	return LOL_GPU_OK;
}
int lol_gpu_scene_view_samples(const lol_gpu* ctx) { return ctx ? ctx->want_scene_view_samples : LOL_GPU_ERR_ARG; }

const char* lol_gpu_scene_view_samples_kernel_name(const lol_gpu* ctx, int cams_per_view, int samples) {
	if (!ctx) return "";
	if (samples <= 1) return lol_gpu_scene_views_kernel_name(ctx, cams_per_view);
	const bool lin = cams_per_view > 1;
	if (structure_kernel(ctx, lin, true)) return lin ? "lol_render_param_batch_aa_lin" : "lol_render_param_batch_aa";
	return lin ? "render_interp_scene_batch_aa_lin" : "render_interp_scene_batch_aa";
}

int lol_gpu_set_scene_views(lol_gpu* ctx, int enable) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	ctx->want_scene_views = enable ? 1 : 0;      /* takes effect at the next lol_gpu_upload_program */
	return LOL_GPU_OK;
}
int lol_gpu_scene_views(const lol_gpu* ctx) { return ctx ? ctx->want_scene_views : LOL_GPU_ERR_ARG; }

const char* lol_gpu_scene_views_kernel_name(const lol_gpu* ctx, int cams_per_view) {
	if (!ctx) return "";
	const bool lin = cams_per_view > 1;
	if (ctx->tiers.structure) return lin ? "lol_render_param_batch_lin" : "lol_render_param_batch";
	return lin ? "render_interp_scene_batch_lin" : "render_interp_scene_batch";
}

int lol_gpu_interp_fast_paths(const lol_gpu* ctx, int* sqrt_kind, unsigned* n_div, unsigned* n_div_no_fixup) {
	if (!ctx || !sqrt_kind || !n_div || !n_div_no_fixup) return LOL_GPU_ERR_ARG;
	*sqrt_kind = ctx->have_prog ? ctx->interp_sqrt_kind : 0;
	*n_div = ctx->have_prog ? (unsigned)ctx->fast.div_ok.size() : 0u;
	*n_div_no_fixup = ctx->have_prog ? (unsigned)ctx->fast.div_nf_ok.size() : 0u;
	return LOL_GPU_OK;
}

int lol_gpu_shade_math(const lol_gpu* ctx, lol_gpu_shade_math_info* out) {
	if (!ctx || !out) return LOL_GPU_ERR_ARG;
	memset(out, 0, sizeof *out);
	if (ctx->have_prog) {
		const FastPaths& F = ctx->fast;
		out->root_kind = F.shade_root; out->rcp_form = F.shade_rcp;
	}
	const IntervalProof* P[2] = { &ctx->shade_proofs.rcp[0], &ctx->shade_proofs.rcp[1] };
	for (int i = 0; i < 2; i++) { out->proof_lo[i] = P[i]->lo; out->proof_hi[i] = P[i]->hi; out->proof_mismatches[i] = P[i]->mismatches; }
	return LOL_GPU_OK;
}

int lol_gpu_scene_views_state(const lol_gpu* ctx) { return ctx ? ctx->tiers.structure_state : LOL_GPU_ERR_ARG; }


}  // extern "C"

/*
 * Light passes and relighting (include/lol_gpu.h; the kernels: lol_kernel_light.h).  A capture is a list query (above), launched as
 * a shading query is (launch_scene_query) with the two skips that rest on the uploaded look cleared, on the interpreter's light_interp
 * always.  A resolve — lol_gpu_relight, and lol_gpu_relight_views below — is refused by relit_refused and look_refused and launched
 * by launch_resolve: it copies the look's tables through a ring of their own (lol_gpu::looks) and launches its kernel behind the copy;
 * with no look it reads the context's own tables and copies nothing.
 */
static int light_query(lol_gpu* ctx, const QuerySource& src, const lol_gpu_light_passes* out) {
	LOL_TRY(source_refused(ctx, src, !out, out));
	lol::LightQuery Q = {};
	Q.stride = out->light_stride ? out->light_stride : src.n;
	Q.out = { reinterpret_cast<lol::LightFactor*>(out->factors), out->hit_id, out->hit_dist, out->march_steps };
	return launch_scene_query(ctx, src, Q, true, nullptr, "light pass launch", [](auto v, auto kind) {
		return reinterpret_cast<const void*>(&lol::light_interp<decltype(v)::ssize, decltype(kind)::value, decltype(v)::tables_global>);
	});
}

/* What `K` — the `noun` of the refusal: a look, or the program planes are said to hold — may not differ from `U` in, or nullptr: the
 * first difference, written to `text` behind `who` (and, for the look of record `record` >= 0, "record <r>"), for the context's error.
 * `look_only`: with the two tests that hold a look to what was captured and that a program which is merely to have U's geometry need
 * not pass — a moved light, a changed shininess. */
static const char* look_differs(const lol_program& U, const lol_program& K, const char* who, int record, const char* noun, bool look_only,
                                char (&text)[200]) {
	auto say = [&](const char* fmt) {
		char of_record[64];
		if (record >= 0) { snprintf(of_record, sizeof of_record, "%s: record %d", who, record); who = of_record; }
		snprintf(text, sizeof text, fmt, who, noun);
		return text;
	};
	if (K.n_ops != U.n_ops || K.n_lights != U.n_lights || K.n_materials != U.n_materials || K.n_roots != U.n_roots || K.max_stack != U.max_stack)
		return say("%s: the %s differs from the uploaded program in a count (ops, lights, materials, roots, max_stack)");
	if ((K.n_ops && !K.ops) || (K.n_lights && !K.lights) || !K.materials || (K.n_roots && !K.root_material))
		return say("%s: malformed %s: a table is missing");
	for (uint32_t i = 0; i < K.n_ops; i++)
		if (K.ops[i].op != U.ops[i].op || K.ops[i].id != U.ops[i].id || memcmp(K.ops[i].f, U.ops[i].f, sizeof K.ops[i].f) != 0)
			return say("%s: the %s differs from the uploaded program in an op (opcode, id or a number): capture again");
	for (uint32_t l = 0; look_only && l < K.n_lights; l++)
		if (memcmp(&K.lights[l].point, &U.lights[l].point, sizeof K.lights[l].point) != 0)
			return say("%s: the %s moves a light: capture again");
	for (uint32_t m = 0; look_only && m < K.n_materials; m++)
		if (memcmp(&K.materials[m].shininess, &U.materials[m].shininess, 4) != 0)
			return say("%s: the %s changes a shininess: capture again");
	for (uint32_t i = 0; i < K.n_roots; i++) {
		if (K.root_material[i] >= K.n_materials) return say("%s: material index out of range in the %s");
		if (K.root_material[i] != U.root_material[i]) return say("%s: the %s gives an object another material: capture again");
	}
	return nullptr;
}

/* The Launch of a resolve under `look` (nullptr: the context's own tables, nothing copied): counts, gamma table and pixel format the
 * context's; a look's tables (pack_tables: its counts are the program's, the refusals have seen to it) go through lol_gpu::looks onto
 * the device behind what `s` holds, and `S` is then the ring's set, which the caller hands to ring_done with its launch. */
static int relight_launch_fields(lol_gpu* ctx, const lol_program* look, hipStream_t s, lol::Launch& L, RingSet*& S) {
	memset(&L, 0, sizeof L);
	scene_launch_fields(ctx, nullptr, L);       /* counts, the context's own tables and ambient colour, gamma table, pixel format */
	S = nullptr;
	if (look) {
		const size_t need = lol::table_dwords(look->n_lights, look->n_materials, look->n_roots);
		S = &ctx->looks.next();
		LOL_TRY(ring_take(ctx, *S, need * 4, std::max<size_t>(1024, need + need / 2) * 4, RING_PINNED, s, nullptr, "tables of a look"));
		pack_tables(S->h_buf, *look);
		const hipError_t ce = ring_copy(*S, need * 4, s);
		if (ce != hipSuccess) return ring_done(ctx, *S, s, ce, "copy of the tables of a look");
		launch_tables(L, S->d_buf);
		L.ambient[0] = look->ambient_color.x; L.ambient[1] = look->ambient_color.y; L.ambient[2] = look->ambient_color.z;
	}
	return LOL_GPU_OK;
}

/* What both resolves refuse, in two halves, because each call refuses its own count of elements between them: first the planes and
 * the outputs ... */
static int relit_refused(lol_gpu* ctx, const lol_gpu_light_passes* in, const lol_gpu_relit* out) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	if (!in || !out) return fail(ctx, LOL_GPU_ERR_ARG, "relight: no planes or no output");
	if (!out->rgb_linear && !out->rgb && !out->pixel) return fail(ctx, LOL_GPU_ERR_ARG, "relight: no output");
	return LOL_GPU_OK;
}
/* ... then, with the count n known to be sound: the program, the planes against n, the look */
static int look_refused(lol_gpu* ctx, const lol_program* look, const lol_gpu_light_passes* in, size_t n) {
	if (!ctx->have_prog) return fail(ctx, LOL_GPU_ERR_NO_PROGRAM, "no scene program uploaded");
	LOL_TRY(passes_refused(ctx, in, n));
	char text[200];
	if (look) if (const char* why = look_differs(ctx->h_prog, *look, "relight", -1, "look", true, text)) return fail(ctx, LOL_GPU_ERR_ARG, why);
	return LOL_GPU_OK;
}

/* Everything behind a resolve's filled query: the Launch under the look, the tables' LDS, a block per lol::BLOCK of `lanes`, the kernel
 * for where the tables lie, and the look's ring set handed back */
template <class Query>
static int launch_resolve(lol_gpu* ctx, const lol_program* look, void* stream, Query& Q, unsigned long long lanes, const void* fn_lds, const void* fn_global) {
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
	lol::Launch L;
	RingSet* S;
	LOL_TRY(relight_launch_fields(ctx, look, s, L, S));
	const lol_program& P = ctx->h_prog;
	const dim3 grid((unsigned)((lanes + lol::BLOCK - 1) / lol::BLOCK));
	void* args[] = { &L, &Q };
	const void* fn = lol::tables_in_lds(P.n_lights, P.n_materials, P.n_roots) ? fn_lds : fn_global;
	const hipError_t e = hipLaunchKernel(fn, grid, dim3(lol::BLOCK), args, tables_lds_bytes(P), s);
	if (S) return ring_done(ctx, *S, s, e, "relight launch");
	if (e != hipSuccess) return fail(ctx, LOL_GPU_ERR_HIP, "relight launch", e);
	return LOL_GPU_OK;
}

/*
 * Relit averaged pixels (include/lol_gpu.h, "Relit views"; the kernel: lol_kernel_light_views.h).  The capture is a host loop over
 * lol_gpu_light_pixels — n_views K launches, record r into the planes at r s^2 w h — and adds no kernel and no capture path; the
 * resolve is lol_gpu_relight's copy of the look and ONE launch of relight_views.
 */
/* What both calls refuse in the shape of the planes, in this order; *n_out = N = n_views K s^2 w h */
static int views_shape_refused(lol_gpu* ctx, int n_views, int cams_per_view, int w, int h, int samples, size_t* n_out) {
	if (n_views < 1 || w < 1 || h < 1) return fail(ctx, LOL_GPU_ERR_ARG, "relit views: n_views < 1 or bad frame geometry");
	const int K = cams_per_view, s = samples;
	if (K != 1 && K != 2 && K != 4 && K != 8 && K != 16) return fail(ctx, LOL_GPU_ERR_ARG, "relit views: cams_per_view must be 1, 2, 4, 8 or 16");
	if (s != 1 && s != 2 && s != 4) return fail(ctx, LOL_GPU_ERR_ARG, "relit views: samples must be 1, 2 or 4");
	const unsigned __int128 N = (unsigned __int128)n_views * (unsigned)K * (unsigned)(s * s) * (unsigned)w * (unsigned)h;
	if (N > 0xFFFFFFFFu) return fail(ctx, LOL_GPU_ERR_ARG, "relit views: more than 2^32 - 1 elements");
	*n_out = (size_t)N;
	return LOL_GPU_OK;
}

/* The planes' half of a resolve's query — a RelightQuery, RelightViewsQuery or RelightSceneViewsQuery, zeroed here —: the planes,
 * over `n_all` elements in all, and the three outputs */
template <class Query>
static void resolve_planes(Query& Q, const lol_gpu_light_passes* in, size_t n_all, const lol_gpu_relit* out) {
	memset(&Q, 0, sizeof Q);
	Q.factors = reinterpret_cast<const lol::LightFactor*>(in->factors);
	Q.stride = in->light_stride ? in->light_stride : n_all;
	Q.hit_id = in->hit_id;
	Q.rgb_linear = out->rgb_linear; Q.rgb = out->rgb; Q.pixel = out->pixel;
}

/* a resolve of n elements whose every refusal has passed */
static int relight_launch(lol_gpu* ctx, const lol_program* look, const lol_gpu_light_passes* in, size_t n, const lol_gpu_relit* out, void* stream) {
	if (n == 0) return LOL_GPU_OK;
	lol::RelightQuery Q;
	resolve_planes(Q, in, n, out);
	Q.n = (uint32_t)n;
	return launch_resolve(ctx, look, stream, Q, Q.n, reinterpret_cast<const void*>(&lol::relight_rays<false>), reinterpret_cast<const void*>(&lol::relight_rays<true>));
}

/* ... and of averaged views over N leaves (not K = 1 with s = 1: that is relight_launch) */
static int relight_views_launch(lol_gpu* ctx, const lol_program* look, const lol_gpu_light_passes* in, size_t N, int n_views, int cams_per_view,
                                int w, int h, int samples, const lol_gpu_relit* out, void* stream) {
	lol::RelightViewsQuery Q;
	resolve_planes(Q, in, N, out);
	Q.n_pixels = (uint32_t)((size_t)n_views * (size_t)w * (size_t)h);
	Q.w = (uint32_t)w; Q.h = (uint32_t)h;
	Q.s_log2 = samples == 4 ? 2u : samples == 2 ? 1u : 0u;
	Q.cams = (uint32_t)cams_per_view;
	Q.last_view = (uint32_t)n_views - 1u;
	/* a wave per 64 pixels, whatever s and K: it takes them in s^2 rounds of 64 / s^2 */
	const unsigned long long lanes = ((unsigned long long)Q.n_pixels + 63u) / 64u * 64u;
	return launch_resolve(ctx, look, stream, Q, lanes, reinterpret_cast<const void*>(&lol::relight_views<false>), reinterpret_cast<const void*>(&lol::relight_views<true>));
}

extern "C" {

int lol_gpu_light_rays(lol_gpu* ctx, const float* rays_dev, size_t n, int max_steps, const lol_gpu_light_passes* out, void* stream) {
	return light_query(ctx, rays_source("light passes", rays_dev, n, max_steps, stream), out);
}

int lol_gpu_light_pixels(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps,
                         const uint32_t* xy_dev, size_t n, const lol_gpu_light_passes* out, void* stream) {
	return light_query(ctx, pixels_source("light passes", cam, w, h, xy_dev, n, max_steps, stream, true), out);
}

int lol_gpu_relight(lol_gpu* ctx, const lol_program* look, const lol_gpu_light_passes* in, size_t n, const lol_gpu_relit* out, void* stream) {
	LOL_TRY(relit_refused(ctx, in, out));
	if (n > 0xFFFFFFFFu) return fail(ctx, LOL_GPU_ERR_ARG, "relight: more than 2^32 - 1 elements");
	LOL_TRY(look_refused(ctx, look, in, n));
	return relight_launch(ctx, look, in, n, out, stream);
}

int lol_gpu_light_views(lol_gpu* ctx, const lol_frame_camera* cams, int n_views, int cams_per_view, int w, int h, int samples,
                        int max_steps, const lol_gpu_light_passes* out, void* stream) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	if (!out) return fail(ctx, LOL_GPU_ERR_ARG, "light passes: no output");
	if (max_steps < 0) return fail(ctx, LOL_GPU_ERR_ARG, "light passes: max_steps < 0 or more than 2^32 - 1 rays");
	if (!cams) return fail(ctx, LOL_GPU_ERR_ARG, "light passes: no camera or bad frame geometry");
	size_t N = 0;
	LOL_TRY(views_shape_refused(ctx, n_views, cams_per_view, w, h, samples, &N));
	QuerySource all = rays_source("light passes", nullptr, N, max_steps, stream);       /* no program; the planes, against all N elements */
	all.list_optional = true;
	LOL_TRY(source_refused(ctx, all, false, out));
	/* the whole call has passed: record r is lol_gpu_light_pixels of the s w x s h frame under cams[r], r s^2 w h elements further on */
	const size_t per = N / ((size_t)n_views * (size_t)cams_per_view);
	const int records = n_views * cams_per_view;
	for (int r = 0; r < records; r++) {
		const size_t at = (size_t)r * per;
		lol_gpu_light_passes sub;
		sub.factors      = out->factors ? out->factors + at : nullptr;
		sub.light_stride = out->light_stride ? out->light_stride : N;
		sub.hit_id       = out->hit_id + at;
		sub.hit_dist     = out->hit_dist ? out->hit_dist + at : nullptr;
		sub.march_steps  = out->march_steps ? out->march_steps + at : nullptr;
		LOL_TRY(lol_gpu_light_pixels(ctx, &cams[r], samples * w, samples * h, max_steps, nullptr, per, &sub, stream));
	}
	return LOL_GPU_OK;
}

int lol_gpu_relight_views(lol_gpu* ctx, const lol_program* look, const lol_gpu_light_passes* in, int n_views, int cams_per_view,
                          int w, int h, int samples, const lol_gpu_relit* out, void* stream) {
	LOL_TRY(relit_refused(ctx, in, out));
	size_t N = 0;
	LOL_TRY(views_shape_refused(ctx, n_views, cams_per_view, w, h, samples, &N));
	if (cams_per_view == 1 && samples == 1) return lol_gpu_relight(ctx, look, in, N, out, stream);      /* a pixel is its one leaf */
	LOL_TRY(look_refused(ctx, look, in, N));
	return relight_views_launch(ctx, look, in, N, n_views, cams_per_view, w, h, samples, out, stream);
}
}  // extern "C"

/*
 * Light updates and the resolves of updated planes (include/lol_gpu.h, "Light updates"; the kernel: lol_kernel_light_update.h).  An
 * update is a list query over the source its capture had (QuerySource, source_refused) and ONE launch of light_update_interp behind the
 * copy of the look's tables through lol_gpu::looks (relight_launch_fields): the Launch's tables are the look's, its macro-op lists the
 * context's.  What the settled shadow loop and the fast SDF rest on is decided as launch_scene_query decides it, from the LOOK
 * (shadow_settle_ok: its light points are part of the test) — what a context that uploaded the look would have cached.  Nothing of the
 * frames' state is read or written, the cached first step included: nothing marches from the eye.
 */
static int light_update(lol_gpu* ctx, const lol_program* look, const QuerySource& src, uint64_t march_lights, uint64_t specular_lights,
                        const lol_gpu_light_passes* planes) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	if (!look) return fail(ctx, LOL_GPU_ERR_ARG, "light update: no look");
	LOL_TRY(source_refused(ctx, src, !planes, planes));
	if (!planes->hit_dist) return fail(ctx, LOL_GPU_ERR_ARG, "light update: no hit_dist plane");
	const lol_program& P = ctx->h_prog;
	const uint64_t masks = march_lights | specular_lights;
	if (P.n_lights < 64u && (masks >> P.n_lights) != 0)
		return fail(ctx, LOL_GPU_ERR_ARG, "light update: a mask names a light the program has not (lights from the 64th on: capture again)");
	char text[200];
	if (const char* why = look_differs(P, *look, "light update", -1, "look", false, text)) return fail(ctx, LOL_GPU_ERR_ARG, why);
	if (src.n == 0 || masks == 0) return LOL_GPU_OK;

	lol::LightUpdateQuery Q = {};
	Q.march_lights = march_lights;
	Q.specular_lights = specular_lights;
	Q.stride = planes->light_stride ? planes->light_stride : src.n;
	Q.factors = reinterpret_cast<lol::LightFactor*>(planes->factors);
	Q.hit_id = planes->hit_id;
	Q.hit_dist = planes->hit_dist;

	LOL_HIP(ctx, hipSetDevice(ctx->device));
	hipStream_t s = src.stream ? static_cast<hipStream_t>(src.stream) : ctx->stream;
	lol::Launch L;
	RingSet* S = nullptr;
	LOL_TRY(relight_launch_fields(ctx, look, s, L, S));       /* the context's lists, counts and gamma table; the look's tables, behind their copy */
	L.flags &= ~(lol::FLAG_MISS_SKIP | lol::FLAG_DARK_SKIP);     /* every factor of every ray, as at a capture */
	/* launch_scene_query's two decisions, with the look's answer in the place of the context's cached ones */
	const bool finite = shadow_settle_ok(*look), sane = !src.pixels || camera_sane(*src.cam);
	if (finite && sane) Q.flags |= lol::SHADE_SCENE_SANE;
	if ((ctx->want_skips & 4u) && finite && sane) L.flags |= lol::FLAG_SHADOW_SETTLED;
	source_fields(src, L, Q);
	if (src.pixels) memcpy(&L.cam, src.cam, sizeof L.cam);
	const dim3 grid((unsigned)(((unsigned long long)Q.n + lol::BLOCK - 1) / lol::BLOCK));
	void* args[] = { &L, &Q };
	const hipError_t e = launch_interp(ctx, grid, args, tables_lds_bytes(P), s, [](auto v, auto kind) {
		return reinterpret_cast<const void*>(&lol::light_update_interp<decltype(v)::ssize, decltype(kind)::value, decltype(v)::tables_global>);
	});
	return ring_done(ctx, *S, s, e, "light update launch");
}

/* look_refused for planes that hold `held`, not the uploaded program: `held` has the program's geometry, and the look equals `held`
 * where a look must equal what was captured — light points and shininess included */
static int held_look_refused(lol_gpu* ctx, const lol_program* look, const lol_program& held, const lol_gpu_light_passes* in, size_t n) {
	if (!ctx->have_prog) return fail(ctx, LOL_GPU_ERR_NO_PROGRAM, "no scene program uploaded");
	LOL_TRY(passes_refused(ctx, in, n));
	char text[200];
	if (const char* why = look_differs(ctx->h_prog, held, "relight", -1, "held program", false, text)) return fail(ctx, LOL_GPU_ERR_ARG, why);
	if (const char* why = look_differs(held, look ? *look : ctx->h_prog, "relight", -1, "look", true, text)) return fail(ctx, LOL_GPU_ERR_ARG, why);
	return LOL_GPU_OK;
}

extern "C" {

int lol_gpu_light_update_rays(lol_gpu* ctx, const lol_program* look, const float* rays_dev, size_t n, uint64_t march_lights,
                              uint64_t specular_lights, const lol_gpu_light_passes* planes, void* stream) {
	return light_update(ctx, look, rays_source("light update", rays_dev, n, 0, stream), march_lights, specular_lights, planes);
}

int lol_gpu_light_update_pixels(lol_gpu* ctx, const lol_program* look, const lol_frame_camera* cam, int w, int h, const uint32_t* xy_dev,
                                size_t n, uint64_t march_lights, uint64_t specular_lights, const lol_gpu_light_passes* planes, void* stream) {
	return light_update(ctx, look, pixels_source("light update", cam, w, h, xy_dev, n, 0, stream, true), march_lights, specular_lights, planes);
}

int lol_gpu_relight_held(lol_gpu* ctx, const lol_program* look, const lol_program* held, const lol_gpu_light_passes* in, size_t n,
                         const lol_gpu_relit* out, void* stream) {
	if (!held) return lol_gpu_relight(ctx, look, in, n, out, stream);
	LOL_TRY(relit_refused(ctx, in, out));
	if (n > 0xFFFFFFFFu) return fail(ctx, LOL_GPU_ERR_ARG, "relight: more than 2^32 - 1 elements");
	LOL_TRY(held_look_refused(ctx, look, *held, in, n));
	return relight_launch(ctx, look, in, n, out, stream);
}

int lol_gpu_relight_views_held(lol_gpu* ctx, const lol_program* look, const lol_program* held, const lol_gpu_light_passes* in, int n_views,
                               int cams_per_view, int w, int h, int samples, const lol_gpu_relit* out, void* stream) {
	if (!held) return lol_gpu_relight_views(ctx, look, in, n_views, cams_per_view, w, h, samples, out, stream);
	LOL_TRY(relit_refused(ctx, in, out));
	size_t N = 0;
	LOL_TRY(views_shape_refused(ctx, n_views, cams_per_view, w, h, samples, &N));
	LOL_TRY(held_look_refused(ctx, look, *held, in, N));
	if (cams_per_view == 1 && samples == 1) return relight_launch(ctx, look, in, N, out, stream);       /* a pixel is its one leaf */
	return relight_views_launch(ctx, look, in, N, n_views, cams_per_view, w, h, samples, out, stream);
}
}  // extern "C"

/*
 * Scene queries (include/lol_gpu.h, "Scene queries"; the kernels: lol_kernel_scene_queries.h): a list query (QuerySource,
 * source_refused) answered under each record's own scene — record_query (with the list queries, above), whose callers here fill their
 * query and name their kernel: ONE launch of the interpreter's, the record in the grid's y.  What
 * ray_query and launch_scene_query decide from the uploaded scene and the call's camera is decided per record, from that record's own.
 * The context's scene, kernels, keys, cached first step, tile-order state, sample settings and other rings are neither read nor
 * changed, and no scene kernel takes over here: the interpreter answers, whatever the module switches say.
 * Last in this file: its kernels are instantiated behind all others (lol_gpu_internal.h).
 */
static int scene_ray_query(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_scenes, const QuerySource& src,
                           size_t list_stride, const lol_gpu_hits* out) {
	const bool no_output = !out || (!out->dist && !out->id && !out->steps && !out->normal);
	return guarded(ctx, "the scenes of a query", [&] {
		return record_query(ctx, cams, scenes, n_scenes, src, list_stride, no_output, nullptr, "scene ray query launch", [&](lol::SceneList& R, hipStream_t s) {
			/* ray_query's RayQuery, without what the record brings: camera, first step, list, RAYS_SCENE_SANE */
			lol::RayQuery Q;
			memset(&Q, 0, sizeof Q);
			Q.rays = src.rays;
			Q.xy = src.xy;
			Q.n = (uint32_t)src.n;
			Q.max_steps = src.max_steps;
			if (src.pixels) { Q.flags = lol::RAYS_FROM_PIXELS; Q.fw = (float)src.w; Q.fh = (float)src.h; }
			if (out->id) Q.flags |= lol::RAYS_WANT_ID;
			if (out->normal) Q.flags |= lol::RAYS_WANT_NORMAL;
			Q.out = { out->dist, out->id, out->steps, out->normal };
			const dim3 grid = record_grid(src.n, 64u, n_scenes);
			void* args[] = { &Q, &R };
			const int kind = ctx->interp_sqrt_kind;
			return stack_class_dispatch(interp_stack_class(ctx->h_prog.max_stack), [&](auto v) {
				constexpr int ssize = decltype(v)::ssize;
				const void* k = kind == 3 ? reinterpret_cast<const void*>(&lol::trace_interp_scenes<ssize, 3>)
				                          : reinterpret_cast<const void*>(&lol::trace_interp_scenes<ssize, 0>);
				return hipLaunchKernel(k, grid, dim3(64), args, 0, s);
			});
		});
	});
}

static int scene_shade_query(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_scenes, const QuerySource& src,
                             size_t list_stride, const lol_gpu_shades* out) {
	const bool no_output = !out || (!out->rgb_linear && !out->rgb && !out->pixel && !out->hit_dist && !out->hit_id && !out->steps);
	return guarded(ctx, "the scenes of a query", [&] {
		return record_query(ctx, cams, scenes, n_scenes, src, list_stride, no_output, nullptr, "scene shading query launch", [&](lol::SceneList& R, hipStream_t s) {
			/* launch_scene_query's Launch, without what the record brings: camera, first step, lists, tables, ambient colour, the skips */
			lol::Launch L;
			memset(&L, 0, sizeof L);
			L.max_steps = src.max_steps;
			context_launch_fields(ctx, L);
			lol::ShadeQuery Q = {};
			source_fields(src, L, Q);
			Q.out = { out->rgb_linear, out->rgb, out->pixel, out->hit_dist, out->hit_id, out->steps };
			void* args[] = { &L, &Q, &R };
			return launch_interp(ctx, record_grid(src.n, lol::BLOCK, n_scenes), args, tables_lds_bytes(ctx->h_prog), s, [](auto v, auto kind) {
				return reinterpret_cast<const void*>(&lol::shade_interp_scenes<decltype(v)::ssize, decltype(kind)::value, decltype(v)::tables_global>);
			});
		});
	});
}

extern "C" {

int lol_gpu_trace_scene_rays(lol_gpu* ctx, const lol_program* scenes, int n_scenes, const float* rays_dev, size_t n, size_t list_stride,
                             int max_steps, const lol_gpu_hits* out, void* stream) {
	return scene_ray_query(ctx, nullptr, scenes, n_scenes, rays_source("scene ray query", rays_dev, n, max_steps, stream), list_stride, out);
}

int lol_gpu_trace_scene_pixels(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_scenes, int w, int h, int max_steps,
                               const uint32_t* xy_dev, size_t n, size_t list_stride, const lol_gpu_hits* out, void* stream) {
	return scene_ray_query(ctx, cams, scenes, n_scenes, pixels_source("scene ray query", cams, w, h, xy_dev, n, max_steps, stream), list_stride, out);
}

int lol_gpu_shade_scene_rays(lol_gpu* ctx, const lol_program* scenes, int n_scenes, const float* rays_dev, size_t n, size_t list_stride,
                             int max_steps, const lol_gpu_shades* out, void* stream) {
	return scene_shade_query(ctx, nullptr, scenes, n_scenes, rays_source("scene shading query", rays_dev, n, max_steps, stream), list_stride, out);
}

int lol_gpu_shade_scene_pixels(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_scenes, int w, int h, int max_steps,
                               const uint32_t* xy_dev, size_t n, size_t list_stride, const lol_gpu_shades* out, void* stream) {
	return scene_shade_query(ctx, cams, scenes, n_scenes, pixels_source("scene shading query", cams, w, h, xy_dev, n, max_steps, stream), list_stride, out);
}
}  // extern "C"

/*
 * Scene light passes (include/lol_gpu.h, "Scene light passes"; the kernels: lol_kernel_scene_light.h): a capture and a resolve whose
 * records are scenes of the uploaded program's structure.  A capture is a scene query (record_query, above) with a capture's planes:
 * scene views' records with the two skips that rest on a look cleared on EVERY record, scene views' ring and ONE launch of
 * light_interp_scenes with the record in the grid's y.  A resolve checks look r against scenes[r] as lol_gpu_relight checks a look
 * against the uploaded program and goes through record_resolve, as the averaged resolve below does: the looks' tables — a LookRecord
 * each and, behind the records, lights | materials | root_material — through lol_gpu::looks and its kernel behind the copy.  The context's scene, kernels, keys, cached first step, tile-order
 * state, sample settings and other rings are neither read nor changed; no scene kernel takes over, and nothing waits for one.
 * Last in this file, its header included here: the kernels are instantiated behind all others (lol_gpu_internal.h).
 */
#include "lol_kernel_scene_light.h"

static int scene_light_query(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_scenes, const QuerySource& src,
                             size_t list_stride, const lol_gpu_light_passes* out) {
	return guarded(ctx, "the scenes of a capture", [&] {
		return record_query(ctx, cams, scenes, n_scenes, src, list_stride, !out, out, "scene light pass launch", [&](lol::SceneList& R, hipStream_t s) {
			/* launch_scene_query's Launch, without what the record brings: camera, first step, lists, tables, ambient colour, the skips —
			 * and without gamma table and pixel format: a capture packs no pixel */
			lol::Launch L;
			memset(&L, 0, sizeof L);
			L.max_steps = src.max_steps;
			launch_counts(ctx, L);
			lol::LightQuery Q = {};
			source_fields(src, L, Q);
			Q.stride = out->light_stride ? out->light_stride : (unsigned long long)n_scenes * (unsigned long long)src.n;
			Q.out = { reinterpret_cast<lol::LightFactor*>(out->factors), out->hit_id, out->hit_dist, out->march_steps };
			void* args[] = { &L, &Q, &R };
			return launch_interp(ctx, record_grid(src.n, lol::BLOCK, n_scenes), args, tables_lds_bytes(ctx->h_prog), s, [](auto v, auto kind) {
				return reinterpret_cast<const void*>(&lol::light_interp_scenes<decltype(v)::ssize, decltype(kind)::value, decltype(v)::tables_global>);
			});
		});
	});
}

/* 4. of both resolves over records: the first looks[r] that is no look of scenes[r], by its record, behind `who` */
static int record_looks_refused(lol_gpu* ctx, const char* who, const lol_program* scenes, const lol_program* looks, int n_records) {
	char text[200];
	for (int r = 0; looks && r < n_records; r++)
		if (const char* why = look_differs(scenes[r], looks[r], who, r, "look", true, text)) return fail(ctx, LOL_GPU_ERR_ARG, why);
	return LOL_GPU_OK;
}

/* The looks of a resolve over records onto the device behind what `s` holds, through lol_gpu::looks: a LookRecord per record and,
 * behind them, each look's tables as an upload lays them out, on multiples of four dwords — look r's at r nt4
 * dwords (lol::look_stride, lol_kernel_scene_light_views.h, is this nt4).  `S` is then the ring's set, which the caller hands to ring_done with its launch. */
static int queue_record_looks(lol_gpu* ctx, const lol_program* scenes, const lol_program* looks, int n_records, hipStream_t s, RingSet*& S,
                              lol::LookList& R) {
	const lol_program& U = ctx->h_prog;
	const size_t nt = lol::table_dwords(U.n_lights, U.n_materials, U.n_roots), nt4 = (nt + 3u) & ~(size_t)3u;
	const size_t head = (size_t)n_records * lol::LOOK_RECORD_DWORDS, need = head + (size_t)n_records * nt4;
	if (need > 0x7FFFFFFFu) return fail(ctx, LOL_GPU_ERR_ARG, "relight scenes: the looks of one call hold more than 2^31 dwords: fewer scenes per call");
	S = &ctx->looks.next();
	LOL_TRY(ring_take(ctx, *S, need * 4, std::max<size_t>(1024, need + need / 2) * 4, RING_PINNED, s, nullptr, "tables of the looks of a relight over scenes"));
	memset(S->h_buf, 0, need * 4);
	for (int r = 0; r < n_records; r++) {
		const lol_program& K = looks ? looks[r] : scenes[r];
		lol::LookRecord rec;
		rec.tables_offset = (uint32_t)((size_t)r * nt4);
		rec.ambient[0] = K.ambient_color.x; rec.ambient[1] = K.ambient_color.y; rec.ambient[2] = K.ambient_color.z;
		memcpy(S->h_buf + (size_t)r * lol::LOOK_RECORD_DWORDS, &rec, sizeof rec);
		pack_tables(S->h_buf + head + rec.tables_offset, K);      /* (its counts are U's: scenes_refused and record_looks_refused have run) */
	}
	const hipError_t ce = ring_copy(*S, need * 4, s);
	if (ce != hipSuccess) return ring_done(ctx, *S, s, ce, "copy of the tables of the looks of a relight over scenes");
	R = { reinterpret_cast<const lol::LookRecord*>(S->d_buf), S->d_buf + head };
	return LOL_GPU_OK;
}

/* Everything behind a filled query of a resolve over records: the call's device and stream, the looks through their ring, the Launch —
 * relight_launch_fields' without the context's tables and ambient colour, which the records bring: context_launch_fields alone —, the
 * launch of `fn` on `grid` with `lds` bytes behind the copy, and the ring's event behind it, `what` its name */
template <class Query>
static int record_resolve(lol_gpu* ctx, const lol_program* scenes, const lol_program* looks, int n_records, void* stream, Query& Q, dim3 grid,
                          unsigned lds, const void* fn, const char* what) {
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
	RingSet* S = nullptr;
	lol::LookList R;
	LOL_TRY(queue_record_looks(ctx, scenes, looks, n_records, s, S, R));
	lol::Launch L;
	memset(&L, 0, sizeof L);
	context_launch_fields(ctx, L);
	void* args[] = { &L, &Q, &R };
	return ring_done(ctx, *S, s, hipLaunchKernel(fn, grid, dim3(lol::BLOCK), args, lds, s), what);
}

static int relight_scenes(lol_gpu* ctx, const lol_program* scenes, const lol_program* looks, int n_scenes, const lol_gpu_light_passes* in,
                          size_t n, const lol_gpu_relit* out, void* stream) {
	/* 1. what lol_gpu_relight refuses before it looks at its look */
	LOL_TRY(relit_refused(ctx, in, out));
	if (n > 0xFFFFFFFFu) return fail(ctx, LOL_GPU_ERR_ARG, "relight: more than 2^32 - 1 elements");
	LOL_TRY(look_refused(ctx, nullptr, in, n));
	/* 2. the records and the planes of all of them */
	if (!scenes) return fail(ctx, LOL_GPU_ERR_ARG, "relight scenes: no scenes");
	if (n_scenes < 1 || n_scenes > LOL_GPU_MAX_VIEWS) return fail(ctx, LOL_GPU_ERR_ARG, "relight scenes: the number of scenes is not in 1 ... LOL_GPU_MAX_VIEWS");
	const unsigned long long N = (unsigned long long)n_scenes * (unsigned long long)n;
	if (N > 0xFFFFFFFFull) return fail(ctx, LOL_GPU_ERR_ARG, "relight scenes: more than 2^32 - 1 elements over all scenes");
	if (in->light_stride != 0 && in->light_stride < N) return fail(ctx, LOL_GPU_ERR_ARG, "relight scenes: light_stride is neither 0 nor at least n_scenes * n");
	/* 3. the scenes: what the planes hold */
	LOL_TRY(scenes_refused(ctx, scenes, n_scenes));
	/* 4. the looks, each against its own scene: the first that is no look of it, by its record */
	LOL_TRY(record_looks_refused(ctx, "relight scenes", scenes, looks, n_scenes));
	if (n == 0) return LOL_GPU_OK;

	const lol_program& U = ctx->h_prog;
	lol::RelightQuery Q;
	resolve_planes(Q, in, N, out);
	Q.n = (uint32_t)n;
	const void* fn = lol::tables_in_lds(U.n_lights, U.n_materials, U.n_roots) ? reinterpret_cast<const void*>(&lol::relight_rays_scenes<false>)
	                                                                          : reinterpret_cast<const void*>(&lol::relight_rays_scenes<true>);
	return record_resolve(ctx, scenes, looks, n_scenes, stream, Q, record_grid(n, lol::BLOCK, n_scenes), tables_lds_bytes(U), fn, "relight scenes launch");
}

extern "C" {

int lol_gpu_light_scene_rays(lol_gpu* ctx, const lol_program* scenes, int n_scenes, const float* rays_dev, size_t n, size_t list_stride,
                             int max_steps, const lol_gpu_light_passes* out, void* stream) {
	return scene_light_query(ctx, nullptr, scenes, n_scenes, rays_source("scene light passes", rays_dev, n, max_steps, stream), list_stride, out);
}

int lol_gpu_light_scene_pixels(lol_gpu* ctx, const lol_frame_camera* cams, const lol_program* scenes, int n_scenes, int w, int h, int max_steps,
                               const uint32_t* xy_dev, size_t n, size_t list_stride, const lol_gpu_light_passes* out, void* stream) {
	return scene_light_query(ctx, cams, scenes, n_scenes, pixels_source("scene light passes", cams, w, h, xy_dev, n, max_steps, stream, true),
	                         list_stride, out);
}

int lol_gpu_relight_scenes(lol_gpu* ctx, const lol_program* scenes, const lol_program* looks, int n_scenes, const lol_gpu_light_passes* in,
                           size_t n, const lol_gpu_relit* out, void* stream) {
	return relight_scenes(ctx, scenes, looks, n_scenes, in, n, out, stream);
}
}  // extern "C"

/*
 * Relit scene views (include/lol_gpu.h, "Relit scene views"; the kernel: lol_kernel_scene_light_views.h): the averaged resolve of
 * relit views over planes whose every record holds a scene of its own, under a look per record.  The refusals of relit views up to
 * its look, then those of the resolve over records (above); the looks' LookRecords and tables go through lol_gpu::looks as
 * relight_scenes lays them out (queue_record_looks), and ONE launch of relight_views_scenes follows the copy, the view in the grid's
 * y.  Nothing is allocated on the host, so nothing throws.  The context's scene, kernels, keys, tile-order state, sample settings and
 * other rings are neither read nor changed.
 * Last in this file, its header included here: the kernels are instantiated behind all others (lol_gpu_internal.h).
 */
#include "lol_kernel_scene_light_views.h"

static int relight_scene_views(lol_gpu* ctx, const lol_program* scenes, const lol_program* looks, const lol_gpu_light_passes* in, int n_views,
                               int cams_per_view, int w, int h, int samples, const lol_gpu_relit* out, void* stream) {
	/* 1. what lol_gpu_relight_views refuses before it looks at its look */
	LOL_TRY(relit_refused(ctx, in, out));
	size_t N = 0;
	LOL_TRY(views_shape_refused(ctx, n_views, cams_per_view, w, h, samples, &N));
	LOL_TRY(look_refused(ctx, nullptr, in, N));
	/* 2. the records */
	if (!scenes) return fail(ctx, LOL_GPU_ERR_ARG, "relight scene views: no scenes");
	const long long records = (long long)n_views * cams_per_view;
	if (records > LOL_GPU_MAX_VIEWS) return fail(ctx, LOL_GPU_ERR_ARG, "relight scene views: more than LOL_GPU_MAX_VIEWS records (n_views * cams_per_view)");
	/* a pixel that is its one leaf: the resolve of single leaves, which refuses 3. and 4. in its own words */
	if (cams_per_view == 1 && samples == 1) return lol_gpu_relight_scenes(ctx, scenes, looks, n_views, in, (size_t)w * (size_t)h, out, stream);
	/* 3. the scenes: what the planes hold */
	LOL_TRY(scenes_refused(ctx, scenes, (int)records));
	/* 4. the looks, each against its own scene: the first that is no look of it, by its record */
	LOL_TRY(record_looks_refused(ctx, "relight scene views", scenes, looks, (int)records));

	const lol_program& U = ctx->h_prog;
	lol::RelightSceneViewsQuery Q;
	resolve_planes(Q, in, N, out);
	Q.w = (uint32_t)w; Q.h = (uint32_t)h;
	Q.s_log2 = samples == 4 ? 2u : samples == 2 ? 1u : 0u;
	Q.cams = (uint32_t)cams_per_view;
	/* a wave per 64 pixels of ONE view, whatever s and K: it takes them in s^2 rounds of 64 / s^2 */
	const unsigned long long lanes = ((unsigned long long)w * (unsigned long long)h + 63u) / 64u * 64u;
	/* the K looks of a view staged as one run where they fit, read where they lie where they do not: the kernel's rule */
	const bool staged = lol::views_looks_in_lds(Q.cams, U.n_lights, U.n_materials, U.n_roots);
	const unsigned lds = staged ? Q.cams * lol::look_stride(U.n_lights, U.n_materials, U.n_roots) * 4u : 0u;
	const void* fn = staged ? reinterpret_cast<const void*>(&lol::relight_views_scenes<false>)
	                        : reinterpret_cast<const void*>(&lol::relight_views_scenes<true>);
	return record_resolve(ctx, scenes, looks, (int)records, stream, Q, record_grid(lanes, lol::BLOCK, n_views), lds, fn, "relight scene views launch");
}

extern "C" {

int lol_gpu_relight_scene_views(lol_gpu* ctx, const lol_program* scenes, const lol_program* looks, const lol_gpu_light_passes* in, int n_views,
                                int cams_per_view, int w, int h, int samples, const lol_gpu_relit* out, void* stream) {
	return relight_scene_views(ctx, scenes, looks, in, n_views, cams_per_view, w, h, samples, out, stream);
}
}  // extern "C"
