/*
 * lol_gpu_internal.h — what the translation units of liblol_gpu.so share: the context (struct lol_gpu), the scene compiler's job,
 * the proven shortcuts (FastPaths), and the few functions that cross from one unit to another.  Nothing here is part of the
 * C ABI (include/lol_gpu.h); everything declared between the visibility pragmas stays inside the library.
 *
 *   lol_gpu.hip      the context and the C ABI around it: upload, frames (device and host surfaces, frames in flight, adaptive
 *                    frames), the first march step, the rings of per-call device sets, batches of views (plain, supersampled,
 *                    blended) and of scene views, the interpreter's ladder, the SDF alone, the list queries (ray queries,
 *                    shading queries, light passes) and the relight resolves, diagnostics
 *   lol_tiers.hip    the tiers of the scene compiler: its runs on their own threads, the kernels they load, the swaps at frame
 *                    boundaries, lol_gpu_specialize_*
 *   lol_proofs.hip   the exhaustive on-device proofs of the fast paths, the gamma table, lol_gpu_verify_*
 *   lol_codegen.hip  exact culling (bounds, plan), the interpreter's macro-op lists, the scene -> HIP source generator,
 *                    hipRTC + the code-object cache + the long-branch trip-wire, lol_gpu_compile_offline
 *   lol_sched.hip    the order in which a frame's tiles are handed out: fixed orders and their trials, longest tiles first,
 *                    pixels dealt by cost (tables and the kernels that make them)
 *   lol_multi.hip    several devices behind the boundary (RCCL exchange)
 */
#pragma once
#include "lol_gpu.h"
#include "lol_gpu_diag.h"
#include "lol_gpu_testing.h"
#include "lol_kernel.h"
#include "lol_kernel_aa.h"
#include "lol_kernel_batch.h"
#include "lol_kernel_batch_aa.h"
#include "lol_kernel_blend.h"
#include "lol_kernel_blend_aa.h"
#include "lol_kernel_rays.h"
#include "lol_kernel_shade.h"
#include "lol_kernel_scenes.h"
#include "lol_kernel_scenes_aa.h"
#include "lol_kernel_light.h"      /* last, and its kernels are instantiated last in lol_gpu.hip: the code objects of the others stay what they are */
#include "lol_kernel_light_views.h"      /* ... and this one behind it, its kernels behind those, for the same reason */
#include "lol_kernel_light_update.h"     /* ... and the light updates' behind both */
#include "lol_kernel_scene_queries.h"    /* ... and the scene queries' behind all three */

#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <dlfcn.h>
#include <pthread.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <memory>
#include <thread>
#include <functional>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>


static_assert(sizeof(lol_light) == lol::LIGHT_DWORDS * 4, "lol_light layout");
static_assert(sizeof(lol_material) == lol::MATERIAL_DWORDS * 4, "lol_material layout");
static_assert(sizeof(lol_frame_camera) == sizeof(lol::Cam), "lol_frame_camera layout");
/* the batch kernels' argument segment is a Launch and a BatchTail behind it at the next multiple of 8 (lol_kernel_batch.h,
 * view_stride_px reads the tail there) */
static_assert(sizeof(lol::Launch) % 8 == 0 && offsetof(lol::BatchArgs, B) == sizeof(lol::Launch) &&
              sizeof(lol::BatchArgs) == sizeof(lol::Launch) + sizeof(lol::BatchTail) && sizeof(lol::View) == 18 * 4,
              "kernel-argument layout of the batch kernels");
/* ... and a shading query's is a Launch and a ShadeQuery behind it (lol_kernel_shade.h, shade_out reads the outputs there) */
/* ... and a batch of scene views' is a Launch and a SceneTail behind it, which begins like a BatchTail (lol_kernel_scenes.h) */
static_assert(offsetof(lol::SceneTail, views) == offsetof(lol::BatchTail, views) && offsetof(lol::SceneTail, view_stride_px) == offsetof(lol::BatchTail, view_stride_px),
              "kernel-argument layout of the scene-view kernels");
static_assert(offsetof(lol::ShadeArgs, Q) == sizeof(lol::Launch) && sizeof(lol::ShadeArgs) == sizeof(lol::Launch) + sizeof(lol::ShadeQuery),
              "kernel-argument layout of the shading kernels");
/* ... and a capture's is a Launch and a LightQuery behind it (lol_kernel_light.h, light_out reads the outputs there) */
static_assert(offsetof(lol::LightArgs, Q) == sizeof(lol::Launch) && sizeof(lol::LightArgs) == sizeof(lol::Launch) + sizeof(lol::LightQuery) &&
              sizeof(lol::LightFactor) == sizeof(lol_gpu_light_factor) && sizeof(lol_gpu_light_factor) == 16,
              "kernel-argument layout of the capture kernels, and the factor's");

#pragma GCC visibility push(hidden)

/* The scene compiler runs on a thread of its own with a LARGE stack: the compiler inside hipRTC recurses over the long
 * dependent chains of a big scene's straight-line SDF — a field of 3000 objects overflowed the usual 8 MB in the hipRTC
 * that PyTorch bundles (ROCm 7.0's; the system's 7.2 survived) and took the process down.  1 GB of address space; only
 * the pages really used are ever committed. */
struct BigStackThread {
	pthread_t t{};
	bool started = false;
	std::function<void()> fn;
	static void* entry(void* self) { static_cast<BigStackThread*>(self)->fn(); return nullptr; }
	bool start(std::function<void()> f) {
		fn = std::move(f);
		pthread_attr_t attr;
		if (pthread_attr_init(&attr) != 0) return false;
		(void)pthread_attr_setstacksize(&attr, (size_t)1 << 30);
		started = pthread_create(&t, &attr, entry, this) == 0;
		if (!started) {                                 /* (no gigabyte of address space to be had: the default stack) */
			pthread_attr_t plain;
			if (pthread_attr_init(&plain) == 0) { started = pthread_create(&t, &plain, entry, this) == 0; pthread_attr_destroy(&plain); }
		}
		pthread_attr_destroy(&attr);
		return started;
	}
	bool joinable() const { return started; }
	void join() { if (started) { pthread_join(t, nullptr); started = false; } }
};

/* What the device has proven about its own arithmetic, as far as the scene at hand needs it (lol_proofs.hip: prove_fast_paths);
 * the generator (lol_codegen.hip) and the interpreter's lists use a shortcut only where this says so. */
/* One exhaustive comparison of a shortcut with the expression it replaces, over all 2^32 floats: on how many they differ, and
 * the interval of bit patterns around 1.0f that holds none of them — (0, 0xFFFFFFFF) when they agree everywhere, empty (lo > hi)
 * when they differ at 1.0f itself. */
struct IntervalProof {
	unsigned long long mismatches = ~0ull;      /* ~0: not run, or could not run */
	uint32_t lo = 1u, hi = 0u;
	bool ran() const { return mismatches != ~0ull; }
	bool covers(uint32_t a, uint32_t b) const { return ran() && lo <= a && b <= hi; }
};
/* ... of the arithmetic of the fast pipeline's shading (lol_kernel.h, ShadeMath) */
struct ShadeProofs {
	bool ran = false;
	IntervalProof rcp[2];                 /* lol::rcp_fast<1>, <2> against 1.0f / x */
};

struct FastPaths {
	/* the shading around the loops (lol_kernel.h, ShadeMath; generated into the fast SDF as its member type Shade): */
	int shade_root = 0;                   /* len() through sqrt_fast<shade_root>: sqrt_kind, or 0 (LOL_GPU_SHADE_MATH=0) */
	int shade_rcp = 0;                    /* 1.0f / len through rcp_fast<shade_rcp>: the cheapest form proven on [2^-48, 2^64]; 0 the division */
	int sqrt_kind = 0;                    /* 0 plain sqrtf; 1 sqrt_pm, 2 sqrt_gs, 3 sqrt_r2 — proven on this device */
	bool sqrt_tiny_ok = false;            /* ... and NaN-or-tiny below its domain: spheres may drop the range tracker (sd_sphere_fast_nr) */
	std::vector<float> div_ok;            /* smoothness constants k whose smin_h_fast verified */
	std::vector<float> div_nf_ok;         /* ... and verified without v_div_fixup as well (smin_h_fast<false>) */
	bool gamma_ok = false;                /* the gamma table route == the powf route for every float in [0, 1] (verify_gamma_kernel) */
	bool has(float k) const {
		for (float v : div_ok) if (memcmp(&v, &k, 4) == 0) return true;
		return false;
	}
	bool has_nf(float k) const {
		for (float v : div_nf_ok) if (memcmp(&v, &k, 4) == 0) return true;
		return false;
	}
};

/* A program and the memory behind its four tables (lol_program itself only points: include/lol_scene.h). */
struct OwnedProgram {
	lol_program p{};
	std::vector<lol_op> ops;
	std::vector<lol_light> lights;
	std::vector<lol_material> materials;
	std::vector<uint32_t> root_material;
	/* all or nothing: the copies are made on the side (any of them may throw std::bad_alloc) and swapped in together, so a
	 * failed assign leaves the old program — tables AND counts — as it was */
	void assign(const lol_program& src) {
		std::vector<lol_op> o(src.ops, src.ops + src.n_ops);
		std::vector<lol_light> l(src.lights, src.lights + src.n_lights);
		std::vector<lol_material> m(src.materials, src.materials + src.n_materials);
		std::vector<uint32_t> r(src.root_material, src.root_material + src.n_roots);
		ops.swap(o); lights.swap(l); materials.swap(m); root_material.swap(r);      /* (noexcept) */
		p = src;
		p.ops = ops.data(); p.lights = lights.data(); p.materials = materials.data(); p.root_material = root_material.data();
	}
	OwnedProgram() = default;
	OwnedProgram(const OwnedProgram&) = delete;
	OwnedProgram& operator=(const OwnedProgram&) = delete;
};

/* The families of render kernels, each of which exists twice: as an instantiation of the interpreter (lol_kernel*.h) and as a symbol
 * of the scene module (generate_source).  THE list: generate_source emits the symbols, load_scene_kernel looks them up, launch_family
 * (lol_gpu.hip) launches one or the other and the reported kernel names come from here.  A new family is one row plus its kernel. */
enum KernelFamily { FAM_FRAME, FAM_FRAME_AA, FAM_FRAME_AA_LIST, FAM_BATCH, FAM_BATCH_AA, FAM_BATCH_AA_LIST, FAM_BATCH_LIN, FAM_BATCH_AA_LIN,
                    N_FAMILIES };
/* the switch that puts a family into the module of the next upload: a row of MODULE_SWITCHES below */
enum ModuleSwitch { SWITCH_NONE, SWITCH_AA, SWITCH_BATCH, SWITCH_BATCH_AA, SWITCH_BATCH_BLEND, SWITCH_BATCH_BLEND_AA, SWITCH_RAYS, SWITCH_SHADE,
                    N_SWITCHES };
constexpr unsigned switch_bit(int sw) { return (1u << sw) >> 1; }      /* 1u << (sw - 1), and none for SWITCH_NONE */
constexpr unsigned ALL_SWITCHES = (1u << (N_SWITCHES - 1)) - 1;
struct FamilyRow {
	const char*  symbol;        /* in the scene module */
	const char*  counting;      /* its twin with the per-lane step counters (modules up to LOL_SPEC_TWO_KERNELS_MAX_OPS ops), or none */
	const char*  interp;        /* the interpreter's kernel, as lol_gpu_kernel_name reports it */
	ModuleSwitch needs;
};
constexpr FamilyRow KERNEL_FAMILIES[N_FAMILIES] = {
	/* FAM_FRAME         (L)              */ { "lol_render_spec",               "lol_render_spec_steps",       "render_interp",               SWITCH_NONE },
	/* FAM_FRAME_AA      (L)              */ { "lol_render_spec_aa",            nullptr,                       "render_interp_aa",            SWITCH_AA },
	/* FAM_FRAME_AA_LIST (L, list, count) */ { "lol_render_spec_aa_list",       nullptr,                       "render_interp_aa_list",       SWITCH_AA },
	/* FAM_BATCH         (L, B)           */ { "lol_render_spec_batch",         "lol_render_spec_batch_steps", "render_interp_batch",         SWITCH_BATCH },
	/* FAM_BATCH_AA      (L, B)           */ { "lol_render_spec_batch_aa",      nullptr,                       "render_interp_batch_aa",      SWITCH_BATCH_AA },
	/* FAM_BATCH_AA_LIST (L, B, Q)        */ { "lol_render_spec_batch_aa_list", nullptr,                       "render_interp_batch_aa_list", SWITCH_BATCH_AA },
	/* FAM_BATCH_LIN     (L, B)           */ { "lol_render_spec_batch_lin",     nullptr,                       "render_interp_batch_lin",     SWITCH_BATCH_BLEND },
	/* FAM_BATCH_AA_LIN  (L, B)           */ { "lol_render_spec_batch_aa_lin",  nullptr,                       "render_interp_batch_aa_lin",  SWITCH_BATCH_BLEND_AA },
};

/* What a scene module carries beside lol_render_spec and lol_sdf_spec, one row per switch.  THE list: a module is a mask of
 * switch_bit()s — the context's (lol_gpu::module_switches, module_kernels_of), an offline compile's (lol_gpu_compile_offline_module,
 * whose documentation in lol_gpu_diag.h restates these rows) —, generate_source includes a row's header in the block it appends for
 * it, and what a switch brings with it is said here alone.  Without any switch the source is exactly what it was before these
 * kernels existed.  A new switch is one row, its block in generate_source, and its public setter. */
struct SwitchRow {
	const char* setter;         /* the public call that sets it before an upload */
	const char* header;         /* what the block generate_source appends for it includes */
	unsigned    brings;         /* the switches that come with it */
};
constexpr SwitchRow MODULE_SWITCHES[N_SWITCHES] = {
	/* SWITCH_NONE */           { nullptr,                          "lol_kernel.h",          0 },
	/* SWITCH_AA (samples > 1 at the upload) */
	                            { "lol_gpu_set_samples",            "lol_kernel_aa.h",       0 },
	/* SWITCH_BATCH */          { "lol_gpu_set_view_batches",       "lol_kernel_batch.h",    0 },
	/* SWITCH_BATCH_AA: the first pass of an adaptive batch is the plain batch kernels' */
	                            { "lol_gpu_set_view_samples",       "lol_kernel_batch_aa.h", switch_bit(SWITCH_BATCH) },
	/* SWITCH_BATCH_BLEND: the linear-colour batch kernel alone */
	                            { "lol_gpu_set_view_blends",        "lol_kernel_blend.h",    0 },
	/* SWITCH_BATCH_BLEND_AA: its supersampled form alone — a switch of its own, NOT implied by BATCH_BLEND and BATCH_AA together */
	                            { "lol_gpu_set_view_blend_samples", "lol_kernel_blend_aa.h", 0 },
	/* SWITCH_RAYS: lol_trace_spec.  That kernel is no row of KERNEL_FAMILIES: launch_family hands a family a Launch, a block of
	 * lol::BLOCK threads, the tables' LDS and perhaps a counting twin, and a query has none of the four — it lives beside lol_sdf_spec
	 * (SceneKernel::trace), the other kernel that is not a frame */
	                            { "lol_gpu_set_ray_queries",        "lol_kernel_rays.h",     0 },
	/* SWITCH_SHADE: lol_shade_spec, beside it for the same reason (SceneKernel::shade): it takes a Launch and the tables' LDS, but a
	 * ShadeQuery and a grid over a list instead of a frame's tiles, and it has no twin */
	                            { "lol_gpu_set_shade_queries",      "lol_kernel_shade.h",    0 },
};
/* `mask` and what its switches bring (one pass: nothing that is brought brings anything itself) */
constexpr unsigned switch_closure(unsigned mask) {
	unsigned all = mask;
	for (int sw = SWITCH_AA; sw < N_SWITCHES; sw++)
		if (mask & switch_bit(sw)) all |= MODULE_SWITCHES[sw].brings;
	return all;
}
struct ModuleKernels {
	unsigned mask = 0;          /* of switch_bit()s, as set: carries() adds what they bring */
	bool carries(ModuleSwitch sw) const { return sw == SWITCH_NONE || (switch_closure(mask) & switch_bit(sw)) != 0; }
};

/* One code object of the scene compiler, loaded with every kernel generate_source put in it or not at all (load_scene_kernel,
 * lol_tiers.hip).  A plain value: whoever holds it calls unload(). */
struct SceneKernel {
	hipModule_t   module = nullptr;
	hipFunction_t fn[N_FAMILIES] = {};         /* by family; nullptr: the module was compiled without it, the interpreter renders that family */
	hipFunction_t counting[N_FAMILIES] = {};   /* the family's counting twin — or fn[] again, where the module holds no twin of it: that one counts */
	hipFunction_t sdf = nullptr;               /* lol_sdf_spec (lol_gpu_sdf_batch) */
	hipFunction_t trace = nullptr;             /* lol_trace_spec (ray queries), or nullptr: the module was compiled without it, trace_interp answers */
	hipFunction_t shade = nullptr;             /* lol_shade_spec (shading queries), or nullptr: the module was compiled without it, shade_interp answers */
	std::string   key;                         /* code_key_hex of the code object (lol_gpu_kernel_key) */
	explicit operator bool() const { return module != nullptr; }
	void unload() { if (module) (void)hipModuleUnload(module); *this = SceneKernel(); }
};

/* The structure module (lol_codegen.hip, generate_structure_source): a code object of its own beside the scene's, with its own load,
 * unload and key — no row of MODULE_SWITCHES.  Both kernels or none.
 * lol_gpu_set_scene_view_samples is no row of MODULE_SWITCHES either, and for the same reason: those rows say what the SCENE's module
 * carries, and the two supersampled kernels belong to this code object — another source of it (generate_structure_source with
 * `samples`), hence another code object and cache entry.  All four kernels or none then; without that switch the last two stay null
 * and the interpreter's render_interp_scene_batch_aa / _aa_lin render the supersampled calls. */
struct StructureKernel {
	hipModule_t   module = nullptr;
	hipFunction_t batch = nullptr;             /* lol_render_param_batch (counts steps) */
	hipFunction_t lin = nullptr;               /* lol_render_param_batch_lin */
	hipFunction_t batch_aa = nullptr;          /* lol_render_param_batch_aa     (only in a module made with `samples`) */
	hipFunction_t aa_lin = nullptr;            /* lol_render_param_batch_aa_lin (... both or neither) */
	std::string   key;                         /* code_key_hex of the code object */
	explicit operator bool() const { return module != nullptr; }
	void unload() { if (module) (void)hipModuleUnload(module); *this = StructureKernel(); }
};

struct SpecJob;
/* The tiers of the scene compiler: interpreter -> [out-of-line kernel ->] scene kernel (lol_tiers.hip) */
struct SpecTiers {
	enum Tier {
		OFF,          /* no scene kernel wanted or possible: the interpreter renders */
		FIRST,        /* `job` is the scene's first run */
		SECOND,       /* `job` compiles the inlined form */
		SETTLED,      /* nothing behind `kernel` */
		FAILED,       /* no scene kernel to be had: the interpreter renders */
	};
	Tier         tier = OFF;
	std::unique_ptr<SpecJob> job;             /* the run of tier FIRST or SECOND, until the frame boundary that takes its outcome */
	bool         second_wanted = false;       /* the inlined form follows the first tier's kernel */
	SceneKernel  kernel;                      /* the kernel frames run; empty: the interpreter */
	SceneKernel  retired;                     /* the first tier's once the second has taken over: frames in flight may still run it, so it
	                                           * stays loaded until the next upload (which drains the device) or the end of the context */
	std::vector<std::unique_ptr<SpecJob>> old_jobs;   /* runs for programs since replaced: dropped when they have finished */
	std::string  log;                         /* lol_gpu_specialize_log */
	/* the structure module of the uploaded program (lol_gpu_set_scene_views before the upload): compiled by the first run's thread
	 * after the scene's own module, loaded at the frame boundary or wait that finds it finished */
	std::unique_ptr<SpecJob> structure_job;   /* that run, from the boundary that took its scene kernel until its structure module is there */
	StructureKernel structure;                /* empty: the interpreter's scene-view kernels render */
	int          structure_state = 0;         /* lol_gpu_scene_views_state: 0 none, 1 compiling, 2 in use, -1 failed */
	std::string  structure_log;
	double       compile_ms = 0;              /* how long the last finished run took (wall clock of its thread) */
	/* what the next upload asks for */
	bool         want = true;                 /* lol_gpu_set_specialize */
	bool         want_second = true;          /* ... (ctx, 5) says no */
	uint32_t     max_ops = 0;                 /* lol_gpu_set_specialize_max_ops: 0 = LOL_SPEC_MAX_OPS */
	int          fail_first = 0;              /* lol_gpu_testing_fail_first_tier: that many out-of-line first runs "fail" */
	SpecTiers();
	~SpecTiers();                             /* waits for every run (a thread must not outlive the library) and unloads both kernels */
};

/* One set of a ring of per-call device sets, and the ring.  A call takes the ring's next set, whatever its stream, queues its work
 * through it and records `done` behind the last of it; the set's next user — N calls later — waits for `done` on its stream, and on
 * the host only where the set must grow or the stream is one of HIP's special handles.  A pinned set is filled by the host, copied to
 * the device on the call's stream and `copied` recorded behind the copy: the host may write the pinned half again once that has run.
 * Written once, for every ring of the context, in lol_gpu.hip (ring_take, ring_copy, ring_done, ring_free). */
struct RingSet {
	uint32_t*  d_buf = nullptr;
	uint32_t*  h_buf = nullptr;              /* pinned, of as many bytes; rings of records only */
	size_t     bytes = 0;                    /* each holds */
	hipEvent_t copied = nullptr, done = nullptr;
	bool       used = false;                 /* the set's events have been recorded: somebody may still be using it */
	bool       done_special = false;         /* `done` was last recorded on one of HIP's special stream handles: the next user waits for it on the host */
};
template <class Set, int N> struct Ring {
	Set      sets[N];
	unsigned rr = 0;
	Set&     next() { return sets[rr++ % N]; }
};

struct lol_gpu {
	int          device = -1;
	hipStream_t  stream = nullptr;
	/* device tables, two sets: an upload fills the set no frame reads and flips `cur` only when every fallible step
	 * has succeeded (lol_gpu_upload_program is all-or-nothing).  Sized by the program (grown when an upload needs more). */
	uint32_t*    d_tables[2] = { nullptr, nullptr };   /* lights | materials | root_material, as dwords */
	size_t       tables_cap[2] = { 0, 0 };             /* ... dwords allocated */
	uint32_t*    d_mops[2] = { nullptr, nullptr };     /* the interpreter's two macro-op lists (lol_kernel.h, Interp) */
	size_t       mops_cap[2] = { 0, 0 };               /* ... dwords allocated */
	int          cur = 0;
	uint32_t     n_mops = 0;
	OwnedProgram h_own;                  /* host copy of the uploaded program ... */
	lol_program& h_prog = h_own.p;       /* ... and its lol_program view (counts, tables, max_stack) */
	bool         have_prog = false;
	/* the surface's pixel format (lol_gpu_set_pixel_format), packed as lol::Launch wants it; default XRGB8888 */
	uint32_t     fmt_shift = 16u | 8u << 8 | 0u << 16, fmt_loss = 0, fmt_amask = 0;
	/* host-surface path */
	uint32_t*    d_frame = nullptr;      /* framebuffer for lol_gpu_render_host */
	size_t       frame_bytes = 0;
	/* lol_gpu_render_host_begin / _end: frames in flight, one device framebuffer each (sized per slot, so frames of
	 * different sizes can be in flight while the host's window is being resized); slot = frame number % PIPE_SLOTS.  The kernel
	 * of a frame with a NEW view goes to the next of the context's frame streams, one under the view of the frame before it
	 * follows that frame (lol_gpu_render_host_begin): consecutive frames of a moving camera overlap */
	static constexpr int PIPE_SLOTS = 4;
	uint32_t*    d_pipe[PIPE_SLOTS] = { nullptr, nullptr, nullptr, nullptr };
	size_t       pipe_bytes[PIPE_SLOTS] = { 0, 0, 0, 0 };
	hipStream_t  copy_stream = nullptr;
	hipEvent_t   pipe_rendered[PIPE_SLOTS] = { nullptr, nullptr, nullptr, nullptr }, pipe_copied[PIPE_SLOTS] = { nullptr, nullptr, nullptr, nullptr };
	hipStream_t  pipe_stream[PIPE_SLOTS] = { nullptr, nullptr, nullptr, nullptr };   /* the stream the slot's kernel was queued on */
	int          pipe_w[PIPE_SLOTS] = { 0, 0, 0, 0 }, pipe_h[PIPE_SLOTS] = { 0, 0, 0, 0 };
	unsigned     pipe_begun = 0, pipe_ended = 0;
	unsigned     pipe_rr = 0;                    /* rotation of the kernels' streams: advanced by every frame whose view is new */
	hipStream_t  pipe_last_stream = nullptr;     /* ... a frame under the view of the frame before it follows that frame on its stream */
	lol_frame_camera pipe_last_cam{};
	int          pipe_last_geom[3] = { 0, 0, 0 };
	SpecTiers    tiers;                  /* the scene compiler's: the kernel frames run, or none (the interpreter) */
	std::string  interp_key;             /* FNV-1a of {this build, the uploaded macro-op lists}: lol_gpu_kernel_key of the interpreter */
	std::string  interp_aa_key;          /* ... and of its supersampling kernel (render_interp_aa) */
	int          samples = 1;            /* lol_gpu_set_samples: samples per pixel along each axis of the frames launched from now on */
	int          adaptive = -1;          /* lol_gpu_set_adaptive_samples: the contrast T, or -1 (off) */
	int          want_scene_views = 0;   /* lol_gpu_set_scene_views: the next upload also compiles the structure module */
	int          want_scene_view_samples = 0;   /* lol_gpu_set_scene_view_samples: ... with its two supersampled kernels (brings want_scene_views) */
	FastPaths    fast;                   /* what the upload proved on the device: the lists of scene views are built with it */
	unsigned     module_switches = 0; /* the switch_bit()s set by lol_gpu_set_view_batches ... lol_gpu_set_shade_queries (MODULE_SWITCHES) */
	void*        d_pick = nullptr;       /* lol_gpu_pick's device memory, from the first pick on: xy [2] | dist | id | steps | normal [3] */
	/* The six rings of per-call device sets (RingSet above; the protocol: ring_take, ring_copy, ring_done, ring_free in lol_gpu.hip).
	 * Sets grow with what they serve and are freed in lol_gpu_destroy.
	 *   view_records        a batch's lol::View records, pinned and on the device (queue_view_records): at least 64 views a set
	 *   scene_view_records  the records of scene views and, behind them, every record's lists, tables and numbers
	 *                       (lol_gpu_render_scene_views): at least 4096 dwords a set, grown by half more than is needed
	 *   adaptive_frames     scratch of adaptive frames (render_adaptive): xrgb [w h] | ids [w h] | list [w h] | count [64] | lane table
	 *                       [64 per refine block].  `done` is TIMED: ev[0] marks a frame's start, ev[1] and ev[2] the ends of its first
	 *                       two passes, `done` its end (lol_gpu_adaptive_pass_ms)
	 *   adaptive_batches    scratch of adaptive batches (render_views_adaptive): xrgb [n w h] | ids [n w h] | lists [n w h] | counts
	 *                       [n + 1] | prefix [n + 1] | lane table — for n views of w x h: 12 n w h bytes + 8 (n + 1) + 256 per refine block
	 *   blends              scratch of blends (render_blend) and of blends of scene views: the linear colours [n K][h][w] of pass 1 —
	 *                       per PIXEL, whatever the samples —, a lol::LinearColour of 16 bytes each
	 *   looks               the tables of a look (lol_gpu_relight): lights | materials | root_material, pinned and on the device, at
	 *                       least 1024 dwords a set, grown by half more than is needed
	 * The two adaptive rings remember their last set, which lol_gpu_adaptive_refined / _pass_ms and lol_gpu_views_refined read. */
	Ring<RingSet, 8> view_records, scene_view_records;
	struct AdaptiveFrameSet : RingSet {
		hipEvent_t ev[3] = { nullptr, nullptr, nullptr };
		uint32_t*  d_count = nullptr;        /* in d_buf: the length of the list of the set's last frame */
	};
	Ring<AdaptiveFrameSet, 4> adaptive_frames;
	AdaptiveFrameSet* adaptive_last = nullptr;
	struct AdaptiveBatchSet : RingSet {
		uint32_t*  d_counts = nullptr;       /* in d_buf: the lengths of the lists of the set's last batch ... */
		int        n_views = 0;              /* ... one per view */
	};
	Ring<AdaptiveBatchSet, 4> adaptive_batches;
	AdaptiveBatchSet* view_adaptive_last = nullptr;
	Ring<RingSet, 4> blends;
	Ring<RingSet, 8> looks;
	int          fail_view_scratch = 0;        /* lol_gpu_testing_fail_view_scratch: that many scratch allocations of adaptive batches and blends still fail */
	uint32_t*    d_adaptive_order = nullptr;   /* the refine pass's block -> lane-table slot table: slot b at tile_slot(b, stride) */
	uint32_t     adaptive_blocks = 0, adaptive_stride = 0;      /* its size in blocks (the most a refine grid has); ceil(blocks / 8) */
	int          fail_uploads = 0;       /* lol_gpu_testing_fail_uploads: that many uploads still fail at the copy */
	int          want_fast = 1;          /* allow the proven-exact shortcuts in the specialised kernel */
	unsigned     want_skips = 7;         /* exact skips allowed when the program qualifies: bit 0 escaped waves, 1 zero incidence, 2 settled shadows */
	int          want_cull = 1;          /* allow the exact culling of top-level objects (plan_culling) */
	bool         miss_skip = false;      /* the uploaded program qualifies (miss_skip_ok) */
	bool         dark_skip = false;      /* the uploaded program qualifies (dark_skip_ok) */
	bool         shadow_settle = false;  /* the uploaded program qualifies (shadow_settle_ok) */
	bool         finite_scene = false;   /* shadow_settle_ok(program), whatever the switches say: the interpreter's no-fixup list may run */
	int          interp_sqrt_kind = 0;   /* fast sqrt of the interpreter: 3 (sqrt_r2) when proven and allowed, else 0 */
	int          sqrt_verified = -1;     /* -1 not run, 0 none proven, else the lol::sqrt_fast KIND proven on this device */
	bool         sqrt_tiny_ok = false;   /* the second counter of that run was 0 too (sd_sphere_fast_nr) */
	struct DivProof { uint32_t k_bits; bool ok, no_fixup_ok; };
	std::vector<DivProof> div_verified;  /* per smoothness constant: smin_h_fast proven / proven without v_div_fixup too */
	ShadeProofs  shade_proofs;           /* the reciprocal of the fast pipeline's shading (lol_proofs.hip, prove_shade_math) */
	unsigned long long* d_bad = nullptr; /* mismatch counter of the verification kernels */
	float*       d_gamma = nullptr;      /* gamma thresholds (lol_kernel.h, gamma_u8_table): GAMMA_LEVELS + 1 floats */
	int          gamma_verified = -1;    /* -1 not run, 1 the table route == the powf route for every float in [0, 1] on this device, 0 not */
	bool         gamma_table = false;    /* frames of the current scene use it (want_fast at the last upload) */
	/* lol_gpu_set_tile_order.  AUTO: the first frames of a (scene, size, partition) alternate between the two orders, each
	 * between two events on its launch stream; later frames collect the finished ones without waiting (tile_auto_*) */
	struct TileAuto {
		int   mode = LOL_GPU_TILES_LPT;
		int   chosen = LOL_GPU_TILES_ROWS;       /* order outside trials */
		bool  deciding = false;
		int   key[6] = { 0, 0, 0, 0, 0, 0 };    /* w, h, max_steps, band_rows, cycle_rows, program generation */
		int   issued = 0, harvested = 0, decisions = 0;
		static constexpr int SKIP = 6, TOTAL = SKIP + 2 * LOL_GPU_TILE_TRIALS;
		/* trial i: untimed row-order frames first, then pairs (rows, columns), (columns, rows), (rows, columns) ... */
		static constexpr int order_of_trial(int i) { return i < SKIP ? LOL_GPU_TILES_ROWS : ((((i - SKIP) >> 1) ^ (i - SKIP)) & 1); }
		hipEvent_t ev[2 * TOTAL] = {};          /* start / end of trial frame i at [2i], [2i + 1]; created on first use */
		bool  have_events = false;
		float ms[TOTAL] = {};
		float typical[2] = { 0.f, 0.f };
		/* after the decision: a timed pair (order in use, other order) every MONITOR_PERIOD frames (tile_order_for_frame) */
		static constexpr unsigned MONITOR_PERIOD = 8, MONITOR_WINDOW = 5;
		unsigned mon_frames = 0, mon_n = 0, swaps = 0;
		bool  mon_pending = false;
		float mon_ratio[MONITOR_WINDOW] = {};
	} tiles;
	int          generation = 0;         /* uploads so far */
	/* the primary march's first step (first_step): program_first_step of program `first_gen` at `first_origin`, kept while the camera
	 * stays where it is */
	float        first_origin[3] = { 0, 0, 0 };
	int          first_gen = -1;
	bool         first_taken = false;
	float        first_dist = 0;
	uint32_t     first_id = 0;
	std::vector<float> first_stack;
	int          kernel_epoch = 0;       /* changes whenever the frames' kernel does: an upload (the interpreter takes over), each swap of
	                                      * finish_specialise — what a kernel's tiles cost says nothing about another kernel's */
	/* LOL_GPU_TILES_LPT: longest tiles first ("longest tiles first" below).  One SET of tables per stream that launches frames
	 * of a repeated view (lpt_table_for_frame): everything about a set happens on its home stream, so frames, the costs they
	 * write and the sorts that read them are ordered by that stream itself — and frames in flight on several streams
	 * (lol_gpu_set_frames_in_flight, lol_gpu_render_host_begin) each keep their schedule. */
	struct TileLpt {
		int      key[7] = { 0, 0, 0, 0, 0, 0, 0 };   /* w, h, max_steps, band_rows, cycle_rows, offset_rows, kernel_epoch */
		uint32_t n_tiles = 0;
		uint32_t* d_order[2] = { nullptr, nullptr };   /* tile_order tables: frames read [cur], a sort writes [cur ^ 1] */
		uint32_t* d_cost = nullptr;          /* what the blocks of the last frame cost, by launch position */
		uint32_t* d_keys = nullptr;          /* the sort's snapshot of the costs (bucket numbers) */
		uint32_t* d_hist = nullptr;          /* 2 x LPT_BUCKETS: bucket sizes, then the scatter's cursors */
		uint32_t* d_lanes = nullptr;         /* the pixel table: 64 entries per wave slot ("pixels dealt by cost") */
		unsigned short* d_pixel_cost = nullptr;   /* what every pixel of the view's first frame cost */
		size_t   lanes_cap = 0, pixels_cap = 0;
		size_t   pixels = 0;                 /* pixels of the frame that last recorded into d_pixel_cost (lol_gpu_testing_pixel_cost) */
		size_t   cap = 0;                    /* tiles the buffers hold */
		int      cur = 0;
		unsigned frames = 0, sorts = 0;      /* frames launched with this key; sorts done */
		hipStream_t home = nullptr;          /* the stream these tables live on; nullptr = the set is free */
		bool     launched = false;           /* a frame (or a table kernel) has been queued on `home` through these tables since the
		                                      * stream last ran dry: they may be in use whatever `key` says (cleared where that stream is
		                                      * waited for: before the tables are freed, or change hands) */
		unsigned long long stamp = 0;        /* when the set was last used (the least recently used one makes room for a fifth stream) */
		lol_frame_camera cam_epoch{};        /* the view the tables' costs belong to */
		hipEvent_t done = nullptr;           /* recorded behind every frame queued through these tables (lpt_frame_queued) */
		bool     done_recorded = false;
	};
	static constexpr int LPT_SETS = 4;
	TileLpt      lpt[LPT_SETS];
	unsigned long long lpt_clock = 0;
	unsigned     lpt_homeless = 0;       /* consecutive still frames on a stream that has no set while all sets are taken */
	int          lpt_last_set = -1;      /* the set the last frame went through, or -1: it was launched in a fixed order (lol_gpu_tile_order) */
	unsigned     lpt_sorts = 0;          /* sorts of all sets so far (lol_gpu_tile_order) */
	/* the frame launched before this one, on whatever stream: its key and view (lpt_table_for_frame: `still`) */
	int          lpt_last_key[7] = { 0, 0, 0, 0, 0, 0, 0 };
	lol_frame_camera lpt_last_cam{};
	bool         lpt_have_last = false;
	/* Frames in flight (lol_gpu_set_frames_in_flight): frames launched with stream == NULL go round-robin over the first
	 * n_frame_streams of these; [0] is `stream`.  lol_gpu_render_host_begin's slots use them too. */
	static constexpr int MAX_FRAME_STREAMS = 4;
	hipStream_t  frame_streams[MAX_FRAME_STREAMS] = { nullptr, nullptr, nullptr, nullptr };
	int          n_frame_streams = 1;
	unsigned     frame_rr = 0;
	char         err[512] = { 0 };
};

/* the module of an upload: the switches set, and supersampling when the context's frames have more than one sample (what is asked
 * for after the upload renders on the interpreter's kernel of that family) */
inline ModuleKernels module_kernels_of(const lol_gpu* ctx) {
	return { ctx->module_switches | (ctx->samples > 1 ? switch_bit(SWITCH_AA) : 0u) };
}

/* an A/B switch from the environment, honoured only beside LOL_GPU_TUNING=1 and recorded when it is (lol_gpu.hip) */
const char* lol_gpu_internal_tuning_env(const char* name);
static inline const char* tuning_env(const char* name) { return lol_gpu_internal_tuning_env(name); }
/* LOL_GPU_SHADE_MATH=0 beside LOL_GPU_TUNING: the shading around the loops with the plain sqrtf and divisions in the fast pipeline too
 * (lol_kernel.h, ShadeMath); every other value, and none, leaves the proven root and reciprocal on */
static inline bool shade_math_wanted() { const char* e = tuning_env("LOL_GPU_SHADE_MATH"); return !(e && e[0] == '0' && !e[1]); }

int fail(lol_gpu* ctx, int status, const char* what, hipError_t e = hipSuccess);
#define LOL_HIP(ctx, call)                                                        \
	do {                                                                          \
		hipError_t e_ = (call);                                                   \
		if (e_ != hipSuccess) return fail((ctx), LOL_GPU_ERR_HIP, #call, e_);     \
	} while (0)
/* ... and for a step that reports a status of its own */
#define LOL_TRY(expr)                                                             \
	do {                                                                          \
		const int st_ = (expr);                                                   \
		if (st_ != LOL_GPU_OK) return st_;                                        \
	} while (0)

/* operand-stack entries under the accumulator a program needs → the instantiation that has them */
constexpr int interp_stack_class(uint32_t max_stack) {
	const uint32_t need = max_stack > 1 ? max_stack - 1 : 1;      /* the accumulator holds the top entry */
	return need <= 1 ? 1 : need <= 3 ? 3 : need <= 7 ? 7 : need < (uint32_t)lol::MOP_DEEP_FROM ? lol::MOP_DEEP_FROM - 1 : lol::MOP_DEEP_SLOTS;
}

/*
 * The kernel shades every pixel with the fast SDF; a wave in which any squared length fell outside
 * [SQRT_FAST_MIN, inf) (a sample within 2^-48 of a sphere centre, or an overflow) shades its pixels
 * again with the plain SDF, so the shortcut never decides a result.
 */
/* Scenes above this many ops get their SDF as an out-of-line function (emit_sdf).  Rounds 2 - 4: 256 — the inlined form took
 * 1.3 s (256 ops) to 15 s (1024) to compile against 0.35 - 2.2 s out of line, and render_prepare WAITED for the compiler.  It
 * no longer does (tiered start-up: the compiler runs on its own thread, frames render on the interpreter meanwhile), so what
 * decides now is the kernel that comes out.  Measured on MI355X in round 5 (tools/large_scene_ab.py, chains of smooth unions at
 * 1080p, profiles/r5_large_scene_ab.jsonl; inlined / out of line / interpreter, Mpixels/s): 284 ops 311 / 165 / 185 (the
 * out-of-line kernel was SLOWER than the interpreter it replaced), 504 ops 174 / 126 / 105, 1024 ops 80.6 / 60.1 / 43.2 — the
 * inlined form +88 % / +38 % / +34 % for 1.4 / 2.6 / 6.6 s of background compile (0.4 / 0.6 / 1.4 out of line) — and at 2048 ops
 * the other way round: 13.7 / 15.6 (960x540; 19 s against 3.8 s: six copies of a 300 KB function no longer pay).
 * LOL_GPU_SPEC_INLINE_MAX (a tuning switch) overrides. */
constexpr uint32_t LOL_SPEC_INLINE_MAX_OPS = 1024;
/* ... and above THIS many ops the inlined form is the scene's SECOND kernel: the out-of-line form, which hipRTC delivers 3 - 6
 * times sooner, renders until it is there (lol_tiers.hip) */
constexpr uint32_t LOL_SPEC_FIRST_TIER_INLINE_MAX_OPS = 256;
/* ... and up to THIS many ops the module holds the pipeline twice: with and without the per-lane step counters (generate_source) */
constexpr uint32_t LOL_SPEC_TWO_KERNELS_MAX_OPS = 256;
/* specialise(): larger scenes stay on the interpreter.  The scene compiler cannot be interrupted, lol_gpu_destroy has to wait
 * for it, and a second upload's run queues behind it — so what it takes on is bounded by what was MEASURED as tolerable
 * (profiles/r4_big_scene_probe.jsonl, fields of N objects on the GPU box: 5.3 s at 1320 ops, 14.6 s at 2640, 40.7 s at 5060,
 * about n^1.5: a minute at 6500, four at 16,384 — round 4's cap).  LOL_GPU_SPEC_MAX_OPS (a tuning switch) moves it. */
constexpr uint32_t LOL_SPEC_MAX_OPS = 6144;

/* which form of the scene's SDF a run of the compiler produces: by the program's size, or the one the tiers ask for */
enum SpecForm { SPEC_BY_SIZE = 0, SPEC_OUT_OF_LINE = 1, SPEC_INLINE = 2 };

/* ---- lol_proofs.hip */
FastPaths prove_fast_paths(lol_gpu* ctx, const lol_program& prog);
float smooth_sat_threshold(float k);

/* ---- lol_codegen.hip */
inline bool culling_enabled(int want) { return want != 0; }      /* (lol_gpu_set_cull) */
bool spec_out_of_line(const lol_program& P, int form = SPEC_BY_SIZE);
bool compile_spec(const lol_program& P, const FastPaths* fast, const std::string& arch, std::vector<char>& code,
                  std::string& log, std::string* src_out = nullptr, bool cull = true, int form = SPEC_BY_SIZE, ModuleKernels carries = {});
/* the interpreter's two macro-op lists for `P`, one after the other (with / without v_div_fixup in the proven blend factors);
 * false: the two differ in length (cannot happen: same records by construction) */
/* the structure module of `P`: source that depends on P's structure alone (opcodes, ids, counts), and its code object */
/* (`samples`: with lol_render_param_batch_aa and lol_render_param_batch_aa_lin — another source, another code object) */
std::string generate_structure_source(const lol_program& P, bool samples = false);
bool compile_structure(const lol_program& P, const std::string& arch, std::vector<char>& code, std::string& log, std::string* src_out = nullptr,
                       bool samples = false);
bool build_interp_lists(const lol_program& P, const FastPaths& fast, bool cull, std::vector<uint32_t>& lists, uint32_t& n_mops);
std::string fnv_hex(const void* data, size_t n);
std::string code_key_hex(const void* code, size_t n);      /* SceneKernel::key: FNV-1a over what the device loads of a code object (lol_code_key.h) */
extern std::mutex g_rtc_mutex;               /* one run of the scene compiler at a time (lol_gpu.hip) */

/* ---- lol_tiers.hip */
/* the scene compiler's first run for the program the context has just committed (the previous scene's kernels go: the caller has
 * drained the device) */
void start_specialise(lol_gpu* ctx, const FastPaths& fast);
/* the frame boundary: a finished run's outcome takes effect, one per call; `wait`: every run is waited for.  True when the state
 * changed.  The device of the context is current. */
bool finish_specialise(lol_gpu* ctx, bool wait);
/* the scene kernel frames run, or nullptr: the interpreter */
inline const SceneKernel* scene_kernel(const lol_gpu* ctx) { return ctx->tiers.kernel ? &ctx->tiers.kernel : nullptr; }

/* all or nothing for what the source carries: both kernels of the structure module, with `samples` all four, or `why` not */
bool load_structure_kernel(const std::vector<char>& code, StructureKernel& k, std::string& why, bool samples = false);
/* does an upload of `P` on this context compile a structure module? */
bool structure_module_wanted(const lol_gpu* ctx, const lol_program& P);

/* ---- lol_sched.hip */
struct FrameTables { const uint32_t* order; uint32_t* cost; const uint32_t* lanes; unsigned short* pixel_cost; uint32_t n_waves; };
void lpt_release(lol_gpu* ctx);
bool lpt_table_for_frame(lol_gpu* ctx, const lol_frame_camera* cam, int w, int h, int max_steps, const lol_gpu_rows* R, int n_rows,
                         int block, hipStream_t s, FrameTables* out);
int tile_order_for_frame(lol_gpu* ctx, int w, int h, int max_steps, const lol_gpu_rows* R, bool diagnostics, int* trial);
void lpt_frame_queued(lol_gpu* ctx, hipStream_t s);

#pragma GCC visibility pop
