/*
 * lol_tiers.hip — the tiers of the scene compiler: interpreter -> [out-of-line kernel ->] scene kernel.
 *
 * An upload commits the program, and the interpreter renders it while hipRTC compiles the scene's own kernel on a host thread
 * (start_specialise).  At a frame boundary a finished run's kernel takes over (finish_specialise).  With its SDF inlined into
 * the three loops a scene of 257 ... 1024 ops renders 14 - 88 % faster than with the one out-of-line function
 * (profiles/r5_large_scene_ab.jsonl, r5_field_inline_ab.jsonl), and takes hipRTC 3 - 18 s instead of 0.4 - 3 s: such a scene
 * gets the out-of-line kernel first and the inlined one behind it.  Same pixels from all three.
 */
#include "lol_gpu_internal.h"

/* One run of the scene compiler on a thread of its own. */
struct SpecJob {
	std::mutex mu;
	std::condition_variable cv;
	bool done = false, ok = false;
	std::vector<char> code;
	std::string log, note;
	std::chrono::steady_clock::time_point started;
	double compile_ms = 0;
	/* what the run compiles — its own copies: the context may take another scene meanwhile */
	std::shared_ptr<OwnedProgram> prog;
	std::shared_ptr<FastPaths> fast;
	std::string arch;
	bool cull = true;
	int form = SPEC_BY_SIZE;
	ModuleKernels carries;             /* what the module holds beside the frame kernel */
	/* the structure module (lol_gpu_set_scene_views), compiled by this run's thread AFTER the scene's own module: `done` says the
	 * scene's kernel is there, `structure_done` that this one is (or was not to be had: structure_ok) */
	bool want_structure = false, structure_done = false, structure_ok = false;
	bool structure_samples = false;    /* lol_gpu_set_scene_view_samples: the structure module with its two supersampled kernels */
	std::vector<char> structure_code;
	std::string structure_log;
	bool all_done() const { return done && (!want_structure || structure_done); }      /* (under `mu`) */
	BigStackThread th;
	/* A run is never left behind: hipRTC cannot be interrupted, and a thread still inside it when the process exits crashes in the
	 * compiler's own teardown (comgr is loaded on first use, so its statics go BEFORE this library's: with a process-lifetime
	 * reaper the C host segfaulted at exit).  What bounds the wait instead is LOL_SPEC_MAX_OPS. */
	~SpecJob() { th.join(); }
};

SpecTiers::SpecTiers() = default;
SpecTiers::~SpecTiers() {
	job.reset();
	structure_job.reset();
	structure.unload();
	old_jobs.clear();
	kernel.unload();
	retired.unload();
}

namespace {

/* the runs of programs since replaced that have finished */
void reap(std::vector<std::unique_ptr<SpecJob>>& jobs) {
	jobs.erase(std::remove_if(jobs.begin(), jobs.end(), [](const std::unique_ptr<SpecJob>& j) {
		std::lock_guard<std::mutex> lock(j->mu);
		return j->all_done();
	}), jobs.end());
}

/* start the run on its own (large-stack) thread; without a thread to be had, or with LOL_GPU_ASYNC_COMPILE=0, it runs / is waited
 * for here */
void launch_job(SpecJob* job) {
	job->started = std::chrono::steady_clock::now();
	auto work = [job]() {
		bool ok = false;
		std::vector<char> code;
		std::string log;
		try {
			std::lock_guard<std::mutex> rtc(g_rtc_mutex);
			ok = compile_spec(job->prog->p, job->fast.get(), job->arch, code, log, nullptr, job->cull, job->form, job->carries);
		} catch (...) { ok = false; log = "the scene compiler ran out of memory"; }
		{
			std::lock_guard<std::mutex> lock(job->mu);
			job->compile_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - job->started).count();
			job->code = std::move(code);
			job->log = std::move(log);
			job->ok = ok;
			job->done = true;
			job->cv.notify_all();
		}
		if (!job->want_structure) return;
		bool sok = false;
		std::vector<char> scode;
		std::string slog;
		try {
			std::lock_guard<std::mutex> rtc(g_rtc_mutex);
			sok = compile_structure(job->prog->p, job->arch, scode, slog, nullptr, job->structure_samples);
		} catch (...) { sok = false; slog = "the scene compiler ran out of memory"; }
		std::lock_guard<std::mutex> lock(job->mu);
		job->structure_code = std::move(scode);
		job->structure_log = std::move(slog);
		job->structure_ok = sok;
		job->structure_done = true;
		job->cv.notify_all();
	};
	const char* async = tuning_env("LOL_GPU_ASYNC_COMPILE");
	bool threaded = !(async && async[0] == '0');
	bool started = false;
	try { started = job->th.start(work); } catch (...) { started = false; }
	if (!started) work();                                  /* no thread to be had: compile here */
	else if (!threaded) job->th.join();
}

/* All or nothing: the module with every kernel generate_source emits for a program of n_ops ops and those switches, or `why` not.
 * A failed call leaves its error behind as the thread's last error, which the host's next HIP call would trip over: cleared. */
bool load_scene_kernel(const std::vector<char>& code, uint32_t n_ops, ModuleKernels carries, SceneKernel& k, std::string& why) {
	auto get = [&](hipFunction_t& fn, const char* name) {
		if (hipModuleGetFunction(&fn, k.module, name) == hipSuccess) return true;
		why = std::string(name) + " not found in the compiled module";
		return false;
	};
	const bool two = n_ops <= LOL_SPEC_TWO_KERNELS_MAX_OPS;
	k.key = code_key_hex(code.data(), code.size());
	bool ok = hipModuleLoadData(&k.module, code.data()) == hipSuccess;
	if (!ok) why = "hipModuleLoadData failed";
	ok = ok && get(k.sdf, "lol_sdf_spec");
	if (ok && carries.carries(SWITCH_RAYS)) ok = get(k.trace, "lol_trace_spec");
	if (ok && carries.carries(SWITCH_SHADE)) ok = get(k.shade, "lol_shade_spec");
	for (int f = 0; ok && f < N_FAMILIES; f++) {
		const FamilyRow& row = KERNEL_FAMILIES[f];
		if (!carries.carries(row.needs)) continue;
		ok = get(k.fn[f], row.symbol);
		if (ok && two && row.counting) ok = get(k.counting[f], row.counting);
		else k.counting[f] = k.fn[f];                  /* (no twin in the module: the kernel itself counts, or nobody asks it to) */
	}
	if (ok) return true;
	k.unload();
	(void)hipGetLastError();
	return false;
}

/* what a finished run leaves the frames: its kernel, loaded, or why there is none */
struct Outcome { SceneKernel kernel; std::string why; };

Outcome outcome_of(SpecTiers& T, const SpecJob& job) {
	Outcome o;
	if (T.tier == SpecTiers::FIRST && T.second_wanted && T.fail_first > 0) {      /* lol_gpu_testing_fail_first_tier */
		T.fail_first--;
		o.why = "injected failure of the first run (lol_gpu_testing_fail_first_tier)";
	} else if (!job.ok) o.why = job.log;
	else load_scene_kernel(job.code, job.prog->p.n_ops, job.carries, o.kernel, o.why);
	return o;
}

/* the scene's second run (the form with the SDF inlined) behind the first: same program and proofs */
bool start_second_tier(SpecTiers& T, const SpecJob& first) {
	T.second_wanted = false;
	std::unique_ptr<SpecJob> next;
	try {
		next = std::make_unique<SpecJob>();
		next->prog = first.prog; next->fast = first.fast; next->arch = first.arch; next->cull = first.cull; next->carries = first.carries;
		next->form = SPEC_INLINE;
	} catch (...) { return false; }
	T.job = std::move(next);
	launch_job(T.job.get());
	return true;
}

/* A finished run's outcome takes effect: its kernel takes over, with the inlined form compiled behind a first tier.  A failure is
 * reported once on stderr; frames still render, through the interpreter or through the first tier's kernel, which stays.  A
 * first run that fails where a second was to follow (the out-of-line form: the one the long-branch trip-wire and the
 * dropped-options refusal of compile_spec are about) does not cost the scene its kernel: the inlined form, which has no
 * out-of-line function to trip them, is compiled all the same while the interpreter renders. */
void apply(lol_gpu* ctx, const SpecJob& job, const Outcome& o) {
	SpecTiers& T = ctx->tiers;
	const bool second = T.tier == SpecTiers::SECOND;
	T.compile_ms = job.compile_ms;
	if (o.kernel) {
		T.retired.unload();                             /* (empty: one second tier per upload) */
		T.retired = T.kernel;
		T.kernel = o.kernel;
		T.log = (second ? T.log + "second tier (SDF inlined): " : job.note) + job.log + (job.log.empty() || job.log.back() == '\n' ? "" : "\n");
		ctx->kernel_epoch++;
		T.tier = T.second_wanted && start_second_tier(T, job) ? SpecTiers::SECOND : SpecTiers::SETTLED;
	} else if (second && T.kernel) {
		T.log += "(the inlined form of the kernel was not to be had: " + o.why + "; the out-of-line form stays)\n";
		T.tier = SpecTiers::SETTLED;
	} else if (T.second_wanted && start_second_tier(T, job)) {
		T.log = "(the out-of-line form of the kernel was not to be had: " + o.why + "; compiling the inlined form)\n";
		T.tier = SpecTiers::SECOND;                     /* (reported as 5 / 6, although the interpreter renders meanwhile) */
	} else {
		T.log = second ? T.log + "(nor was the inlined form: " + o.why + ")\n" : o.why;
		T.tier = SpecTiers::FAILED;
		fprintf(stderr, "lol_gpu: scene specialisation failed, using the interpreter kernel: %s\n", T.log.c_str());
	}
}

/* the current tier's run once it has finished (with `wait`: waited for); nullptr while there is none or it still compiles */
std::unique_ptr<SpecJob> take_finished(SpecTiers& T, bool wait) {
	if (!T.job) return nullptr;
	SpecJob& job = *T.job;
	{
		std::unique_lock<std::mutex> lock(job.mu);
		if (!job.done && !wait) return nullptr;
		job.cv.wait(lock, [&] { return job.done; });
	}
	return std::move(T.job);
}

/* the run whose structure module is awaited, once that is there (with `wait`: waited for): its outcome takes effect */
bool finish_structure(SpecTiers& T, bool wait) {
	if (!T.structure_job) return false;
	SpecJob& job = *T.structure_job;
	{
		std::unique_lock<std::mutex> lock(job.mu);
		if (!job.structure_done && !wait) return false;
		job.cv.wait(lock, [&] { return job.structure_done; });
	}
	std::string why = job.structure_log;
	if (job.structure_ok && load_structure_kernel(job.structure_code, T.structure, why, job.structure_samples)) {
		T.structure_state = 2;
		T.structure_log = job.structure_log;
	} else {
		T.structure_state = -1;
		T.structure_log = why;
		fprintf(stderr, "lol_gpu: the structure module was not to be had, scene views render on the interpreter: %s\n", why.c_str());
	}
	T.structure_job.reset();
	return true;
}

}  // namespace

bool load_structure_kernel(const std::vector<char>& code, StructureKernel& k, std::string& why, bool samples) {
	k.key = code_key_hex(code.data(), code.size());
	bool ok = hipModuleLoadData(&k.module, code.data()) == hipSuccess;
	if (!ok) why = "hipModuleLoadData failed";
	if (ok && hipModuleGetFunction(&k.batch, k.module, "lol_render_param_batch") != hipSuccess) { ok = false; why = "lol_render_param_batch not found in the compiled module"; }
	if (ok && hipModuleGetFunction(&k.lin, k.module, "lol_render_param_batch_lin") != hipSuccess) { ok = false; why = "lol_render_param_batch_lin not found in the compiled module"; }
	if (ok && samples && hipModuleGetFunction(&k.batch_aa, k.module, "lol_render_param_batch_aa") != hipSuccess) { ok = false; why = "lol_render_param_batch_aa not found in the compiled module"; }
	if (ok && samples && hipModuleGetFunction(&k.aa_lin, k.module, "lol_render_param_batch_aa_lin") != hipSuccess) { ok = false; why = "lol_render_param_batch_aa_lin not found in the compiled module"; }
	if (ok) return true;
	k.unload();
	(void)hipGetLastError();
	return false;
}

bool structure_module_wanted(const lol_gpu* ctx, const lol_program& P) {
	return (ctx->want_scene_views || ctx->want_scene_view_samples) && P.n_ops <= LOL_SPEC_FIRST_TIER_INLINE_MAX_OPS;
}

void start_specialise(lol_gpu* ctx, const FastPaths& fast) {
	SpecTiers& T = ctx->tiers;
	T.kernel.unload();
	T.retired.unload();
	T.structure.unload();
	T.structure_state = 0;
	T.structure_log.clear();
	ctx->kernel_epoch++;                                /* the interpreter renders the new scene until its kernel is there */
	T.log.clear();
	T.tier = SpecTiers::OFF;
	T.second_wanted = false;
	if (std::unique_ptr<SpecJob> prev = std::move(T.job)) T.old_jobs.push_back(std::move(prev));      /* its result is not wanted any more */
	if (std::unique_ptr<SpecJob> prev = std::move(T.structure_job)) T.old_jobs.push_back(std::move(prev));
	reap(T.old_jobs);
	const char* env = tuning_env("LOL_GPU_SPECIALIZE");
	if (!T.want || (env && env[0] == '0')) return;
	/* every program up to LOL_SPEC_MAX_OPS is specialised, large ones with their SDF out of line (emit_sdf).  Beyond that the
	 * straight-line source (two SDF bodies of ~150 bytes per op) takes hipRTC minutes, and programs no longer have a
	 * capacity (lol_scene.h): such a scene renders on the interpreter, which reads it as data.  Not a failure: no complaint. */
	uint32_t limit = T.max_ops ? T.max_ops : LOL_SPEC_MAX_OPS;
	if (const char* e = tuning_env("LOL_GPU_SPEC_MAX_OPS")) limit = (uint32_t)strtoul(e, nullptr, 10);
	if (ctx->h_prog.n_ops > limit) {
		char b[160];
		snprintf(b, sizeof b, "%u ops: above the %u the scene compiler takes on (lol_gpu_set_specialize_max_ops / LOL_GPU_SPEC_MAX_OPS); rendered by the interpreter", ctx->h_prog.n_ops, limit);
		T.log = b;
		return;
	}
	hipDeviceProp_t prop;
	std::string arch = "gfx950";
	if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.gcnArchName[0]) {
		std::string name = prop.gcnArchName;             /* e.g. "gfx950:sramecc+:xnack-" */
		arch = name.substr(0, name.find(':'));
	}
	std::unique_ptr<SpecJob> job;
	try {
		job = std::make_unique<SpecJob>();
		job->prog = std::make_shared<OwnedProgram>();
		job->prog->assign(ctx->h_prog);
		job->fast = std::make_shared<FastPaths>(fast);
		job->arch = arch;
		char b[160];
		snprintf(b, sizeof b, "fast paths proven on device: sqrt=%d, smin divisors=%zu (without div_fixup: %zu)\n", fast.sqrt_kind,
		         fast.div_ok.size(), fast.div_nf_ok.size());
		job->note = b;
		const std::string sw = lol_gpu_tuning_switches();
		if (!sw.empty()) job->note += "tuning switches in effect (LOL_GPU_TUNING=1): " + sw + "\n";
	} catch (...) { T.log = "out of host memory"; return; }
	job->cull = culling_enabled(ctx->want_cull);
	job->carries = module_kernels_of(ctx);
	job->want_structure = structure_module_wanted(ctx, ctx->h_prog);
	job->structure_samples = ctx->want_scene_view_samples != 0;
	if (job->want_structure) T.structure_state = 1;
	/* (LOL_GPU_SPEC_INLINE_MAX, a tuning switch, pins ONE form by size) */
	const bool first_tier = !tuning_env("LOL_GPU_SPEC_INLINE_MAX") && ctx->h_prog.n_ops > LOL_SPEC_FIRST_TIER_INLINE_MAX_OPS &&
	                        ctx->h_prog.n_ops <= LOL_SPEC_INLINE_MAX_OPS;
	T.second_wanted = first_tier && T.want_second;
	/* a mid-size scene's first kernel is the out-of-line form whether or not the inlined one follows: lol_gpu_set_specialize(ctx, 5)
	 * declines the SECOND run, it does not ask for the slow compile in place of the first */
	job->form = first_tier ? SPEC_OUT_OF_LINE : SPEC_BY_SIZE;
	try { job->note += spec_out_of_line(ctx->h_prog, job->form) ? "form: SDF out of line\n" : "form: SDF inlined\n"; } catch (...) {}
	T.job = std::move(job);
	T.tier = SpecTiers::FIRST;
	launch_job(T.job.get());
}

bool finish_specialise(lol_gpu* ctx, bool wait) {
	bool changed = false;
	std::unique_ptr<SpecJob> job;
	while ((wait || !changed) && (job = take_finished(ctx->tiers, wait))) {
		apply(ctx, *job, outcome_of(ctx->tiers, *job));
		changed = true;
		if (job->want_structure) ctx->tiers.structure_job = std::move(job);      /* its thread is still at work on the structure module */
	}
	if (finish_structure(ctx->tiers, wait)) changed = true;
	return changed;
}

extern "C" {

int lol_gpu_set_specialize(lol_gpu* ctx, int enable) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	/* 0 interpreter, plain | 1 specialised + proven fast paths (default) | 3 specialised, plain | 4 interpreter + fast paths |
	 * 5 = 1 without the second tier of a mid-size scene (the out-of-line kernel stays: nothing compiles behind it) */
	if (enable < 0 || enable == 2 || enable > 5) return LOL_GPU_ERR_ARG;
	ctx->tiers.want = enable == 1 || enable == 3 || enable == 5;
	ctx->want_fast = (enable == 1 || enable == 4 || enable == 5) ? 1 : 0;
	ctx->tiers.want_second = enable != 5;
	return LOL_GPU_OK;
}

int lol_gpu_set_specialize_max_ops(lol_gpu* ctx, unsigned max_ops) {
	if (!ctx || max_ops > LOL_MAX_OPS) return LOL_GPU_ERR_ARG;
	ctx->tiers.max_ops = max_ops;            /* takes effect at the next lol_gpu_upload_program */
	return LOL_GPU_OK;
}

const char* lol_gpu_specialize_log(const lol_gpu* ctx) { return ctx ? ctx->tiers.log.c_str() : ""; }

int lol_gpu_specialize_wait(lol_gpu* ctx) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	LOL_HIP(ctx, hipSetDevice(ctx->device));
	finish_specialise(ctx, true);
	return LOL_GPU_OK;
}

int lol_gpu_specialize_state(lol_gpu* ctx, double* compile_ms) {
	if (!ctx) return LOL_GPU_ERR_ARG;
	const SpecTiers& T = ctx->tiers;
	bool done = false;
	double ms = T.compile_ms;                          /* the last finished run's */
	if (T.job) {                                       /* has the compiler finished?  (the swap itself happens at a frame or a wait) */
		std::lock_guard<std::mutex> lock(T.job->mu);
		done = T.job->done;
		ms = done ? T.job->compile_ms : T.tier == SpecTiers::SECOND ? T.compile_ms : 0.0;
	}
	if (compile_ms) *compile_ms = ms;
	switch (T.tier) {
	case SpecTiers::FIRST:   return done ? 3 : 1;
	case SpecTiers::SECOND:  return done ? 6 : 5;
	case SpecTiers::SETTLED: return 2;
	case SpecTiers::FAILED:  return -1;
	default:                 return 0;
	}
}

int lol_gpu_testing_fail_first_tier(lol_gpu* ctx, int n) {
	if (!ctx || n < 0) return LOL_GPU_ERR_ARG;
	ctx->tiers.fail_first = n;
	return LOL_GPU_OK;
}

}  // extern "C"
