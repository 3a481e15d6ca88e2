/*
 * spec_source — what the scene compiler WRITES for a scene, without compiling it: the scene module's source (generate_source), the
 * structure module's with and without samples (generate_structure_source) and the interpreter's macro-op lists (build_interp_lists),
 * straight from lol_codegen.hip.  Host only, no GPU, no hipRTC run: a quarter of a second per scene.  tools/source_identity.py builds
 * it against two trees and compares what they print; the functions it calls have kept their signatures for that.
 *
 *     hipcc -std=c++17 -O1 -Iinclude -Iloltracer_amd/csrc -c -o spec_source.o tools/spec_source.cpp
 *     hipcc -o spec_source spec_source.o loltracer_amd/lib/obj/[a-z]*.o -Lloltracer_amd/lib -llol_scene -lhiprtc -ldl \
 *           -Wl,-rpath,$PWD/loltracer_amd/lib
 *     spec_source [options] scene.lol ...        one line per text: <file> <what> <sha256> <bytes>
 *
 * (Two commands: handed the .cpp and the objects at once, hipcc reads the objects as HIP source.  The internal header pulls in the
 * kernel headers, so it is hipcc and not a plain host compiler.)  Options — the fast paths default to none proven:
 *     --assume-fast K    every shortcut proven, as lol_gpu_compile_offline_module assumes them, with sqrt_kind K (1, 2 or 3)
 *     --no-tiny          ... but sqrt_tiny_ok off          --no-nf      ... but no k proven without v_div_fixup (div_nf_ok empty)
 *     --no-shade         ... but shade_root 0
 *     --cull 0|1         culling (default 1)               --form 0|1|2 by size, out of line, inlined (default 0)
 *     --switches MASK    the module switches (default 0)
 *     --text WHAT        print that text itself (source, structure, structure_samples) or the lists as hex words (lists)
 *     --selftest         the writer of lol_codegen.hip on a line far beyond any fixed buffer; built with the sanitizers, this is
 *                        what shows a write out of bounds
 * The LOL_GPU_* tuning switches are read from the environment as the library reads them.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lol_gpu_internal.h"

std::string generate_source(const lol_program& P, const FastPaths* fast, bool cull, int form, ModuleKernels carries);
std::string generate_structure_source(const lol_program& P, bool samples);
/* (only a tree that has the writer defines it: elsewhere --selftest says so) */
void appendf(std::string& s, const char* fmt, ...) __attribute__((weak, format(printf, 2, 3)));

/* ---------------------------------------------------------------- SHA-256 (FIPS 180-4) */
static std::string sha256(const void* data, size_t n) {
	static const uint32_t K[64] = {
		0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
		0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
		0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
		0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
		0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
		0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2 };
	uint32_t h[8] = { 0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19 };
	std::vector<unsigned char> m(static_cast<const unsigned char*>(data), static_cast<const unsigned char*>(data) + n);
	m.push_back(0x80);
	while (m.size() % 64 != 56) m.push_back(0);
	for (int i = 7; i >= 0; i--) m.push_back((unsigned char)(((unsigned long long)n * 8) >> (8 * i)));
	auto rotr = [](uint32_t x, int r) { return (x >> r) | (x << (32 - r)); };
	for (size_t at = 0; at < m.size(); at += 64) {
		uint32_t w[64];
		for (int i = 0; i < 16; i++) w[i] = (uint32_t)m[at + 4 * i] << 24 | (uint32_t)m[at + 4 * i + 1] << 16 | (uint32_t)m[at + 4 * i + 2] << 8 | m[at + 4 * i + 3];
		for (int i = 16; i < 64; i++)
			w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
		uint32_t v[8];
		memcpy(v, h, sizeof v);
		for (int i = 0; i < 64; i++) {
			const uint32_t t1 = v[7] + (rotr(v[4], 6) ^ rotr(v[4], 11) ^ rotr(v[4], 25)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) + K[i] + w[i];
			const uint32_t t2 = (rotr(v[0], 2) ^ rotr(v[0], 13) ^ rotr(v[0], 22)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
			for (int j = 7; j > 0; j--) v[j] = v[j - 1];
			v[4] += t1;
			v[0] = t1 + t2;
		}
		for (int i = 0; i < 8; i++) h[i] += v[i];
	}
	char hex[65];
	for (int i = 0; i < 8; i++) snprintf(hex + 8 * i, 9, "%08x", h[i]);
	return hex;
}

/* ---------------------------------------------------------------- --selftest */
static int selftest() {
	if (sha256("abc", 3) != "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad") { printf("FAIL: sha256\n"); return 1; }
	if (!appendf) { printf("this build of lol_codegen.hip has no appendf\n"); return 2; }
	int bad = 0;
	/* one call, 4000 and some bytes: a literal's worth of text a hundred times over, numbers between */
	const std::string piece(37, 'x');
	std::string all, got = "head ";
	for (int i = 0; i < 100; i++) all += piece + " " + std::to_string(1000 + i) + ";";
	appendf(got, "%s", all.c_str());
	if (got != "head " + all || got.size() < 4000) { printf("FAIL: one long argument\n"); bad++; }
	/* ... and many arguments in one literal: 22 integers and 7 strings, like the longest site of the emitter, each string 300 bytes */
	const std::string lit(300, 'L');
	const char* l = lit.c_str();
	std::string many;
	appendf(many, "%d%d%d%s%d%d%d%s%d%d%d%s%d%d%d%s%d%d%d%s%d%d%d%s%d%d%d%d%s|%u|%08x", 1, 2, 3, l, 4, 5, 6, l, 7, 8, 9, l, 10, 11, 12, l, 13, 14, 15, l,
	        16, 17, 18, l, 19, 20, 21, 22, l, 4000000000u, 0xbeefu);
	const std::string many_want = "123" + lit + "456" + lit + "789" + lit + "101112" + lit + "131415" + lit + "161718" + lit + "19202122" + lit +
	                              "|4000000000|0000beef";
	if (many != many_want || many.size() < 2 * 768) { printf("FAIL: many arguments\n"); bad++; }
	/* ... appended to what stood there, byte for byte, the empty result too */
	std::string keep = "kept";
	appendf(keep, "%s", "");
	appendf(keep, "%c", '!');
	if (keep != "kept!") { printf("FAIL: appending\n"); bad++; }
	printf("selftest: %zu and %zu bytes formatted, %d failures\n", got.size(), many.size(), bad);
	return bad ? 1 : 0;
}

/* ---------------------------------------------------------------- one scene */
static bool read_file(const char* path, std::string& out) {
	FILE* f = fopen(path, "rb");
	if (!f) return false;
	char buf[65536];
	for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) out.append(buf, n);
	fclose(f);
	return true;
}

static void show(const char* file, const char* what, const std::string& text, const char* want_text) {
	if (!want_text) printf("%s %s %s %zu\n", file, what, sha256(text.data(), text.size()).c_str(), text.size());
	else if (!strcmp(want_text, what)) fputs(text.c_str(), stdout);
}

int main(int argc, char** argv) {
	int assume = 0, form = SPEC_BY_SIZE;
	bool cull = true, tiny = true, nf = true, shade = true;
	unsigned switches = 0;
	const char* want_text = nullptr;
	int at = 1;
	for (; at < argc && argv[at][0] == '-' && argv[at][1] == '-'; at++) {
		const char* o = argv[at];
		auto value = [&]() -> const char* { if (at + 1 >= argc) { fprintf(stderr, "%s needs a value\n", o); exit(2); } return argv[++at]; };
		if (!strcmp(o, "--selftest")) return selftest();
		else if (!strcmp(o, "--assume-fast")) assume = atoi(value());
		else if (!strcmp(o, "--no-tiny")) tiny = false;
		else if (!strcmp(o, "--no-nf")) nf = false;
		else if (!strcmp(o, "--no-shade")) shade = false;
		else if (!strcmp(o, "--cull")) cull = atoi(value()) != 0;
		else if (!strcmp(o, "--form")) form = atoi(value());
		else if (!strcmp(o, "--switches")) switches = (unsigned)strtoul(value(), nullptr, 0);
		else if (!strcmp(o, "--text")) want_text = value();
		else { fprintf(stderr, "unknown option %s\n", o); return 2; }
	}
	if (at >= argc || assume < 0 || assume > 3 || form < 0 || form > 2 || switches > ALL_SWITCHES) {
		fprintf(stderr, "usage: %s [--selftest] [--assume-fast 1|2|3] [--no-tiny] [--no-nf] [--no-shade] [--cull 0|1] [--form 0|1|2] [--switches MASK] "
		        "[--text source|structure|structure_samples|lists] scene.lol ...\n", argv[0]);
		return 2;
	}
	for (; at < argc; at++) {
		const char* file = argv[at];
		std::string text;
		if (!read_file(file, text)) { perror(file); return 2; }
		lol_scene* scene = nullptr;
		char err[256] = "";
		if (lol_scene_parse_string(text.data(), text.size(), &scene, err, sizeof err) != 0) { fprintf(stderr, "%s: %s\n", file, err); return 2; }
		lol_program P;
		memset(&P, 0, sizeof P);
		const int st = lol_scene_flatten(scene, &P);
		lol_scene_free(scene);
		if (st != 0) { fprintf(stderr, "%s: lol_scene_flatten: %d\n", file, st); return 2; }
		FastPaths fast;
		if (assume) {
			fast.sqrt_kind = assume;
			fast.sqrt_tiny_ok = tiny;
			if (shade) { fast.shade_root = fast.sqrt_kind; fast.shade_rcp = 1; }
			for (uint32_t i = 0; i < P.n_ops; i++)
				if ((P.ops[i].op == LOL_OP_SMIN || P.ops[i].op == LOL_OP_SMIN_R) && !fast.has(P.ops[i].f[0])) {
					fast.div_ok.push_back(P.ops[i].f[0]);
					if (nf) fast.div_nf_ok.push_back(P.ops[i].f[0]);
				}
		}
		show(file, "source", generate_source(P, &fast, cull, form, ModuleKernels{ switches }), want_text);
		show(file, "structure", generate_structure_source(P, false), want_text);
		show(file, "structure_samples", generate_structure_source(P, true), want_text);
		std::vector<uint32_t> lists;
		uint32_t n_mops = 0;
		if (!build_interp_lists(P, fast, cull, lists, n_mops)) { fprintf(stderr, "%s: the two lists differ in length\n", file); return 1; }
		if (!want_text) printf("%s lists %s %u\n", file, sha256(lists.data(), lists.size() * 4).c_str(), n_mops);
		else if (!strcmp(want_text, "lists"))
			for (size_t i = 0; i < lists.size(); i++) printf("%08x%c", lists[i], (i + 1) % lol::MOP_DWORDS ? ' ' : '\n');
		lol_program_free(&P);
	}
	return 0;
}
