/*
 * code_key_check — lol_key::code_key (loltracer_amd/csrc/lol_code_key.h) on buffers that are not sound code objects.  Host only;
 * meant to be built with the sanitizers, which is what catches a read out of bounds:
 *
 *     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iloltracer_amd/csrc \
 *         -o tools/code_key_check tools/code_key_check.cpp  &&  tools/code_key_check some_module.co
 *
 * Every buffer is copied into a heap block of exactly its size, so one byte beyond it is an error.  Checks: the sound file's key is
 * not the whole-file hash; every truncation of the file, and the file with each ELF header field and each field of each section
 * header set to a few hostile values, gives either a key or the whole-file hash and never a fault; the cases
 * tests/test_rays_cabi.py names (10, 63, 64 bytes, e_shoff beyond the end) give the whole-file hash.
 */
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "lol_code_key.h"

static unsigned long long key_of(const std::vector<unsigned char>& v) {
	std::unique_ptr<unsigned char[]> exact(new unsigned char[v.size()]);      /* (size 0: a valid pointer to nothing) */
	if (!v.empty()) memcpy(exact.get(), v.data(), v.size());
	return lol_key::code_key(exact.get(), v.size());
}

int main(int argc, char** argv) {
	if (argc != 2) { fprintf(stderr, "usage: %s module.co\n", argv[0]); return 2; }
	FILE* f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	std::vector<unsigned char> co;
	for (int c; (c = fgetc(f)) != EOF;) co.push_back((unsigned char)c);
	fclose(f);
	int bad = 0;
	auto expect_whole = [&](const std::vector<unsigned char>& v, const char* what) {
		if (key_of(v) != lol_key::fnv64(v.data(), v.size())) { printf("FAIL: %s is not keyed by the whole buffer\n", what); bad++; }
	};
	if (co.size() < 128 || key_of(co) == lol_key::fnv64(co.data(), co.size())) { printf("FAIL: %s is not keyed as a code object\n", argv[1]); bad++; }
	for (size_t n : { (size_t)0, (size_t)10, (size_t)63, (size_t)64 }) expect_whole(std::vector<unsigned char>(co.begin(), co.begin() + n), "a truncated file");
	{
		std::vector<unsigned char> v = co;
		const uint64_t past = co.size() + 1;
		memcpy(&v[40], &past, 8);
		expect_whole(v, "a file whose e_shoff lies beyond its end");
	}
	size_t runs = 0;
	for (size_t n = 0; n <= co.size(); n += n < 4096 ? 1 : 509) { (void)key_of(std::vector<unsigned char>(co.begin(), co.begin() + n)); runs++; }
	uint64_t shoff;
	uint16_t shnum;
	memcpy(&shoff, &co[40], 8);
	memcpy(&shnum, &co[60], 2);
	const uint64_t hostile[] = { 0, 1, 63, 64, co.size() - 1, co.size(), co.size() + 1, 1ull << 31, 1ull << 32, 1ull << 62, ~0ull, ~0ull - 63, 0x8000000000000000ull };
	for (uint64_t h : hostile) {
		for (size_t at : { (size_t)40, (size_t)58, (size_t)60, (size_t)62 }) {                     /* e_shoff, e_shentsize, e_shnum, e_shstrndx */
			std::vector<unsigned char> v = co;
			memcpy(&v[at], &h, at == 40 ? 8 : 2);
			(void)key_of(v); runs++;
		}
		for (uint16_t i = 0; i < shnum; i++)
			for (size_t field : { (size_t)4, (size_t)8, (size_t)24, (size_t)32 }) {                    /* sh_type, sh_flags, sh_offset, sh_size */
				std::vector<unsigned char> v = co;
				memcpy(&v[shoff + 64ull * i + field], &h, field == 4 ? 4 : 8);
				(void)key_of(v); runs++;
			}
	}
	printf("%zu malformed buffers keyed, %d failures\n", runs, bad);
	return bad ? 1 : 0;
}
