/*
 * lol_code_key.h — what names a compiled kernel: FNV-1a over the parts of a code object that the device loads and runs.
 *
 * A code object is an ELF64 little-endian file.  The device gets its allocated sections of type PROGBITS or NOTE: for a scene
 * module .note (the kernels' metadata), .rodata (the kernel descriptors) and .text.  The rest of the file — symbol and string
 * tables, their hash tables, .comment — also holds hipRTC's compilation-unit id, a symbol __hip_cuid_<16 hex digits> that follows
 * the text of every header the compiler was handed, so the whole file differs between two builds whose instructions do not.
 * The key is over the former: each such section's size, then its bytes, in section-header order.
 *
 * Plain C++ with no HIP header: a host program can include this file alone.
 */
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace lol_key {

constexpr unsigned long long FNV_BASIS = 0xcbf29ce484222325ull, FNV_PRIME = 0x100000001b3ull;

inline unsigned long long fnv64(const void* data, size_t n, unsigned long long h = FNV_BASIS) {
	for (size_t i = 0; i < n; i++) { h ^= static_cast<const unsigned char*>(data)[i]; h *= FNV_PRIME; }
	return h;
}

/* The key of the code object in code[0 .. n).  Every offset and size is checked against n before anything is read there; a buffer
 * that is no ELF64 little-endian file, or one of whose headers points outside it, gets the FNV-1a of the whole buffer. */
inline unsigned long long code_key(const void* code, size_t n) {
	constexpr size_t EHDR = 64, SHDR = 64;                               /* sizeof(Elf64_Ehdr), sizeof(Elf64_Shdr) */
	constexpr uint32_t SHT_PROGBITS = 1, SHT_NOTE = 7;
	constexpr uint64_t SHF_ALLOC = 2;
	const unsigned char* b = static_cast<const unsigned char*>(code);
	const unsigned long long whole = fnv64(code, n);
	auto get = [&](size_t at, size_t bytes) { uint64_t v = 0; memcpy(&v, b + at, bytes); return v; };      /* (a little-endian host: gfx950's are) */
	if (n < EHDR || memcmp(b, "\177ELF", 4) != 0 || b[4] != 2 /* ELFCLASS64 */ || b[5] != 1 /* ELFDATA2LSB */) return whole;
	const uint64_t shoff = get(40, 8), shentsize = get(58, 2), shnum = get(60, 2);
	if (shentsize != SHDR || shnum == 0 || shoff > n || shnum * SHDR > n - shoff) return whole;
	unsigned long long h = FNV_BASIS;
	bool any = false;
	for (uint64_t i = 0; i < shnum; i++) {
		const size_t sh = (size_t)(shoff + i * SHDR);
		const uint64_t type = get(sh + 4, 4), flags = get(sh + 8, 8), offset = get(sh + 24, 8), size = get(sh + 32, 8);
		if (!(flags & SHF_ALLOC) || (type != SHT_PROGBITS && type != SHT_NOTE)) continue;
		if (offset > n || size > n - offset) return whole;
		h = fnv64(&size, 8, h);
		h = fnv64(b + offset, (size_t)size, h);
		any = true;
	}
	return any ? h : whole;
}

}  // namespace lol_key
