/*
 * SDL.h — a stand-in, NOT SDL.  TEST INFRASTRUCTURE ONLY.
 *
 * Written from SDL2's public documentation (wiki.libsdl.org: SDL_PixelFormat, SDL_Surface, SDL_MapRGB, SDL_SemWait, SDL_SemPost,
 * SDL_AtomicGet, SDL_AtomicAdd).  It declares exactly the names the reference's naive_renderer.c and renderer.h use and nothing
 * else, so that the unmodified file compiles where SDL2 is not installed (oracle/Makefile, target `ref`).  The five functions are
 * defined in oracle/ref_render.c.
 */
#ifndef LOL_SDL_STANDIN_H
#define LOL_SDL_STANDIN_H

typedef unsigned char Uint8;
typedef unsigned int  Uint32;

typedef struct { int value; } SDL_atomic_t;
typedef struct SDL_semaphore SDL_sem;

typedef struct SDL_PixelFormat {
	Uint8  BytesPerPixel;
	Uint8  Rloss, Gloss, Bloss;
	Uint8  Rshift, Gshift, Bshift;
	Uint32 Amask;
} SDL_PixelFormat;

typedef struct SDL_Surface {
	SDL_PixelFormat *format;
	int   w, h;
	int   pitch;
	void *pixels;
} SDL_Surface;

int    SDL_SemWait(SDL_sem *sem);
int    SDL_SemPost(SDL_sem *sem);
int    SDL_AtomicGet(SDL_atomic_t *a);
int    SDL_AtomicAdd(SDL_atomic_t *a, int v);
Uint32 SDL_MapRGB(const SDL_PixelFormat *format, Uint8 r, Uint8 g, Uint8 b);

#endif
