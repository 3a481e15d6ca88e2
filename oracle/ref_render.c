/*
 * ref_render.c — what the REAL naive_renderer.c needs round it to render one frame.  TEST INFRASTRUCTURE ONLY.
 *
 * Compiled only where the reference tree exists (oracle/Makefile target `ref`), beside ref_harness.c, together with the
 * reference's own naive_renderer.c — unmodified, where it lies — against oracle/sdl_standin/SDL.h.  Everything here is ours:
 * the four globals of renderer.h, the five SDL functions the file calls, and two entry points for tests/golden/make_golden.py
 * and tests/test_reference_renderer.py.  render_thread() runs on the calling thread: one line counter, one "worker".
 */
#include <stddef.h>

#include "renderer.h"   /* reference: the globals' declarations, struct render_data, render_thread (and our stand-in <SDL.h>) */

struct SDL_semaphore { int waits; };

static SDL_sem entry_sem, exit_sem;

SDL_atomic_t exiting;
SDL_atomic_t current_line;
SDL_sem*     frame_entry_barrier = &entry_sem;
SDL_sem*     frame_exit_barrier = &exit_sem;

/* SDL_MapRGB for a non-palettised format, as SDL2 documents it (and include/lol_gpu.h restates it):
 * (r >> Rloss) << Rshift | (g >> Gloss) << Gshift | (b >> Bloss) << Bshift | Amask */
Uint32 SDL_MapRGB(const SDL_PixelFormat* f, Uint8 r, Uint8 g, Uint8 b) {
	return (Uint32)(r >> f->Rloss) << f->Rshift | (Uint32)(g >> f->Gloss) << f->Gshift | (Uint32)(b >> f->Bloss) << f->Bshift | f->Amask;
}

/* single-threaded: plain ints.  SDL_AtomicAdd returns the PREVIOUS value. */
int SDL_AtomicGet(SDL_atomic_t* a) { return a->value; }
int SDL_AtomicAdd(SDL_atomic_t* a, int v) { int old = a->value; a->value += v; return old; }

/* render_thread waits on the entry barrier before every frame: the first wait lets it through, the second one (after the frame)
 * raises `exiting`, which is what makes it return.  The exit barrier is only posted. */
int SDL_SemWait(SDL_sem* s) {
	if (s == frame_entry_barrier && s->waits++ > 0)
		exiting.value = 1;
	return 0;
}
int SDL_SemPost(SDL_sem* s) { return 0; }

/* One frame of render_thread into `pixels` (XRGB8888, `pitch` bytes per row). */
void ref_render_frame(struct scene* scene, int w, int h, void* pixels, int pitch) {
	SDL_PixelFormat fmt = { .BytesPerPixel = 4, .Rloss = 0, .Gloss = 0, .Bloss = 0, .Rshift = 16, .Gshift = 8, .Bshift = 0, .Amask = 0 };
	SDL_Surface surf = { .format = &fmt, .w = w, .h = h, .pitch = pitch, .pixels = pixels };
	struct render_data data = { .surf = &surf, .scene = scene, .private = NULL };
	exiting.value = 0;
	current_line.value = 0;
	entry_sem.waits = 0;
	render_thread(&data);
}

/* point[3], direction[3], fov: the camera is data of the struct scene */
void ref_scene_set_camera(struct scene* scene, const float cam[7]) {
	scene->camera.point = (v3){ cam[0], cam[1], cam[2] };
	scene->camera.direction = (v3){ cam[3], cam[4], cam[5] };
	scene->camera.fov = cam[6];
}
