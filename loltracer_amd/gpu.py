"""ctypes mirror of include/lol_gpu.h — the gfx950 renderer behind the renderer.h boundary.

`Renderer` plays the role of the reference's renderer plug-in
(render_prepare / render_thread / render_destroy, renderer.h:24-26):
    r = Renderer(device=0); r.prepare(scene)        # render_prepare
    r.render_into(dev_ptr, w, h, max_steps=256)     # one frame of render_thread
    r.close()                                       # render_destroy
All rendering happens in liblol_gpu.so (HIP).  There is no CPU path: if the
library or a device is missing this raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import scene as S

LOL_GPU_OK = 0
LOL_GPU_ABI_VERSION = 6          # include/lol_gpu.h
_STATUS = {0: "ok", -1: "no HIP device", -2: "HIP runtime error", -3: "bad argument",
           -4: "no scene program uploaded", -5: "unsupported"}


class Rows(C.Structure):
    """lol_gpu_rows: the rows one launch renders — `band_rows` rows at `offset_rows` of every `cycle_rows` (multi-GPU
    row tiles; include/lol_gpu.h)."""
    _fields_ = [("band_rows", C.c_int32), ("cycle_rows", C.c_int32), ("offset_rows", C.c_int32)]

    @classmethod
    def equal(cls, band_rows: int, n_parts: int, part: int) -> "Rows":
        """Part `part` of n_parts equal parts with bands of band_rows rows."""
        return cls(band_rows, band_rows * n_parts, band_rows * part)


class PixelFormat(C.Structure):
    """lol_gpu_pixel_format: the SDL_PixelFormat fields SDL_MapRGB reads (renderer.h:17-22)."""
    _fields_ = [("r_shift", C.c_uint8), ("g_shift", C.c_uint8), ("b_shift", C.c_uint8),
                ("r_loss", C.c_uint8), ("g_loss", C.c_uint8), ("b_loss", C.c_uint8),
                ("bytes_per_pixel", C.c_uint8), ("palettised", C.c_uint8), ("a_mask", C.c_uint32)]


# SDL's names for the packed 32-bit formats (SDL_pixels.h) + two the renderer must refuse
PIXEL_FORMATS = {
    "xrgb8888": PixelFormat(16, 8, 0, 0, 0, 0, 4, 0, 0x00000000),
    "argb8888": PixelFormat(16, 8, 0, 0, 0, 0, 4, 0, 0xFF000000),
    "bgrx8888": PixelFormat(8, 16, 24, 0, 0, 0, 4, 0, 0x00000000),
    "rgba8888": PixelFormat(24, 16, 8, 0, 0, 0, 4, 0, 0x000000FF),
    "abgr8888": PixelFormat(0, 8, 16, 0, 0, 0, 4, 0, 0xFF000000),
    "rgb565": PixelFormat(11, 5, 0, 3, 2, 3, 2, 0, 0),
    "index8": PixelFormat(0, 0, 0, 8, 8, 8, 1, 1, 0),
}


class TileOrderInfo(C.Structure):
    """lol_gpu_tile_order_info: what lol_gpu_set_tile_order(AUTO) measured and took."""
    _fields_ = [("mode", C.c_int32), ("order", C.c_int32), ("deciding", C.c_int32), ("decisions", C.c_int32),
                ("rows_ms", C.c_float), ("cols_ms", C.c_float)]


TILES_ROWS, TILES_COLS, TILES_AUTO, TILES_LPT = 0, 1, 2, 3
TILE_TRIALS = 16                     # LOL_GPU_TILE_TRIALS: trial frames per order (after 6 untimed ones)
TILE_TRIAL_FRAMES = 6 + 2 * TILE_TRIALS


def _tile_order_arg(order) -> int:
    if isinstance(order, str):
        return {"rows": TILES_ROWS, "cols": TILES_COLS, "columns": TILES_COLS, "auto": TILES_AUTO, "lpt": TILES_LPT}[order]
    return int(order)                # False / True = rows / columns (the round-3 meaning of the argument), 2 = auto


class Debug(C.Structure):
    _fields_ = [("rgb", C.c_void_p), ("hit_dist", C.c_void_p), ("hit_id", C.c_void_p), ("steps", C.c_void_p)]


class Hits(C.Structure):             # lol_gpu_hits: device pointers, each may be NULL (not all four)
    _fields_ = [("dist", C.c_void_p), ("id", C.c_void_p), ("steps", C.c_void_p), ("normal", C.c_void_p)]


class Shades(C.Structure):           # lol_gpu_shades: device pointers, each may be NULL (not all six)
    _fields_ = [("rgb_linear", C.c_void_p), ("rgb", C.c_void_p), ("pixel", C.c_void_p), ("hit_dist", C.c_void_p),
                ("hit_id", C.c_void_p), ("steps", C.c_void_p)]


class LightFactor(C.Structure):      # lol_gpu_light_factor: 16 bytes
    _fields_ = [("shadow", C.c_float), ("diffuse_incidence", C.c_float), ("specular_incidence", C.c_float), ("shadow_steps", C.c_uint32)]


class LightPasses(C.Structure):      # lol_gpu_light_passes: device pointers; hit_dist and march_steps are optional
    _fields_ = [("factors", C.c_void_p), ("light_stride", C.c_size_t), ("hit_id", C.c_void_p), ("hit_dist", C.c_void_p),
                ("march_steps", C.c_void_p)]


class Relit(C.Structure):            # lol_gpu_relit: device pointers, each may be NULL (not all three)
    _fields_ = [("rgb_linear", C.c_void_p), ("rgb", C.c_void_p), ("pixel", C.c_void_p)]


class ShadeMathInfo(C.Structure):    # lol_gpu_shade_math_info (include/lol_gpu_diag.h)
    _fields_ = [("root_kind", C.c_int32), ("rcp_form", C.c_int32), ("proof_lo", C.c_uint32 * 2), ("proof_hi", C.c_uint32 * 2),
                ("proof_mismatches", C.c_uint64 * 2)]


class Hit(C.Structure):              # lol_gpu_hit
    _fields_ = [("dist", C.c_float), ("id", C.c_uint32), ("steps", C.c_uint32), ("normal", C.c_float * 3)]


STREAM_DEFAULT = 1        # LOL_GPU_STREAM_DEFAULT: HIP's legacy default stream (hipStreamLegacy)


def _stream_arg(stream):
    """None → NULL (the context's own stream).  A handle of 0 is how HIP (and torch.cuda.current_stream()
    .cuda_stream for the default stream) spells the legacy default stream: pass it on as such, never as NULL."""
    if stream is None:
        return None
    return C.c_void_p(STREAM_DEFAULT if stream == 0 else stream)


def _ref(obj):
    """byref(obj), or NULL for None"""
    return C.byref(obj) if obj is not None else None


class GpuError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"lol_gpu: {_STATUS.get(status, status)}: {message}")
        self.status = status


class _ScheduleInfo(C.Structure):    # lol_gpu_testing_schedule_info (include/lol_gpu_testing.h)
    _fields_ = [("n_tiles", C.c_uint32), ("frames", C.c_uint32), ("sorts", C.c_uint32), ("region_w", C.c_uint32),
                ("region_h", C.c_uint32), ("w", C.c_uint32), ("n_rows", C.c_uint32)]


# The C prototypes, one table per header: function -> (restype, argtypes), in the order the symbol lists below have always had.  A new
# entry point is declared here and nowhere else; tests/test_cabi_prototypes.py holds every entry, and the struct mirrors above, to the
# headers' text.  Lists in device memory (rays_dev, xy_dev, the buffers of the two *_batch probes) are c_void_p where the header says
# float* / uint32_t*: callers pass integer addresses.
_P, _vp, _int, _size, _str = C.POINTER, C.c_void_p, C.c_int, C.c_size_t, C.c_char_p
_prog, _cam, _u16p, _u32p = _P(S.Program), _P(S.FrameCamera), _P(C.c_ushort), _P(C.c_uint32)

_LOL_GPU_H = {                                                          # include/lol_gpu.h
    "lol_gpu_abi_version": (_int, []),
    "lol_gpu_device_count": (_int, []),
    "lol_gpu_create": (_int, [_int, _P(_vp)]),
    "lol_gpu_destroy": (None, [_vp]),
    "lol_gpu_error": (_str, [_vp]),
    "lol_gpu_upload_program": (_int, [_vp, _prog]),
    "lol_gpu_part_rows": (_int, [_int, _P(Rows)]),
    "lol_gpu_render_device": (_int, [_vp, _cam, _int, _int, _int, _P(Rows), _vp, _size, _P(Debug), _vp]),
    "lol_gpu_render_host": (_int, [_vp, _cam, _int, _int, _int, _vp, _size]),
    "lol_gpu_sync": (_int, [_vp]),
    "lol_gpu_malloc": (_int, [_vp, _size, _P(_vp)]),
    "lol_gpu_free": (_int, [_vp, _vp]),
    "lol_gpu_memcpy_d2h": (_int, [_vp, _vp, _vp, _size]),
    "lol_gpu_kernel_name": (_str, [_vp]),
    "lol_gpu_set_specialize": (_int, [_vp, _int]),
    "lol_gpu_specialize_log": (_str, [_vp]),
    "lol_gpu_specialize_wait": (_int, [_vp]),
    "lol_gpu_specialize_state": (_int, [_vp, _P(C.c_double)]),
    "lol_gpu_multi_specialize_wait": (_int, [_vp]),
    "lol_gpu_compile_offline": (_int, [_prog, _str, _str, _int, _str, _size]),
    "lol_gpu_set_miss_skip": (_int, [_vp, _int]),
    "lol_gpu_miss_skip_active": (_int, [_vp]),
    "lol_gpu_set_exact_skips": (_int, [_vp, C.c_uint]),
    "lol_gpu_device": (_int, [_vp]),
    "lol_gpu_set_cull": (_int, [_vp, _int]),
    "lol_gpu_set_tile_order": (_int, [_vp, _int]),
    "lol_gpu_tile_order": (_int, [_vp, _P(TileOrderInfo)]),
    "lol_gpu_render_host_begin": (_int, [_vp, _cam, _int, _int, _int]),
    "lol_gpu_render_host_end": (_int, [_vp, _vp, _size, _int, _int]),
    "lol_gpu_render_host_pending": (_int, [_vp]),
    # several devices (include/lol_gpu.h, "Several devices behind the same boundary")
    "lol_gpu_multi_create": (_int, [_P(_int), _int, _P(_vp)]),
    "lol_gpu_multi_destroy": (None, [_vp]),
    "lol_gpu_multi_error": (_str, [_vp]),
    "lol_gpu_multi_device_count": (_int, [_vp]),
    "lol_gpu_multi_context": (_vp, [_vp, _int]),
    "lol_gpu_multi_upload_program": (_int, [_vp, _prog]),
    "lol_gpu_choose_band_rows": (_int, [_int, _int]),
    "lol_gpu_multi_set_band_rows": (_int, [_vp, _int]),
    "lol_gpu_part_frame_row": (_int, [_int, _P(Rows), _int]),
    "lol_gpu_multi_render_device": (_int, [_vp, _cam, _int, _int, _int, _vp, _size]),
    "lol_gpu_multi_render_host": (_int, [_vp, _cam, _int, _int, _int, _vp, _size]),
    "lol_gpu_multi_sync": (_int, [_vp]),
    "lol_gpu_multi_malloc": (_int, [_vp, _size, _P(_vp)]),
    "lol_gpu_multi_free": (_int, [_vp, _vp]),
    "lol_gpu_multi_memcpy_d2h": (_int, [_vp, _vp, _vp, _size]),
    "lol_gpu_assemble_parts": (_int, [_vp, _vp, _int, _int, _int, _int, _vp, _size, _vp]),
    "lol_gpu_multi_set_parts_per_device": (_int, [_vp, _int]),
    "lol_gpu_multi_set_host_via_root": (_int, [_vp, _int]),
    "lol_gpu_set_pixel_format": (_int, [_vp, _P(PixelFormat)]),
    "lol_gpu_render_host_pending_size": (_int, [_vp, _P(_int), _P(_int)]),
    "lol_gpu_render_host_discard": (_int, [_vp]),
    "lol_gpu_kernel_key": (_str, [_vp]),
    "lol_gpu_assemble_parts_at": (_int, [_vp, _vp, _P(Rows), _u32p, _int, _int, _int, _vp, _size, _vp]),
    "lol_gpu_split_rows": (_int, [_int, _int, _int, _int, _P(Rows)]),
    "lol_gpu_multi_set_root_band_rows": (_int, [_vp, _int]),
    "lol_gpu_multi_set_pixel_format": (_int, [_vp, _P(PixelFormat)]),
    "lol_gpu_multi_set_tile_order": (_int, [_vp, _int]),
    "lol_gpu_set_frames_in_flight": (_int, [_vp, _int]),
    "lol_gpu_frames_in_flight": (_int, [_vp]),
    "lol_gpu_next_stream": (_vp, [_vp]),
    "lol_gpu_set_specialize_max_ops": (_int, [_vp, C.c_uint]),
    # supersampling, batches of views and blends
    "lol_gpu_set_samples": (_int, [_vp, _int]),
    "lol_gpu_samples": (_int, [_vp]),
    "lol_gpu_multi_set_samples": (_int, [_vp, _int]),
    "lol_gpu_set_adaptive_samples": (_int, [_vp, _int]),
    "lol_gpu_adaptive_samples": (_int, [_vp]),
    "lol_gpu_render_views": (_int, [_vp, _cam, _int, _int, _int, _int, _vp, _size, _size, _P(Debug), _vp]),
    "lol_gpu_set_view_batches": (_int, [_vp, _int]),
    "lol_gpu_view_batches": (_int, [_vp]),
    "lol_gpu_render_views_samples": (_int, [_vp, _cam, _int, _int, _int, _int, _int, _int, _vp, _size, _size, _P(Debug), _vp]),
    "lol_gpu_set_view_samples": (_int, [_vp, _int]),
    "lol_gpu_view_samples": (_int, [_vp]),
    "lol_gpu_render_views_blend": (_int, [_vp, _cam, _int, _int, _int, _int, _int, _vp, _size, _size, _P(Debug), _vp]),
    "lol_gpu_set_view_blends": (_int, [_vp, _int]),
    "lol_gpu_view_blends": (_int, [_vp]),
    "lol_gpu_render_views_blend_samples": (_int, [_vp, _cam, _int, _int, _int, _int, _int, _int, _vp, _size, _size, _P(Debug), _vp]),
    "lol_gpu_set_view_blend_samples": (_int, [_vp, _int]),
    "lol_gpu_view_blend_samples": (_int, [_vp]),
    # ray queries (include/lol_gpu.h, "Ray queries")
    "lol_gpu_trace_rays": (_int, [_vp, _vp, _size, _int, _P(Hits), _vp]),
    "lol_gpu_trace_pixels": (_int, [_vp, _cam, _int, _int, _int, _vp, _size, _P(Hits), _vp]),
    "lol_gpu_pick": (_int, [_vp, _cam, _int, _int, _int, _int, _int, _P(Hit)]),
    "lol_gpu_set_ray_queries": (_int, [_vp, _int]),
    "lol_gpu_ray_queries": (_int, [_vp]),
    # shading queries (include/lol_gpu.h, "Shading queries")
    "lol_gpu_shade_rays": (_int, [_vp, _vp, _size, _int, _P(Shades), _vp]),
    "lol_gpu_shade_pixels": (_int, [_vp, _cam, _int, _int, _int, _vp, _size, _P(Shades), _vp]),
    "lol_gpu_set_shade_queries": (_int, [_vp, _int]),
    "lol_gpu_shade_queries": (_int, [_vp]),
    "lol_gpu_memcpy_h2d": (_int, [_vp, _vp, _vp, _size]),
    # scene views and scene queries (include/lol_gpu.h, "Scene views", "Scene queries")
    "lol_gpu_render_scene_views": (_int, [_vp, _cam, _prog, _int, _int, _int, _int, _int, _vp, _size, _size, _P(Debug), _vp]),
    "lol_gpu_set_scene_views": (_int, [_vp, _int]),
    "lol_gpu_scene_views": (_int, [_vp]),
    "lol_gpu_render_scene_views_samples": (_int, [_vp, _cam, _prog, _int, _int, _int, _int, _int, _int, _vp, _size, _size, _P(Debug), _vp]),
    "lol_gpu_set_scene_view_samples": (_int, [_vp, _int]),
    "lol_gpu_scene_view_samples": (_int, [_vp]),
    "lol_gpu_trace_scene_rays": (_int, [_vp, _prog, _int, _vp, _size, _size, _int, _P(Hits), _vp]),
    "lol_gpu_trace_scene_pixels": (_int, [_vp, _cam, _prog, _int, _int, _int, _int, _vp, _size, _size, _P(Hits), _vp]),
    "lol_gpu_shade_scene_rays": (_int, [_vp, _prog, _int, _vp, _size, _size, _int, _P(Shades), _vp]),
    "lol_gpu_shade_scene_pixels": (_int, [_vp, _cam, _prog, _int, _int, _int, _int, _vp, _size, _size, _P(Shades), _vp]),
    # light passes and relighting (include/lol_gpu.h, "Light passes and relighting")
    "lol_gpu_light_rays": (_int, [_vp, _vp, _size, _int, _P(LightPasses), _vp]),
    "lol_gpu_light_pixels": (_int, [_vp, _cam, _int, _int, _int, _vp, _size, _P(LightPasses), _vp]),
    "lol_gpu_relight": (_int, [_vp, _prog, _P(LightPasses), _size, _P(Relit), _vp]),
    # relit views (include/lol_gpu.h, "Relit views")
    "lol_gpu_light_views": (_int, [_vp, _cam, _int, _int, _int, _int, _int, _int, _P(LightPasses), _vp]),
    "lol_gpu_relight_views": (_int, [_vp, _prog, _P(LightPasses), _int, _int, _int, _int, _int, _P(Relit), _vp]),
    # light updates (include/lol_gpu.h, "Light updates")
    "lol_gpu_light_update_rays": (_int, [_vp, _prog, _vp, _size, C.c_uint64, C.c_uint64, _P(LightPasses), _vp]),
    "lol_gpu_light_update_pixels": (_int, [_vp, _prog, _cam, _int, _int, _vp, _size, C.c_uint64, C.c_uint64, _P(LightPasses), _vp]),
    "lol_gpu_relight_held": (_int, [_vp, _prog, _prog, _P(LightPasses), _size, _P(Relit), _vp]),
    "lol_gpu_relight_views_held": (_int, [_vp, _prog, _prog, _P(LightPasses), _int, _int, _int, _int, _int, _P(Relit), _vp]),
    # scene light passes (include/lol_gpu.h, "Scene light passes"); their device lists are typed as the header types them
    "lol_gpu_light_scene_rays": (_int, [_vp, _prog, _int, _P(C.c_float), _size, _size, _int, _P(LightPasses), _vp]),
    "lol_gpu_light_scene_pixels": (_int, [_vp, _cam, _prog, _int, _int, _int, _int, _u32p, _size, _size, _P(LightPasses), _vp]),
    "lol_gpu_relight_scenes": (_int, [_vp, _prog, _prog, _int, _P(LightPasses), _size, _P(Relit), _vp]),
    # relit scene views (include/lol_gpu.h, "Relit scene views")
    "lol_gpu_relight_scene_views": (_int, [_vp, _prog, _prog, _P(LightPasses), _int, _int, _int, _int, _int, _P(Relit), _vp]),
}

_LOL_GPU_DIAG_H = {                                                     # include/lol_gpu_diag.h
    "lol_gpu_tuning_switches": (_str, []),
    "lol_gpu_roctx_ranges": (C.c_long, []),
    "lol_gpu_verify_fast_paths": (_int, [_vp, C.c_float, _P(C.c_ulonglong), _P(C.c_ulonglong)]),
    "lol_gpu_verify_smin_no_fixup": (_int, [_vp, C.c_float, _P(C.c_ulonglong)]),
    "lol_gpu_verify_gamma_table": (_int, [_vp, _P(C.c_ulonglong), _P(C.c_float)]),
    "lol_gpu_cull_bounds": (_int, [_prog, C.c_uint32, _P(C.c_float), _P(C.c_float)]),
    "lol_gpu_cull_bounds_clusters": (_int, [_prog, C.c_uint32, _P(C.c_float * 4)]),
    "lol_gpu_powf_batch": (_int, [_vp, _vp, _vp, _vp, _size, _vp]),
    "lol_gpu_sdf_batch": (_int, [_vp, _vp, _vp, _vp, _size, _vp]),
    "lol_gpu_compile_offline_samples": (_int, [_prog, _str, _str, _int, _int, _str, _size]),
    "lol_gpu_adaptive_refined": (_int, [_vp, _P(C.c_int64)]),
    "lol_gpu_adaptive_pass_ms": (_int, [_vp, _P(C.c_float)]),
    "lol_gpu_compile_offline_views": (_int, [_prog, _str, _str, _int, _int, _int, _str, _size]),
    "lol_gpu_compile_offline_view_samples": (_int, [_prog, _str, _str, _int, _int, _int, _str, _size]),
    "lol_gpu_view_samples_kernel_name": (_str, [_vp, _int, _int]),
    "lol_gpu_views_refined": (_int, [_vp, _P(C.c_int64)]),
    "lol_gpu_interp_variant": (_int, [_vp, _P(_int), _P(_int)]),
    "lol_gpu_compile_offline_view_blends": (_int, [_prog, _str, _str, _int, _int, _int, _str, _size]),
    "lol_gpu_view_blend_kernel_name": (_str, [_vp, _int]),
    "lol_gpu_compile_offline_view_blend_samples": (_int, [_prog, _str, _str, _int, _int, _int, _int, _str, _size]),
    "lol_gpu_view_blend_samples_kernel_name": (_str, [_vp, _int, _int]),
    "lol_gpu_trace_kernel_name": (_str, [_vp]),
    "lol_gpu_compile_offline_rays": (_int, [_prog, _str, _str, _int, _int, _int, _int, _str, _size]),
    "lol_gpu_code_key": (None, [_str, _size, _str]),
    "lol_gpu_shade_kernel_name": (_str, [_vp]),
    "lol_gpu_compile_offline_shade": (_int, [_prog, _str, _str, _int, _int, _int, _int, _str, _size]),
    "lol_gpu_compile_offline_module": (_int, [_prog, _str, _str, _int, C.c_uint, _int, _str, _size]),
    "lol_gpu_scene_views_kernel_name": (_str, [_vp, _int]),
    "lol_gpu_scene_views_state": (_int, [_vp]),
    "lol_gpu_compile_offline_scene_views": (_int, [_prog, _str, _str, _str, _size]),
    "lol_gpu_interp_fast_paths": (_int, [_vp, _P(_int), _P(C.c_uint), _P(C.c_uint)]),
    "lol_gpu_shade_math": (_int, [_vp, _P(ShadeMathInfo)]),
    "lol_gpu_scene_view_samples_kernel_name": (_str, [_vp, _int, _int]),
    "lol_gpu_compile_offline_scene_view_samples": (_int, [_prog, _str, _str, _str, _size]),
    "lol_gpu_interp_list_info": (_int, [_prog, _int, _u32p, _u32p, _u32p, _u32p, _u32p, _size]),
}

_LOL_GPU_TESTING_H = {                                                  # include/lol_gpu_testing.h
    "lol_gpu_testing_fail_uploads": (_int, [_vp, _int]),
    "lol_gpu_testing_fail_first_tier": (_int, [_vp, _int]),
    "lol_gpu_testing_has_return_clobbering_branch": (_int, [_str, _size]),
    "lol_gpu_multi_testing_root_stride": (_int, [_vp, _int]),
    "lol_gpu_multi_testing_force_copier_threads": (_int, [_vp, _int]),
    "lol_gpu_testing_fail_view_scratch": (_int, [_vp, _int]),
    "lol_gpu_testing_pixel_cost": (_int, [_vp, _u16p, _size]),
    "lol_gpu_testing_deal": (_int, [_vp, _u16p, _int, _int, _u32p, _size]),
    "lol_gpu_testing_sort_tiles": (_int, [_vp, _u32p, _u32p, _u32p, _size, _u32p, _u32p, _u32p]),
    "lol_gpu_testing_schedule": (_int, [_vp, _P(_ScheduleInfo), _u32p, _u32p, _u32p, _u32p, _size, _u32p, _size]),
}

EXPORTED_SYMBOLS, DIAG_SYMBOLS, TESTING_SYMBOLS = list(_LOL_GPU_H), list(_LOL_GPU_DIAG_H), list(_LOL_GPU_TESTING_H)

_lib = None


def gpu_lib() -> C.CDLL:
    global _lib
    if _lib is None:
        path = os.environ.get("LOL_GPU_LIB") or os.path.join(S.LIB_DIR, "liblol_gpu.so")     # LOL_GPU_LIB: A/B another build
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: the HIP extension was not built "
                               "(run __graft_entry__.build()); there is no CPU fallback")
        lib = C.CDLL(path)
        S._bind_prototypes(lib, {"lol_gpu_abi_version": _LOL_GPU_H["lol_gpu_abi_version"]})
        if lib.lol_gpu_abi_version() != LOL_GPU_ABI_VERSION:
            raise RuntimeError(f"{path} speaks ABI version {lib.lol_gpu_abi_version()}, this mirror {LOL_GPU_ABI_VERSION}: "
                               "rebuild (__graft_entry__.build())")
        S._bind_prototypes(lib, _LOL_GPU_H, _LOL_GPU_DIAG_H, _LOL_GPU_TESTING_H)
        _lib = lib
    return _lib


def tuning_switches() -> str:
    """lol_gpu_tuning_switches: the LOL_GPU_* A/B switches this process has honoured so far (needs LOL_GPU_TUNING=1)."""
    return gpu_lib().lol_gpu_tuning_switches().decode()


def code_key(code: bytes) -> str:
    """lol_gpu_code_key: the kernel_key of a code object's bytes (a .co of compile_offline*).  Needs no device."""
    out = C.create_string_buffer(17)
    gpu_lib().lol_gpu_code_key(code, len(code), out)
    return out.value.decode()


def interp_list_info(program: S.Program, cull: bool = True) -> dict:
    """lol_gpu_interp_list_info: the interpreter list the scene-record calls build for `program` — n_mops, n_tests, n_unbounded and,
    per object in evaluation order, its root id (order) and whether the record that finishes it carries MOP_TIE (tie).  No device."""
    cap = int(program.n_roots)
    n_mops, n_tests, n_unbounded = C.c_uint32(), C.c_uint32(), C.c_uint32()
    order, tie = (C.c_uint32 * max(cap, 1))(), (C.c_uint32 * max(cap, 1))()
    n = gpu_lib().lol_gpu_interp_list_info(C.byref(program), int(bool(cull)), C.byref(n_mops), C.byref(n_tests), C.byref(n_unbounded),
                                           order, tie, cap)
    if n < 0 or n > cap:
        raise GpuError(n, "lol_gpu_interp_list_info failed")
    return {"n_mops": n_mops.value, "n_tests": n_tests.value, "n_unbounded": n_unbounded.value,
            "order": tuple(order[:n]), "tie": tuple(tie[:n])}


# the module switches, by their setters' names: bit i of lol_gpu_compile_offline_module's mask (include/lol_gpu_diag.h)
MODULE_SWITCHES = ("samples", "view_batches", "view_samples", "view_blends", "view_blend_samples", "ray_queries", "shade_queries")


def compile_offline_module(program: S.Program, out_base: str, switches=(), form: int = 0, arch: str = "gfx950",
                           assume_fast: bool = False) -> str:
    """hipRTC-compile the scene module a context with `switches` set before its upload gets (names of MODULE_SWITCHES; "samples":
    set_samples > 1), without a device: writes out_base.hip and out_base.co and returns the compiler log.  form: 0 by the scene's
    size, 1 the SDF out of line, 2 inlined (the two kernels of a 257 ... 1024-op scene)."""
    unknown = set(switches) - set(MODULE_SWITCHES)
    if unknown:
        raise ValueError("no module switch: " + ", ".join(sorted(unknown)))
    mask = sum(1 << MODULE_SWITCHES.index(name) for name in set(switches))
    log = C.create_string_buffer(1 << 16)
    st = gpu_lib().lol_gpu_compile_offline_module(C.byref(program), arch.encode(), os.fsencode(out_base), int(assume_fast), mask,
                                                  int(form), log, len(log))
    if st != LOL_GPU_OK:
        raise GpuError(st, "hipRTC compile failed:\n" + log.value.decode(errors="replace"))
    return log.value.decode(errors="replace")


# The entry points from before compile_offline_module, one per switch: `enable` is that switch, the keywords the others beside it.
def _offline(program, out_base, form, arch, assume_fast, **switches) -> str:
    return compile_offline_module(program, out_base, [name for name, on in switches.items() if on], form, arch, assume_fast)


def compile_offline(program: S.Program, out_base: str, arch: str = "gfx950", assume_fast: bool = False) -> str:
    return _offline(program, out_base, 0, arch, assume_fast)


def compile_offline_samples(program: S.Program, out_base: str, samples: int, arch: str = "gfx950",
                            assume_fast: bool = False) -> str:
    if samples not in (1, 2, 4):
        raise GpuError(-3, "samples per axis must be 1, 2 or 4")
    return _offline(program, out_base, 0, arch, assume_fast, samples=samples > 1)


def compile_offline_views(program: S.Program, out_base: str, enable: bool = True, form: int = 0, arch: str = "gfx950",
                          assume_fast: bool = False) -> str:
    return _offline(program, out_base, form, arch, assume_fast, view_batches=enable)


def compile_offline_view_samples(program: S.Program, out_base: str, enable: bool = True, form: int = 0, arch: str = "gfx950",
                                 assume_fast: bool = False) -> str:
    return _offline(program, out_base, form, arch, assume_fast, view_samples=enable)


def compile_offline_view_blends(program: S.Program, out_base: str, enable: bool = True, form: int = 0, arch: str = "gfx950",
                                assume_fast: bool = False, samples: bool = False, view_batches: bool = False,
                                view_samples: bool = False) -> str:
    return _offline(program, out_base, form, arch, assume_fast, view_blends=enable, samples=samples, view_batches=view_batches,
                    view_samples=view_samples)


def compile_offline_view_blend_samples(program: S.Program, out_base: str, enable: bool = True, form: int = 0, arch: str = "gfx950",
                                       assume_fast: bool = False, view_blends: bool = False, samples: bool = False,
                                       view_batches: bool = False, view_samples: bool = False) -> str:
    return _offline(program, out_base, form, arch, assume_fast, view_blend_samples=enable, view_blends=view_blends, samples=samples,
                    view_batches=view_batches, view_samples=view_samples)


def compile_offline_rays(program: S.Program, out_base: str, enable: bool = True, form: int = 0, arch: str = "gfx950",
                         assume_fast: bool = False, view_blends: bool = False, samples: bool = False, view_batches: bool = False,
                         view_samples: bool = False, view_blend_samples: bool = False) -> str:
    return _offline(program, out_base, form, arch, assume_fast, ray_queries=enable, view_blends=view_blends, samples=samples,
                    view_batches=view_batches, view_samples=view_samples, view_blend_samples=view_blend_samples)


def compile_offline_shade(program: S.Program, out_base: str, enable: bool = True, form: int = 0, arch: str = "gfx950",
                          assume_fast: bool = False, view_blends: bool = False, samples: bool = False, view_batches: bool = False,
                          view_samples: bool = False, view_blend_samples: bool = False, ray_queries: bool = False) -> str:
    return _offline(program, out_base, form, arch, assume_fast, shade_queries=enable, view_blends=view_blends, samples=samples,
                    view_batches=view_batches, view_samples=view_samples, view_blend_samples=view_blend_samples, ray_queries=ray_queries)


def _offline_structure(compile_fn, program, out_base, arch) -> str:
    log = C.create_string_buffer(1 << 16)
    st = compile_fn(C.byref(program), arch.encode(), os.fsencode(out_base), log, len(log))
    if st != LOL_GPU_OK:
        raise GpuError(st, "hipRTC compile failed:\n" + log.value.decode(errors="replace"))
    return log.value.decode(errors="replace")


def compile_offline_scene_views(program: S.Program, out_base: str, arch: str = "gfx950") -> str:
    """hipRTC-compile the STRUCTURE module of `program` (Renderer.set_scene_views) without a device: writes out_base.hip and
    out_base.co and returns the compiler log.  The source depends on the program's structure alone — opcodes, ids and counts — so
    two programs of one structure give the same two files, byte for byte."""
    return _offline_structure(gpu_lib().lol_gpu_compile_offline_scene_views, program, out_base, arch)


def compile_offline_scene_view_samples(program: S.Program, out_base: str, arch: str = "gfx950") -> str:
    """compile_offline_scene_views for the structure module that Renderer.set_scene_view_samples asks for: the same SDF and the two
    kernels of that module, and lol_render_param_batch_aa / lol_render_param_batch_aa_lin behind them.  Another source than
    compile_offline_scene_views writes, hence another code object; it too depends on the program's structure alone."""
    return _offline_structure(gpu_lib().lol_gpu_compile_offline_scene_view_samples, program, out_base, arch)


MAX_VIEWS = 4096                     # LOL_GPU_MAX_VIEWS
MAX_BLEND = 16                       # LOL_GPU_MAX_BLEND


def part_rows(h: int, rows: Rows | None) -> int:
    return gpu_lib().lol_gpu_part_rows(h, _ref(rows))


def split_rows(n_parts: int, band_rows: int, root_band_rows: int = 0, root_stride: int = 1) -> list:
    """lol_gpu_split_rows (pure host logic, no device needed): the Rows of every part of a frame cut into n_parts
    parts with bands of band_rows rows, those of parts p % root_stride == 0 root_band_rows tall (0 = band_rows)."""
    arr = (Rows * n_parts)()
    st = gpu_lib().lol_gpu_split_rows(n_parts, band_rows, root_band_rows, root_stride, arr)
    if st != LOL_GPU_OK:
        raise GpuError(st, f"lol_gpu_split_rows({n_parts}, {band_rows}, {root_band_rows}, {root_stride})")
    return [Rows(r.band_rows, r.cycle_rows, r.offset_rows) for r in arr]


def assemble_parts_at(ctx_renderer, parts_ptr: int, part_rows: list, part_row0: list, w: int, h: int, dst_ptr: int,
                      pitch_bytes: int, stream: int | None):
    """lol_gpu_assemble_parts_at on the renderer's device: un-interleave gathered parts (device pointers)."""
    n = len(part_rows)
    rows = (Rows * n)(*part_rows)
    row0 = (C.c_uint32 * n)(*part_row0)
    st = gpu_lib().lol_gpu_assemble_parts_at(ctx_renderer._ctx, C.c_void_p(parts_ptr), rows, row0, n, w, h,
                                             C.c_void_p(dst_ptr), pitch_bytes, _stream_arg(stream))
    if st != LOL_GPU_OK:
        raise GpuError(st, "lol_gpu_assemble_parts_at")


class Renderer:
    def __init__(self, device: int = 0, specialize: bool | int = True):
        self._lib = gpu_lib()
        self._ctx = C.c_void_p()
        st = self._lib.lol_gpu_create(device, C.byref(self._ctx))
        if st != LOL_GPU_OK:
            self._ctx = C.c_void_p()
            raise GpuError(st, f"lol_gpu_create(device={device}) failed")
        self._lib.lol_gpu_set_specialize(self._ctx, int(specialize))
        self.scene: S.Scene | None = None
        self.program: S.Program | None = None

    def _check(self, st: int):
        if st != LOL_GPU_OK:
            raise GpuError(st, self._lib.lol_gpu_error(self._ctx).decode())

    def _frame_camera(self, frame_camera, w: int, h: int, camera):
        """frame_camera, or the prepared scene's for a w x h frame under `camera` (None: the scene's own)"""
        return frame_camera if frame_camera is not None else self.scene.frame_camera(w, h, camera)

    def _camera_array(self, cameras, w: int, h: int):
        """scene.Camera or ready scene.FrameCamera objects as one ctypes array of FrameCamera for w x h frames (never of length 0)"""
        arr = (S.FrameCamera * max(1, len(cameras)))()
        for i, c in enumerate(cameras):
            fc = c if isinstance(c, S.FrameCamera) else self.scene.frame_camera(w, h, c)
            C.memmove(C.byref(arr, i * C.sizeof(S.FrameCamera)), C.byref(fc), C.sizeof(S.FrameCamera))
        return arr

    @staticmethod
    def _look_program(look):
        """A `look` or `held` argument — a scene.Scene (flattened here), a ready scene.Program or None — as a Program or None.  The
        caller keeps the result until its C call has returned: a flattened program's tables go when the object does."""
        return look if look is None or isinstance(look, S.Program) else look.flatten()

    @staticmethod
    def _pitch_and_stride(w: int, h: int, pitch_bytes, view_stride_bytes):
        """the batch methods' defaults: dense rows, dense views"""
        pitch = pitch_bytes if pitch_bytes is not None else w * 4
        return pitch, view_stride_bytes if view_stride_bytes is not None else h * pitch

    # render_prepare (renderer.h:25): flatten + upload the scene
    def prepare(self, scene: S.Scene, wait: bool = True):
        """wait=True (tests, benchmarks): also wait for the scene's own kernel, so that the frames that follow all run it.
        wait=False is what the C host does: return as soon as the interpreter can render (tiered start-up, lol_gpu.h)."""
        self.scene = scene
        self.program = scene.flatten()
        self._check(self._lib.lol_gpu_upload_program(self._ctx, C.byref(self.program)))
        if wait:
            self.specialize_wait()

    def upload_program(self, program: S.Program, wait: bool = True):
        self.program = program
        self._check(self._lib.lol_gpu_upload_program(self._ctx, C.byref(program)))
        if wait:
            self.specialize_wait()

    def set_specialize_max_ops(self, max_ops: int):
        """The largest program the scene compiler takes on (0 = the default, 6144 ops); takes effect at the next prepare()."""
        self._check(self._lib.lol_gpu_set_specialize_max_ops(self._ctx, max_ops))

    def specialize_wait(self):
        self._check(self._lib.lol_gpu_specialize_wait(self._ctx))

    def specialize_state(self):
        """(state, compile_ms): 0 none, 1 compiling, 3 compiled (takes over at the next frame), 2 in use, -1 failed; scenes of
        257 ... 1024 ops: 5 = the first kernel (SDF out of line) in use, the second (SDF inlined) compiling, 6 = the second compiled."""
        ms = C.c_double()
        st = self._lib.lol_gpu_specialize_state(self._ctx, C.byref(ms))
        return st, ms.value

    def render_into(self, dst_ptr: int, w: int, h: int, max_steps: int = 256, camera: S.Camera | None = None,
                    rows: Rows | None = None, pitch_bytes: int | None = None, debug: Debug | None = None,
                    stream: int | None = None, frame_camera: S.FrameCamera | None = None):
        """Asynchronously render (a part of) a frame into device memory at dst_ptr."""
        fc = self._frame_camera(frame_camera, w, h, camera)
        self._check(self._lib.lol_gpu_render_device(
            self._ctx, C.byref(fc), w, h, max_steps, _ref(rows), C.c_void_p(dst_ptr), pitch_bytes if pitch_bytes is not None else w * 4,
            _ref(debug), _stream_arg(stream)))

    def set_view_batches(self, enable: bool):
        """Before prepare(): the scene's own module also carries the batch kernel (lol_render_spec_batch); without it — and until
        that kernel is ready — render_views_into runs on the interpreter's render_interp_batch.  Same pixels either way."""
        self._check(self._lib.lol_gpu_set_view_batches(self._ctx, 1 if enable else 0))

    @property
    def view_batches(self) -> bool:
        return bool(self._lib.lol_gpu_view_batches(self._ctx))

    def set_view_samples(self, enable: bool):
        """Before prepare(): the scene's own module also carries the supersampled batch kernels (lol_render_spec_batch_aa,
        lol_render_spec_batch_aa_list, and the batch kernels of set_view_batches); without it — and until that module is ready —
        render_views_into(samples=2 or 4) runs on the interpreter's instantiations.  Same pixels either way."""
        self._check(self._lib.lol_gpu_set_view_samples(self._ctx, 1 if enable else 0))

    @property
    def view_samples(self) -> bool:
        return bool(self._lib.lol_gpu_view_samples(self._ctx))

    def view_samples_kernel_name(self, samples: int, adaptive: int = -1) -> str:
        """the kernel the next render_views_into(..., samples, adaptive) launches (an adaptive batch: its refine pass)"""
        return self._lib.lol_gpu_view_samples_kernel_name(self._ctx, int(samples), int(adaptive)).decode()

    def views_refined(self) -> int:
        """how many pixels of the last adaptive batch, all views together, were refined (waits for that batch)"""
        n = C.c_int64(0)
        self._check(self._lib.lol_gpu_views_refined(self._ctx, C.byref(n)))
        return int(n.value)

    def interp_variant(self) -> tuple:
        """(ssize, tables_global) of the interpreter instantiation the uploaded program runs on, as the launches themselves choose it
        (lol_gpu_interp_variant): ssize 1, 3, 7, 11 or 63; tables_global True = tables read from global memory (ssize 3, 11 or 63)"""
        ssize, tg = C.c_int(), C.c_int()
        self._check(self._lib.lol_gpu_interp_variant(self._ctx, C.byref(ssize), C.byref(tg)))
        return int(ssize.value), bool(tg.value)

    def testing_fail_view_scratch(self, n: int):
        """lol_gpu_testing.h: the next n scratch allocations of adaptive batches and of blends fail"""
        self._check(self._lib.lol_gpu_testing_fail_view_scratch(self._ctx, int(n)))

    def render_views_into(self, dst_ptr: int, cameras, w: int, h: int, max_steps: int = 256, pitch_bytes: int | None = None,
                          view_stride_bytes: int | None = None, debug: Debug | None = None, stream: int | None = None,
                          samples: int = 1, adaptive: int = -1):
        """Asynchronously render len(cameras) views of w x h in ONE launch (lol_gpu_render_views): view v is exactly the frame
        render_into renders under cameras[v] in a fixed tile order, its row y at dst_ptr + v * view_stride_bytes + y * pitch_bytes;
        the diagnostics of `debug` are dense [view, y, x] arrays.  cameras: scene.Camera or ready scene.FrameCamera objects (the
        array is copied before the call returns).
        samples = 2 or 4 (and adaptive = a contrast 0 ... 255): the supersampled batch of lol_gpu_render_views_samples — view v is the
        frame of set_samples(samples) / set_adaptive_samples(adaptive), whatever this renderer's own set_samples says."""
        cams = list(cameras)
        arr = self._camera_array(cams, w, h)
        pitch, stride = self._pitch_and_stride(w, h, pitch_bytes, view_stride_bytes)
        dbg = _ref(debug)
        if samples == 1 and adaptive == -1:
            self._check(self._lib.lol_gpu_render_views(
                self._ctx, arr, len(cams), w, h, max_steps, C.c_void_p(dst_ptr), pitch, stride, dbg, _stream_arg(stream)))
        else:
            self._check(self._lib.lol_gpu_render_views_samples(
                self._ctx, arr, len(cams), w, h, max_steps, int(samples), int(adaptive), C.c_void_p(dst_ptr), pitch, stride, dbg,
                _stream_arg(stream)))

    def set_view_blends(self, enable: bool):
        """Before prepare(): the scene's own module also carries the linear-colour batch kernel (lol_render_spec_batch_lin); without
        it — and until that module is ready — render_blended_views_into runs its first pass on the interpreter's
        render_interp_batch_lin.  Same pixels either way."""
        self._check(self._lib.lol_gpu_set_view_blends(self._ctx, 1 if enable else 0))

    @property
    def view_blends(self) -> bool:
        return bool(self._lib.lol_gpu_view_blends(self._ctx))

    def view_blend_kernel_name(self, cameras_per_view: int) -> str:
        """the kernel the first pass of the next render_blended_views_into(..., cameras_per_view, ...) launches"""
        return self._lib.lol_gpu_view_blend_kernel_name(self._ctx, int(cameras_per_view)).decode()

    def set_view_blend_samples(self, enable: bool):
        """Before prepare(): the scene's own module also carries the supersampled linear-colour batch kernel
        (lol_render_spec_batch_aa_lin); without it — and until that module is ready — render_blended_views_into(..., samples > 1)
        runs its first pass on the interpreter's render_interp_batch_aa_lin.  Same pixels either way.  A switch of its own:
        set_view_blends and set_view_samples together do not imply it."""
        self._check(self._lib.lol_gpu_set_view_blend_samples(self._ctx, 1 if enable else 0))

    @property
    def view_blend_samples(self) -> bool:
        return bool(self._lib.lol_gpu_view_blend_samples(self._ctx))

    def view_blend_samples_kernel_name(self, cameras_per_view: int, samples: int) -> str:
        """the kernel the first pass of the next render_blended_views_into(..., cameras_per_view, ..., samples=samples) launches"""
        return self._lib.lol_gpu_view_blend_samples_kernel_name(self._ctx, int(cameras_per_view), int(samples)).decode()

    def render_blended_views_into(self, dst_ptr: int, cameras, cameras_per_view: int, w: int, h: int, max_steps: int = 256,
                                  pitch_bytes: int | None = None, view_stride_bytes: int | None = None, debug: Debug | None = None,
                                  stream: int | None = None, samples: int = 1):
        """Asynchronously render len(cameras) / cameras_per_view views of w x h, each the mean IN LINEAR LIGHT of the frames under its
        K = cameras_per_view cameras (lol_gpu_render_views_blend): view v averages cameras[v K ... v K + K - 1] — the cameras of a
        shutter interval (scene.shutter_cameras: motion blur) or of a lens (scene.lens_cameras: depth of field).  K in {1, 2, 4, 8,
        16}; K = 1 is render_views_into.  Addressing and `debug` as render_views_into (with K > 1: rgb alone, the mean after gamma).
        cameras: scene.Camera or ready scene.FrameCamera objects (the array is copied before the call returns).
        samples > 1: samples x samples samples per pixel under EVERY camera (lol_gpu_render_views_blend_samples): each camera's
        supersampled linear mean first, then the mean over the cameras; samples in {1, 2, 4}."""
        cams = list(cameras)
        k = int(cameras_per_view)
        if k < 1 or len(cams) % k:
            raise ValueError("render_blended_views_into: len(cameras) must be a multiple of cameras_per_view")
        arr = self._camera_array(cams, w, h)
        pitch, stride = self._pitch_and_stride(w, h, pitch_bytes, view_stride_bytes)
        dbg = _ref(debug)
        if samples == 1:
            self._check(self._lib.lol_gpu_render_views_blend(
                self._ctx, arr, len(cams) // k, k, w, h, max_steps, C.c_void_p(dst_ptr), pitch, stride, dbg, _stream_arg(stream)))
        else:
            self._check(self._lib.lol_gpu_render_views_blend_samples(
                self._ctx, arr, len(cams) // k, k, w, h, max_steps, int(samples), C.c_void_p(dst_ptr), pitch, stride, dbg,
                _stream_arg(stream)))

    def set_scene_views(self, enable: bool):
        """Before prepare(): the scene compiler also makes the STRUCTURE module behind the scene's own (lol_render_param_batch,
        lol_render_param_batch_lin: the scene's SDF specialised on its structure alone, every number read from the view's record);
        render_scene_views_into runs on it once it is loaded (specialize_wait waits for it too).  Without it — and until it is
        loaded, with specialisation off, or for a program of more than 256 ops — the interpreter's render_interp_scene_batch /
        _lin render on every record's own lists.  Same pixels either way; the scene's own module and kernel_key() do not change.
        Opt-in for a reason: for scene4 the interpreter with the upload's proven fast paths was the faster of the two (DESIGN.md
        3.18, tools/scene_views_rate.py measures a host's own scenes)."""
        self._check(self._lib.lol_gpu_set_scene_views(self._ctx, 1 if enable else 0))

    @property
    def scene_views(self) -> bool:
        return bool(self._lib.lol_gpu_scene_views(self._ctx))

    def scene_views_kernel_name(self, cameras_per_view: int = 1) -> str:
        """the kernel the next render_scene_views_into(..., cameras_per_view=...) launches (of a blend: its first pass)"""
        return self._lib.lol_gpu_scene_views_kernel_name(self._ctx, int(cameras_per_view)).decode()

    def set_scene_view_samples(self, enable: bool):
        """Before prepare(): set_scene_views, and the structure module is made with two more kernels (lol_render_param_batch_aa,
        lol_render_param_batch_aa_lin) on which render_scene_views_into(..., samples=2 or 4) runs once the module is loaded.  Without
        it — and until the module is loaded — the interpreter's render_interp_scene_batch_aa / _aa_lin render those calls.  Same
        pixels either way.  Another source of the structure module, hence another code object: without this switch that module is
        byte for byte what set_scene_views alone gives."""
        self._check(self._lib.lol_gpu_set_scene_view_samples(self._ctx, 1 if enable else 0))

    @property
    def scene_view_samples(self) -> bool:
        return bool(self._lib.lol_gpu_scene_view_samples(self._ctx))

    def scene_view_samples_kernel_name(self, cameras_per_view: int = 1, samples: int = 2) -> str:
        """the kernel the next render_scene_views_into(..., cameras_per_view=..., samples=...) launches (of a blend: its first pass)"""
        return self._lib.lol_gpu_scene_view_samples_kernel_name(self._ctx, int(cameras_per_view), int(samples)).decode()

    def scene_views_state(self) -> int:
        """the structure module of the uploaded program: 0 none, 1 compiling, 2 in use, -1 failed"""
        return int(self._lib.lol_gpu_scene_views_state(self._ctx))

    def interp_fast_paths(self) -> tuple:
        """(sqrt_kind, proven, proven_without_fixup): what the last upload proved for the interpreter's kernels — the sqrt kind they
        run with (0 plain, 3 the proven fast root) and how many smoothness constants of the program have a proven fast blend factor
        (and how many of those also without v_div_fixup).  The lists of scene views are built with exactly this."""
        kind, n, nf = C.c_int(), C.c_uint(), C.c_uint()
        self._check(self._lib.lol_gpu_interp_fast_paths(self._ctx, C.byref(kind), C.byref(n), C.byref(nf)))
        return int(kind.value), int(n.value), int(nf.value)

    def shade_math(self) -> dict:
        """lol_gpu_shade_math: the arithmetic of the per-pixel code around the loops in the scene kernel's fast pipeline — "root_kind",
        "rcp_form" as the last upload decided them — and under "proofs" the two exhaustive comparisons behind the reciprocal ("rcp1",
        "rcp2": mismatches over all 2^32 floats, None when not run, and the interval of bit patterns around 1.0f without one)."""
        info = ShadeMathInfo()
        self._check(self._lib.lol_gpu_shade_math(self._ctx, C.byref(info)))
        proofs = {}
        for i, name in enumerate(("rcp1", "rcp2")):
            n = int(info.proof_mismatches[i])
            proofs[name] = {"mismatches": None if n == 2 ** 64 - 1 else n, "interval": (int(info.proof_lo[i]), int(info.proof_hi[i]))}
        return {"root_kind": int(info.root_kind), "rcp_form": int(info.rcp_form), "proofs": proofs}

    def render_scene_views_into(self, dst_ptr: int, cameras, scenes, w: int, h: int, cameras_per_view: int = 1, max_steps: int = 256,
                                pitch_bytes: int | None = None, view_stride_bytes: int | None = None, debug: Debug | None = None,
                                stream: int | None = None, samples: int = 1):
        """Asynchronously render len(scenes) / cameras_per_view views of w x h, every RECORD under a camera and a scene of its own
        (lol_gpu_render_scene_views): record r is the frame this renderer would render under cameras[r] after prepare(scenes[r]).
        With K = cameras_per_view = 1 view v is that frame, with every diagnostic of `debug`; with K in {2, 4, 8, 16} view v is the
        mean IN LINEAR LIGHT of records v K ... v K + K - 1, as render_blended_views_into averages cameras (rgb alone).
        scenes: scene.Scene objects (flattened here) or ready scene.Program objects, all of the prepared scene's structure
        (scene.same_structure; scene.tween gives such scenes).  cameras: scene.Camera / scene.FrameCamera objects, one per record,
        or None: every record's own scene's camera.  Both arrays are copied before the call returns.  Addressing as
        render_views_into.
        samples = s in {2, 4} (lol_gpu_render_scene_views_samples): s x s samples per pixel under every record — each record's pixel
        is the linear mean of its samples as a frame after set_samples(s) takes it, on that record's own scene; then the mean over
        the K records as before, gamma and packing.  `debug` then takes rgb alone.  samples = 1 is the call without it."""
        items = list(scenes)
        k = int(cameras_per_view)
        if k < 1 or len(items) % k:
            raise ValueError("render_scene_views_into: len(scenes) must be a multiple of cameras_per_view")
        keep, progs, arr = self._scene_records("render_scene_views_into", items, cameras, (w, h))
        pitch, stride = self._pitch_and_stride(w, h, pitch_bytes, view_stride_bytes)
        dbg = _ref(debug)
        if int(samples) == 1:
            self._check(self._lib.lol_gpu_render_scene_views(
                self._ctx, arr, progs, len(items) // k, k, w, h, max_steps, C.c_void_p(dst_ptr), pitch, stride, dbg, _stream_arg(stream)))
        else:
            self._check(self._lib.lol_gpu_render_scene_views_samples(
                self._ctx, arr, progs, len(items) // k, k, w, h, max_steps, int(samples), C.c_void_p(dst_ptr), pitch, stride, dbg,
                _stream_arg(stream)))
        del keep

    # ---- scene queries (include/lol_gpu.h, "Scene queries")
    def _scene_records(self, who: str, scenes, cameras=None, size=None):
        """(keep, programs, frame cameras or None) of the records of render_scene_views_into (`who`, for its errors) or of a scene
        query: scenes as render_scene_views_into takes them; size = (w, h): one camera per scene as there (None: every scene's own)."""
        items = list(scenes)
        cams = list(cameras) if cameras is not None else [None] * len(items)
        if size is not None and len(cams) != len(items):
            raise ValueError(who + ": one camera per scene")
        keep = []                                    # the flattened programs live until the call has copied them
        progs = (S.Program * max(1, len(items)))()
        for i, sc in enumerate(items):
            prog = sc if isinstance(sc, S.Program) else sc.flatten()
            keep.append(prog)
            C.memmove(C.byref(progs, i * C.sizeof(S.Program)), C.byref(prog), C.sizeof(S.Program))
        if size is None:
            return keep, progs, None
        w, h = size
        arr = (S.FrameCamera * max(1, len(items)))()
        for i, (sc, c) in enumerate(zip(items, cams)):
            if isinstance(c, S.FrameCamera):
                fc = c
            elif isinstance(sc, S.Program):
                if c is None:
                    raise ValueError(who + ": a Program has no camera of its own")
                fc = self.scene.frame_camera(w, h, c)
            else:
                fc = sc.frame_camera(w, h, c)
            C.memmove(C.byref(arr, i * C.sizeof(S.FrameCamera)), C.byref(fc), C.sizeof(S.FrameCamera))
        return keep, progs, arr

    def _record_looks(self, who: str, looks, n_records: int):
        """(keep, programs or None) of the looks of a resolve over n_records records (`who`, for its error): one per record as
        _scene_records takes scenes, or None: the scenes' own"""
        if looks is None:
            return [], None
        look_items = list(looks)
        if len(look_items) != n_records:
            raise ValueError(who + ": one look per scene")
        keep, look_progs, _ = self._scene_records(who, look_items)
        return keep, look_progs

    def trace_scene_rays_into(self, scenes, rays_ptr: int, n: int, list_stride: int = 0, max_steps: int = 256, dist_ptr: int = 0,
                              id_ptr: int = 0, steps_ptr: int = 0, normal_ptr: int = 0, stream: int | None = None):
        """Asynchronously trace n rays under EACH of len(scenes) scenes of the prepared scene's structure (lol_gpu_trace_scene_rays):
        element (r, i), at index r n + i of every output, is what trace_rays_into answers for ray i of record r after
        prepare(scenes[r]).  list_stride = 0: one list of n rays (device memory) serves every record; else record r's list begins
        list_stride rays behind record r - 1's.  scenes: scene.Scene or scene.Program objects, copied before the call returns."""
        items = list(scenes)
        keep, progs, _ = self._scene_records("trace_scene_rays_into", items)
        hits = Hits(dist_ptr or None, id_ptr or None, steps_ptr or None, normal_ptr or None)
        self._check(self._lib.lol_gpu_trace_scene_rays(self._ctx, progs, len(items), C.c_void_p(rays_ptr), n, list_stride, max_steps,
                                                       C.byref(hits), _stream_arg(stream)))
        del keep

    def trace_scene_pixels_into(self, scenes, xy_ptr: int, n: int, w: int, h: int, list_stride: int = 0, max_steps: int = 256,
                                dist_ptr: int = 0, id_ptr: int = 0, steps_ptr: int = 0, normal_ptr: int = 0,
                                stream: int | None = None, cameras=None):
        """... the primary rays of n pixels (device memory, n x {x, y} uint32) of the w x h frame under each record's own camera
        (lol_gpu_trace_scene_pixels).  cameras: as render_scene_views_into takes them; None: every scene's own."""
        items = list(scenes)
        keep, progs, arr = self._scene_records("trace_scene_pixels_into", items, cameras, (w, h))
        hits = Hits(dist_ptr or None, id_ptr or None, steps_ptr or None, normal_ptr or None)
        self._check(self._lib.lol_gpu_trace_scene_pixels(self._ctx, arr, progs, len(items), w, h, max_steps, C.c_void_p(xy_ptr), n,
                                                         list_stride, C.byref(hits), _stream_arg(stream)))
        del keep

    def shade_scene_rays_into(self, scenes, rays_ptr: int, n: int, list_stride: int = 0, max_steps: int = 256, rgb_linear_ptr: int = 0,
                              rgb_ptr: int = 0, pixel_ptr: int = 0, dist_ptr: int = 0, id_ptr: int = 0, steps_ptr: int = 0,
                              stream: int | None = None):
        """shade_rays_into under each of len(scenes) scenes (lol_gpu_shade_scene_rays); records, lists and outputs as
        trace_scene_rays_into."""
        items = list(scenes)
        keep, progs, _ = self._scene_records("shade_scene_rays_into", items)
        out = Shades(rgb_linear_ptr or None, rgb_ptr or None, pixel_ptr or None, dist_ptr or None, id_ptr or None, steps_ptr or None)
        self._check(self._lib.lol_gpu_shade_scene_rays(self._ctx, progs, len(items), C.c_void_p(rays_ptr), n, list_stride, max_steps,
                                                       C.byref(out), _stream_arg(stream)))
        del keep

    def shade_scene_pixels_into(self, scenes, xy_ptr: int, n: int, w: int, h: int, list_stride: int = 0, max_steps: int = 256,
                                rgb_linear_ptr: int = 0, rgb_ptr: int = 0, pixel_ptr: int = 0, dist_ptr: int = 0, id_ptr: int = 0,
                                steps_ptr: int = 0, stream: int | None = None, cameras=None):
        """shade_pixels_into under each record's own scene and camera (lol_gpu_shade_scene_pixels); records as
        trace_scene_pixels_into."""
        items = list(scenes)
        keep, progs, arr = self._scene_records("shade_scene_pixels_into", items, cameras, (w, h))
        out = Shades(rgb_linear_ptr or None, rgb_ptr or None, pixel_ptr or None, dist_ptr or None, id_ptr or None, steps_ptr or None)
        self._check(self._lib.lol_gpu_shade_scene_pixels(self._ctx, arr, progs, len(items), w, h, max_steps, C.c_void_p(xy_ptr), n,
                                                         list_stride, C.byref(out), _stream_arg(stream)))
        del keep

    def pick_scenes(self, scenes, x: int, y: int, w: int, h: int, cameras=None, max_steps: int = 256) -> list:
        """What is under pixel (x, y) of the w x h frame in EACH scene: a list of pick()'s dicts in host memory, from one
        trace_scene_pixels_into call on the context's own stream (waits)."""
        items = list(scenes)
        if not (0 <= int(x) < w and 0 <= int(y) < h):
            raise ValueError("pick_scenes: the pixel lies outside the frame")
        r = len(items)
        host = (C.c_uint32 * (2 + 6 * max(1, r)))(int(x), int(y))      # xy | dist [r] | id [r] | steps [r] | normal [3 r]
        dev = self.malloc(C.sizeof(host))
        try:
            self.memcpy_h2d(dev, C.addressof(host), 8)
            at = lambda k: dev + 4 * (2 + k * r)      # noqa: E731
            self.trace_scene_pixels_into(items, dev, 1, w, h, 0, max_steps, dist_ptr=at(0), id_ptr=at(1), steps_ptr=at(2),
                                         normal_ptr=at(3), cameras=cameras)
            self.sync()
            self.memcpy_d2h(C.addressof(host), dev, C.sizeof(host))
        finally:
            self.free(dev)
        f = C.cast(host, C.POINTER(C.c_float))
        return [{"id": int(host[2 + r + i]), "dist": float(f[2 + i]), "steps": int(host[2 + 2 * r + i]),
                 "normal": tuple(float(f[2 + 3 * r + 3 * i + k]) for k in range(3))} for i in range(r)]

    def render_host(self, host_ptr: int, w: int, h: int, max_steps: int = 256, camera: S.Camera | None = None,
                    pitch_bytes: int | None = None):
        """What render_thread does with surf->pixels: whole frame into a host surface, synchronous."""
        fc = self.scene.frame_camera(w, h, camera)
        self._check(self._lib.lol_gpu_render_host(self._ctx, C.byref(fc), w, h, max_steps, C.c_void_p(host_ptr),
                                                  pitch_bytes if pitch_bytes is not None else w * 4))

    def render_host_begin(self, w: int, h: int, max_steps: int = 256, camera: S.Camera | None = None):
        """Queue a frame for the host-surface path (two may be in flight, up to four after set_frames_in_flight);
        render_host_end() delivers the oldest."""
        fc = self.scene.frame_camera(w, h, camera)
        self._check(self._lib.lol_gpu_render_host_begin(self._ctx, C.byref(fc), w, h, max_steps))

    def render_host_end(self, host_ptr: int, pitch_bytes: int, w: int, h: int):
        """Deliver the oldest queued frame into a surface of w x h (refused when the frame has another size)."""
        self._check(self._lib.lol_gpu_render_host_end(self._ctx, C.c_void_p(host_ptr), pitch_bytes, w, h))

    def render_host_pending(self) -> int:
        return int(self._lib.lol_gpu_render_host_pending(self._ctx))

    def render_host_pending_size(self):
        w, h = C.c_int(), C.c_int()
        self._check(self._lib.lol_gpu_render_host_pending_size(self._ctx, C.byref(w), C.byref(h)))
        return w.value, h.value

    def render_host_discard(self):
        self._check(self._lib.lol_gpu_render_host_discard(self._ctx))

    def set_pixel_format(self, fmt: "PixelFormat | str | None"):
        """The surface's SDL_PixelFormat (None = XRGB8888); raises for palettised / non-32-bit formats."""
        if isinstance(fmt, str):
            fmt = PIXEL_FORMATS[fmt]
        self._check(self._lib.lol_gpu_set_pixel_format(self._ctx, _ref(fmt)))


    def kernel_key(self) -> str:
        return self._lib.lol_gpu_kernel_key(self._ctx).decode()

    def testing_fail_first_tier(self, n: int):
        """lol_gpu_testing_fail_first_tier: the next n out-of-line first runs of the scene compiler count as failed."""
        self._check(self._lib.lol_gpu_testing_fail_first_tier(self._ctx, n))

    def testing_pixel_cost(self, w: int, n_rows: int):
        """lol_gpu_testing_pixel_cost: the steps every pixel of the repeated view's recording frame ran, (n_rows, w) uint16."""
        import numpy as np
        out = np.zeros((n_rows, w), dtype=np.uint16)
        self._check(self._lib.lol_gpu_testing_pixel_cost(self._ctx, out.ctypes.data_as(_u16p), out.size))
        return out

    def testing_deal(self, cost, w: int, n_rows: int):
        """lol_gpu_testing_deal: the lane table of a w x n_rows frame — rectangles (cost None) or dealt by cost (n_rows, w) uint16 —
        made by the library's own kernels on scratch; flat uint32, 64 entries per wave slot."""
        import numpy as np
        rw, rh = 64, 16                                             # (only to size the buffer: the library checks it against its own)
        out = np.zeros(((w + rw - 1) // rw) * ((n_rows + rh - 1) // rh) * rw * rh, dtype=np.uint32)
        if cost is not None:
            cost = np.ascontiguousarray(cost, dtype=np.uint16)
            assert cost.shape == (n_rows, w)
        self._check(self._lib.lol_gpu_testing_deal(self._ctx, cost.ctypes.data_as(_u16p) if cost is not None else None, w, n_rows,
                                                   out.ctypes.data_as(_u32p), out.size))
        return out

    def testing_sort_tiles(self, cost, order_in, lanes=None):
        """lol_gpu_testing_sort_tiles: one longest-first sort on scratch, everything by launch position.  Returns (order_out,
        keys, starts)."""
        import numpy as np
        cost = np.ascontiguousarray(cost, dtype=np.uint32)
        order_in = np.ascontiguousarray(order_in, dtype=np.uint32)
        n = cost.size
        assert order_in.shape == cost.shape == (n,)
        if lanes is not None:
            lanes = np.ascontiguousarray(lanes, dtype=np.uint32)
            assert lanes.shape == (n * 64,)
        order_out, keys, starts = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(1024, dtype=np.uint32)
        u32 = lambda a: a.ctypes.data_as(_u32p) if a is not None else None      # noqa: E731
        self._check(self._lib.lol_gpu_testing_sort_tiles(self._ctx, u32(cost), u32(order_in), u32(lanes), n, u32(order_out), u32(keys),
                                                         u32(starts)))
        return order_out, keys, starts

    def testing_schedule(self):
        """lol_gpu_testing_schedule: the tables of the repeated view the last frame belongs to, by launch position, or None when that
        frame went out in a fixed order.  Waits for the device; changes nothing."""
        import numpy as np
        fn = self._lib.lol_gpu_testing_schedule
        info = _ScheduleInfo()
        rc = fn(self._ctx, C.byref(info), None, None, None, None, 0, None, 0)
        if rc == -3:                                                # LOL_GPU_ERR_ARG: no table
            return None
        self._check(rc)
        n = int(info.n_tiles)
        t = {k: np.zeros(n, dtype=np.uint32) for k in ("order", "order_before", "keys", "cost")}
        lanes = np.zeros(n * 64, dtype=np.uint32)
        u32 = lambda a: a.ctypes.data_as(_u32p)                     # noqa: E731
        self._check(fn(self._ctx, C.byref(info), u32(t["order"]), u32(t["order_before"]), u32(t["keys"]), u32(t["cost"]), n, u32(lanes),
                       lanes.size))
        return dict({k: int(getattr(info, k)) for k, _ in _ScheduleInfo._fields_}, lanes=lanes, **t)

    def testing_fail_uploads(self, n: int):
        """include/lol_gpu_testing.h: the next n uploads fail at their copy step."""
        self._check(self._lib.lol_gpu_testing_fail_uploads(self._ctx, n))

    def sync(self):
        self._check(self._lib.lol_gpu_sync(self._ctx))

    def malloc(self, nbytes: int) -> int:
        """lol_gpu_malloc: device memory on the renderer's device, for hosts without torch (free() it)."""
        ptr = C.c_void_p()
        self._check(self._lib.lol_gpu_malloc(self._ctx, nbytes, C.byref(ptr)))
        return int(ptr.value or 0)

    def free(self, dev_ptr: int):
        self._check(self._lib.lol_gpu_free(self._ctx, C.c_void_p(dev_ptr)))

    def memcpy_d2h(self, host_ptr: int, dev_ptr: int, nbytes: int):
        """lol_gpu_memcpy_d2h: waits for the renderer's own streams, then copies device memory to the host."""
        self._check(self._lib.lol_gpu_memcpy_d2h(self._ctx, C.c_void_p(host_ptr), C.c_void_p(dev_ptr), nbytes))

    def memcpy_h2d(self, dev_ptr: int, host_ptr: int, nbytes: int):
        """lol_gpu_memcpy_h2d: copies host memory to the device and waits for the copy (the list of a query, for hosts without torch)."""
        self._check(self._lib.lol_gpu_memcpy_h2d(self._ctx, C.c_void_p(dev_ptr), C.c_void_p(host_ptr), nbytes))

    def set_frames_in_flight(self, n: int):
        """Frames launched with stream=None go to n streams of the context in turn (1 = sequential, the default; <= 4):
        consecutive frames overlap.  Give frames that may be in flight together destinations of their own."""
        self._check(self._lib.lol_gpu_set_frames_in_flight(self._ctx, n))

    def frames_in_flight(self) -> int:
        return int(self._lib.lol_gpu_frames_in_flight(self._ctx))

    def next_stream(self) -> int:
        """hipStream_t handle the next frame launched with stream=None goes to (for events around a frame)."""
        return int(self._lib.lol_gpu_next_stream(self._ctx) or 0)

    def kernel_name(self) -> str:
        return self._lib.lol_gpu_kernel_name(self._ctx).decode()

    def set_samples(self, s: int):
        """s x s samples per pixel (1, 2 or 4; 1 = one ray per pixel, the default) from the next frame on: the mean of the
        reference's s w x s h frame's linear colours, in a fixed order (lol_gpu.h).  Set it before prepare() for the scene's own
        kernel to carry the supersampling form; otherwise such frames render on the interpreter (same pixels)."""
        self._check(self._lib.lol_gpu_set_samples(self._ctx, int(s)))

    @property
    def samples(self) -> int:
        return int(self._lib.lol_gpu_samples(self._ctx))

    def set_adaptive_samples(self, contrast: int):
        """Adaptive supersampling from the next frame on: with set_samples(s > 1), only pixels on an edge of the plain frame (an
        object id, or an 8-bit channel more than `contrast` away, among the 8 neighbours) get s x s samples; the others are the
        plain pixel (lol_gpu.h).  0 <= contrast <= 255; -1 turns it off (the default).  Whole frames only."""
        self._check(self._lib.lol_gpu_set_adaptive_samples(self._ctx, int(contrast)))

    @property
    def adaptive_samples(self) -> int:
        """the contrast of adaptive supersampling, or -1 (off)"""
        return int(self._lib.lol_gpu_adaptive_samples(self._ctx))

    def adaptive_refined(self) -> int:
        """how many pixels of the last adaptive frame were refined (waits for that frame)"""
        n = C.c_int64()
        self._check(self._lib.lol_gpu_adaptive_refined(self._ctx, C.byref(n)))
        return int(n.value)

    def adaptive_pass_ms(self) -> tuple:
        """(plain frame, mask and list, refined pixels): milliseconds each pass of the last adaptive frame took on the device"""
        ms = (C.c_float * 3)()
        self._check(self._lib.lol_gpu_adaptive_pass_ms(self._ctx, ms))
        return tuple(float(v) for v in ms)

    def verify_fast_paths(self, k: float = 3.0):
        """([sqrt_pm, sqrt_gs, sqrt_r2], x/k) mismatch counts over all 2^32 float inputs; 0 means proven exact."""
        sq, dv = (C.c_ulonglong * 3)(), C.c_ulonglong()
        self._check(self._lib.lol_gpu_verify_fast_paths(self._ctx, k, sq, C.byref(dv)))
        return list(sq), dv.value

    def verify_smin_no_fixup(self, k: float = 3.0) -> int:
        """Mismatch count of the blend factor without v_div_fixup over all 2^32 inputs; 0 means proven."""
        n = C.c_ulonglong()
        self._check(self._lib.lol_gpu_verify_smin_no_fixup(self._ctx, k, C.byref(n)))
        return n.value

    def verify_gamma_table(self):
        """(mismatches, thresholds): floats in [0, 1] on which gamma through the table and through powf give different channel
        values (0 means proven), and the 257 thresholds of the table."""
        n = C.c_ulonglong()
        t = (C.c_float * 257)()
        self._check(self._lib.lol_gpu_verify_gamma_table(self._ctx, C.byref(n), t))
        return n.value, list(t)

    def powf_batch(self, x_ptr: int, y_ptr: int, out_ptr: int, n: int, stream: int | None = None):
        """out[i] = the kernel's powf(x[i], y[i]) on device arrays (diagnostic for tests)."""
        self._check(self._lib.lol_gpu_powf_batch(self._ctx, C.c_void_p(x_ptr), C.c_void_p(y_ptr), C.c_void_p(out_ptr), n,
                                                 _stream_arg(stream)))

    def sdf_batch(self, pts_ptr: int, dist_ptr: int, id_ptr: int, n: int, stream: int | None = None):
        """dist[i], id[i] = the scene SDF at pts[i] (n x 3 floats), through the SDF code the frames use (diagnostic)."""
        self._check(self._lib.lol_gpu_sdf_batch(self._ctx, C.c_void_p(pts_ptr), C.c_void_p(dist_ptr), C.c_void_p(id_ptr), n,
                                                _stream_arg(stream)))

    # ---- ray queries (include/lol_gpu.h, "Ray queries")
    def set_ray_queries(self, enable: bool):
        """Before prepare(): the scene's own module also carries the query kernel (lol_trace_spec); without it — and until that
        module is ready — queries run on the interpreter's trace_interp.  Same answers either way."""
        self._check(self._lib.lol_gpu_set_ray_queries(self._ctx, 1 if enable else 0))

    @property
    def ray_queries(self) -> bool:
        return bool(self._lib.lol_gpu_ray_queries(self._ctx))

    def trace_kernel_name(self) -> str:
        """the kernel the next trace_rays_into / trace_pixels_into / pick launches"""
        return self._lib.lol_gpu_trace_kernel_name(self._ctx).decode()

    def trace_rays_into(self, rays_ptr: int, n: int, max_steps: int = 256, dist_ptr: int = 0, id_ptr: int = 0, steps_ptr: int = 0,
                        normal_ptr: int = 0, stream: int | None = None):
        """Asynchronously trace n rays (device memory, n x {ox, oy, oz, dx, dy, dz} floats): ray i is the reference's
        get_intersection + get_normal.  dist / id / steps: n elements each, normal: 3 n floats; 0 = not wanted (not all four)."""
        hits = Hits(dist_ptr or None, id_ptr or None, steps_ptr or None, normal_ptr or None)
        self._check(self._lib.lol_gpu_trace_rays(self._ctx, C.c_void_p(rays_ptr), n, max_steps, C.byref(hits), _stream_arg(stream)))

    def trace_pixels_into(self, xy_ptr: int, n: int, w: int, h: int, max_steps: int = 256, dist_ptr: int = 0, id_ptr: int = 0,
                          steps_ptr: int = 0, normal_ptr: int = 0, stream: int | None = None, camera: S.Camera | None = None,
                          frame_camera: S.FrameCamera | None = None):
        """Asynchronously trace the primary rays of n pixels (device memory, n x {x, y} uint32) of the w x h frame under the
        camera: what a frame's lol_gpu_debug planes hold for those pixels, and the normal."""
        fc = self._frame_camera(frame_camera, w, h, camera)
        hits = Hits(dist_ptr or None, id_ptr or None, steps_ptr or None, normal_ptr or None)
        self._check(self._lib.lol_gpu_trace_pixels(self._ctx, C.byref(fc), w, h, max_steps, C.c_void_p(xy_ptr), n, C.byref(hits),
                                                   _stream_arg(stream)))

    def pick(self, x: int, y: int, w: int, h: int, max_steps: int = 256, camera: S.Camera | None = None,
             frame_camera: S.FrameCamera | None = None) -> dict:
        """What is under pixel (x, y) of the w x h frame: {"id", "dist", "steps", "normal"} in host memory (waits)."""
        fc = self._frame_camera(frame_camera, w, h, camera)
        hit = Hit()
        self._check(self._lib.lol_gpu_pick(self._ctx, C.byref(fc), w, h, max_steps, int(x), int(y), C.byref(hit)))
        return {"id": int(hit.id), "dist": float(hit.dist), "steps": int(hit.steps), "normal": tuple(float(v) for v in hit.normal)}

    # ---- shading queries (include/lol_gpu.h, "Shading queries")
    def set_shade_queries(self, enable: bool):
        """Before prepare(): the scene's own module also carries the shading-query kernel (lol_shade_spec); without it — and until
        that module is ready — shading queries run on the interpreter's shade_interp.  Same answers either way."""
        self._check(self._lib.lol_gpu_set_shade_queries(self._ctx, 1 if enable else 0))

    @property
    def shade_queries(self) -> bool:
        return bool(self._lib.lol_gpu_shade_queries(self._ctx))

    def shade_kernel_name(self) -> str:
        """the kernel the next shade_rays_into / shade_pixels_into launches"""
        return self._lib.lol_gpu_shade_kernel_name(self._ctx).decode()

    def shade_rays_into(self, rays_ptr: int, n: int, max_steps: int = 256, rgb_linear_ptr: int = 0, rgb_ptr: int = 0,
                        pixel_ptr: int = 0, dist_ptr: int = 0, id_ptr: int = 0, steps_ptr: int = 0, stream: int | None = None):
        """Asynchronously shade n rays (device memory, n x {ox, oy, oz, dx, dy, dz} floats): ray i is the reference's pixel
        pipeline with the eye at the ray's origin.  rgb_linear / rgb: 3 n floats (before / after gamma), pixel (the context's
        pixel format) / dist / id / steps: n elements each; 0 = not wanted (not all six)."""
        out = Shades(rgb_linear_ptr or None, rgb_ptr or None, pixel_ptr or None, dist_ptr or None, id_ptr or None, steps_ptr or None)
        self._check(self._lib.lol_gpu_shade_rays(self._ctx, C.c_void_p(rays_ptr), n, max_steps, C.byref(out), _stream_arg(stream)))

    def shade_pixels_into(self, xy_ptr: int, n: int, w: int, h: int, max_steps: int = 256, rgb_linear_ptr: int = 0, rgb_ptr: int = 0,
                          pixel_ptr: int = 0, dist_ptr: int = 0, id_ptr: int = 0, steps_ptr: int = 0, stream: int | None = None,
                          camera: S.Camera | None = None, frame_camera: S.FrameCamera | None = None):
        """Asynchronously shade the primary rays of n pixels (device memory, n x {x, y} uint32) of the w x h frame under the
        camera: what a frame and its lol_gpu_debug planes hold for those pixels, and the linear colour."""
        fc = self._frame_camera(frame_camera, w, h, camera)
        out = Shades(rgb_linear_ptr or None, rgb_ptr or None, pixel_ptr or None, dist_ptr or None, id_ptr or None, steps_ptr or None)
        self._check(self._lib.lol_gpu_shade_pixels(self._ctx, C.byref(fc), w, h, max_steps, C.c_void_p(xy_ptr), n, C.byref(out),
                                                   _stream_arg(stream)))

    def light_rays_into(self, rays_ptr: int, n: int, max_steps: int = 256, factors_ptr: int = 0, id_ptr: int = 0, dist_ptr: int = 0,
                        steps_ptr: int = 0, light_stride: int = 0, stream: int | None = None):
        """Asynchronously capture the light passes of n rays (device memory, n x {ox, oy, oz, dx, dy, dz} floats, the rays of
        shade_rays_into): per light l of the scene, in file order, one LightFactor (16 bytes: shadow factor, diffuse and specular
        incidence, shadow steps) at factors[l * light_stride + i] (light_stride = 0: n), and id (needed) / dist / march steps: n
        elements each.  Every factor is the reference's, for every ray: no skip that rests on the look applies.  relight_into makes
        pixels of them under any look."""
        out = LightPasses(factors_ptr or None, light_stride, id_ptr or None, dist_ptr or None, steps_ptr or None)
        self._check(self._lib.lol_gpu_light_rays(self._ctx, C.c_void_p(rays_ptr), n, max_steps, C.byref(out), _stream_arg(stream)))

    def light_pixels_into(self, n: int, w: int, h: int, max_steps: int = 256, xy_ptr: int = 0, factors_ptr: int = 0, id_ptr: int = 0,
                          dist_ptr: int = 0, steps_ptr: int = 0, light_stride: int = 0, stream: int | None = None,
                          camera: S.Camera | None = None, frame_camera: S.FrameCamera | None = None):
        """light_rays_into for the primary rays of n pixels (device memory, n x {x, y} uint32) of the w x h frame under the camera;
        xy_ptr = 0: every pixel of the frame, element i = y w + x, and n must be w h."""
        fc = self._frame_camera(frame_camera, w, h, camera)
        out = LightPasses(factors_ptr or None, light_stride, id_ptr or None, dist_ptr or None, steps_ptr or None)
        self._check(self._lib.lol_gpu_light_pixels(self._ctx, C.byref(fc), w, h, max_steps, C.c_void_p(xy_ptr) if xy_ptr else None, n,
                                                   C.byref(out), _stream_arg(stream)))

    def relight_into(self, look, n: int, factors_ptr: int = 0, id_ptr: int = 0, rgb_linear_ptr: int = 0, rgb_ptr: int = 0,
                     pixel_ptr: int = 0, light_stride: int = 0, stream: int | None = None, held=None):
        """Asynchronously make n elements of captured light passes into colours under `look`: a scene.Scene (flattened here) or a
        ready scene.Program with the prepared scene's geometry (scene.same_geometry; scene.Scene.with_look gives such scenes), or
        None: the prepared scene itself.  Element i is the pixel shade_rays_into gives ray i on a renderer that prepared the look,
        bit for bit: rgb_linear / rgb: 3 n floats, pixel: n elements in this renderer's pixel format; 0 = not wanted (not all
        three).  The look's tables are copied before the call returns.  held (a Scene or a Program; None: the prepared scene): what
        the planes hold after light_update_*_into brought them to another look — the look must then stand where `held` stands
        (lol_gpu_relight_held)."""
        prog = self._look_program(look)
        planes = LightPasses(factors_ptr or None, light_stride, id_ptr or None, None, None)
        out = Relit(rgb_linear_ptr or None, rgb_ptr or None, pixel_ptr or None)
        if held is not None:
            hp = self._look_program(held)
            self._check(self._lib.lol_gpu_relight_held(self._ctx, _ref(prog), C.byref(hp), C.byref(planes), n, C.byref(out),
                                                       _stream_arg(stream)))
            return
        self._check(self._lib.lol_gpu_relight(self._ctx, _ref(prog), C.byref(planes), n, C.byref(out), _stream_arg(stream)))

    def light_update_rays_into(self, look, rays_ptr: int, n: int, march_lights: int = 0, specular_lights: int = 0, factors_ptr: int = 0,
                               id_ptr: int = 0, dist_ptr: int = 0, light_stride: int = 0, stream: int | None = None):
        """Asynchronously bring the planes of a capture of n rays (light_rays_into of the same rays: factors, id and dist, all
        needed) to `look` — as relight_into takes it, but not None: the prepared scene's geometry with other light points or
        shininesses (scene.Scene.with_lighting) — without the primary march (lol_gpu_light_update_rays).  Bit l of march_lights:
        light l's whole factor is computed again; bit l of specular_lights (and not of march_lights): its specular incidence alone,
        with no shadow march.  scene.light_changes gives both masks.  Resolve with relight_into(..., held=look)."""
        prog = self._look_program(look)
        planes = LightPasses(factors_ptr or None, light_stride, id_ptr or None, dist_ptr or None, None)
        self._check(self._lib.lol_gpu_light_update_rays(self._ctx, _ref(prog), C.c_void_p(rays_ptr), n, int(march_lights),
                                                        int(specular_lights), C.byref(planes), _stream_arg(stream)))

    def light_update_pixels_into(self, look, n: int, w: int, h: int, march_lights: int = 0, specular_lights: int = 0, xy_ptr: int = 0,
                                 factors_ptr: int = 0, id_ptr: int = 0, dist_ptr: int = 0, light_stride: int = 0,
                                 stream: int | None = None, camera: S.Camera | None = None, frame_camera: S.FrameCamera | None = None):
        """light_update_rays_into for the planes of light_pixels_into: the same n, w, h, camera and xy_ptr (0: every pixel)."""
        fc = self._frame_camera(frame_camera, w, h, camera)
        prog = self._look_program(look)
        planes = LightPasses(factors_ptr or None, light_stride, id_ptr or None, dist_ptr or None, None)
        self._check(self._lib.lol_gpu_light_update_pixels(self._ctx, _ref(prog), C.byref(fc), w, h, C.c_void_p(xy_ptr) if xy_ptr else None,
                                                          n, int(march_lights), int(specular_lights), C.byref(planes), _stream_arg(stream)))

    def light_views_into(self, cameras, cameras_per_view: int, w: int, h: int, samples: int = 1, max_steps: int = 256,
                         factors_ptr: int = 0, id_ptr: int = 0, dist_ptr: int = 0, steps_ptr: int = 0, light_stride: int = 0,
                         stream: int | None = None):
        """Asynchronously capture the light passes of every LEAF of len(cameras) / cameras_per_view views of w x h with samples x
        samples samples per pixel (lol_gpu_light_views): camera r's samples x w by samples x h sample grid is light_pixels_into of
        that frame, into the planes r samples^2 w h elements further on — one capture launch per camera.  Element
        ((v K + k) s h + Y) s w + X is sample column X, sample row Y under cameras[v K + k]; N = len(cameras) s^2 w h elements,
        light_stride = 0: N.  cameras: scene.Camera or ready scene.FrameCamera objects.  relight_views_into makes the averaged
        pixels of any look from them."""
        cams = list(cameras)
        k = int(cameras_per_view)
        if k < 1 or len(cams) % k:
            raise ValueError("light_views_into: len(cameras) must be a multiple of cameras_per_view")
        arr = self._camera_array(cams, w, h)
        out = LightPasses(factors_ptr or None, light_stride, id_ptr or None, dist_ptr or None, steps_ptr or None)
        self._check(self._lib.lol_gpu_light_views(self._ctx, arr, len(cams) // k, k, w, h, int(samples), max_steps, C.byref(out),
                                                  _stream_arg(stream)))

    def relight_views_into(self, look, n_views: int, cameras_per_view: int, w: int, h: int, samples: int = 1, factors_ptr: int = 0,
                           id_ptr: int = 0, rgb_linear_ptr: int = 0, rgb_ptr: int = 0, pixel_ptr: int = 0, light_stride: int = 0,
                           stream: int | None = None):
        """Asynchronously make the n_views averaged views of w x h under `look` (as relight_into takes it: a scene.Scene, a ready
        scene.Program, or None) from the planes of light_views_into (lol_gpu_relight_views): per leaf relight_into's linear colour,
        per camera the tree mean over its samples x samples leaves, then the tree mean over the cameras_per_view cameras, then gamma
        and this renderer's pixel format — the supersampled frame, the blend, or the supersampled blend of a renderer that prepared
        the look, bit for bit, in one copy and one launch.  rgb_linear / rgb: 3 floats per pixel, pixel: one element, dense over
        [view, y, x]; 0 = not wanted (not all three).  Planes that a light update brought to another look: relight_views_held_into."""
        prog = self._look_program(look)
        planes = LightPasses(factors_ptr or None, light_stride, id_ptr or None, None, None)
        out = Relit(rgb_linear_ptr or None, rgb_ptr or None, pixel_ptr or None)
        self._check(self._lib.lol_gpu_relight_views(self._ctx, _ref(prog), C.byref(planes), int(n_views), int(cameras_per_view), w, h,
                                                    int(samples), C.byref(out), _stream_arg(stream)))

    def relight_views_held_into(self, look, held, n_views: int, cameras_per_view: int, w: int, h: int, samples: int = 1,
                                factors_ptr: int = 0, id_ptr: int = 0, rgb_linear_ptr: int = 0, rgb_ptr: int = 0, pixel_ptr: int = 0,
                                light_stride: int = 0, stream: int | None = None):
        """relight_views_into for planes that hold `held` (a Scene or a Program; None: the prepared scene, which is
        relight_views_into itself) after light_update_pixels_into brought them there record by record: the look must stand where
        `held` stands (lol_gpu_relight_views_held).  What relight_into's held= is to relight_into."""
        prog = self._look_program(look)
        hp = self._look_program(held)
        planes = LightPasses(factors_ptr or None, light_stride, id_ptr or None, None, None)
        out = Relit(rgb_linear_ptr or None, rgb_ptr or None, pixel_ptr or None)
        self._check(self._lib.lol_gpu_relight_views_held(self._ctx, _ref(prog), _ref(hp), C.byref(planes), int(n_views),
                                                         int(cameras_per_view), w, h, int(samples), C.byref(out), _stream_arg(stream)))

    # ---- scene light passes (include/lol_gpu.h, "Scene light passes")
    def light_scene_rays_into(self, scenes, rays_ptr: int, n: int, list_stride: int = 0, max_steps: int = 256, factors_ptr: int = 0,
                              id_ptr: int = 0, dist_ptr: int = 0, steps_ptr: int = 0, light_stride: int = 0, stream: int | None = None):
        """Asynchronously capture the light passes of n rays under EACH of len(scenes) scenes of the prepared scene's structure
        (lol_gpu_light_scene_rays), in one launch: element (r, i), at index e = r n + i of id / dist / steps and at
        factors[l * light_stride + e] (light_stride = 0: len(scenes) n), is what light_rays_into writes for ray i of record r after
        prepare(scenes[r]).  scenes and list_stride as trace_scene_rays_into takes them."""
        items = list(scenes)
        keep, progs, _ = self._scene_records("light_scene_rays_into", items)
        out = LightPasses(factors_ptr or None, light_stride, id_ptr or None, dist_ptr or None, steps_ptr or None)
        rays = C.cast(C.c_void_p(rays_ptr), _P(C.c_float)) if rays_ptr else None
        self._check(self._lib.lol_gpu_light_scene_rays(self._ctx, progs, len(items), rays, n, list_stride, max_steps, C.byref(out),
                                                       _stream_arg(stream)))
        del keep

    def light_scene_pixels_into(self, scenes, n: int, w: int, h: int, list_stride: int = 0, max_steps: int = 256, xy_ptr: int = 0,
                                factors_ptr: int = 0, id_ptr: int = 0, dist_ptr: int = 0, steps_ptr: int = 0, light_stride: int = 0,
                                stream: int | None = None, cameras=None):
        """light_scene_rays_into for the primary rays of n pixels of the w x h frame under each record's own scene and camera
        (lol_gpu_light_scene_pixels); xy_ptr = 0: every pixel of the frame, element (r, y w + x), and n must be w h — with equal
        scenes the planes of light_views_into.  cameras: as render_scene_views_into takes them; None: every scene's own."""
        items = list(scenes)
        keep, progs, arr = self._scene_records("light_scene_pixels_into", items, cameras, (w, h))
        out = LightPasses(factors_ptr or None, light_stride, id_ptr or None, dist_ptr or None, steps_ptr or None)
        xy = C.cast(C.c_void_p(xy_ptr), _u32p) if xy_ptr else None
        self._check(self._lib.lol_gpu_light_scene_pixels(self._ctx, arr, progs, len(items), w, h, max_steps, xy, n, list_stride,
                                                         C.byref(out), _stream_arg(stream)))
        del keep

    def relight_scenes_into(self, scenes, looks=None, n: int = 0, factors_ptr: int = 0, id_ptr: int = 0, rgb_linear_ptr: int = 0,
                            rgb_ptr: int = 0, pixel_ptr: int = 0, light_stride: int = 0, stream: int | None = None):
        """Asynchronously make the len(scenes) n elements of the planes of light_scene_*_into into colours, record r under looks[r]
        (lol_gpu_relight_scenes): scenes says what the planes hold, looks[r] (a scene.Scene or scene.Program with scenes[r]'s geometry,
        light points and shininess: scene.Scene.with_look) the look of record r; looks = None: the scenes' own.  Element (r, i) is
        relight_into's on a renderer that prepared scenes[r]; outputs dense over r n + i, as relight_into's."""
        items = list(scenes)
        keep, progs, _ = self._scene_records("relight_scenes_into", items)
        keep_looks, look_progs = self._record_looks("relight_scenes_into", looks, len(items))
        planes = LightPasses(factors_ptr or None, light_stride, id_ptr or None, None, None)
        out = Relit(rgb_linear_ptr or None, rgb_ptr or None, pixel_ptr or None)
        self._check(self._lib.lol_gpu_relight_scenes(self._ctx, progs, look_progs, len(items), C.byref(planes), n, C.byref(out),
                                                     _stream_arg(stream)))
        del keep, keep_looks

    # ---- relit scene views (include/lol_gpu.h, "Relit scene views")
    def relight_scene_views_into(self, scenes, looks=None, n_views: int = 0, cameras_per_view: int = 1, w: int = 0, h: int = 0,
                                 samples: int = 1, factors_ptr: int = 0, id_ptr: int = 0, rgb_linear_ptr: int = 0, rgb_ptr: int = 0,
                                 pixel_ptr: int = 0, light_stride: int = 0, stream: int | None = None):
        """Asynchronously make the n_views averaged views of w x h from the leaves light_scene_pixels_into captured over
        len(scenes) = n_views cameras_per_view records of the samples w x samples h grid (lol_gpu_relight_scene_views): per leaf
        relight_scenes_into's linear colour under looks[r], per record the tree mean over its samples x samples leaves, then the tree
        mean over the view's cameras_per_view records, then gamma and this renderer's pixel format — the pixel and rgb of
        render_scene_views_into(cameras, looks, ..., cameras_per_view, samples=samples), bit for bit, in one copy and one launch.
        scenes says what the planes hold; looks as relight_scenes_into takes them (None: the scenes' own).  rgb_linear / rgb: 3 floats
        per pixel, pixel: one element, dense over [view, y, x]; 0 = not wanted (not all three)."""
        items = list(scenes)
        k = int(cameras_per_view)
        if len(items) != int(n_views) * k:
            raise ValueError("relight_scene_views_into: len(scenes) must be n_views * cameras_per_view")
        keep, progs, _ = self._scene_records("relight_scene_views_into", items)
        keep_looks, look_progs = self._record_looks("relight_scene_views_into", looks, len(items))
        planes = LightPasses(factors_ptr or None, light_stride, id_ptr or None, None, None)
        out = Relit(rgb_linear_ptr or None, rgb_ptr or None, pixel_ptr or None)
        self._check(self._lib.lol_gpu_relight_scene_views(self._ctx, progs, look_progs, C.byref(planes), int(n_views), k, w, h,
                                                          int(samples), C.byref(out), _stream_arg(stream)))
        del keep, keep_looks

    def set_cull(self, enable: bool):
        """Exact bounding-sphere culling of top-level objects in the specialised kernel; takes effect at the next prepare()."""
        self._check(self._lib.lol_gpu_set_cull(self._ctx, 1 if enable else 0))

    def set_tile_order(self, order):
        """0 / False / "rows", 1 / True / "cols", 2 / "auto" (the library times both fixed orders on the first frames of a scene
        and size and keeps the faster), 3 / "lpt" (the default: a repeated view is scheduled by what the frame before cost, any
        other frame runs in auto's fixed order) — same pixels either way (lol_gpu.h)."""
        self._check(self._lib.lol_gpu_set_tile_order(self._ctx, _tile_order_arg(order)))

    def tile_order(self) -> dict:
        """lol_gpu_tile_order: mode asked for, order in use, whether trials are still running, the two typical trial frames."""
        info = TileOrderInfo()
        self._check(self._lib.lol_gpu_tile_order(self._ctx, C.byref(info)))
        names = {TILES_ROWS: "rows", TILES_COLS: "cols", TILES_AUTO: "auto", TILES_LPT: "lpt"}
        return {"mode": names[info.mode], "order": names[info.order], "deciding": bool(info.deciding), "decisions": info.decisions,
                "trial_ms": {"rows": round(info.rows_ms, 4), "cols": round(info.cols_ms, 4)}}

    def set_miss_skip(self, enable: bool):
        self._check(self._lib.lol_gpu_set_miss_skip(self._ctx, 1 if enable else 0))

    def set_exact_skips(self, mask: int):
        """bit 0 escaped waves, bit 1 zero incidence, bit 2 settled shadows."""
        self._check(self._lib.lol_gpu_set_exact_skips(self._ctx, mask))

    def miss_skip_active(self) -> int:
        """bit 0: escaped-wave skip active; bit 1: zero-incidence shadow skip active."""
        return int(self._lib.lol_gpu_miss_skip_active(self._ctx))

    def specialize_log(self) -> str:
        return self._lib.lol_gpu_specialize_log(self._ctx).decode(errors="replace")

    # render_destroy (renderer.h:26)
    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.lol_gpu_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiRenderer:
    """ctypes mirror of the lol_gpu_multi_* entry points: one frame over several devices of this process,
    parts exchanged with RCCL and assembled on devices[0] (include/lol_gpu.h)."""

    def __init__(self, devices, specialize: bool | int = True):
        self._lib = gpu_lib()
        self._m = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        st = self._lib.lol_gpu_multi_create(arr, len(devices), C.byref(self._m))
        if st != LOL_GPU_OK:
            self._m = C.c_void_p()
            raise GpuError(st, f"lol_gpu_multi_create(devices={list(devices)}) failed")
        for i in range(len(devices)):
            self._lib.lol_gpu_set_specialize(self._lib.lol_gpu_multi_context(self._m, i), int(specialize))
        self.scene = None
        self.program = None

    def _check(self, st: int):
        if st != LOL_GPU_OK:
            raise GpuError(st, self._lib.lol_gpu_multi_error(self._m).decode())

    def prepare(self, scene: S.Scene, wait: bool = True):
        self.scene = scene
        self.program = scene.flatten()
        self._check(self._lib.lol_gpu_multi_upload_program(self._m, C.byref(self.program)))
        if wait:
            self._check(self._lib.lol_gpu_multi_specialize_wait(self._m))

    def set_band_rows(self, band_rows: int):
        self._check(self._lib.lol_gpu_multi_set_band_rows(self._m, band_rows))

    def set_parts_per_device(self, parts: int):
        self._check(self._lib.lol_gpu_multi_set_parts_per_device(self._m, parts))

    def set_host_via_root(self, enable: bool):
        self._check(self._lib.lol_gpu_multi_set_host_via_root(self._m, 1 if enable else 0))

    def testing_root_stride(self, stride: int):
        """include/lol_gpu_testing.h: every stride-th part gets the root's band height, even on one device."""
        self._check(self._lib.lol_gpu_multi_testing_root_stride(self._m, stride))

    def testing_force_copier_threads(self, enable: bool):
        """include/lol_gpu_testing.h: host-surface copies through the per-device threads even with one device."""
        self._check(self._lib.lol_gpu_multi_testing_force_copier_threads(self._m, 1 if enable else 0))

    def set_root_band_rows(self, rows: int):
        """Band height of the root's parts (0 = like the others): its smaller share of the rows."""
        self._check(self._lib.lol_gpu_multi_set_root_band_rows(self._m, rows))

    def set_pixel_format(self, fmt):
        if isinstance(fmt, str):
            fmt = PIXEL_FORMATS[fmt]
        self._check(self._lib.lol_gpu_multi_set_pixel_format(self._m, _ref(fmt)))

    def set_tile_order(self, order):
        self._check(self._lib.lol_gpu_multi_set_tile_order(self._m, _tile_order_arg(order)))

    def set_samples(self, s: int):
        """Renderer.set_samples on every device (bands are output rows: the exchange is unchanged)."""
        self._check(self._lib.lol_gpu_multi_set_samples(self._m, int(s)))

    def tile_order(self, i: int = 0) -> dict:
        """lol_gpu_tile_order of device index i's context."""
        info = TileOrderInfo()
        st = self._lib.lol_gpu_tile_order(self._lib.lol_gpu_multi_context(self._m, i), C.byref(info))
        if st != LOL_GPU_OK:
            raise GpuError(st, "lol_gpu_tile_order")
        names = {TILES_ROWS: "rows", TILES_COLS: "cols", TILES_AUTO: "auto", TILES_LPT: "lpt"}
        return {"mode": names[info.mode], "order": names[info.order], "deciding": bool(info.deciding), "decisions": info.decisions,
                "trial_ms": {"rows": round(info.rows_ms, 4), "cols": round(info.cols_ms, 4)}}

    def render_into(self, dst_ptr: int, w: int, h: int, max_steps: int = 256, camera: S.Camera | None = None,
                    pitch_bytes: int | None = None, frame_camera: S.FrameCamera | None = None):
        fc = frame_camera if frame_camera is not None else self.scene.frame_camera(w, h, camera)
        self._check(self._lib.lol_gpu_multi_render_device(self._m, C.byref(fc), w, h, max_steps, C.c_void_p(dst_ptr),
                                                          pitch_bytes if pitch_bytes is not None else w * 4))

    def render_host(self, host_ptr: int, w: int, h: int, max_steps: int = 256, camera: S.Camera | None = None,
                    pitch_bytes: int | None = None):
        fc = self.scene.frame_camera(w, h, camera)
        self._check(self._lib.lol_gpu_multi_render_host(self._m, C.byref(fc), w, h, max_steps, C.c_void_p(host_ptr),
                                                        pitch_bytes if pitch_bytes is not None else w * 4))

    def sync(self):
        self._check(self._lib.lol_gpu_multi_sync(self._m))

    def kernel_name(self, i: int = 0) -> str:
        return self._lib.lol_gpu_kernel_name(self._lib.lol_gpu_multi_context(self._m, i)).decode()

    def close(self):
        if getattr(self, "_m", None) and self._m.value:
            self._lib.lol_gpu_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
