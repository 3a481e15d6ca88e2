"""Relit views at the C ABI: the two symbols, what can be refused without a device, and the Python signatures against the header."""
import ctypes as C
import inspect
import os
import re

from loltracer_amd import gpu, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lol_gpu_light_views", "lol_gpu_relight_views")


def test_the_two_symbols_exist_and_refuse_a_null_context():
    lib = gpu.gpu_lib()
    for name in SYMBOLS:
        assert name in gpu.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    passes, relit, fc = gpu.LightPasses(), gpu.Relit(), S.FrameCamera()
    assert lib.lol_gpu_light_views(None, C.byref(fc), 1, 1, 8, 8, 2, 256, C.byref(passes), None) == -3
    assert lib.lol_gpu_relight_views(None, None, C.byref(passes), 1, 1, 8, 8, 2, C.byref(relit), None) == -3


def declaration(name):
    """the parameter (type, name) pairs of `name` as include/lol_gpu.h declares it"""
    hdr = open(os.path.join(ROOT, "include", "lol_gpu.h")).read()
    text = re.search(r"^int\s+%s\((.*?)\);" % name, hdr, flags=re.S | re.M).group(1)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = []
    for p in text.split(","):
        m = re.match(r"\s*(.*?)(\w+)\s*$", p, flags=re.S)
        out.append((" ".join(m.group(1).split()), m.group(2)))
    return out


def test_the_header_declares_what_python_calls():
    vp, i = C.c_void_p, C.c_int
    want = {
        "lol_gpu_light_views": [("lol_gpu*", "ctx", vp), ("const lol_frame_camera*", "cams", C.POINTER(S.FrameCamera)), ("int", "n_views", i),
                                ("int", "cams_per_view", i), ("int", "w", i), ("int", "h", i), ("int", "samples", i), ("int", "max_steps", i),
                                ("const lol_gpu_light_passes*", "out", C.POINTER(gpu.LightPasses)), ("void*", "stream", vp)],
        "lol_gpu_relight_views": [("lol_gpu*", "ctx", vp), ("const lol_program*", "look", C.POINTER(S.Program)),
                                  ("const lol_gpu_light_passes*", "in", C.POINTER(gpu.LightPasses)), ("int", "n_views", i),
                                  ("int", "cams_per_view", i), ("int", "w", i), ("int", "h", i), ("int", "samples", i),
                                  ("const lol_gpu_relit*", "out", C.POINTER(gpu.Relit)), ("void*", "stream", vp)],
    }
    lib = gpu.gpu_lib()
    for name, params in want.items():
        assert declaration(name) == [(t, n) for t, n, _ in params], name
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [c for _, _, c in params] and fn.restype is C.c_int, name
    hdr = open(os.path.join(ROOT, "include", "lol_gpu.h")).read()
    assert re.search(r"#define\s+LOL_GPU_ABI_VERSION\s+6\b", hdr)                 # nothing existing changed: the version stays


def test_the_renderer_methods_have_the_documented_signatures():
    lv = inspect.signature(gpu.Renderer.light_views_into)
    assert list(lv.parameters) == ["self", "cameras", "cameras_per_view", "w", "h", "samples", "max_steps", "factors_ptr", "id_ptr",
                                   "dist_ptr", "steps_ptr", "light_stride", "stream"]
    assert (lv.parameters["samples"].default, lv.parameters["max_steps"].default, lv.parameters["light_stride"].default) == (1, 256, 0)
    rv = inspect.signature(gpu.Renderer.relight_views_into)
    assert list(rv.parameters) == ["self", "look", "n_views", "cameras_per_view", "w", "h", "samples", "factors_ptr", "id_ptr",
                                   "rgb_linear_ptr", "rgb_ptr", "pixel_ptr", "light_stride", "stream"]
    assert rv.parameters["samples"].default == 1 and rv.parameters["stream"].default is None


def test_the_resolve_kernel_is_not_handed_to_the_scene_compiler():
    """ahead of time and scene-independent, like relight_rays: no scene module includes the new header, and there is no new switch"""
    src = open(os.path.join(ROOT, "loltracer_amd", "csrc", "lol_codegen.hip")).read()
    assert "lol_kernel_light_views.h" not in src and "relight_views" not in src
    mk = open(os.path.join(ROOT, "loltracer_amd", "csrc", "Makefile")).read()
    kernel_hdrs = re.search(r"^KERNEL_HDRS := (.*)$", mk, flags=re.M).group(1).split()
    assert "lol_kernel_light_views.h" not in kernel_hdrs
    assert "lol_kernel_light_views.h" in re.search(r"^AOT_HDRS := (.*)$", mk, flags=re.M).group(1).split()
