"""Light passes and relighting at the C ABI: the three symbols, the struct layouts, and what can be refused without a device."""
import ctypes as C
import os
import re

from loltracer_amd import gpu, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lol_gpu_light_rays", "lol_gpu_light_pixels", "lol_gpu_relight")


def test_the_three_symbols_exist_and_refuse_a_null_context():
    lib = gpu.gpu_lib()
    for name in SYMBOLS:
        assert name in gpu.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    passes, relit, fc = gpu.LightPasses(), gpu.Relit(), S.FrameCamera()
    assert lib.lol_gpu_light_rays(None, None, 0, 256, C.byref(passes), None) == -3
    assert lib.lol_gpu_light_pixels(None, C.byref(fc), 8, 8, 256, None, 64, C.byref(passes), None) == -3
    assert lib.lol_gpu_relight(None, None, C.byref(passes), 0, C.byref(relit), None) == -3


def test_struct_sizes_match_the_header():
    assert C.sizeof(gpu.LightFactor) == 16
    assert [f for f, _ in gpu.LightFactor._fields_] == ["shadow", "diffuse_incidence", "specular_incidence", "shadow_steps"]
    vp = C.sizeof(C.c_void_p)
    assert C.sizeof(gpu.LightPasses) == 4 * vp + C.sizeof(C.c_size_t) and gpu.LightPasses.light_stride.offset == vp
    assert C.sizeof(gpu.Relit) == 3 * vp
    hdr = open(os.path.join(ROOT, "include", "lol_gpu.h")).read()
    for struct, mirror in (("lol_gpu_light_factor", gpu.LightFactor), ("lol_gpu_light_passes", gpu.LightPasses), ("lol_gpu_relit", gpu.Relit)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"\b([a-z_]+)\s*(?:,|$)", decl.strip())]
        assert names == [f for f, _ in mirror._fields_], struct


def test_the_kernels_header_is_not_handed_to_the_scene_compiler():
    """the capture is the interpreter's alone: no scene module includes lol_kernel_light.h, and no module switch names it"""
    src = open(os.path.join(ROOT, "loltracer_amd", "csrc", "lol_codegen.hip")).read()
    assert "lol_kernel_light.h" not in src and "light_interp" not in src
    assert not any("light" in s for s in gpu.MODULE_SWITCHES)
