"""Shading queries, the part that needs no GPU: the symbols, the scene compiler's source with and without lol_gpu_set_shade_queries,
the gfx950 code object, and scene.panorama_rays."""
import math
import re

import numpy as np
import pytest

import scene_shapes as C
from loltracer_amd import gpu
from loltracer_amd import scene as S
from test_rays_cabi import ROOT, kernel_notes, read

KERNEL = "lol_shade_spec"
HEAD = "void %s(const lol::Launch L, const lol::ShadeQuery Q) {" % KERNEL
INCLUDE = '#include "lol_kernel_shade.h"\n'
EXPORTED = ("lol_gpu_shade_rays", "lol_gpu_shade_pixels", "lol_gpu_set_shade_queries", "lol_gpu_shade_queries", "lol_gpu_memcpy_h2d")
DIAG = ("lol_gpu_shade_kernel_name", "lol_gpu_compile_offline_shade")
OTHERS = ("view_blends", "samples", "view_batches", "view_samples", "view_blend_samples", "ray_queries")


def test_the_symbols_exist():
    lib = gpu.gpu_lib()
    hdr, diag = read(ROOT + "/include/lol_gpu.h"), read(ROOT + "/include/lol_gpu_diag.h")
    for name in EXPORTED:
        assert getattr(lib, name) is not None and name in gpu.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % name, hdr), name
    for name in DIAG:
        assert getattr(lib, name) is not None and name in gpu.DIAG_SYMBOLS and re.search(r"\b%s\(" % name, diag), name
    assert int(re.search(r"#define\s+LOL_GPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6 == lib.lol_gpu_abi_version()      # new entry points only
    # refusals that need no device: no context
    out = gpu.Shades(8, 8, 8, 8, 8, 8)
    assert lib.lol_gpu_shade_rays(None, 8, 1, 256, out, None) == -3
    assert lib.lol_gpu_shade_pixels(None, None, 8, 8, 256, 8, 1, out, None) == -3
    assert lib.lol_gpu_set_shade_queries(None, 1) == -3 and lib.lol_gpu_shade_queries(None) == -3
    assert lib.lol_gpu_shade_kernel_name(None) == b""
    assert lib.lol_gpu_memcpy_h2d(None, 8, 8, 4) == -3
    for method in ("set_shade_queries", "shade_queries", "shade_kernel_name", "shade_rays_into", "shade_pixels_into", "memcpy_h2d"):
        assert hasattr(gpu.Renderer, method), method
    for text in ("per-light shadow-factor output", "lol_gpu_multi_", "rays in host memory", "a shading pick", "renderer.h protocol",
                 "camera.point = ro", "the leaves of that pixel's tree"):
        assert text in hdr, text                     # what is out of scope, whose eye a ray's is, and what the sample rays are


def modules_beside(prog, tmp_path):
    """{switch: a function that compiles the module with that switch (or all of them) and without shading queries}"""
    return {
        "none": lambda p: gpu.compile_offline(prog, p),
        "view_blends": lambda p: gpu.compile_offline_view_blends(prog, p),
        "samples": lambda p: gpu.compile_offline_samples(prog, p, 2),
        "view_batches": lambda p: gpu.compile_offline_views(prog, p),
        "view_samples": lambda p: gpu.compile_offline_view_samples(prog, p),
        "view_blend_samples": lambda p: gpu.compile_offline_view_blend_samples(prog, p),
        "ray_queries": lambda p: gpu.compile_offline_rays(prog, p),
        "all": lambda p: gpu.compile_offline_rays(prog, p, view_blends=True, samples=True, view_batches=True, view_samples=True,
                                                  view_blend_samples=True),
    }


def others_of(switch):
    return {} if switch == "none" else {k: True for k in OTHERS} if switch == "all" else {switch: True}


def test_the_switch_beside_every_other_switch(tmp_path, scenes):
    """Without the switch a module — alone, beside each other switch and beside all of them — has the source text, the code object
    and the code key it has without the feature; with it, it is THAT module with lol_shade_spec appended last, it compiles for
    gfx950, and its key differs."""
    prog = scenes["scene4"].flatten()
    lib = gpu.gpu_lib()
    assert lib.lol_gpu_compile_offline_shade(None, b"gfx950", b"", 0, 1, 0, 0, None, 0) == -3
    assert lib.lol_gpu_compile_offline_shade(prog, b"gfx950", b"", 0, 1, 64, 0, None, 0) == -3
    assert lib.lol_gpu_compile_offline_shade(prog, b"gfx950", b"", 0, 1, -1, 0, None, 0) == -3
    for switch, compile_base in modules_beside(prog, tmp_path).items():
        base_path, on, off = (str(tmp_path / (k + "_" + switch)) for k in ("base", "on", "off"))
        compile_base(base_path)
        gpu.compile_offline_shade(prog, off, enable=False, **others_of(switch))
        for ext in (".hip", ".co"):
            assert read(off + ext, "rb") == read(base_path + ext, "rb"), (switch, ext)
        base = read(base_path + ".hip")
        assert KERNEL not in base and "shade_rays" not in base and "ShadeQuery" not in base, switch
        gpu.compile_offline_shade(prog, on, **others_of(switch))          # (raises unless it compiled)
        src = read(on + ".hip")
        assert src.startswith(base), switch                                 # appended after everything else
        tail = src[len(base):]
        assert tail.startswith(INCLUDE) and tail.count(HEAD) == 1 and src.count(KERNEL) == 1 and src.rstrip().endswith("}"), switch
        assert "lol::shade_rays<false>(exact, exact, false, L, Q, lds)" in tail and "lol::stage_common(L, lds)" in tail, switch
        assert not re.search(r"void lol_render_spec\w*\(", tail) and "shade_pixel" not in tail, switch      # no frame kernel comes with it
        assert kernel_notes(on + ".co").keys() == kernel_notes(base_path + ".co").keys() | {KERNEL}, switch
        assert gpu.code_key(read(on + ".co", "rb")) != gpu.code_key(read(base_path + ".co", "rb")) == gpu.code_key(read(off + ".co", "rb")), switch
    fast = str(tmp_path / "fast")
    gpu.compile_offline_shade(prog, fast, assume_fast=True)
    tail = read(fast + ".hip").split(INCLUDE)[1]
    assert "lol::SpecSdfFast fast;" in tail and "lol::shade_rays<false>(fast, exact, true, L, Q, lds)" in tail


def test_every_example_scene_and_large_tables(tmp_path, scenes):
    for name in ("scene", "scene2", "scene3"):
        prog = scenes[name].flatten()
        plain, off, on = (str(tmp_path / (name + k)) for k in ("_plain", "_off", "_on"))
        gpu.compile_offline(prog, plain)
        gpu.compile_offline_shade(prog, off, enable=False)
        gpu.compile_offline_shade(prog, on)
        assert read(off + ".hip", "rb") == read(plain + ".hip", "rb") and read(off + ".co", "rb") == read(plain + ".co", "rb"), name
        assert KERNEL in kernel_notes(on + ".co") and KERNEL not in kernel_notes(plain + ".co"), name
    # tables beyond the LDS limit are read from global memory: the other instantiation, no staging
    big = [f.shape for f in C.FORMS if f.name == "tables-global"][0]
    base = str(tmp_path / "tables_global")
    gpu.compile_offline_shade(C.scene_of(big).flatten(), base)
    tail = read(base + ".hip").split(INCLUDE)[1]
    assert "lol::shade_rays<true>(" in tail and "stage_common" not in tail
    assert KERNEL in kernel_notes(base + ".co")


def test_both_tiers_of_a_mid_size_scene_carry_it(tmp_path):
    prog = C.scene_of(C.MID).flatten()
    assert 256 < prog.n_ops <= 1024
    for form, out_of_line in ((1, True), (2, False)):
        base = str(tmp_path / ("tier%d" % form))
        gpu.compile_offline_shade(prog, base, form=form)
        src = read(base + ".hip")
        assert ("SdfOut" in src) == out_of_line, form
        assert src.count("void %s(" % KERNEL) == 1 and src.count(INCLUDE) == 1, form
        assert KERNEL in kernel_notes(base + ".co"), form
    with pytest.raises(gpu.GpuError) as e:
        gpu.compile_offline_shade(prog, str(tmp_path / "bad"), form=3)
    assert e.value.status == -3


def test_panorama_rays(scenes):
    cam = scenes["scene4"].camera
    for w, h in ((9, 5), (8, 4), (1, 1)):
        rays = S.panorama_rays(cam, w, h)
        assert rays.dtype == np.float32 and rays.shape == (h * w, 6)
        assert (rays[:, :3] == np.array(cam.point.tuple(), np.float32)).all()
        rd = rays[:, 3:].astype(np.float64).reshape(h, w, 3)
        assert np.abs(np.linalg.norm(rd, axis=-1) - 1).max() < 2e-7            # unit directions, to within float rounding
        fc = scenes["scene4"].frame_camera(w, h)
        d, right, up = (np.array(v.tuple(), np.float64) / np.linalg.norm(v.tuple()) for v in (fc.dir, fc.right, fc.up))
        lon = np.arctan2(rd @ right, rd @ d)
        lat = np.arcsin(np.clip(rd @ up, -1, 1))
        want_lon = ((np.arange(w) + .5) / w * 2 - 1) * math.pi
        want_lat = (.5 - (np.arange(h) + .5) / h) * math.pi
        assert np.abs(lon - want_lon[None, :]).max() < 1e-6 and np.abs(lat - want_lat[:, None]).max() < 1e-6
        # the first and last columns lie half a pixel of longitude either side of the seam at +-pi
        assert abs(lon[0, 0] + math.pi - math.pi / w) < 1e-6 and abs(lon[0, -1] - math.pi + math.pi / w) < 1e-6
        if w % 2 and h % 2:                                                    # odd both ways: the centre pixel looks where the camera does
            assert np.abs(rd[h // 2, w // 2] - d).max() < 2e-7
    with pytest.raises(ValueError):
        S.panorama_rays(cam, 0, 4)
