"""Scene light passes (lol_gpu_light_scene_rays, lol_gpu_light_scene_pixels, lol_gpu_relight_scenes), the part that needs no GPU: the
C ABI's symbols and the refusal a NULL context gets, the header's words on the contract — in the order the header makes them —, the
Python mirror, and that the feature is neither a module switch nor known to the scene compiler."""
import inspect
import os
import re

from loltracer_amd import gpu
from test_rays_cabi import ROOT, read

EXPORTED = ("lol_gpu_light_scene_rays", "lol_gpu_light_scene_pixels", "lol_gpu_relight_scenes")
METHODS = ("light_scene_rays_into", "light_scene_pixels_into", "relight_scenes_into")
SWITCHES = ("samples", "view_batches", "view_samples", "view_blends", "view_blend_samples", "ray_queries", "shade_queries")
CSRC = os.path.join(ROOT, "loltracer_amd", "csrc")
HEADER = "lol_kernel_scene_light.h"


def flatten(text):
    return " ".join(line.strip().lstrip("*").strip() for line in text.splitlines())


def header_section():
    hdr = read(os.path.join(ROOT, "include", "lol_gpu.h"))
    return hdr, hdr[hdr.index("Scene light passes:"):hdr.index("int  lol_gpu_light_scene_rays(")]


def test_the_symbols_exist():
    lib = gpu.gpu_lib()
    hdr, _ = header_section()
    for name in EXPORTED:
        assert getattr(lib, name) is not None and name in gpu.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % name, hdr), name
    assert int(re.search(r"#define\s+LOL_GPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6 == lib.lol_gpu_abi_version()      # new entry points only
    for method in METHODS:
        assert hasattr(gpu.Renderer, method), method
    assert list(inspect.signature(gpu.Renderer.relight_scenes_into).parameters)[:3] == ["self", "scenes", "looks"]
    assert inspect.signature(gpu.Renderer.relight_scenes_into).parameters["looks"].default is None
    # the section stands behind "Light updates", the last one before it
    assert hdr.index("Light updates:") < hdr.index("int  lol_gpu_relight_views_held(") < hdr.index("Scene light passes:")


def test_a_null_context_is_refused():
    lib = gpu.gpu_lib()
    assert lib.lol_gpu_light_scene_rays(None, None, 1, None, 0, 0, 256, None, None) == -3
    assert lib.lol_gpu_light_scene_pixels(None, None, None, 1, 8, 8, 256, None, 0, 0, None, None) == -3
    assert lib.lol_gpu_relight_scenes(None, None, None, 1, None, 0, None, None) == -3


def test_the_header_says_what_is_promised():
    _, text = header_section()
    flat = flatten(text)
    # the contract's words, in the order the section makes them: layout, capture, latitude, refusals, consequence, launches, kernel
    words = ("r * n + i", "light_stride", "bit for bit", "lol_gpu_upload_program(&scenes[r])",
             "One latitude", "LIST OF RAYS", "the steps really marched", "lol_gpu_set_exact_skips(ctx, 0)", "For pixel sources all 16 bytes are equal",
             "in this order", "1. what the single-scene call refuses", "2. LOL_GPU_ERR_ARG for NULL scenes", "NULL cams in the pixel form",
             "neither 0 nor >= n", "N > 2^32 - 1", "a light_stride that is neither 0 nor >= N",
             "3. the scene refusals of lol_gpu_render_scene_views", "4. for the relight, the first looks[r] that is not a look of scenes[r]",
             "n == 0 returns LOL_GPU_OK",
             "lol_gpu_light_views", "ONE launch", "always")
    at = [flat.index(word) for word in words]
    assert at == sorted(at), [w for w, a, b in zip(words, at, sorted(at)) if a != b]
    # ... and what else is promised
    for word in ("64-bit", "LOL_GPU_MAX_VIEWS", "all 16 bytes of every factor", "whatever the other rays and the other records hold",
                 "OFF for every record", "No proof runs on the device", "looks == NULL", "an id beyond n_roots is taken for 0",
                 "lol_gpu_shade_scene_rays / lol_gpu_shade_scene_pixels on `looks`", "frame r of lol_gpu_render_scene_views on `looks`",
                 "byte for byte", "lol_gpu_relight_views_held resolve them unchanged", "ring of 8 sets", "No scratch, no host wait",
                 "the interpreter's light_interp_scenes and relight_rays_scenes, always", "No module switch has an effect"):
        assert word in flat, word
    scope = flat[flat.index("Out of scope"):]
    for word in ("an averaged resolve over records", "light updates over records", "a structure-module or scene-module form", "lol_gpu_multi_",
                 "planes or lists in host memory", "lol_gpu_light_views made of this call"):
        assert word in scope, word


def test_the_older_sections_point_to_the_new_calls():
    """every sentence that called the feature out of scope stands (other tests pin them), with a pointer to the new section beside it"""
    hdr, _ = header_section()
    for start, end, kept in (("Scene queries:", "int  lol_gpu_trace_scene_rays(", "light passes over records"),
                             ("Light passes and relighting:", "int  lol_gpu_light_rays(", "per-record scenes"),
                             ("Relit views:", "int  lol_gpu_light_views(", "per-record scenes")):
        section = hdr[hdr.index(start):hdr.index(end)]
        scope = flatten(section[section.index("Out of scope"):])
        assert kept in scope and '"Scene light passes", below' in scope, start
    assert "capture in ONE launch over batches, blends or samples" in flatten(hdr)


def test_no_module_switch_and_no_scene_module_knows_of_it():
    assert gpu.MODULE_SWITCHES == SWITCHES
    codegen = read(os.path.join(CSRC, "lol_codegen.hip"))
    assert "lol_kernel_scene_light" not in codegen and "lol_kernel_light.h" not in codegen
    makefile = read(os.path.join(CSRC, "Makefile"))
    kernel_hdrs = next(line for line in makefile.splitlines() if line.startswith("KERNEL_HDRS :="))
    aot_hdrs = next(line for line in makefile.splitlines() if line.startswith("AOT_HDRS :="))
    assert HEADER not in kernel_hdrs and HEADER in aot_hdrs.split()             # not handed to hipRTC; in the build id
    assert "$(AOT_HDRS)" in next(line for line in makefile.splitlines() if line.startswith("lol_build_id.inc:"))
    # the header is no include of lol_gpu_internal.h: lol_gpu.hip includes it, behind every other kernel's host code
    assert HEADER not in read(os.path.join(CSRC, "lol_gpu_internal.h"))
    unit = read(os.path.join(CSRC, "lol_gpu.hip"))
    include = unit.index('#include "%s"' % HEADER)
    for older in ("lol::trace_interp_scenes<", "lol::shade_interp_scenes<", "lol::light_update_interp<", "lol::light_interp<", "lol::relight_rays<"):
        assert unit.rindex(older) < include, older
    assert include < unit.index("lol::light_interp_scenes<") and include < unit.index("lol::relight_rays_scenes<")
    assert unit.count('#include "%s"' % HEADER) == 1


def test_the_kernels_are_the_issues():
    kernels = read(os.path.join(CSRC, HEADER))
    assert "blockIdx.y" in read(os.path.join(CSRC, "lol_kernel_scene_queries.h")) and "record_of_block()" in kernels      # the record
    assert "__shared__ u32 lds[]" in kernels and kernels.count("__shared__") == 2        # no LDS beyond the staged tables
    assert re.search(r"template <int SSIZE, int KIND, bool TABLES_GLOBAL = false>\s*__global__ __launch_bounds__\(BLOCK\)\s*void light_interp_scenes\(", kernels)
    assert re.search(r"template <bool TABLES_GLOBAL = false>\s*__global__ __launch_bounds__\(BLOCK\)\s*void relight_rays_scenes\(", kernels)
    # the per-ray body is light_ray, called (twice: the fast and the exact pipeline), not copied
    assert len(re.findall(r"\blight_ray<Sdf(Fast|Exact), TABLES_GLOBAL>\(", kernels)) == 2 and "soft_shadow" not in kernels and "march<" not in kernels
    # no instruction is written by hand: every asm statement is the empty one that makes a value opaque
    statements = re.findall(r'asm volatile\("([^"]*)" : "\+([sv])"\((\w+)\)\);', kernels)
    assert len(statements) == kernels.count("asm volatile") and statements and all(text == "" for text, _, _ in statements), statements
    assert "__builtin_amdgcn_s_" not in kernels
