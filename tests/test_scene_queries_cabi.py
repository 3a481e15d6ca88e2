"""Scene queries (lol_gpu_trace_scene_rays, lol_gpu_trace_scene_pixels, lol_gpu_shade_scene_rays, lol_gpu_shade_scene_pixels), the part
that needs no GPU: the C ABI's symbols and the refusal a NULL context gets, the header's words on the contract, its one latitude and
the order of the refusals, the Python mirror, and that the feature is neither a module switch nor known to the scene compiler."""
import inspect
import os
import re

from loltracer_amd import gpu
from test_rays_cabi import ROOT, read

EXPORTED = ("lol_gpu_trace_scene_rays", "lol_gpu_trace_scene_pixels", "lol_gpu_shade_scene_rays", "lol_gpu_shade_scene_pixels")
METHODS = ("trace_scene_rays_into", "trace_scene_pixels_into", "shade_scene_rays_into", "shade_scene_pixels_into", "pick_scenes")
SWITCHES = ("samples", "view_batches", "view_samples", "view_blends", "view_blend_samples", "ray_queries", "shade_queries")
CSRC = os.path.join(ROOT, "loltracer_amd", "csrc")


def header_section():
    hdr = read(os.path.join(ROOT, "include", "lol_gpu.h"))
    return hdr, hdr[hdr.index("Scene queries:"):hdr.index("int  lol_gpu_trace_scene_rays(")]


def test_the_symbols_exist():
    lib = gpu.gpu_lib()
    hdr, _ = header_section()
    for name in EXPORTED:
        assert getattr(lib, name) is not None and name in gpu.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % name, hdr), name
    assert int(re.search(r"#define\s+LOL_GPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6 == lib.lol_gpu_abi_version()      # new entry points only
    for method in METHODS:
        assert hasattr(gpu.Renderer, method), method
    assert list(inspect.signature(gpu.Renderer.pick_scenes).parameters)[:7] == ["self", "scenes", "x", "y", "w", "h", "cameras"]


def test_a_null_context_is_refused():
    lib = gpu.gpu_lib()
    assert lib.lol_gpu_trace_scene_rays(None, None, 1, None, 0, 0, 256, None, None) == -3
    assert lib.lol_gpu_trace_scene_pixels(None, None, None, 1, 8, 8, 256, None, 0, 0, None, None) == -3
    assert lib.lol_gpu_shade_scene_rays(None, None, 1, None, 0, 0, 256, None, None) == -3
    assert lib.lol_gpu_shade_scene_pixels(None, None, None, 1, 8, 8, 256, None, 0, 0, None, None) == -3


def test_the_header_says_what_is_promised():
    _, text = header_section()
    flat = " ".join(line.strip().lstrip("*").strip() for line in text.splitlines())
    # the contract and the records
    for word in ("r * n + i", "list_stride == 0", "list_stride >= n", "64-bit", "bit for bit", "lol_gpu_upload_program(&scenes[r])",
                 "whatever the other rays and the other records hold", "a NaN centre in one record is that record's business alone",
                 "No proof runs on the device", "ONE launch", "ring of 8 sets", "no scratch", "LOL_GPU_MAX_VIEWS"):
        assert word in flat, word
    # the one latitude
    for word in ("One latitude", "LIST OF RAYS", "high 16 bits of lol_gpu_shades.steps", "the steps really marched",
                 "lol_gpu_set_exact_skips(ctx, 0)", "For pixel sources all 32 bits are equal"):
        assert word in flat, word
    # the refusals, in their order
    at = [flat.index(word) for word in ("in this order", "1. what the single-scene query refuses", "2. LOL_GPU_ERR_ARG for NULL scenes",
                                        "NULL cams in a pixel form", "neither 0 nor >= n", "n_scenes * n > 2^32 - 1",
                                        "3. the scene refusals of lol_gpu_render_scene_views", "n == 0 returns LOL_GPU_OK")]
    assert at == sorted(at), at
    # which kernel, and what is out of scope
    for word in ("the interpreter's trace_interp_scenes / shade_interp_scenes, always", "lol_gpu_set_scene_views, lol_gpu_set_ray_queries and "
                 "lol_gpu_set_shade_queries have no effect", "a structure-module form", "light passes over records", "lists in host memory",
                 "lol_gpu_multi_", "a C pick over records"):
        assert word in flat, word
    # ... and the scene views' comments no longer call the feature out of scope
    hdr, _ = header_section()
    for start, end in (("Scene views:", "int  lol_gpu_render_scene_views("), ("Supersampled scene views:", "int  lol_gpu_render_scene_views_samples(")):
        scope = hdr[hdr.index(start):hdr.index(end)]
        scope = " ".join(line.strip().lstrip("*").strip() for line in scope[scope.index("Out of scope"):].splitlines())
        assert re.search(r"ray and shading queries over per-record scenes are (built|lol_gpu_trace_scene_rays')", scope), scope


def test_no_module_switch_and_no_scene_module_knows_of_it():
    assert gpu.MODULE_SWITCHES == SWITCHES
    assert "lol_kernel_scene_queries" not in read(os.path.join(CSRC, "lol_codegen.hip"))
    makefile = read(os.path.join(CSRC, "Makefile"))
    kernel_hdrs = next(line for line in makefile.splitlines() if line.startswith("KERNEL_HDRS :="))
    aot_hdrs = next(line for line in makefile.splitlines() if line.startswith("AOT_HDRS :="))
    assert "lol_kernel_scene_queries.h" not in kernel_hdrs and aot_hdrs.rstrip().endswith("lol_kernel_scene_queries.h")      # not handed to hipRTC; in the build id
    includes = re.findall(r'#include "(lol_kernel[a-z_]*\.h)"', read(os.path.join(CSRC, "lol_gpu_internal.h")))
    assert includes[-1] == "lol_kernel_scene_queries.h", includes                   # last: the code objects of the others stay what they are
    unit = read(os.path.join(CSRC, "lol_gpu.hip"))
    assert unit.index("lol::trace_interp_scenes<") > max(unit.rindex("lol::light_update_interp<"), unit.rindex("lol::shade_interp<"))
    kernels = read(os.path.join(CSRC, "lol_kernel_scene_queries.h"))
    assert "blockIdx.y" in kernels and "__shared__ u32 lds[]" in kernels
    # no instruction is written by hand: every asm statement is the empty one that makes a value opaque (ray_out, fetch_ray)
    statements = re.findall(r'asm volatile\("([^"]*)" : "\+([sv])"\((\w+)\)\);', kernels)
    assert len(statements) == kernels.count("asm volatile") == 3 and all(text == "" for text, _, _ in statements), statements
