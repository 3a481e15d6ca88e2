"""Relit scene views (lol_gpu_relight_scene_views), the part that needs no GPU: the C ABI's symbol and the refusal a NULL context
gets, the header's words on the contract — in the order the header makes them —, the Python mirror, where the kernel's header is
built and included, and that the feature is neither a module switch nor known to the scene compiler."""
import inspect
import os
import re

from loltracer_amd import gpu
from test_rays_cabi import ROOT, read
from test_scene_light_cabi import CSRC, SWITCHES, flatten

NAME = "lol_gpu_relight_scene_views"
HEADER = "lol_kernel_scene_light_views.h"


def header_section():
    hdr = read(os.path.join(ROOT, "include", "lol_gpu.h"))
    return hdr, hdr[hdr.index("Relit scene views:"):hdr.index("int  %s(" % NAME)]


def test_the_symbol_exists():
    lib = gpu.gpu_lib()
    hdr, _ = header_section()
    assert getattr(lib, NAME) is not None and NAME in gpu.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % NAME, hdr)
    assert int(re.search(r"#define\s+LOL_GPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6 == lib.lol_gpu_abi_version()      # new entry point only
    sig = inspect.signature(gpu.Renderer.relight_scene_views_into)
    assert list(sig.parameters) == ["self", "scenes", "looks", "n_views", "cameras_per_view", "w", "h", "samples", "factors_ptr", "id_ptr",
                                    "rgb_linear_ptr", "rgb_ptr", "pixel_ptr", "light_stride", "stream"]
    assert sig.parameters["looks"].default is None and sig.parameters["cameras_per_view"].default == 1
    assert sig.parameters["samples"].default == 1 and sig.parameters["stream"].default is None
    # the section stands behind lol_gpu_relight_scenes, the last call before it
    assert hdr.index("Scene light passes:") < hdr.index("int  lol_gpu_relight_scenes(") < hdr.index("Relit scene views:")


def test_a_null_context_is_refused():
    lib = gpu.gpu_lib()
    assert lib.lol_gpu_relight_scene_views(None, None, None, None, 1, 2, 8, 8, 2, None, None) == -3
    passes, relit = gpu.LightPasses(), gpu.Relit()
    assert lib.lol_gpu_relight_scene_views(None, None, None, passes, 1, 1, 8, 8, 1, relit, None) == -3


def test_the_header_says_what_is_promised():
    _, text = header_section()
    flat = flatten(text)
    # in the header's order: the layout, the four steps of the contract, the identities, the four refusals, the launch, the scope
    words = ("K = cams_per_view in {1, 2, 4, 8, 16}, s = samples in {1, 2, 4}", "Record r = v K + k", "e = (r s h + Y) s w + X of N = n_views K s^2 w h",
             "light_stride 0 = N, else >= N", "hit_id is dense over e", "(v h + y) w + x",
             "1. per leaf, c = the rgb_linear of lol_gpu_relight_scenes for its element under looks[r]", "an id beyond n_roots is taken for 0",
             "2. per record k, m_k = the balanced binary32 tree over its s^2 leaves (s x + i, s y + j) in order j s + i, times 1 / s^2",
             "3. the balanced tree over m_0 ... m_{K-1} in order of k, times 1 / K",
             "4. gamma and the context's pixel format",
             "the order lol_gpu_render_views_blend_samples fixes",
             "bit for bit", "lol_gpu_render_scene_views_samples(cams, looks, n_views, K, w, h, max_steps, s)", "lol_gpu_render_scene_views;",
             "with K = 1 and s = 1 the call is lol_gpu_relight_scenes with n = w * h", "forwards to it", "lol_gpu_relight_views(L)",
             "rgb_linear is the mean before gamma", "NaN and infinite looks are included",
             "look_differs' sense", "K different looks and K different scenes",
             "Refused, with nothing launched and nothing written, in this order",
             "1. everything lol_gpu_relight_views refuses before it looks at its look", "the planes against N",
             "2. LOL_GPU_ERR_ARG for NULL scenes or n_views * K > LOL_GPU_MAX_VIEWS",
             "3. the scene refusals of lol_gpu_render_scene_views",
             "4. the first looks[r] that is no look of scenes[r]", '"relight scene views: record r: "',
             "ring of 8 sets", "HIP's special stream handles included", "ONE launch", "No scratch, no host wait",
             "neither read nor changed", "No module switch has an effect", "Out of scope")
    at = [flat.index(word) for word in words]
    assert at == sorted(at), [w for w, a, b in zip(words, at, sorted(at)) if a != b]
    scope = flat[flat.index("Out of scope"):]
    for word in ("light updates over records", "an edge-adaptive relit form", "a structure-module or scene-module form", "lol_gpu_multi_",
                 "planes in host memory", "pitch or stride addressing of the outputs", "lol_gpu_light_views made of the scene capture",
                 "--tween-shutter refusal"):
        assert word in scope, word


def test_the_older_sections_keep_their_words_and_point_here():
    """the sentences that called the feature out of scope stand word for word (other tests pin them), a pointer beside each"""
    hdr, _ = header_section()
    for start, end, kept in (("Scene light passes:", "int  lol_gpu_light_scene_rays(", "Out of scope: an averaged resolve over records (K records per view, or s x s samples"),
                             ("Relit views:", "int  lol_gpu_light_views(", "edge-adaptive relit supersampling; per-record scenes; lol_gpu_multi_*")):
        section = hdr[hdr.index(start):hdr.index(end)]
        scope = flatten(section[section.index("Out of scope"):])
        assert kept in scope and 'built since' in scope and '"Relit scene views", below' in scope, start


def test_where_the_kernel_is_built_and_included():
    assert gpu.MODULE_SWITCHES == SWITCHES
    codegen = read(os.path.join(CSRC, "lol_codegen.hip"))
    assert "lol_kernel_scene_light_views" not in codegen and "relight_views_scenes" not in codegen
    makefile = read(os.path.join(CSRC, "Makefile"))
    kernel_hdrs = next(line for line in makefile.splitlines() if line.startswith("KERNEL_HDRS :="))
    aot_hdrs = next(line for line in makefile.splitlines() if line.startswith("AOT_HDRS :="))
    assert HEADER not in kernel_hdrs.split() and HEADER in aot_hdrs.split()     # not handed to hipRTC; in the build id
    assert HEADER not in read(os.path.join(CSRC, "lol_gpu_internal.h"))
    unit = read(os.path.join(CSRC, "lol_gpu.hip"))
    include = unit.index('#include "%s"' % HEADER)
    assert unit.count('#include "%s"' % HEADER) == 1
    # behind the host code of scene light passes, and so behind every other kernel's; no other #include follows
    for older in ("lol::relight_rays_scenes<", "lol::light_interp_scenes<", "lol::relight_views<", '#include "lol_kernel_scene_light.h"',
                  "int lol_gpu_relight_scenes("):
        assert unit.rindex(older) < include, older
    assert include < unit.index("lol::relight_views_scenes<") and "#include" not in unit[include + 1:]
    for other in ("lol_tiers.hip", "lol_proofs.hip", "lol_sched.hip", "lol_multi.hip"):
        assert HEADER not in read(os.path.join(CSRC, other)), other


def test_the_kernel_is_the_issues():
    kernel = read(os.path.join(CSRC, HEADER))
    assert re.search(r"template <bool TABLES_GLOBAL = false>\s*__global__ __launch_bounds__\(BLOCK\)\s*void relight_views_scenes\(", kernel)
    assert kernel.count("__global__") == 1 and "blockIdx.y" in kernel
    assert "__shared__ u32 lds[]" in kernel and kernel.count("__shared__") == 1          # no LDS beyond the staged tables
    assert kernel.count("__syncthreads()") == 1
    assert "address_space(4)" in kernel and "aa_add_xor" in kernel and kernel.count("pack_pixel(") == 1
    # the look goes to the leaf's colour as arguments; no Launch is copied to be patched
    assert re.search(r"relit_linear_under\(L, Q, l_light, l_mat, l_rootm, ambient, e\)", kernel) and not re.search(r"\bLaunch\s+\w+\s*=", kernel)
    # no instruction is written by hand: every asm statement, if there is one, is the empty one that makes a value opaque
    statements = re.findall(r'asm volatile\("([^"]*)" : "\+([sv])"\((\w+)\)\);', kernel)
    assert len(statements) == kernel.count("asm volatile") and all(text == "" for text, _, _ in statements), statements
    assert "__builtin_amdgcn_s_" not in kernel
    # the two older headers are included, not copied from
    assert '#include "lol_kernel_light_views.h"' in kernel and '#include "lol_kernel_scene_light.h"' in kernel
