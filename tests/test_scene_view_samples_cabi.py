"""Supersampled scene views, the part that needs no GPU: the C ABI's symbols and refusals, the structure module's source and code
object with and without lol_gpu_set_scene_view_samples (without it: what it was), and the documents' quotes of the rate record."""
import hashlib
import json
import os
import re

from loltracer_amd import gpu
from test_rays_cabi import ROOT, kernel_notes, read
from test_scene_views_cabi import changed_scene4
from test_views_cabi import SOURCE_BEFORE_BATCHES

EXPORTED = ("lol_gpu_render_scene_views_samples", "lol_gpu_set_scene_view_samples", "lol_gpu_scene_view_samples")
DIAG = ("lol_gpu_scene_view_samples_kernel_name", "lol_gpu_compile_offline_scene_view_samples")
PLAIN = ("lol_render_param_batch", "lol_render_param_batch_lin")
AA = ("lol_render_param_batch_aa", "lol_render_param_batch_aa_lin")
RECORD = os.path.join(ROOT, "profiles", "r19_scene_view_samples_rate.json")


def test_the_symbols_exist():
    lib = gpu.gpu_lib()
    hdr, diag = read(os.path.join(ROOT, "include", "lol_gpu.h")), read(os.path.join(ROOT, "include", "lol_gpu_diag.h"))
    for name in EXPORTED:
        assert getattr(lib, name) is not None and name in gpu.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % name, hdr), name
    for name in DIAG:
        assert getattr(lib, name) is not None and name in gpu.DIAG_SYMBOLS and re.search(r"\b%s\(" % name, diag), name
    assert int(re.search(r"#define\s+LOL_GPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6 == lib.lol_gpu_abi_version()      # new entry points only
    # the contract's words, and what is out of scope, are in the header
    text = hdr[hdr.index("Supersampled scene views:"):hdr.index("int  lol_gpu_render_scene_views_samples(")]
    for word in ("(s x + i, s y + j)", "j s + i", "1 / s^2", "1 / K", "two trees", "forwards to it", "lol_gpu_render_views_blend_samples",
                 "an adaptive form", "ray and shading queries", "row partitions", "lol_gpu_multi_", "host surfaces", "renderer.h",
                 "65535 tiles", "2^32 - 1", "No new ring"):
        assert word in text, word
    # ... and of the scene views' own comment only the adaptive form remains out of scope
    scope = hdr[hdr.index("Scene views:"):hdr.index("int  lol_gpu_render_scene_views(")]
    assert "Out of scope: an adaptive form" in scope and "lol_gpu_render_scene_views_samples" in scope
    # refusals that need no device: no context
    assert lib.lol_gpu_render_scene_views_samples(None, None, None, 1, 1, 8, 8, 1, 2, None, 32, 256, None, None) == -3
    assert lib.lol_gpu_set_scene_view_samples(None, 1) == -3 and lib.lol_gpu_scene_view_samples(None) == -3
    assert lib.lol_gpu_scene_view_samples_kernel_name(None, 1, 2) == b""
    assert lib.lol_gpu_compile_offline_scene_view_samples(None, b"gfx950", b"", None, 0) == -3
    for method in ("set_scene_view_samples", "scene_view_samples", "scene_view_samples_kernel_name"):
        assert hasattr(gpu.Renderer, method), method
    assert hasattr(gpu, "compile_offline_scene_view_samples")
    import inspect
    assert inspect.signature(gpu.Renderer.render_scene_views_into).parameters["samples"].default == 1
    # the switch is no module switch: seven of those still
    assert len(gpu.MODULE_SWITCHES) == 7 and not any("scene" in name for name in gpu.MODULE_SWITCHES)


def without_the_new_kernels(text):
    """the source of a structure module made with the switch, its two supersampled kernels and their body taken out again"""
    assert text.startswith('#include "lol_kernel_scenes_aa.h"\n')
    text = '#include "lol_kernel_scenes.h"\n' + text[len('#include "lol_kernel_scenes_aa.h"\n'):]
    return text[:text.index("template <bool LIN> __device__ __forceinline__ void lol_param_body_aa(")]


def test_without_the_switch_the_structure_module_is_what_it_was(tmp_path, scenes):
    prog = scenes["scene4"].flatten()
    a, b, c = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    gpu.compile_offline_scene_views(prog, a)
    gpu.compile_offline_scene_views(prog, b)
    gpu.compile_offline_scene_view_samples(prog, c)
    plain, with_switch = read(a + ".hip"), read(c + ".hip")
    assert read(a + ".hip", "rb") == read(b + ".hip", "rb") and read(a + ".co", "rb") == read(b + ".co", "rb")
    assert "lol_render_param_batch_aa" not in plain and "lol_kernel_scenes_aa.h" not in plain and "sample_launch" not in plain
    assert plain.startswith('#include "lol_kernel_scenes.h"\n')
    assert without_the_new_kernels(with_switch) == plain                        # the new text is an addition and nothing else
    notes = kernel_notes(a + ".co")
    assert set(PLAIN) <= notes.keys() and not set(AA) & notes.keys()


def test_with_the_switch_all_four_kernels(tmp_path, scenes):
    prog = scenes["scene4"].flatten()
    base = str(tmp_path / "aa")
    gpu.compile_offline_scene_view_samples(prog, base)
    src = read(base + ".hip")
    for kernel in PLAIN + AA:
        assert re.search(r"void %s\(const lol::Launch L, const lol::SceneTail B\)" % kernel, src), kernel
    body = src[src.index("void lol_param_body_aa("):]
    assert "lol::sample_launch(R)" in body and "lol::store_pixel_view_aa(L, lol::batch_tail(B), P.rgb)" in body
    assert "lol::store_linear_view_aa(L, P.rgb)" in body and "lol::shade_pixel<lol::ParamSdf, false, false>(S, sdf, lds)" in body
    assert src.count("struct ParamSdf") == 1                                    # the same SDF serves all four
    code = read(base + ".co", "rb")
    assert code[:4] == b"\x7fELF"
    notes = kernel_notes(base + ".co")
    for kernel in PLAIN + AA:
        assert kernel in notes, kernel
    plain_base = str(tmp_path / "plain")
    gpu.compile_offline_scene_views(prog, plain_base)
    before = kernel_notes(plain_base + ".co")
    for kernel in PLAIN:                                                         # the two old kernels of the larger module keep their resources
        for field in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"):
            assert notes[kernel][field] == before[kernel][field], (kernel, field)
    for kernel in AA:                                                            # the same LDS; what they report is in DESIGN.md 3.19
        assert notes[kernel]["group_segment_fixed_size"] == notes["lol_render_param_batch_lin"]["group_segment_fixed_size"]
        print(kernel, {f: notes[kernel][f] for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
    for kernel in PLAIN:
        print(kernel, {f: notes[kernel][f] for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})


def test_two_scenes_of_one_structure_share_source_and_code_object(tmp_path, scenes):
    a = scenes["scene4"]
    b = changed_scene4(a)
    pa, pb, pc = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    gpu.compile_offline_scene_view_samples(a.flatten(), pa)
    gpu.compile_offline_scene_view_samples(b.flatten(), pb)
    gpu.compile_offline_scene_view_samples(scenes["scene"].flatten(), pc)
    assert read(pa + ".hip", "rb") == read(pb + ".hip", "rb") and read(pa + ".co", "rb") == read(pb + ".co", "rb")
    assert read(pa + ".hip", "rb") != read(pc + ".hip", "rb")                  # another structure is another source
    for kernel in PLAIN + AA:
        assert kernel in kernel_notes(pc + ".co"), kernel


def test_the_scenes_own_module_is_what_it_was(tmp_path, scenes):
    for name, want in SOURCE_BEFORE_BATCHES.items():
        base = str(tmp_path / name)
        gpu.compile_offline_module(scenes[name].flatten(), base, ())
        src = read(base + ".hip", "rb")
        assert hashlib.sha256(src).hexdigest() == want, name
        assert b"scenes" not in src and b"param" not in src
        assert not set(PLAIN + AA) & kernel_notes(base + ".co").keys()


def test_the_documents_quote_the_committed_record():
    """README.md and DESIGN.md quote the rate record's own medians and name the fastest arm as the record names it; the record says
    what the feature was accepted on: every one-call arm faster than the per-frame uploads by more than the arms' spread.  Until
    the record exists the documents say "not measured"."""
    design, readme = read(os.path.join(ROOT, "DESIGN.md")), read(os.path.join(ROOT, "README.md"))
    section = design[design.index("### 3.19"):]
    row = next(line for line in readme.splitlines() if "lol_gpu_render_scene_views_samples" in line)
    if not os.path.exists(RECORD):
        assert "not measured" in section and "not measured" in row
        return
    rec = json.load(open(RECORD))
    assert rec["scene"] == "scene4" and (rec["w"], rec["h"], rec["frames"], rec["samples"]) == (128, 128, 64, 2) and rec["window_s"] >= 1.0
    assert rec["frames_equal_across_arms"] and rec["distinct_frames"] == 64
    assert rec["blend"]["frames_equal_across_arms"] and rec["blend"]["scenes_per_frame"] == 4
    assert "set_samples(2)" in rec["arms_are"]["a"] and "specialisation off" in rec["arms_are"]["b"] and "fast paths" in rec["arms_are"]["f"]
    assert "render_interp_scene_batch_aa" in rec["arms_are"]["b"] and "render_interp_scene_batch_aa" in rec["arms_are"]["f"]
    assert "lol_render_param_batch_aa" in rec["arms_are"]["c"]
    assert rec["fast_interpreter_proofs"]["sqrt_kind"] == 3 and rec["fast_interpreter_proofs"]["proven_blend_factors"] >= 1
    arms = {x: rec["arms"][x] for x in "abfc"}
    spread = max(x["max_ms"] - x["min_ms"] for x in arms.values())
    for x in "bfc":
        assert rec[x + "_faster_than_a_by_more_than_the_spread"] and arms["a"]["min_ms"] - arms[x]["max_ms"] > spread, x
    fastest = [x for x in "bfc" if all(arms[x]["max_ms"] < arms[y]["min_ms"] for y in "bfc" if y != x)]
    assert rec["fastest_of_b_f_c"] == (fastest[0] if fastest else "none (windows overlap)")
    quoted = [arms[x]["median_ms"] for x in "abfc"] + [rec["blend"]["arms"][x]["median_ms"] for x in "bfc"]
    assert "r19_scene_view_samples_rate.json" in section and "r19_scene_view_samples_rate.json" in row
    for v in quoted:
        assert "%s ms" % v in section, ("DESIGN.md", v)
    for v in quoted[:4]:
        assert "%s ms" % v in row, ("README.md", v)
    assert "not measured" not in section and "not measured" not in row
    says = "**(%s) is the fastest of the three**" % rec["fastest_of_b_f_c"] if fastest else "**none of the three is the fastest: their windows overlap**"
    assert says in section
