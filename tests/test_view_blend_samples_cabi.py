"""Supersampled blends, the part that needs no GPU: the symbols, the scene compiler's source with and without
lol_gpu_set_view_blend_samples, and the gfx950 code object with its resources."""
import json
import os
import re
import subprocess

import pytest

import scene_shapes as C
from loltracer_amd import gpu
from test_views_cabi import SOURCE_BEFORE_BATCHES

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "lol_render_spec_batch_aa_lin"
HEAD = "void %s(const lol::Launch L, const lol::BatchTail B) {" % KERNEL
INCLUDE = '#include "lol_kernel_blend_aa.h"\n'
EXPORTED = ("lol_gpu_render_views_blend_samples", "lol_gpu_set_view_blend_samples", "lol_gpu_view_blend_samples")
DIAG = ("lol_gpu_compile_offline_view_blend_samples", "lol_gpu_view_blend_samples_kernel_name")


def read(path, mode="r"):
    with open(path, mode) as f:
        return f.read()


def kernel_notes(path):
    """{kernel: {field: value}} of a code object's metadata"""
    text = subprocess.run([READELF, "--notes", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    out = {}
    for blk in text.split("- .agpr_count")[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", blk))
        out[f["name"]] = f
    return out


def test_the_symbols_exist():
    lib = gpu.gpu_lib()
    hdr, diag = read(os.path.join(ROOT, "include", "lol_gpu.h")), read(os.path.join(ROOT, "include", "lol_gpu_diag.h"))
    for name in EXPORTED:
        assert getattr(lib, name) is not None and name in gpu.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % name, hdr), name
    for name in DIAG:
        assert getattr(lib, name) is not None and name in gpu.DIAG_SYMBOLS and re.search(r"\b%s\(" % name, diag), name
    assert int(re.search(r"#define\s+LOL_GPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6 == lib.lol_gpu_abi_version()      # new entry points only
    # refusals that need no device: no context, no cameras
    assert lib.lol_gpu_render_views_blend_samples(None, None, 1, 2, 8, 8, 1, 2, None, 32, 256, None, None) == -3
    assert lib.lol_gpu_set_view_blend_samples(None, 1) == -3 and lib.lol_gpu_view_blend_samples(None) == -3
    assert lib.lol_gpu_view_blend_samples_kernel_name(None, 2, 2) == b""
    for method in ("set_view_blend_samples", "view_blend_samples", "view_blend_samples_kernel_name"):
        assert hasattr(gpu.Renderer, method), method


def test_without_the_switch_every_module_is_what_it_was(tmp_path, scenes):
    for name in SOURCE_BEFORE_BATCHES:
        prog = scenes[name].flatten()
        plain, off = str(tmp_path / (name + "_plain")), str(tmp_path / (name + "_off"))
        gpu.compile_offline(prog, plain)
        gpu.compile_offline_view_blend_samples(prog, off, enable=False)
        src = read(plain + ".hip", "rb")
        assert read(off + ".hip", "rb") == src, name
        assert read(off + ".co", "rb") == read(plain + ".co", "rb"), name
        assert b"_aa_lin" not in src and b"blend" not in src


def test_the_switch_appends_the_supersampled_linear_kernel(tmp_path, scenes):
    for name in SOURCE_BEFORE_BATCHES:
        prog = scenes[name].flatten()
        plain, on = str(tmp_path / (name + "_plain")), str(tmp_path / (name + "_on"))
        gpu.compile_offline(prog, plain)
        gpu.compile_offline_view_blend_samples(prog, on)                   # (raises unless it compiled for gfx950)
        src, base = read(on + ".hip"), read(plain + ".hip")
        assert src.startswith(base), name                                   # appended after everything else
        tail = src[len(base):]
        assert tail.startswith(INCLUDE), name
        assert tail.count(HEAD) == 1 and src.count("void %s(" % KERNEL) == 1, name
        assert "lol::sample_launch(lol::view_launch(L, B.views))" in tail and "lol::store_linear_view_aa(L, P.rgb)" in tail, name
        assert "store_pixel" not in tail and "_steps" not in tail and "COUNT" not in tail, name
        # the switch brings its own kernel alone: none of the other families' (their headers come in through the include)
        assert "void lol_render_spec_batch(" not in src and "void lol_render_spec_batch_lin(" not in src, name
        assert KERNEL in kernel_notes(on + ".co") and KERNEL not in kernel_notes(plain + ".co"), name
    # with the proven fast paths the RECORD's flags choose between the fast and the plain pipeline: the exact fallback comes first,
    # the store after it
    fast = str(tmp_path / "fast")
    gpu.compile_offline_view_blend_samples(scenes["scene4"].flatten(), fast, assume_fast=True)
    tail = read(fast + ".hip").split(INCLUDE)[1]
    assert "bool plain = !(S.flags & lol::FLAG_SHADOW_SETTLED);" in tail and "L.flags" not in tail
    assert tail.index("lol::SpecSdfFast fast;") < tail.index("lol::SpecSdfExact exact;") < tail.index("lol::store_linear_view_aa(L, P.rgb)")


def test_both_tiers_of_a_mid_size_scene_carry_it(tmp_path):
    prog = C.scene_of(C.MID).flatten()
    assert 256 < prog.n_ops <= 1024
    for form, out_of_line in ((1, True), (2, False)):
        base = str(tmp_path / ("tier%d" % form))
        gpu.compile_offline_view_blend_samples(prog, base, form=form)
        src = read(base + ".hip")
        assert ("SdfOut" in src) == out_of_line, form
        assert src.count("void %s(" % KERNEL) == 1 and src.count(INCLUDE) == 1, form
        assert KERNEL in kernel_notes(base + ".co"), form
    with pytest.raises(gpu.GpuError) as e:
        gpu.compile_offline_view_blend_samples(prog, str(tmp_path / "bad"), form=3)
    assert e.value.status == -3


def test_the_switch_goes_with_the_other_switches(tmp_path, scenes):
    """Beside each other switch the module is THAT switch's module with this kernel appended last, and it compiles for gfx950
    whichever headers the other switch had hipRTC handed; with the bit off it is that switch's module byte for byte.  The switch
    is its own: the blend and view-samples switches together do not bring the kernel."""
    prog = scenes["scene4"].flatten()
    lib = gpu.gpu_lib()
    assert lib.lol_gpu_compile_offline_view_blend_samples(None, b"gfx950", b"", 0, 1, 0, 0, None, 0) == -3
    assert lib.lol_gpu_compile_offline_view_blend_samples(prog, b"gfx950", b"", 0, 1, 16, 0, None, 0) == -3
    assert lib.lol_gpu_compile_offline_view_blend_samples(prog, b"gfx950", b"", 0, 1, -1, 0, None, 0) == -3
    bases = {}
    for switch, compile_base in (("view_blends", lambda p: gpu.compile_offline_view_blends(prog, p)),
                                 ("samples", lambda p: gpu.compile_offline_samples(prog, p, 2)),
                                 ("view_batches", lambda p: gpu.compile_offline_views(prog, p)),
                                 ("view_samples", lambda p: gpu.compile_offline_view_samples(prog, p))):
        bases[switch] = str(tmp_path / ("base_" + switch))
        compile_base(bases[switch])
    for switch, base_path in bases.items():
        both, alone = str(tmp_path / ("both_" + switch)), str(tmp_path / ("alone_" + switch))
        gpu.compile_offline_view_blend_samples(prog, both, **{switch: True})  # (raises unless it compiled)
        src, base = read(both + ".hip"), read(base_path + ".hip")
        assert KERNEL not in base, switch
        assert src.startswith(base), switch
        tail = src[len(base):]
        assert tail.startswith(INCLUDE) and tail.count(HEAD) == 1, switch
        assert kernel_notes(both + ".co").keys() == kernel_notes(base_path + ".co").keys() | {KERNEL}, switch
        gpu.compile_offline_view_blend_samples(prog, alone, enable=False, **{switch: True})
        for ext in (".hip", ".co"):
            assert read(alone + ext, "rb") == read(base_path + ext, "rb"), (switch, ext)
    # every existing switch and NOT this one: the module ends with the linear kernel, as tests/test_view_blends_cabi.py pins
    four, four_off = str(tmp_path / "four"), str(tmp_path / "four_off")
    gpu.compile_offline_view_blends(prog, four, samples=True, view_batches=True, view_samples=True)
    gpu.compile_offline_view_blend_samples(prog, four_off, enable=False, view_blends=True, samples=True, view_batches=True, view_samples=True)
    for ext in (".hip", ".co"):
        assert read(four_off + ext, "rb") == read(four + ext, "rb"), ext
    assert KERNEL not in read(four + ".hip")
    # every switch on: it compiles, the new kernel is the last, and lol_render_spec_batch_lin directly precedes it
    everything = str(tmp_path / "everything")
    gpu.compile_offline_view_blend_samples(prog, everything, view_blends=True, samples=True, view_batches=True, view_samples=True)
    src = read(everything + ".hip")
    assert src.startswith(read(four + ".hip")) and src.rstrip().endswith("}")
    kernels = re.findall(r"void (lol_render_spec\w*)\(", src)
    assert kernels[-2:] == ["lol_render_spec_batch_lin", KERNEL] and len(set(kernels)) == len(kernels), kernels
    assert src.rindex("void lol_render_spec") == src.index("void " + KERNEL + "(")
    headers = ["lol_kernel.h", "lol_kernel_aa.h", "lol_kernel_batch.h", "lol_kernel_batch_aa.h", "lol_kernel_blend.h", "lol_kernel_blend_aa.h"]
    order = [src.index('#include "%s"' % h) for h in headers]
    assert order == sorted(order)
    assert set(kernels) <= kernel_notes(everything + ".co").keys()


RESOURCE_MODULES = (("scene4", True, 0), ("scene", True, 0), ("chain140", False, 1), ("chain140", False, 2))
VGPR_CAP = 64                            # 8 waves per SIMD


def test_resources_of_the_new_kernel(tmp_path, scenes):
    """From the code object's own metadata, for scene4, scene.lol and the mid-size scene in both forms: no scratch, and at most the
    64 VGPRs that keep 8 waves per SIMD.  profiles/r12_blend_aa_kernel_resources.json records the figures of the same scenes and forms, there compiled beside
    lol_gpu_set_view_samples so that lol_render_spec_batch_aa stands next to the new kernel."""
    recorded = json.loads(read(os.path.join(ROOT, "profiles", "r12_blend_aa_kernel_resources.json")))["kernels"]
    assert len(recorded) == len(RESOURCE_MODULES)
    for (name, fast, form), rec in zip(RESOURCE_MODULES, recorded):
        prog = (scenes[name] if name in scenes else C.scene_of(C.MID)).flatten()
        base = str(tmp_path / ("%s_%d" % (name, form)))
        gpu.compile_offline_view_blend_samples(prog, base, assume_fast=fast, form=form)
        k = kernel_notes(base + ".co")[KERNEL]
        assert int(k["private_segment_fixed_size"]) == 0, (name, form, k)
        assert int(k["vgpr_count"]) <= VGPR_CAP, (name, form, k)
        assert (rec["scene"], rec["form"], rec["assume_fast"]) == (name, form, fast)
        # (the record is one compiler's figures: held to the same bounds, not to equality with this compiler's)
        assert rec[KERNEL]["scratch_bytes_per_lane"] == 0 and rec[KERNEL]["vgprs"] <= VGPR_CAP, (name, form)
