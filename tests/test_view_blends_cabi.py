"""Views averaged over K cameras, the part that needs no GPU: the symbols, the scene compiler's source with and without
lol_gpu_set_view_blends, and the gfx950 code object."""
import hashlib
import os
import re
import subprocess

import pytest

import scene_shapes as C
from loltracer_amd import gpu
from test_views_cabi import SOURCE_BEFORE_BATCHES

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "lol_render_spec_batch_lin"


def read(path, mode="r"):
    with open(path, mode) as f:
        return f.read()


def test_the_symbols_exist():
    lib = gpu.gpu_lib()
    for name in ("lol_gpu_render_views_blend", "lol_gpu_set_view_blends", "lol_gpu_view_blends"):
        assert getattr(lib, name) is not None and name in gpu.EXPORTED_SYMBOLS
    for name in ("lol_gpu_compile_offline_view_blends", "lol_gpu_view_blend_kernel_name"):
        assert getattr(lib, name) is not None and name in gpu.DIAG_SYMBOLS
    hdr = read(os.path.join(ROOT, "include", "lol_gpu.h"))
    assert int(re.search(r"#define\s+LOL_GPU_MAX_BLEND\s+(\d+)", hdr).group(1)) == gpu.MAX_BLEND == 16
    assert int(re.search(r"#define\s+LOL_GPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6 == lib.lol_gpu_abi_version()      # new entry points only
    for name in ("lol_gpu_render_views_blend", "lol_gpu_set_view_blends", "lol_gpu_view_blends"):
        assert re.search(r"\b%s\(" % name, hdr), name
    # refusals that need no device: no context, no cameras
    assert lib.lol_gpu_render_views_blend(None, None, 1, 2, 8, 8, 1, None, 32, 256, None, None) == -3
    assert lib.lol_gpu_set_view_blends(None, 1) == -3 and lib.lol_gpu_view_blends(None) == -3
    assert lib.lol_gpu_view_blend_kernel_name(None, 2) == b""


def test_without_the_switch_every_module_is_what_it_was(tmp_path, scenes):
    for name, want in SOURCE_BEFORE_BATCHES.items():
        prog = scenes[name].flatten()
        plain, off = str(tmp_path / (name + "_plain")), str(tmp_path / (name + "_off"))
        gpu.compile_offline(prog, plain)
        gpu.compile_offline_view_blends(prog, off, enable=False)
        src = read(plain + ".hip", "rb")
        assert hashlib.sha256(src).hexdigest() == want, name
        assert read(off + ".hip", "rb") == src, name
        assert read(off + ".co", "rb") == read(plain + ".co", "rb"), name
        assert b"_lin" not in src and b"blend" not in src


def kernels_of(path):
    text = subprocess.run([READELF, "--notes", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return set(re.findall(r"\.name:\s+(\S+)", text))


def test_the_switch_appends_the_linear_kernel(tmp_path, scenes):
    for name in SOURCE_BEFORE_BATCHES:
        prog = scenes[name].flatten()
        plain, on = str(tmp_path / (name + "_plain")), str(tmp_path / (name + "_on"))
        gpu.compile_offline(prog, plain)
        gpu.compile_offline_view_blends(prog, on)                          # (raises unless it compiled for gfx950)
        src, base = read(on + ".hip"), read(plain + ".hip")
        assert src.startswith(base), name                                   # appended after everything else
        tail = src[len(base):]
        assert tail.startswith('#include "lol_kernel_blend.h"\n'), name
        assert src.count("void %s(const lol::Launch L, const lol::BatchTail B) {" % KERNEL) == 1, name
        assert "lol::view_launch(L, B.views)" in tail and "lol::store_linear_view(L, P.rgb)" in tail, name
        assert "store_pixel" not in tail and "_steps" not in tail and "COUNT" not in tail, name
        assert os.path.getsize(on + ".co") > os.path.getsize(plain + ".co"), name
        if os.path.exists(READELF):
            assert KERNEL in kernels_of(on + ".co") and KERNEL not in kernels_of(plain + ".co"), name
    # with the proven fast paths the RECORD's flags choose between the fast and the plain pipeline: the exact fallback comes first,
    # the store after it
    fast = str(tmp_path / "fast")
    gpu.compile_offline_view_blends(scenes["scene4"].flatten(), fast, assume_fast=True)
    tail = read(fast + ".hip").split('#include "lol_kernel_blend.h"\n')[1]
    assert "bool plain = !(S.flags & lol::FLAG_SHADOW_SETTLED);" in tail and "L.flags" not in tail
    assert tail.index("lol::SpecSdfExact exact;") < tail.index("lol::store_linear_view(L, P.rgb)")


def test_both_tiers_of_a_mid_size_scene_carry_it(tmp_path):
    prog = C.scene_of(C.MID).flatten()
    assert 256 < prog.n_ops <= 1024
    for form, out_of_line in ((1, True), (2, False)):
        base = str(tmp_path / ("tier%d" % form))
        gpu.compile_offline_view_blends(prog, base, form=form)
        src = read(base + ".hip")
        assert ("SdfOut" in src) == out_of_line, form
        assert src.count("void %s(" % KERNEL) == 1 and src.count('#include "lol_kernel_blend.h"') == 1, form
        assert os.path.getsize(base + ".co") > 1000
        if os.path.exists(READELF):
            assert KERNEL in kernels_of(base + ".co"), form
    with pytest.raises(gpu.GpuError) as e:
        gpu.compile_offline_view_blends(prog, str(tmp_path / "bad"), form=3)
    assert e.value.status == -3


def test_the_switch_goes_with_the_other_switches(tmp_path, scenes):
    """The switch brings its own kernel alone; beside each of the other switches the module is THAT switch's module with the linear
    kernel appended last, and it compiles for gfx950 — whichever headers the other switch had hipRTC handed (one, two, three or
    four of them before lol_kernel_blend.h)."""
    prog = scenes["scene4"].flatten()
    lib = gpu.gpu_lib()
    assert lib.lol_gpu_compile_offline_view_blends(None, b"gfx950", b"", 0, 1, 0, None, 0) == -3
    assert lib.lol_gpu_compile_offline_view_blends(prog, b"gfx950", b"", 0, 16, 0, None, 0) == -3
    views, on = str(tmp_path / "views"), str(tmp_path / "on")
    gpu.compile_offline_views(prog, views)
    gpu.compile_offline_view_blends(prog, on)
    assert "lol_render_spec_batch(" not in read(on + ".hip")
    assert KERNEL not in read(views + ".hip")
    aa, vs = str(tmp_path / "aa"), str(tmp_path / "vs")
    gpu.compile_offline_samples(prog, aa, 2)
    gpu.compile_offline_view_samples(prog, vs)
    others = {"samples": (aa, ("lol_render_spec_aa", "lol_render_spec_aa_list")),
              "view_batches": (views, ("lol_render_spec_batch", "lol_render_spec_batch_steps")),
              "view_samples": (vs, ("lol_render_spec_batch", "lol_render_spec_batch_aa", "lol_render_spec_batch_aa_list"))}
    for switch, (base_path, kernels) in others.items():
        both = str(tmp_path / ("blend_" + switch))
        gpu.compile_offline_view_blends(prog, both, **{switch: True})         # (raises unless it compiled)
        src, base = read(both + ".hip"), read(base_path + ".hip")
        assert src.startswith(base), switch
        tail = src[len(base):]
        assert tail.startswith('#include "lol_kernel_blend.h"\n') and tail.count("void %s(" % KERNEL) == 1, switch
        assert src.count('#include "lol_kernel_batch.h"') == (1 if switch != "samples" else 0), switch
        # without the blend bit the mask is the other switch's module, byte for byte
        alone = str(tmp_path / ("alone_" + switch))
        gpu.compile_offline_view_blends(prog, alone, enable=False, **{switch: True})
        for ext in (".hip", ".co"):
            assert read(alone + ext, "rb") == read(base_path + ext, "rb"), (switch, ext)
        if os.path.exists(READELF):
            assert kernels_of(both + ".co") >= set(kernels) | {KERNEL, "lol_render_spec"}, switch
    everything = str(tmp_path / "everything")
    gpu.compile_offline_view_blends(prog, everything, samples=True, view_batches=True, view_samples=True)
    src = read(everything + ".hip")
    order = [src.index('#include "%s"' % h) for h in ("lol_kernel.h", "lol_kernel_aa.h", "lol_kernel_batch.h", "lol_kernel_batch_aa.h", "lol_kernel_blend.h")]
    assert order == sorted(order) and src.rstrip().endswith("}") and src.rindex("void lol_render_spec") == src.index("void " + KERNEL)
