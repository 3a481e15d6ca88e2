"""Supersampled batches of views, the part that needs no GPU: the symbols, the scene compiler's source with and without
lol_gpu_set_view_samples, the gfx950 code object, and what its disassembly may not contain."""
import hashlib
import os
import re
import subprocess

import pytest

from loltracer_amd import gpu, scene as S

OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/llvm/bin/llvm-readelf"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# SHA-256 of the source lol_gpu_compile_offline wrote for the four example scenes before batches of views existed (restated from
# tests/test_views_cabi.py): a module built without any switch is still that text.
SOURCE_BEFORE_BATCHES = {
    "scene": "a3be620c56c7cc994cc10c39d2c6758a7929f116e3cd498ac61b186643c754a0",
    "scene2": "39f876248b4685c86ea6b6fcbfd9f155039d0ac9d8693f34098f2084760de5fc",
    "scene3": "fac927f3b6c992a86308baa4172318a078ffa28afd521954c50ae6304a3bb360",
    "scene4": "4c8df42aaea2abfbc62bc419852472b5c84e5d81e6d446372f516459e876f937",
}
# SHA-256 of what compile_offline_samples(samples=2) and compile_offline_views() wrote for them on the commit before supersampled
# batches existed (recorded from that commit's build): "set_samples alone" and "set_view_batches alone" are the text they were.
SOURCE_OF_THE_PARENT = {
    "scene": ("4e6522273c3efd2cb888d66c11092d30b3f71da30b3bcd8f770eb33d8b62b884", "25840776c38eb7cfcdd4da20e5cecf0fc7e505376811a68c5f3c2225ae2220f8"),
    "scene2": ("8e5f4b2090eea5fe3b16f17cfb96a6d46e9a6ad660ffa1ab247e97679716c1f9", "cfa0f2a504d136c0467a66a6a2d004b3861759b04485458b4756c1ec3b88ef23"),
    "scene3": ("c330c3a4eeb4a639344bd8d73b402da145c5d189a91fedc61c584c29bf561708", "22142a839107447601e19111c86773fc4a8deefdd9ed4c972427dec85ab4b292"),
    "scene4": ("281eb8537c18cad068f217c02f9f471105dbc6223e6352e34167b76e006018e6", "6876177d66b9d873281274da75444c6954401968f1a97f3c6e060648fea8751f"),
}

# bytes of scratch per lane the new kernels may have (lol_render_spec_aa_list has 32)
SCRATCH_STATED = {"lol_render_spec_batch_aa": 0, "lol_render_spec_batch_aa_list": 16}
NEW_KERNELS = tuple(SCRATCH_STATED)


def field(n):
    """n spheres, each a top-level object: 2 n ops"""
    objs = ", ".join("sphere { material = #1, point = (%d, %d, -5), radius = 0.4 }" % (i % 20, i // 20) for i in range(n))
    return S.Scene.parse_string("materials { { shininess = 1 }, { shininess = 2 } } scene { point_light { point = (0,9,0) }, "
                                "plane { material = #0, y = -1 }, %s }" % objs)


def read(path, mode="r"):
    with open(path, mode) as f:
        return f.read()


def sha(path):
    return hashlib.sha256(read(path, "rb")).hexdigest()


def test_the_symbols_exist():
    lib = gpu.gpu_lib()
    for name in ("lol_gpu_render_views_samples", "lol_gpu_set_view_samples", "lol_gpu_view_samples",
                 "lol_gpu_compile_offline_view_samples", "lol_gpu_view_samples_kernel_name", "lol_gpu_views_refined",
                 "lol_gpu_testing_fail_view_scratch"):
        assert getattr(lib, name) is not None
    for name in ("lol_gpu_render_views_samples", "lol_gpu_set_view_samples", "lol_gpu_view_samples"):
        assert name in gpu.EXPORTED_SYMBOLS
    hdr = read(os.path.join(ROOT, "include", "lol_gpu.h"))
    assert int(re.search(r"#define\s+LOL_GPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6 == lib.lol_gpu_abi_version()
    for name in ("lol_gpu_render_views_samples", "lol_gpu_set_view_samples", "lol_gpu_view_samples"):
        assert re.search(r"\b%s\(" % name, hdr), name
    assert "batches are not built" not in hdr
    # refusals that need no device: no context, no cameras
    assert lib.lol_gpu_render_views_samples(None, None, 1, 8, 8, 1, 2, -1, None, 32, 256, None, None) == -3
    assert lib.lol_gpu_set_view_samples(None, 1) == -3 and lib.lol_gpu_view_samples(None) == -3
    assert lib.lol_gpu_views_refined(None, None) == -3 and lib.lol_gpu_testing_fail_view_scratch(None, 1) == -3
    assert lib.lol_gpu_view_samples_kernel_name(None, 2, -1) == b""


def test_without_the_switch_every_module_is_what_it_was(tmp_path, scenes):
    for name, want in SOURCE_BEFORE_BATCHES.items():
        prog = scenes[name].flatten()
        base = {k: str(tmp_path / (name + "_" + k)) for k in ("plain", "off", "aa", "aa1", "views", "views_off")}
        gpu.compile_offline(prog, base["plain"])
        gpu.compile_offline_view_samples(prog, base["off"], enable=False)
        assert sha(base["plain"] + ".hip") == want, name
        for ext in (".hip", ".co"):
            assert read(base["off"] + ext, "rb") == read(base["plain"] + ext, "rb"), (name, ext)
        assert b"batch" not in read(base["plain"] + ".hip", "rb")
        # set_samples alone, set_view_batches alone: the text the parent commit wrote, and no trace of the new kernels
        gpu.compile_offline_samples(prog, base["aa"], 2)
        gpu.compile_offline_views(prog, base["views"])
        assert (sha(base["aa"] + ".hip"), sha(base["views"] + ".hip")) == SOURCE_OF_THE_PARENT[name], name
        for k in ("aa", "views"):
            assert b"batch_aa" not in read(base[k] + ".hip", "rb"), (name, k)
            text = subprocess.run([READELF, "--notes", base[k] + ".co"], check=True, stdout=subprocess.PIPE, text=True).stdout \
                if os.path.exists(READELF) else ""
            assert "batch_aa" not in text, (name, k)
        # ... and the switches off are the plain module, byte for byte, through every offline form
        gpu.compile_offline_samples(prog, base["aa1"], 1)
        gpu.compile_offline_views(prog, base["views_off"], enable=False)
        for k in ("aa1", "views_off"):
            for ext in (".hip", ".co"):
                assert read(base[k] + ext, "rb") == read(base["plain"] + ext, "rb"), (name, k, ext)


def test_the_switch_appends_the_new_kernels_to_the_batch_module(tmp_path, scenes):
    prog = scenes["scene4"].flatten()
    views, on = str(tmp_path / "views"), str(tmp_path / "on")
    gpu.compile_offline_views(prog, views)
    gpu.compile_offline_view_samples(prog, on)
    src, base = read(on + ".hip"), read(views + ".hip")
    assert src.startswith(base)                            # the batch module's source, then the new kernels
    tail = src[len(base):]
    assert tail.startswith('#include "lol_kernel_batch_aa.h"\n')
    assert src.count('#include "lol_kernel_batch_aa.h"') == 1 and src.count('#include "lol_kernel_batch.h"') == 1
    assert src.count("void lol_render_spec_batch_aa(") == 1 and src.count("void lol_render_spec_batch_aa_list(") == 1
    assert src.count("void lol_render_spec_batch(") == 1 and src.count("void lol_render_spec_batch_steps(") == 1
    assert "lol::sample_launch(lol::view_launch(L, B.views))" in tail and "lol::store_pixel_view_aa(L, B, P.rgb)" in tail
    assert "lol::render_aa_view_lists<" in tail and "store_pixel<" not in tail and "_steps" not in tail
    assert os.path.getsize(on + ".co") > os.path.getsize(views + ".co")
    # with the proven fast paths the VIEW's flags choose between the fast and the plain pipeline, in both kernels
    fast = str(tmp_path / "fast")
    gpu.compile_offline_view_samples(prog, fast, assume_fast=True)
    tail = read(fast + ".hip").split('#include "lol_kernel_batch_aa.h"\n')[1]
    assert tail.count("bool plain = !(S.flags & lol::FLAG_SHADOW_SETTLED);") == 2 and "L.flags" not in tail


def test_both_tiers_of_a_mid_size_scene_carry_them(tmp_path):
    prog = field(150).flatten()
    assert 256 < prog.n_ops <= 1024
    for form, out_of_line in ((1, True), (2, False)):
        base = str(tmp_path / ("tier%d" % form))
        gpu.compile_offline_view_samples(prog, base, form=form)
        src = read(base + ".hip")
        assert ("SdfOut" in src) == out_of_line, form
        assert src.count("void lol_render_spec_batch_aa(") == 1 and src.count("void lol_render_spec_batch_aa_list(") == 1, form
        assert src.count("void lol_render_spec_batch(") == 1 and src.count('#include "lol_kernel_batch_aa.h"') == 1, form
        assert os.path.getsize(base + ".co") > 1000
    with pytest.raises(gpu.GpuError) as e:
        gpu.compile_offline_view_samples(prog, str(tmp_path / "bad"), form=3)
    assert e.value.status == -3


def kernel_notes(path):
    """{kernel: {field: value}} of a code object's metadata"""
    text = subprocess.run([READELF, "--notes", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    out = {}
    for blk in text.split("- .agpr_count")[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", blk))
        out[f["name"]] = f
    return out


def test_the_new_kernels_have_no_scalar_stores_and_the_scratch_stated(tmp_path, scenes):
    """gfx950 code objects of scene and scene4 with the switch: the new kernels are there, none of the scalar-store, scalar-atomic
    or scalar-cache write-back instructions anywhere, 8 waves per SIMD (at most 64 VGPRs) and no more scratch than DESIGN.md §3.12
    states — which is no more than lol_render_spec_aa_list has."""
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm-objdump / llvm-readelf are not installed: the code objects were built, they cannot be read")
    s = "s" + "_"
    banned = re.compile(r"\b" + s + r"(?:buffer_|scratch_)?" + "sto" + r"re_|\b" + s + r"(?:buffer_)?" + "ato" + r"mic_|\b" + s + "dca" +
                        r"che_(?:wb|discard)", re.I)
    design = read(os.path.join(ROOT, "DESIGN.md"))
    for kernel, scratch in SCRATCH_STATED.items():
        assert re.search(r"`%s`[^\n]*\b%d bytes of scratch" % (kernel, scratch), design), kernel
    for name in ("scene", "scene4"):
        prog = scenes[name].flatten()
        on, aa = str(tmp_path / (name + "_on")), str(tmp_path / (name + "_aa"))
        gpu.compile_offline_view_samples(prog, on, assume_fast=True)
        gpu.compile_offline_samples(prog, aa, 2, assume_fast=True)
        text = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", on + ".co"], check=True, stdout=subprocess.PIPE, text=True).stdout
        for kernel in NEW_KERNELS + ("lol_render_spec_batch", "lol_render_spec_batch_steps"):
            assert "<%s>:" % kernel in text, (name, kernel)
        assert not banned.search(text), banned.search(text).group(0)
        notes, ref = kernel_notes(on + ".co"), kernel_notes(aa + ".co")["lol_render_spec_aa_list"]
        for kernel in NEW_KERNELS:
            k = notes[kernel]
            assert int(k["private_segment_fixed_size"]) <= SCRATCH_STATED[kernel] <= int(ref["private_segment_fixed_size"]), (name, kernel, k)
            assert int(k["vgpr_count"]) <= 64, (name, kernel, k)


def test_every_kernel_of_the_module_has_its_own_argument_list_and_body(tmp_path, scenes):
    """The symbols come from one table of kernel families (lol_gpu_internal.h, KERNEL_FAMILIES), which the host also launches by: a
    row with another row's symbol would hand a kernel the wrong arguments.  Each symbol heads the argument list of its family, and
    what tells its body from its neighbours' follows before the next kernel."""
    prog = scenes["scene4"].flatten()
    both, aa = str(tmp_path / "both"), str(tmp_path / "aa")
    gpu.compile_offline_view_samples(prog, both)
    gpu.compile_offline_samples(prog, aa, 2)
    src = read(both + ".hip") + read(aa + ".hip")
    L, B = "const lol::Launch L", "const lol::BatchTail B"
    expect = {
        "lol_render_spec_steps": ("(%s)" % L, "lol_spec_body<true>(L, lds)"),
        "lol_render_spec": ("(%s)" % L, "lol_spec_body<false>(L, lds)"),
        "lol_render_spec_aa": ("(%s)" % L, "lol::store_pixel_aa<"),
        "lol_render_spec_aa_list": ("(%s, const lol::u32* list, const lol::u32* count)" % L, "lol::render_aa_list<"),
        "lol_render_spec_batch_steps": ("(%s, %s)" % (L, B), "lol_spec_batch_body<true>(L, B, lds)"),
        "lol_render_spec_batch": ("(%s, %s)" % (L, B), "lol_spec_batch_body<false>(L, B, lds)"),
        "lol_render_spec_batch_aa": ("(%s, %s)" % (L, B), "lol::store_pixel_view_aa("),
        "lol_render_spec_batch_aa_list": ("(%s, %s, const lol::BatchLists Q)" % (L, B), "lol::render_aa_view_lists<"),
    }
    for symbol, (args, mark) in expect.items():
        at = src.index("void %s%s {" % (symbol, args))
        body = src[at:src.find('extern "C"', at + 1) if src.find('extern "C"', at + 1) > 0 else len(src)]
        assert mark in body, symbol
