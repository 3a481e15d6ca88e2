"""Batches of views, the part that needs no GPU: the scene compiler's source with and without lol_gpu_set_view_batches, the gfx950
code object, and what its disassembly may not contain."""
import hashlib
import os
import re
import subprocess

import pytest

from loltracer_amd import gpu, scene as S

OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"

# SHA-256 of the source lol_gpu_compile_offline wrote for the four example scenes BEFORE batches of views existed (recorded from
# the parent commit's build): "a module built without the switch is the same source text as before" is checked, not assumed.
SOURCE_BEFORE_BATCHES = {
    "scene": "a3be620c56c7cc994cc10c39d2c6758a7929f116e3cd498ac61b186643c754a0",
    "scene2": "39f876248b4685c86ea6b6fcbfd9f155039d0ac9d8693f34098f2084760de5fc",
    "scene3": "fac927f3b6c992a86308baa4172318a078ffa28afd521954c50ae6304a3bb360",
    "scene4": "4c8df42aaea2abfbc62bc419852472b5c84e5d81e6d446372f516459e876f937",
}


def field(n):
    """n spheres, each a top-level object: 2 n ops"""
    objs = ", ".join("sphere { material = #1, point = (%d, %d, -5), radius = 0.4 }" % (i % 20, i // 20) for i in range(n))
    return S.Scene.parse_string("materials { { shininess = 1 }, { shininess = 2 } } scene { point_light { point = (0,9,0) }, "
                                "plane { material = #0, y = -1 }, %s }" % objs)


def read(path, mode="r"):
    with open(path, mode) as f:
        return f.read()


def test_the_symbols_exist():
    lib = gpu.gpu_lib()
    for name in ("lol_gpu_render_views", "lol_gpu_set_view_batches", "lol_gpu_view_batches", "lol_gpu_compile_offline_views"):
        assert getattr(lib, name) is not None
    hdr = read(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lol_gpu.h"))
    assert int(re.search(r"#define\s+LOL_GPU_MAX_VIEWS\s+(\d+)", hdr).group(1)) == gpu.MAX_VIEWS >= 4096
    assert int(re.search(r"#define\s+LOL_GPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6
    # refusals that need no device: no context, no cameras
    assert lib.lol_gpu_render_views(None, None, 1, 8, 8, 1, None, 32, 256, None, None) == -3
    assert lib.lol_gpu_set_view_batches(None, 1) == -3 and lib.lol_gpu_view_batches(None) == -3


def test_switch_off_is_the_parent_source(tmp_path, scenes):
    for name, want in SOURCE_BEFORE_BATCHES.items():
        prog = scenes[name].flatten()
        plain, off = str(tmp_path / (name + "_plain")), str(tmp_path / (name + "_off"))
        gpu.compile_offline(prog, plain)
        gpu.compile_offline_views(prog, off, enable=False)
        src = read(plain + ".hip", "rb")
        assert hashlib.sha256(src).hexdigest() == want, name
        assert read(off + ".hip", "rb") == src, name
        assert read(off + ".co", "rb") == read(plain + ".co", "rb"), name
        assert b"batch" not in src


def test_switch_on_appends_the_batch_kernel(tmp_path, scenes):
    prog = scenes["scene4"].flatten()
    plain, on = str(tmp_path / "plain"), str(tmp_path / "on")
    gpu.compile_offline(prog, plain)
    gpu.compile_offline_views(prog, on)
    src, base = read(on + ".hip"), read(plain + ".hip")
    assert src.startswith(base)                            # appended after everything else
    tail = src[len(base):]
    assert tail.startswith('#include "lol_kernel_batch.h"\n')
    assert src.count("void lol_render_spec_batch(") == 1 and src.count("void lol_render_spec_batch_steps(") == 1
    assert src.count('#include "lol_kernel_batch.h"') == 1
    assert "lol::view_launch(L, B.views)" in tail and "lol::store_pixel_view(L, B, P)" in tail and "store_pixel<" not in tail
    assert os.path.getsize(on + ".co") > os.path.getsize(plain + ".co")
    # with the proven fast paths the VIEW's flags choose between the fast and the plain pipeline
    fast = str(tmp_path / "fast")
    gpu.compile_offline_views(prog, fast, assume_fast=True)
    tail = read(fast + ".hip").split('#include "lol_kernel_batch.h"\n')[1]
    assert "bool plain = !(S.flags & lol::FLAG_SHADOW_SETTLED);" in tail and "L.flags" not in tail


def test_both_tiers_of_a_mid_size_scene_carry_it(tmp_path):
    prog = field(150).flatten()
    assert 256 < prog.n_ops <= 1024
    for form, out_of_line in ((1, True), (2, False)):
        base = str(tmp_path / ("tier%d" % form))
        gpu.compile_offline_views(prog, base, form=form)
        src = read(base + ".hip")
        assert ("SdfOut" in src) == out_of_line, form
        # (above 256 ops a module holds the counting pipeline alone, under the plain name)
        assert src.count("void lol_render_spec_batch(") == 1 and "lol_render_spec_batch_steps" not in src, form
        assert src.count('#include "lol_kernel_batch.h"') == 1 and "lol_spec_batch_body<true>(L, B, lds)" in src, form
        assert os.path.getsize(base + ".co") > 1000
    with pytest.raises(gpu.GpuError) as e:
        gpu.compile_offline_views(prog, str(tmp_path / "bad"), form=3)
    assert e.value.status == -3


def disassembly(path):
    return subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", path], check=True, stdout=subprocess.PIPE, text=True).stdout


def test_the_batch_module_has_no_scalar_stores_and_no_scratch(tmp_path, scenes):
    """gfx950 code objects of the example scenes with the batch kernel: none of the scalar-store, scalar-atomic or scalar-cache
    write-back instructions, and no scratch where the plain module has none."""
    if not os.path.exists(OBJDUMP):
        pytest.skip(OBJDUMP + " is not installed: the code objects were built, their disassembly cannot be read")
    s = "s" + "_"
    banned = re.compile(r"\b" + s + r"(?:buffer_|scratch_)?" + "sto" + r"re_|\b" + s + r"(?:buffer_)?" + "ato" + r"mic_|\b" + s + "dca" +
                        r"che_(?:wb|discard)", re.I)
    for name in ("scene", "scene4"):
        prog = scenes[name].flatten()
        plain, on = str(tmp_path / (name + "_plain")), str(tmp_path / (name + "_on"))
        gpu.compile_offline(prog, plain, assume_fast=True)
        gpu.compile_offline_views(prog, on, assume_fast=True)
        text = disassembly(on + ".co")
        assert "<lol_render_spec_batch>:" in text and "<lol_render_spec_batch_steps>:" in text
        assert not banned.search(text), banned.search(text).group(0)
        scratch = re.compile(r"\bscratch_(?:load|store)")
        if not scratch.search(disassembly(plain + ".co")):
            assert not scratch.search(text), name
