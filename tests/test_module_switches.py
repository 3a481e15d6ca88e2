"""The module switches as one mask (lol_gpu_compile_offline_module, gpu.compile_offline_module): its refusals, the entry points from
before it write what it writes, what a switch brings with it, and the bit values lol_gpu_diag.h documents.  Needs no GPU."""
import os
import re

import pytest

from loltracer_amd import gpu
from test_rays_cabi import ROOT, kernel_notes, read

ALL = gpu.MODULE_SWITCHES


@pytest.fixture(scope="module")
def prog(scenes):
    return scenes["scene4"].flatten()


@pytest.fixture(scope="module")
def module(prog, tmp_path_factory):
    """the base path of compile_offline_module's files for a set of switches, compiled once"""
    made, d = {}, tmp_path_factory.mktemp("modules")

    def get(*switches):
        if switches not in made:
            made[switches] = str(d / ("m_" + "_".join(switches)))
            gpu.compile_offline_module(prog, made[switches], switches)
        return made[switches]
    return get


def files(base):
    return read(base + ".hip", "rb"), read(base + ".co", "rb")


def test_refusals(prog, tmp_path):
    lib = gpu.gpu_lib()
    assert "lol_gpu_compile_offline_module" in gpu.DIAG_SYMBOLS
    assert re.search(r"\blol_gpu_compile_offline_module\(", read(os.path.join(ROOT, "include", "lol_gpu_diag.h")))
    assert lib.lol_gpu_compile_offline_module(None, b"gfx950", b"", 0, 0, 0, None, 0) == -3
    assert lib.lol_gpu_compile_offline_module(prog, b"gfx950", b"", 0, 128, 0, None, 0) == -3
    assert lib.lol_gpu_compile_offline_module(prog, b"gfx950", b"", 0, 0, 3, None, 0) == -3
    with pytest.raises(ValueError):
        gpu.compile_offline_module(prog, str(tmp_path / "bad"), ["view_batches", "view_batch"])
    assert not os.listdir(tmp_path)


# the entry point each switch had before, called for that switch alone; the last one with every other switch beside it is the full set
BEFORE = {
    ("samples",): lambda prog, p: gpu.compile_offline_samples(prog, p, 2),
    ("view_batches",): lambda prog, p: gpu.compile_offline_views(prog, p),
    ("view_samples",): lambda prog, p: gpu.compile_offline_view_samples(prog, p),
    ("view_blends",): lambda prog, p: gpu.compile_offline_view_blends(prog, p),
    ("view_blend_samples",): lambda prog, p: gpu.compile_offline_view_blend_samples(prog, p),
    ("ray_queries",): lambda prog, p: gpu.compile_offline_rays(prog, p),
    ("shade_queries",): lambda prog, p: gpu.compile_offline_shade(prog, p),
    ALL: lambda prog, p: gpu.compile_offline_shade(prog, p, enable=True, **{name: True for name in ALL if name != "shade_queries"}),
}


def test_every_switch_had_an_entry_point():
    assert [k[0] for k in BEFORE if len(k) == 1] == list(ALL) and ALL in BEFORE


@pytest.mark.parametrize("switches", BEFORE, ids="+".join)
def test_the_entry_point_before_it_writes_the_same_files(switches, prog, module, tmp_path):
    base = str(tmp_path / "before")
    BEFORE[switches](prog, base)
    assert files(base) == files(module(*switches))


def test_view_samples_brings_view_batches(module):
    base = module("view_samples")
    assert files(base) == files(module("view_samples", "view_batches"))
    assert "void lol_render_spec_batch(" in read(base + ".hip") and "lol_render_spec_batch" in kernel_notes(base + ".co")
    base = module("view_blend_samples")         # ... and nothing else brings anything: not even the two kernels this one is named after
    src, notes = read(base + ".hip"), kernel_notes(base + ".co")
    assert "lol_render_spec_batch_aa_lin" in notes and "void lol_render_spec_batch_aa_lin(" in src
    for kernel in ("lol_render_spec_batch_aa", "lol_render_spec_batch_lin"):
        assert kernel not in notes and not re.search(r"\b%s\b" % kernel, src), kernel


def test_the_documented_bits_are_the_librarys(prog, tmp_path):
    diag = read(os.path.join(ROOT, "include", "lol_gpu_diag.h"))
    documented = {name: int(bit) for bit, name in re.findall(r"^ \*\s+(\d+)\s+lol_gpu_set_(\w+)", diag, re.M)}
    assert documented == {name: 1 << i for i, name in enumerate(ALL)}
    lib = gpu.gpu_lib()
    for name, kernel in (("ray_queries", "lol_trace_spec"), ("shade_queries", "lol_shade_spec")):
        base = str(tmp_path / name)
        assert lib.lol_gpu_compile_offline_module(prog, b"gfx950", os.fsencode(base), 0, documented[name], 0, None, 0) == 0
        notes = kernel_notes(base + ".co")
        assert kernel in notes and not ({"lol_trace_spec", "lol_shade_spec"} - {kernel}) & notes.keys(), name
