"""Ray queries, the part that needs no GPU: the symbols, the scene compiler's source with and without lol_gpu_set_ray_queries, and
the gfx950 code object with its resources."""
import hashlib
import json
import os
import re
import struct
import subprocess

import pytest

import scene_shapes as C
from loltracer_amd import gpu
from test_views_cabi import SOURCE_BEFORE_BATCHES

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "lol_trace_spec"
NEIGHBOUR = "lol_render_spec_steps"
HEAD = "void %s(const lol::RayQuery Q) {" % KERNEL
INCLUDE = '#include "lol_kernel_rays.h"\n'
EXPORTED = ("lol_gpu_trace_rays", "lol_gpu_trace_pixels", "lol_gpu_pick", "lol_gpu_set_ray_queries", "lol_gpu_ray_queries")
DIAG = ("lol_gpu_trace_kernel_name", "lol_gpu_compile_offline_rays")
OTHERS = ("view_blends", "samples", "view_batches", "view_samples", "view_blend_samples")


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
    # refusals that need no device: no context
    hits = gpu.Hits(8, 8, 8, 8)
    assert lib.lol_gpu_trace_rays(None, 8, 1, 256, hits, None) == -3
    assert lib.lol_gpu_trace_pixels(None, None, 8, 8, 256, 8, 1, hits, None) == -3
    assert lib.lol_gpu_pick(None, None, 8, 8, 256, 0, 0, None) == -3
    assert lib.lol_gpu_set_ray_queries(None, 1) == -3 and lib.lol_gpu_ray_queries(None) == -3
    assert lib.lol_gpu_trace_kernel_name(None) == b""
    for method in ("set_ray_queries", "ray_queries", "trace_kernel_name", "trace_rays_into", "trace_pixels_into", "pick"):
        assert hasattr(gpu.Renderer, method), method
    for text in ("shading or shadow queries", "lol_gpu_multi_", "rays in host memory", "renderer.h protocol", "(s x + i, s y + j)"):
        assert text in hdr, text                     # what is out of scope, and which pixels the sample rays are, is said in the header


def test_without_the_switch_every_module_is_what_it_was(tmp_path, scenes):
    for name, want in SOURCE_BEFORE_BATCHES.items():
        prog = scenes[name].flatten()
        plain, off = str(tmp_path / (name + "_plain")), str(tmp_path / (name + "_off"))
        gpu.compile_offline(prog, plain)
        gpu.compile_offline_rays(prog, off, enable=False)
        src = read(plain + ".hip", "rb")
        assert hashlib.sha256(src).hexdigest() == want, name
        assert read(off + ".hip", "rb") == src, name
        assert read(off + ".co", "rb") == read(plain + ".co", "rb"), name
        assert b"trace" not in src and b"rays" not in src


def fnv64(data, h=0xcbf29ce484222325):
    for c in data:
        h = ((h ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def loaded_sections(path):
    """[(name, offset, size)] of a code object's allocated PROGBITS and NOTE sections, in section-header order"""
    text = subprocess.run([READELF, "-S", "-W", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    rows = re.findall(r"\]\s+(\.\S+)\s+(\w+)\s+[0-9a-f]+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+[0-9a-f]+\s+([A-Za-z]*)\s+\d+\s+\d+\s+\d+", text)
    return [(name, int(off, 16), int(size, 16)) for name, kind, off, size, flags in rows if "A" in flags and kind in ("PROGBITS", "NOTE")]


def test_the_key_covers_what_the_device_loads(tmp_path, scenes):
    """lol_gpu_kernel_key's function of a code object (gpu.code_key): FNV-1a over the sections the device loads, each as its size and
    its bytes.  The compilation-unit id hipRTC derives from the header texts — a symbol's NAME — is not in it, so a kernel header may
    change its text without renaming the instructions of modules that do not change; every loaded byte is; and a buffer that is no
    sound ELF file gets the hash of all its bytes, whatever its headers claim."""
    base = str(tmp_path / "scene4")
    gpu.compile_offline(scenes["scene4"].flatten(), base)
    co = read(base + ".co", "rb")
    key = gpu.code_key(co)
    assert re.fullmatch(r"[0-9a-f]{16}", key) and key != "%016x" % fnv64(co)
    secs = loaded_sections(base + ".co")
    assert sorted(n for n, _, _ in secs) == [".note", ".rodata", ".text"]
    h = 0xcbf29ce484222325
    for _, off, size in secs:
        h = fnv64(co[off:off + size], fnv64(struct.pack("<Q", size), h))
    assert key == "%016x" % h                                             # the definition of include/lol_gpu.h, restated
    renamed = re.sub(rb"(__hip_cuid_)[0-9a-f]{16}", rb"\g<1>0123456789abcdef", co)
    assert renamed != co and len(renamed) == len(co) and gpu.code_key(renamed) == key
    for _, off, size in secs:
        for at in (off, off + size // 2, off + size - 1):
            flipped = co[:at] + bytes([co[at] ^ 1]) + co[at + 1:]
            assert gpu.code_key(flipped) != key, (at, off, size)
    for n in (10, 63, 64):
        assert gpu.code_key(co[:n]) == "%016x" % fnv64(co[:n]), n
    past = co[:40] + struct.pack("<Q", len(co) + 1) + co[48:]                # e_shoff beyond the end
    assert gpu.code_key(past) == "%016x" % fnv64(past)
    e_shoff, = struct.unpack_from("<Q", co, 40)
    e_shnum, = struct.unpack_from("<H", co, 60)
    text_off = dict((n, off) for n, off, _ in secs)[".text"]
    for i in range(e_shnum):                                              # .text's header claims a size beyond the file
        if struct.unpack_from("<Q", co, e_shoff + 64 * i + 24)[0] == text_off:
            wild = co[:e_shoff + 64 * i + 32] + struct.pack("<Q", len(co)) + co[e_shoff + 64 * i + 40:]
            assert gpu.code_key(wild) == "%016x" % fnv64(wild)
            break
    else:
        assert False, "no section header for .text"
    assert gpu.code_key(b"") == "%016x" % fnv64(b"")


def test_the_switch_appends_the_query_kernel(tmp_path, scenes):
    for name in SOURCE_BEFORE_BATCHES:
        prog = scenes[name].flatten()
        plain, on = str(tmp_path / (name + "_plain")), str(tmp_path / (name + "_on"))
        gpu.compile_offline(prog, plain)
        gpu.compile_offline_rays(prog, on)                                  # (raises unless it compiled for gfx950)
        src, base = read(on + ".hip"), read(plain + ".hip")
        assert src.startswith(base), name                                   # appended after everything else
        tail = src[len(base):]
        assert tail.startswith(INCLUDE), name
        assert tail.count(HEAD) == 1 and src.count(KERNEL) == 1, name
        assert "lol::trace_rays(exact, exact, false, Q)" in tail, name
        assert "Launch" not in tail and "lds" not in tail and "shade_pixel" not in tail, name
        assert not re.search(r"void lol_render_spec\w*\(", tail), name      # no frame kernel comes with it
        assert KERNEL in kernel_notes(on + ".co") and KERNEL not in kernel_notes(plain + ".co"), name
    fast = str(tmp_path / "fast")
    gpu.compile_offline_rays(scenes["scene4"].flatten(), fast, assume_fast=True)
    tail = read(fast + ".hip").split(INCLUDE)[1]
    assert "lol::SpecSdfFast fast;" in tail and "lol::trace_rays(fast, exact, true, Q)" in tail


def test_both_tiers_of_a_mid_size_scene_carry_it(tmp_path):
    prog = C.scene_of(C.MID).flatten()
    assert 256 < prog.n_ops <= 1024
    for form, out_of_line in ((0, False), (1, True), (2, False)):
        base = str(tmp_path / ("tier%d" % form))
        gpu.compile_offline_rays(prog, base, form=form)
        src = read(base + ".hip")
        assert ("SdfOut" in src) == out_of_line, form
        assert src.count("void %s(" % KERNEL) == 1 and src.count(INCLUDE) == 1, form
        assert KERNEL in kernel_notes(base + ".co"), form
    with pytest.raises(gpu.GpuError) as e:
        gpu.compile_offline_rays(prog, str(tmp_path / "bad"), form=3)
    assert e.value.status == -3


def test_the_switch_goes_with_the_other_switches(tmp_path, scenes):
    """Beside each other switch, and beside all of them, the module is THAT module with this kernel appended last, and it compiles
    for gfx950 whichever headers the others had hipRTC handed; with the switch off it is that module byte for byte."""
    prog = scenes["scene4"].flatten()
    lib = gpu.gpu_lib()
    assert lib.lol_gpu_compile_offline_rays(None, b"gfx950", b"", 0, 1, 0, 0, None, 0) == -3
    assert lib.lol_gpu_compile_offline_rays(prog, b"gfx950", b"", 0, 1, 32, 0, None, 0) == -3
    assert lib.lol_gpu_compile_offline_rays(prog, b"gfx950", b"", 0, 1, -1, 0, None, 0) == -3
    bases = {
        "view_blends": lambda p: gpu.compile_offline_view_blends(prog, p),
        "samples": lambda p: gpu.compile_offline_samples(prog, p, 2),
        "view_batches": lambda p: gpu.compile_offline_views(prog, p),
        "view_samples": lambda p: gpu.compile_offline_view_samples(prog, p),
        "view_blend_samples": lambda p: gpu.compile_offline_view_blend_samples(prog, p),
        "all": lambda p: gpu.compile_offline_view_blend_samples(prog, p, view_blends=True, samples=True, view_batches=True, view_samples=True),
    }
    for switch, compile_base in bases.items():
        base_path, both, alone = (str(tmp_path / (k + "_" + switch)) for k in ("base", "both", "alone"))
        compile_base(base_path)
        others = {k: True for k in OTHERS} if switch == "all" else {switch: True}
        gpu.compile_offline_rays(prog, both, **others)                      # (raises unless it compiled)
        src, base = read(both + ".hip"), read(base_path + ".hip")
        assert KERNEL not in base, switch
        assert src.startswith(base), switch
        tail = src[len(base):]
        assert tail.startswith(INCLUDE) and tail.count(HEAD) == 1 and src.rstrip().endswith("}"), switch
        assert kernel_notes(both + ".co").keys() == kernel_notes(base_path + ".co").keys() | {KERNEL}, switch
        gpu.compile_offline_rays(prog, alone, enable=False, **others)
        for ext in (".hip", ".co"):
            assert read(alone + ext, "rb") == read(base_path + ext, "rb"), (switch, ext)


RESOURCE_MODULES = (("scene4", True, 0), ("scene", True, 0), ("chain140", False, 1), ("chain140", False, 2))
VGPR_CAP = 64                            # 8 waves per SIMD: what tests/test_view_blend_samples_cabi.py holds the neighbouring kernels to
RECORD = os.path.join(ROOT, "profiles", "r13_rays_kernel_resources.json")


def resources(tmp_path, scenes):
    out = []
    for name, fast, form in RESOURCE_MODULES:
        prog = (scenes[name] if name in scenes else C.scene_of(C.MID)).flatten()
        base = str(tmp_path / ("%s_%d" % (name, form)))
        gpu.compile_offline_rays(prog, base, assume_fast=fast, form=form)
        notes = kernel_notes(base + ".co")
        rec = dict(scene=name, form=form, assume_fast=fast)
        # (a module above 256 ops holds no counting twin: lol_render_spec itself counts there)
        rec["neighbour"] = NEIGHBOUR if NEIGHBOUR in notes else "lol_render_spec"
        for k in (KERNEL, rec["neighbour"]):
            if k in notes:
                rec[k] = dict(vgprs=int(notes[k]["vgpr_count"]), sgprs=int(notes[k]["sgpr_count"]),
                              scratch_bytes_per_lane=int(notes[k]["private_segment_fixed_size"]),
                              lds_bytes=int(notes[k]["group_segment_fixed_size"]))
        out.append(rec)
    return out


def test_resources_of_the_new_kernel(tmp_path, scenes):
    """From the code object's own metadata, for scene4, scene.lol and the mid-size scene in both forms: no scratch, no LDS, and at
    most the 64 VGPRs that keep 8 waves per SIMD.  profiles/r13_rays_kernel_resources.json records the figures beside those of
    lol_render_spec_steps of the same module (a module above 256 ops holds no counting twin: lol_render_spec counts there)."""
    recorded = json.loads(read(RECORD))["kernels"]
    assert len(recorded) == len(RESOURCE_MODULES)
    for now, rec in zip(resources(tmp_path, scenes), recorded):
        k = now[KERNEL]
        assert k["scratch_bytes_per_lane"] == 0 and k["lds_bytes"] == 0, now
        assert k["vgprs"] <= VGPR_CAP, now
        assert (rec["scene"], rec["form"], rec["assume_fast"]) == (now["scene"], now["form"], now["assume_fast"])
        # (the record is one compiler's figures: held to the same bounds, not to equality with this compiler's)
        assert rec[KERNEL]["scratch_bytes_per_lane"] == 0 and rec[KERNEL]["vgprs"] <= VGPR_CAP, rec
