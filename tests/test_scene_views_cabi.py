"""Scene views, the part that needs no GPU: the structure module's source and code object (two scenes of one structure give the same
bytes), the scene's own module left as it was, the C ABI's symbols and refusals, and the host's scene helpers (clone, same_structure,
tween)."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from loltracer_amd import gpu, scene as S
from test_rays_cabi import ROOT, kernel_notes, read
from test_views_cabi import SOURCE_BEFORE_BATCHES

EXPORTED = ("lol_gpu_render_scene_views", "lol_gpu_set_scene_views", "lol_gpu_scene_views")
DIAG = ("lol_gpu_scene_views_kernel_name", "lol_gpu_scene_views_state", "lol_gpu_compile_offline_scene_views", "lol_gpu_interp_fast_paths")
KERNELS = ("lol_render_param_batch", "lol_render_param_batch_lin")


def changed_scene4(sc):
    """scene4 with a sphere moved and a radius, a smoothness, a light and a material changed: same structure, other numbers"""
    out = sc.clone()
    nodes = out.c.nodes
    spheres = [i for i in range(out.c.n_nodes) if nodes[i].type == S.NODE_SPHERE]
    unions = [i for i in range(out.c.n_nodes) if nodes[i].type == S.NODE_SMOOTH_UNION]
    nodes[spheres[0]].point.x += 0.75
    nodes[spheres[1]].radius *= 1.5
    nodes[unions[0]].smoothness = 2.7182817
    out.c.lights[0].point.y += 2.0
    out.c.materials[1].diffuse.x = 0.125
    return out


def test_the_symbols_exist():
    lib = gpu.gpu_lib()
    hdr, diag = read(os.path.join(ROOT, "include", "lol_gpu.h")), read(os.path.join(ROOT, "include", "lol_gpu_diag.h"))
    for name in EXPORTED:
        assert getattr(lib, name) is not None and name in gpu.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % name, hdr), name
    for name in DIAG:
        assert getattr(lib, name) is not None and name in gpu.DIAG_SYMBOLS and re.search(r"\b%s\(" % name, diag), name
    assert int(re.search(r"#define\s+LOL_GPU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6 == lib.lol_gpu_abi_version()      # new entry points only
    # what is out of scope is said in the header
    text = hdr[hdr.index("Scene views:"):hdr.index("int  lol_gpu_render_scene_views(")]
    for word in ("supersampled and adaptive", "ray and shading queries", "row partitions", "lol_gpu_multi_", "host surfaces", "renderer.h",
                 "not kept across uploads"):
        assert word in text, word
    # refusals that need no device: no context, no cameras, no scenes
    assert lib.lol_gpu_render_scene_views(None, None, None, 1, 1, 8, 8, 1, None, 32, 256, None, None) == -3
    assert lib.lol_gpu_set_scene_views(None, 1) == -3 and lib.lol_gpu_scene_views(None) == -3
    assert lib.lol_gpu_scene_views_kernel_name(None, 1) == b"" and lib.lol_gpu_scene_views_state(None) == -3
    assert lib.lol_gpu_compile_offline_scene_views(None, b"gfx950", b"", None, 0) == -3
    assert lib.lol_gpu_interp_fast_paths(None, C.byref(C.c_int()), C.byref(C.c_uint()), C.byref(C.c_uint())) == -3
    for method in ("set_scene_views", "scene_views", "scene_views_kernel_name", "scene_views_state", "render_scene_views_into"):
        assert hasattr(gpu.Renderer, method), method
    # the structure module is no module switch: seven of those, and their mask ends at 127 (tests/test_module_switches.py)
    assert len(gpu.MODULE_SWITCHES) == 7 and not any("scene" in name for name in gpu.MODULE_SWITCHES)


def test_two_scenes_of_one_structure_share_source_and_code_object(tmp_path, scenes):
    a = scenes["scene4"]
    b = changed_scene4(a)
    assert S.same_structure(a, b) and a.flatten().tables() != b.flatten().tables()
    pa, pb = str(tmp_path / "a"), str(tmp_path / "b")
    # each scene in a process of its own with the disk cache off: both code objects come out of the compiler — the same compiler,
    # whichever hipRTC this process may have loaded by now — and not out of a cache keyed by the (equal) source
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from loltracer_amd import gpu, scene as S\n"
            "import test_scene_views_cabi as T\n"
            "sc = S.Scene.parse_file(%r)\n"
            "log = gpu.compile_offline_scene_views((T.changed_scene4(sc) if sys.argv[2] == 'changed' else sc).flatten(), sys.argv[1])\n"
            "assert 'cache' not in log, log\n") % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden", "scenes", "scene4.lol"))
    for base, which in ((pa, "as-it-is"), (pb, "changed")):
        p = subprocess.run([sys.executable, "-c", code, base, which], env=dict(os.environ, LOL_GPU_CACHE_DIR=""), capture_output=True,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stderr
    src = read(pa + ".hip", "rb")
    assert src == read(pb + ".hip", "rb")
    assert read(pa + ".co", "rb") == read(pb + ".co", "rb")
    notes = kernel_notes(pa + ".co")
    for kernel in KERNELS:
        assert kernel in notes, kernel
    text = src.decode()
    # every number is a read of the record: no literal of the scene in the SDF, the objects in file order, no culling test, no fast path
    sdf = text[text.index("struct ParamSdf"):text.index("}  // namespace lol")]
    assert "__builtin_bit_cast(float" not in sdf and "vote(" not in sdf and "_fast" not in sdf and "fastdiv" not in sdf
    assert sdf.count("sd_sphere(p, K[") == 2 * 5 and sdf.count("sminf_(") == 2 * 4 and "K[70]" in sdf      # (eval and eval_dist)
    assert sdf.index("best_id = 1u") < sdf.index("best_id = 2u")
    assert text.startswith('#include "lol_kernel_scenes.h"\n')


def test_another_structure_is_another_source(tmp_path, scenes):
    pa, pb = str(tmp_path / "scene4"), str(tmp_path / "scene")
    gpu.compile_offline_scene_views(scenes["scene4"].flatten(), pa)
    gpu.compile_offline_scene_views(scenes["scene"].flatten(), pb)
    assert read(pa + ".hip", "rb") != read(pb + ".hip", "rb")
    assert not S.same_structure(scenes["scene4"], scenes["scene"])
    # scene.lol has four top-level objects: the primary march asks for the id once, as in the scene's own kernel
    assert "ASK_ID_ONCE = true" in read(pb + ".hip") and "ASK_ID_ONCE = false" in read(pa + ".hip")
    for kernel in KERNELS:
        assert kernel in kernel_notes(pb + ".co"), kernel


def test_the_scenes_own_module_is_what_it_was(tmp_path, scenes):
    """the structure module is a code object of its own: the scene's module without any switch is the source it was before batches
    existed (tests/test_views_cabi.py records it), is not handed the new header's name, and compiles to the same bytes twice"""
    for name, want in SOURCE_BEFORE_BATCHES.items():
        base, again = str(tmp_path / name), str(tmp_path / (name + "_again"))
        gpu.compile_offline_module(scenes[name].flatten(), base, ())
        src = read(base + ".hip", "rb")
        assert hashlib.sha256(src).hexdigest() == want, name
        assert b"scenes" not in src and b"param" not in src
        gpu.compile_offline(scenes[name].flatten(), again)
        assert read(again + ".co", "rb") == read(base + ".co", "rb"), name
        assert not set(KERNELS) & kernel_notes(base + ".co").keys()


def test_clone_round_trips_to_equal_bytes(scenes):
    lib = S.host_lib()
    for name in ("scene", "scene4"):
        a = scenes[name]
        b = a.clone()
        assert b.ptr and C.addressof(b.c) != C.addressof(a.c)
        assert a.tables() == b.tables() and a.flatten().tables() == b.flatten().tables()
        b.c.nodes[0].point.x += 1.0                                 # the copy is its own
        assert a.tables() != b.tables()
    out = C.POINTER(S.SceneStruct)()
    assert lib.lol_scene_clone(None, C.byref(out)) == S.LOL_ERR_IO and not out      # (what the header says of a NULL argument)
    assert lib.lol_scene_clone(scenes["scene"].ptr, None) == S.LOL_ERR_IO
    empty = S.Scene(lib.lol_scene_new())
    assert empty.clone().tables() == empty.tables()


def test_same_structure(scenes):
    a = scenes["scene4"]
    assert S.same_structure(a, a) and S.same_structure(a, changed_scene4(a))
    assert not S.same_structure(a, scenes["scene"]) and not S.same_structure(scenes["scene"], a)
    b = a.clone()
    union = next(i for i in range(b.c.n_nodes) if b.c.nodes[i].type == S.NODE_SMOOTH_UNION)
    b.c.nodes[union].a, b.c.nodes[union].b = b.c.nodes[union].b, b.c.nodes[union].a
    assert not S.same_structure(a, b)
    c = a.clone()
    c.c.nodes[c.c.roots[0]].material = 0                            # which material an object wears is a number
    assert S.same_structure(a, c)


def scene_floats(sc):
    """every float tween interpolates, as one float32 array, in tween's order"""
    c = sc.c
    out = []
    for i in range(c.n_nodes):
        n = c.nodes[i]
        out += [n.point.x, n.point.y, n.point.z, n.half_extent.x, n.half_extent.y, n.half_extent.z, n.radius, n.smoothness]
    for i in range(c.n_lights):
        out += list((C.c_float * 9).from_buffer_copy(c.lights[i]))
    for i in range(c.n_materials):
        out += list((C.c_float * 10).from_buffer_copy(c.materials[i]))
    out += list(c.ambient_color.tuple())
    return np.array(out, dtype=np.float32)


def test_tween_is_the_float32_interpolation(scenes):
    a = scenes["scene4"]
    b = changed_scene4(a)
    b.c.ambient_color.y = 0.375
    b.c.camera.point.x += 5.0                                        # the camera is a's whatever b's is
    fa, fb = scene_floats(a), scene_floats(b)
    for t in (0.0, 1.0, 0.5, 0.3):
        m = S.tween(a, b, t)
        want = fa + (fb - fa) * np.float32(t)                        # numpy float32: every operation rounded to binary32
        assert np.array_equal(scene_floats(m).view(np.uint32), want.astype(np.float32).view(np.uint32)), t
        assert S.same_structure(a, m)
        assert bytes(memoryview(m.c.camera).cast("B")) == bytes(memoryview(a.c.camera).cast("B"))
    assert np.array_equal(scene_floats(S.tween(a, b, 0.0)), fa) and np.array_equal(scene_floats(S.tween(a, b, 1.0)), fb)
    with pytest.raises(ValueError):
        S.tween(a, scenes["scene"], 0.5)
    # numbers whose exponents lie far apart, subnormals, infinities: still one binary32 operation each (a sum or difference taken
    # in doubles and rounded afterwards is rounded twice, and differs from these on such operands)
    wild = [1.0, -1.0000001, 3.4e38, -3.4e38, 1e-45, 1.17549435e-38, 16777216.0, 0.99999994, 1e30, -1e-30, float("inf"), 5e-324]
    x, y = a.clone(), a.clone()
    sphere = next(i for i in range(a.c.n_nodes) if a.c.nodes[i].type == S.NODE_SPHERE)
    for j, (u, v) in enumerate(zip(wild, wild[5:] + wild[:5])):
        n = x.c.nodes[(sphere + j) % a.c.n_nodes], y.c.nodes[(sphere + j) % a.c.n_nodes]
        n[0].point.x, n[1].point.x, n[0].radius, n[1].radius = u, v, v, u
    fx, fy = scene_floats(x), scene_floats(y)
    for t in (0.5, 0.3, 0.99999994):
        with np.errstate(all="ignore"):
            want = fx + (fy - fx) * np.float32(t)
        got = scene_floats(S.tween(x, y, t))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), t
    assert S._lerp32(np.float32(1.0), np.float32(3.0), np.float32(0.5)).dtype == np.float32      # (no double in between)
    # two tweened scenes flatten to equal opcodes and ids, and to other numbers
    p, q = S.tween(a, b, 0.25).flatten(), S.tween(a, b, 0.75).flatten()
    assert (p.n_ops, p.n_lights, p.n_materials, p.n_roots, p.max_stack) == (q.n_ops, q.n_lights, q.n_materials, q.n_roots, q.max_stack)
    assert [(p.ops[i].op, p.ops[i].id) for i in range(p.n_ops)] == [(q.ops[i].op, q.ops[i].id) for i in range(q.n_ops)]
    assert p.tables() != q.tables()
    assert S.shutter_times(0, 1, 1) == [0.5] and S.shutter_times(1, 2, 2) == [0.625, 0.875]
    with pytest.raises(ValueError):
        S.shutter_times(2, 2, 1)


def test_the_documents_quote_the_committed_record():
    """README.md and DESIGN.md quote the rate record's own numbers and name the arm the record found fastest, and the record says what
    the feature was accepted on: every one-call arm faster than the per-frame uploads by more than the arms' spread"""
    import json
    rec = json.load(open(os.path.join(ROOT, "profiles", "r18_scene_views_rate.json")))
    assert rec["scene"] == "scene4" and (rec["w"], rec["h"], rec["frames"]) == (128, 128, 64) and rec["window_s"] >= 1.0
    assert rec["frames_equal_across_arms"] and rec["distinct_frames"] == 64 and rec["blend"]["frames_equal_across_arms"]
    assert "specialisation off" in rec["arms_are"]["b"] and "fast paths" in rec["arms_are"]["f"]
    assert rec["fast_interpreter_proofs"]["sqrt_kind"] == 3 and rec["fast_interpreter_proofs"]["proven_blend_factors"] >= 1
    arms = {x: rec["arms"][x] for x in "abfc"}
    spread = max(x["max_ms"] - x["min_ms"] for x in arms.values())
    for x in "bfc":
        assert rec[x + "_faster_than_a_by_more_than_the_spread"] and arms["a"]["min_ms"] - arms[x]["max_ms"] > spread, x
    fastest = [x for x in "bfc" if all(arms[x]["max_ms"] < arms[y]["min_ms"] for y in "bfc" if y != x)]
    assert rec["fastest_of_b_f_c"] == (fastest[0] if fastest else "none (windows overlap)")
    quoted = [arms[x]["median_ms"] for x in "abfc"] + [rec["blend"]["arms"][x]["median_ms"] for x in "bfc"]
    for doc in ("README.md", "DESIGN.md"):
        text = read(os.path.join(ROOT, doc))
        at = text.index("r18_scene_views_rate.json")
        part = text[max(0, at - 4000):at + 4000]
        for v in quoted:
            assert "%s ms" % v in part, (doc, v)
    # which arm is fastest is said as the record says it: nowhere is the structure module called the faster kernel unless it was
    design, readme = read(os.path.join(ROOT, "DESIGN.md")), read(os.path.join(ROOT, "README.md"))
    assert ("**(%s) is the fastest of the three**" % rec["fastest_of_b_f_c"]) in design
    assert ("NOT the default context's interpreter" in readme) == (rec["fastest_of_b_f_c"] != "c")
