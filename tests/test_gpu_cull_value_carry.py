"""The object's own last value folded into the carried culling bound (lol_codegen.hip, value_carry_constants) changes nothing a frame
holds: with the switch on and off, at 160x90 and 256x144, with 256 march steps and with 7, every field of the debug buffers — hit
distance, id, march and shadow step counts, the colour after gamma and the packed pixel — is the oracle's bit for bit (the host-libm
proviso of test_gpu_parity.check_against_oracle apart), in a fresh frame and in the third frame of a repeated view, whose pixels are
dealt to the waves by what they cost: lanes that are not neighbours then vote together.

Scenes: scene4; an object that is a chain of smooth unions with a round box in it; two culled objects (the bound is not generated for
a run of several: the policy, held here too); scene4 seen from inside the blob's bounding sphere; an object whose leaves differ in
scale by four orders of magnitude (a sphere of radius -20000, which the bound's radius does not cover).  These sizes are the smallest at
which the march and shadow loops, the cool-down and the per-wave votes all occur: several 64x16 regions, ragged at 160x90.  The bound
itself is proven in tests/test_cull_value_carry_bound.py; the oracle's frames are computed once per (scene, size, steps)."""
import os
import tempfile

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_views as V
from loltracer_amd import gpu, scene as S
from test_gpu_parity import check_against_oracle, gpu_render

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATS = ("materials { { shininess = 0, diffuse = (0,0,0), specular = (0,0,0), ambient = (0,0,0) },"
        " { shininess = 16, diffuse = (.15,.22,.19), specular = (.08,.08,.08), ambient = (.15,.22,.19) },"
        " { shininess = 25, diffuse = (.04,.03,.02), specular = (.05,.05,.05), ambient = (.04,.03,.02) } }\n")
HEAD = ("camera { point = %s, direction = (0.3, -0.7, -1), fov = 150 },\n"
        "point_light { point = (-2, 10, -1), diffuse_intensity = (4,4,4), specular_intensity = (4,4,4) },\n"
        "point_light { point = (-7, 2, -5), diffuse_intensity = (1,1.5,2), specular_intensity = (1,1.5,2) },\n")
BLOB = ("smooth_union { material = #1, smoothness = 3, a = smooth_union { smoothness = 3, a = sphere { point = (0, 1, -6), radius = 1 },"
        " b = sphere { point = (-1, 0.5, -3), radius = 3 } }, b = smooth_union { smoothness = 3, a = sphere { point = (-3, 4.5, -3), radius = 0.5 },"
        " b = smooth_union { smoothness = 3, a = sphere { point = (2, 2, -10), radius = 2 }, b = sphere { point = (6, 2, -10), radius = 5 } } } }")
CHAIN = ("smooth_union { material = #1, smoothness = 1.5, a = smooth_union { smoothness = 1, a = smooth_union { smoothness = 2,"
         " a = sphere { point = (0, 1, -6), radius = 1 }, b = box { point = (5, 1, -10), point2 = (1.5, 0.5, 1), radius = 0.25 } },"
         " b = sphere { point = (-3, 2, -4), radius = 1.2 } }, b = sphere { point = (7, 2.5, -12), radius = 2 } }")
SECOND = ("smooth_union { material = #2, smoothness = 1, a = smooth_union { smoothness = 1, a = sphere { point = (-8, 0, -9), radius = 1 },"
          " b = sphere { point = (-9, 1, -14), radius = 1.5 } }, b = sphere { point = (-12, 0.5, -6), radius = 1 } }")
# two small spheres in a union with a sphere of radius -20000: the bound takes radius 0 for it, its value is |p - c| + 20000, and the
# union's sum is rounded at ulp(20000) / 2 where that operand is saturated (tests/test_cull_value_carry_bound.py, mixed_scale_text)
MIXED = ("smooth_union { material = #1, smoothness = 1, a = smooth_union { smoothness = 1, a = sphere { point = (-5, 1, -8), radius = 1.5 },"
         " b = sphere { point = (5, 1, -8), radius = 1.5 } }, b = sphere { point = (0, 1, -8), radius = -20000 } }")
FLOOR = "plane { material = #2, y = -1 }"
CAMERA = "(-2, 6, 3)"


def text(camera, *objects):
    return MATS + "scene { " + HEAD % camera + ",\n".join(objects) + " }\n"


# name -> (text or None for the golden scene4, whether the value bound is generated with the switches on)
SCENES = {
    "scene4": (None, True),
    "chain-with-a-round-box": (text(CAMERA, CHAIN, FLOOR), True),
    "two-culled-objects": (text(CAMERA, BLOB, SECOND, FLOOR), False),
    "camera-inside-the-bound": (text("(-2, 4, -1)", BLOB, FLOOR), True),
    "mixed-scale-leaves": (text(CAMERA, MIXED, FLOOR), True),
}
ON = {"LOL_GPU_CULL_CARRY": "1", "LOL_GPU_CULL_VALUE_CARRY": "1"}
OFF = {"LOL_GPU_CULL_VALUE_CARRY": "0"}
_scenes, _frames, _dist, _generated = {}, {}, {}, {}


def scene_of(name):
    if name not in _scenes:
        t = SCENES[name][0]
        _scenes[name] = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", "scene4.lol")) if t is None else S.Scene.parse_string(t)
    return _scenes[name]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module", autouse=True)
def oracle_frames_once():
    """oracle_lib.render_rows, remembered (read-only arrays; last_counters restored), as in tests/test_gpu_hostile.py"""
    real = O.render_rows

    def render_rows(scene, w, h, y0, y1, max_steps=256, camera=None, want_steps=False):
        assert camera is None
        key = (id(scene), w, h, y0, y1, max_steps, want_steps)
        if key not in _frames:
            out = real(scene, w, h, y0, y1, max_steps, camera=camera, want_steps=want_steps)
            for a in out:
                if a is not None:
                    a.setflags(write=False)
            _frames[key] = (scene, out, O.last_counters)
        _, out, O.last_counters = _frames[key]
        return out
    O.render_rows = render_rows
    yield
    O.render_rows = real


def oracle_dist(name, sc, w, h, max_steps):
    key = (name, w, h, max_steps)
    if key not in _dist:
        d = np.zeros((h, w), dtype=np.float32)
        for y in range(h):
            for x in range(w):
                d[y, x] = O.probe(sc, w, h, x, y, max_steps).hit_dist
        _dist[key] = d
    return _dist[key]


def assert_frame_is_oracle(g, name, sc, w, h, max_steps, what):
    try:
        mism = check_against_oracle(g, sc, w, h, max_steps=max_steps)
        assert np.array_equal(V.bits(g["dist"]), V.bits(oracle_dist(name, sc, w, h, max_steps))), "hit distances differ"
    except AssertionError as err:
        raise AssertionError(f"{name} {w}x{h}, {max_steps} steps, {what}: {err}") from err
    return mism


def has_value_bound(name, switches):
    """whether the scene's own kernel, generated under these switches, folds the object's value into the carried bound (no device)"""
    key = (name, tuple(sorted(switches.items())))
    if key not in _generated:
        with tempfile.TemporaryDirectory() as d:
            gpu.compile_offline(scene_of(name).flatten(), os.path.join(d, "s"), assume_fast=True)
            src = open(os.path.join(d, "s.hip")).read()
        _generated[key] = "const float vg = " in src[src.index("struct SpecSdfFast"):]
    return _generated[key]


@pytest.mark.parametrize("switch", ["on", "off"])
@pytest.mark.parametrize("max_steps", [256, 7])
@pytest.mark.parametrize("w,h", [(160, 90), (256, 144)])
@pytest.mark.parametrize("name", list(SCENES))
def test_every_debug_field_is_the_oracles(torch_cuda, monkeypatch, name, w, h, max_steps, switch):
    monkeypatch.setenv("LOL_GPU_TUNING", "1")                # (the library honours A/B switches only beside this)
    switches = ON if switch == "on" else OFF
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    sc = scene_of(name)
    assert has_value_bound(name, switches) == (switch == "on" and SCENES[name][1])
    r = gpu.Renderer(0)
    r.want_kernel = "lol_render_spec"
    try:
        assert_frame_is_oracle(gpu_render(torch_cuda, r, sc, w, h, max_steps=max_steps), name, sc, w, h, max_steps, "fresh")
        assert "LOL_GPU_CULL_VALUE_CARRY=" + switches["LOL_GPU_CULL_VALUE_CARRY"] in gpu.tuning_switches()
        g = gpu_render(torch_cuda, r, sc, w, h, max_steps=max_steps, repeat=3)          # the table-dealt order
        assert_frame_is_oracle(g, name, sc, w, h, max_steps, "third frame of a repeated view")
    finally:
        r.close()


def test_the_default_is_on_for_scene4_alone(torch_cuda):
    """no switch set: scene4's kernel carries the value bound, the other three scenes' kernels do not force anything"""
    assert "LOL_GPU_TUNING" not in os.environ
    assert has_value_bound("scene4", {})
    assert not has_value_bound("two-culled-objects", {})
    sc = scene_of("scene4")
    r = gpu.Renderer(0)
    r.want_kernel = "lol_render_spec"
    try:
        assert_frame_is_oracle(gpu_render(torch_cuda, r, sc, 160, 90, repeat=3), "scene4", sc, 160, 90, 256, "default switches, third frame")
    finally:
        r.close()
