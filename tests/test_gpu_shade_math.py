"""The per-pixel work around the loops of the scene kernel's fast pipeline (lol_kernel.h, ShadeMath): the proven root and reciprocal
of the five normalisations.  It is an A/B switch (LOL_GPU_SHADE_MATH beside LOL_GPU_TUNING: 0 off, 1 the roots alone, 3 both), and
nothing a frame holds may depend on it: with the switch on and off every field of the debug buffers — hit
distance bits, id, march and shadow step counts, the float colour — and the packed pixels are the same arrays, and the oracle's
(test_gpu_parity.check_against_oracle: no tolerance of its own beyond that function's host-libm proviso).

Sizes: 67x35 — odd both ways, so that one pixel looks exactly along the camera's direction, and no multiple of the 16x4 patch, so
clamped lanes occur; several waves.  Scenes: scene4 and scene.lol, and two scenes built to leave the proven domain of the roots: a
light exactly on the surface point the centre pixel hits (squared length 0) and a floor so far from the origin that the four normal
taps are equal (a zero normal).  Their waves are shaded again by the plain pipeline, so the frame stays the oracle's.  The oracle's
frames are computed once per scene."""
import os

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_views as V
from loltracer_amd import gpu, scene as S
from test_gpu_parity import check_against_oracle, gpu_render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 67, 35
MATS = ("materials { { shininess = 0, diffuse = (0,0,0), specular = (0,0,0), ambient = (0,0,0) },"
        " { shininess = 16, diffuse = (.15,.22,.19), specular = (.3,.2,.1), ambient = (.15,.22,.19) },"
        " { shininess = 25, diffuse = (.04,.03,.02), specular = (.05,.05,.05), ambient = (.04,.03,.02) } }\n")
WALL = "box { material = #1, point = (0, 0, -10), point2 = (5, 5, 0.75), radius = 0.25 }"          # its front face: z = -9


def text(camera, lights, *objects):
    lights = "".join("point_light { point = %s, diffuse_intensity = (4,4,4), specular_intensity = (4,3,2) },\n" % p for p in lights)
    return MATS + "scene { camera { %s },\n" % camera + lights + ",\n".join(objects) + " }\n"


SCENES = {
    "scene4": None,
    "scene": None,
    # the centre pixel looks along (0, 0, -1) and hits the wall at (0, 0, -9) after one step of 9: the light is that point
    "light-on-the-hit": text("point = (0, 0, 0), direction = (0, 0, -1), fov = 90", ["(0, 0, -9)", "(3, 4, 2)"], WALL),
    # ulp(999990) = 1/16 and dist / 100 < 1/32: the taps p.y +- h round to p.y, the four values are equal and their sum is 0
    "equal-taps": text("point = (0, 999992, 0), direction = (0, -1, -0.5), fov = 90", ["(0, 999995, 0)"], "plane { material = #1, y = 999990 }"),
}
_scenes, _frames, _renders = {}, {}, {}
FIELDS = ("xrgb", "rgb", "dist", "id", "steps")


def scene_of(name):
    if name not in _scenes:
        t = SCENES[name]
        _scenes[name] = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol")) if t is None else S.Scene.parse_string(t)
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


def render(torch, monkeypatch, name, switches):
    """the debug frame of `name` under `switches`, and the frame of the non-counting kernel beside it; remembered"""
    key = (name, tuple(sorted(switches.items())))
    if key not in _renders:
        monkeypatch.setenv("LOL_GPU_TUNING", "1")                # (the library honours A/B switches only beside this)
        for k, v in switches.items():
            monkeypatch.setenv(k, v)
        sc = scene_of(name)
        r = gpu.Renderer(0)
        r.want_kernel = "lol_render_spec"
        try:
            g = gpu_render(torch, r, sc, W, H)
            for k, v in switches.items():
                assert k + "=" + v in gpu.tuning_switches()
            g["math"] = r.shade_math()
            frame = torch.full((H, W), 0x55AA55, dtype=torch.int32, device="cuda:0")
            r.render_into(frame.data_ptr(), W, H, 256, pitch_bytes=W * 4, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            g["plain_frame"] = frame.cpu().numpy().view(np.uint32)
        finally:
            r.close()
        _renders[key] = g
    return _renders[key]


def assert_same(a, b, what):
    for f in FIELDS:
        assert np.array_equal(V.bits(a[f]), V.bits(b[f])), "%s: %s differs" % (what, f)
    assert np.array_equal(a["plain_frame"], b["plain_frame"]), "%s: the non-counting kernel's frame differs" % what
    assert np.array_equal(a["plain_frame"], a["xrgb"]), "%s: the two kernels' frames differ" % what


def test_the_fast_sdf_names_its_shading_arithmetic_and_the_plain_one_does_not(tmp_path, monkeypatch):
    """no device: the generated source carries the member type Shade in the fast SDF alone, and not at all with the switch off"""
    assert "LOL_GPU_TUNING" not in os.environ
    prog = scene_of("scene4").flatten()
    gpu.compile_offline(prog, str(tmp_path / "on"), assume_fast=True)
    src = (tmp_path / "on.hip").read_text()
    exact, fast = src[src.index("struct SpecSdfExact"):src.index("struct SpecSdfFast")], src[src.index("struct SpecSdfFast"):]
    assert "struct Shade { static constexpr int ROOT = 3, RCP = 1; };" in fast
    assert "struct Shade" not in exact
    gpu.compile_offline(prog, str(tmp_path / "plain"), assume_fast=False)
    assert "struct Shade" not in (tmp_path / "plain.hip").read_text()
    monkeypatch.setenv("LOL_GPU_TUNING", "1")
    monkeypatch.setenv("LOL_GPU_SHADE_MATH", "0")
    gpu.compile_offline(prog, str(tmp_path / "off"), assume_fast=True)
    off = (tmp_path / "off.hip").read_text()
    assert off == "".join(line for line in src.splitlines(True) if "struct Shade {" not in line)          # nothing else differs


@pytest.mark.gpu
def test_the_proofs_are_reported_and_decide_the_forms(torch_cuda, monkeypatch):
    """MI355X: sqrt_r2 and the one-correction reciprocal — a proof that failed would leave the division in quietly, and every
    on / off comparison would still pass"""
    m = render(torch_cuda, monkeypatch, "scene4", {"LOL_GPU_SHADE_MATH": "1"})["math"]
    print("shade math:", m)
    assert m["root_kind"] == 3                                   # sqrt_r2, as for the SDF's own roots on this device
    p = m["proofs"]
    assert all(p[k]["mismatches"] is not None for k in ("rcp1", "rcp2"))
    lo, hi = 0x27800000, 0x5f800000                              # 2^-48 ... 2^64: the roots of squared lengths in [2^-96, inf)
    for k in p:                                                  # both forms are proven on that interval, so the cheaper is in use
        assert p[k]["interval"][0] <= lo and hi <= p[k]["interval"][1], (k, p[k])
    assert m["rcp_form"] == 1
    for k in p:                                                  # an interval free of mismatches holds 1.0f, or is empty
        a, b = p[k]["interval"]
        assert a > b or a <= 0x3f800000 <= b
        assert (p[k]["mismatches"] == 0) == ((a, b) == (0, 0xFFFFFFFF))
    off = render(torch_cuda, monkeypatch, "scene4", {"LOL_GPU_SHADE_MATH": "0"})["math"]
    assert (off["root_kind"], off["rcp_form"]) == (0, 0)


def test_the_degenerate_scenes_leave_the_roots_domain():
    """no device: by the oracle's own arithmetic the two built scenes feed a normalisation a squared length of exactly 0.  The centre
    pixel's ray is (0, 0, -1) and its hit distance 9: the hit point is the light's position, bit for bit.  Two thirds of the far
    floor's pixels have a normal of NaN — the reference's 0 * (1 / sqrt(0)) for a summed normal of exactly (0, 0, 0)."""
    sc = scene_of("light-on-the-hit")
    p = O.probe(sc, W, H, W // 2, H // 2)
    assert tuple(p.rd) == (0.0, 0.0, -1.0) and p.hit_dist == 9.0 and p.hit_id == 1
    hit = np.float32(0) + np.array(p.rd, dtype=np.float32) * np.float32(p.hit_dist)          # ro + rd * dist, ro = (0, 0, 0)
    light = np.array([0, 0, -9], dtype=np.float32)
    assert np.array_equal(hit, light) and float(((light - hit) ** 2).sum()) == 0.0
    sc = scene_of("equal-taps")
    zero = 0
    for y in range(0, H, 2):                                     # (the rays to the frame's upper edge are longer than 100 / 32)
        for x in range(0, W, 3):
            p = O.probe(sc, W, H, x, y)
            assert p.hit_id == 1
            zero += all(np.isnan(v) for v in p.normal)
    assert zero > 64 * 4 and all(np.isnan(v) for v in O.probe(sc, W, H, W // 2, H // 2).normal)          # whole waves of them


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene4", "scene", "light-on-the-hit", "equal-taps"])
def test_shade_math_on_and_off_are_the_oracles_frame(torch_cuda, monkeypatch, name):
    """... in the two degenerate scenes too (test_the_degenerate_scenes_leave_the_roots_domain).  For the light on the hit point the
    fast root of 0 is NaN where the reference's light distance is 0, which bounds that pixel's shadow march: its step count, held
    to the oracle's here, is the plain pipeline's.  (No diagnostic says which pipeline shaded a wave; for the zero normal both
    roots end in a NaN normal, so that scene holds the frame and nothing more.)"""
    on = render(torch_cuda, monkeypatch, name, {"LOL_GPU_SHADE_MATH": "1"})
    off = render(torch_cuda, monkeypatch, name, {"LOL_GPU_SHADE_MATH": "0"})
    assert (on["math"]["root_kind"], on["math"]["rcp_form"]) == (3, 1) and off["math"]["root_kind"] == 0
    assert_same(on, off, name)
    check_against_oracle(on, scene_of(name), W, H)
    if name == "light-on-the-hit":
        assert on["id"][H // 2, W // 2] == 1 and on["dist"][H // 2, W // 2] == 9.0
    if name == "equal-taps":
        assert (on["id"] == 1).all()
