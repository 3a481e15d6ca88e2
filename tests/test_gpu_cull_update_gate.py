"""The gated fold of the value bound (lol_codegen.hip, SdfForm::vgate) changes nothing a frame holds, and nothing the frame is
scheduled by: with LOL_GPU_CULL_UPDATE_GATED on and off (beside LOL_GPU_TUNING) the packed pixels, float colours, hit ids, hit-distance
bits and march and shadow step counts are the oracle's bit for bit (the host-libm proviso of test_gpu_parity.check_against_oracle
apart) and equal between the two, in a fresh frame and in the third frame of a repeated view — whose pixels are dealt to the waves by
what they cost, so that lanes which are no neighbours vote together — and the table of executed steps the pixels are dealt by
(lol_gpu_testing_pixel_cost) is the same table.

Sizes 67x35 and 160x90: neither a multiple of the 16x4 patch of a wave; one region of 64x16 and a ragged rest, and several.
Scenes: scene4 (gated by default); scene3 (no value bound, so no gate: its kernel is what it was); a chain of smooth unions with a
round box in it over a floor, the cluster carry forced on (gated).  Cameras: the scene's own; one just above the line where scene4's
blob meets the floor, looking along the floor at it (rays that graze both objects, the blob's value and the floor's nearly equal for
many turns: the gate's vote flips from turn to turn); one about 90 units away along the scene4 camera's axis with a narrow field of
view (march distances near MAX_DIST, long steps).

The other families that march, take the normal or march shadows on the scene's fast SDF — batches of views, supersampled frames, ray
queries, shading queries and light passes — go through the same scenes, sizes and cameras (the supersampled frame: the scene's own
camera, which is what its reference renders): each is the oracle's, directly or through the frame that is, and every field of every
output has the same bits with the gate on and off.  The helpers are those of the families' own test files.  The replay of the gate's
argument is tests/test_cull_update_gate.py."""
import os
import tempfile

import numpy as np
import pytest

import scene_shapes as C
import test_gpu_views as V
from loltracer_amd import gpu, scene as S
from test_gpu_cull_value_carry import CHAIN, CAMERA, FLOOR, text
from test_gpu_hostile import assert_frame_is_oracle, oracle_frames_once  # noqa: F401  (the fixture)
from test_gpu_light import capture_pixels
from test_gpu_parity import gpu_render
from test_gpu_rays import assert_is_reference as assert_rays_are_reference, probe_frame, trace_pixels
from test_gpu_shades import all_pixels, shade_pixels
from test_gpu_supersample import assert_equal_to_reference, reference as aa_reference, render_aa

pytestmark = pytest.mark.gpu

SIZES = [(67, 35), (160, 90)]
SCENES = {
    # name: (text or None for the golden file, switches beside the gate's, whether the gate is generated when it is on)
    "scene4": (None, {}, True),
    "scene3": (None, {}, False),
    "chain-with-a-round-box": (text(CAMERA, CHAIN, FLOOR), {"LOL_GPU_CULL_CARRY": "1"}, True),
}
_scenes = {}


def scene_of(name):
    if name not in _scenes:
        t = SCENES[name][0]
        _scenes[name] = S.Scene.parse_file(os.path.join(C.SCENES_DIR, name + ".lol")) if t is None else S.Scene.parse_string(t)
    return _scenes[name]


def cameras(sc):
    """(view, camera or None for the scene's own)"""
    return [("own", None),
            ("over-the-seam", V.cam_at(-1.0, -0.7, 1.5, 0.0, -0.1, -1.0, fov=90.0)),
            ("far", V.cam_at(-23.5, 56.1, 74.6, 0.3, -0.7, -1.0, fov=20.0))]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def set_switches(monkeypatch, name, gate):
    monkeypatch.setenv("LOL_GPU_TUNING", "1")                # (the library honours A/B switches only beside this)
    monkeypatch.setenv("LOL_GPU_CULL_UPDATE_GATED", "1" if gate else "0")
    for k, v in SCENES[name][1].items():
        monkeypatch.setenv(k, v)


def is_gated(name):
    """whether the scene's own kernel, generated under the switches in the environment, carries the gate (no device)"""
    with tempfile.TemporaryDirectory() as d:
        gpu.compile_offline(scene_of(name).flatten(), os.path.join(d, "s"), assume_fast=True)
        with open(os.path.join(d, "s.hip")) as f:
            return "this->carry && vote(" in f.read()


FIELDS = ("xrgb", "rgb", "dist", "id", "steps")


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", list(SCENES))
def test_frames_and_costs_with_the_gate_on_and_off(torch_cuda, monkeypatch, name, w, h):
    sc = scene_of(name)
    e = C.Hostile(name, "gate on / off", "")
    got = {}
    for gate in (False, True):
        set_switches(monkeypatch, name, gate)
        assert is_gated(name) == (gate and SCENES[name][2])
        r = gpu.Renderer(0)
        r.want_kernel = "lol_render_spec"
        try:
            for view, cam in cameras(sc):
                g = gpu_render(torch_cuda, r, sc, w, h, camera=cam)
                assert "LOL_GPU_CULL_UPDATE_GATED=%d" % gate in gpu.tuning_switches()
                assert_frame_is_oracle(g, e, sc, w, h, "%s, gate %s, fresh" % (view, gate), cam=cam, view=view)
                g3 = gpu_render(torch_cuda, r, sc, w, h, camera=cam, repeat=3)          # the table-dealt order
                assert r.tile_order()["order"] == "lpt"
                assert_frame_is_oracle(g3, e, sc, w, h, "%s, gate %s, third frame of a repeated view" % (view, gate), cam=cam, view=view)
                got[(gate, view)] = (g, g3, r.testing_pixel_cost(w, h).copy())
        finally:
            r.close()
    for view, _ in cameras(sc):
        (a, a3, cost_a), (b, b3, cost_b) = got[(False, view)], got[(True, view)]
        for f in FIELDS:
            assert np.array_equal(V.bits(a[f]) if a[f].dtype == np.float32 else a[f], V.bits(b[f]) if b[f].dtype == np.float32 else b[f]), (view, f)
            assert np.array_equal(V.bits(a3[f]) if a3[f].dtype == np.float32 else a3[f], V.bits(b3[f]) if b3[f].dtype == np.float32 else b3[f]), (view, f)
        assert np.array_equal(cost_a, cost_b), "%s: the pixels are dealt by another table of executed steps" % view
        if name == "scene4" and view != "far":
            assert {1, 2} <= set(b["id"].ravel().tolist())                         # (both objects are seen)


def same(a, b):
    return np.array_equal(V.bits(a) if a.dtype == np.float32 else a, V.bits(b) if b.dtype == np.float32 else b)


def families(torch, sc, name, w, h):
    """every family beside the plain frame that marches, takes the normal or marches shadows on the scene's fast SDF, under the
    switches in the environment, each held to the oracle (directly, or through the frame that assert_frame_is_oracle holds): a batch
    of the three cameras; per camera a ray query, a shading query and a light pass of every pixel; the 2x2 supersampled frame of the
    scene's own camera (tests/aa_reference.py renders that camera).  -> {what: {field: array}} for the comparison between the arms"""
    e = C.Hostile(name, "families", "")
    out = {}
    r = gpu.Renderer(0)
    try:
        r.set_view_batches(True)
        r.set_ray_queries(True)
        r.set_shade_queries(True)
        r.prepare(sc)
        assert r.kernel_name() == "lol_render_spec" and r.trace_kernel_name() == "lol_trace_spec", r.specialize_log()
        views = cameras(sc)
        cams = [V.copy_camera(sc.camera) if cam is None else cam for _, cam in views]
        b = V.render_batch(torch, r, cams, w, h)
        xy = all_pixels(w, h)
        for v, (view, cam) in enumerate(views):
            what = "%s %dx%d %s" % (name, w, h, view)
            g = gpu_render(torch, r, sc, w, h, camera=cam)
            assert_frame_is_oracle(g, e, sc, w, h, what + ", the frame beside the queries", cam=cam, view=view)
            V.assert_view_is_frame(b, v, g, what + ", view of a batch")
            out["batch " + view] = {f: b[f][v] for f in FIELDS}
            t = trace_pixels(torch, r, xy, w, h, camera=cam)
            assert_rays_are_reference(t, probe_frame((name, view), sc, w, h, cam), what + ", ray query")
            out["rays " + view] = t
            q = shade_pixels(torch, r, xy, w, h, camera=cam)
            assert np.array_equal(q["steps"].reshape(h, w), g["steps"]) and np.array_equal(q["id"].reshape(h, w), g["id"]), what + ", shading query"
            assert same(q["dist"].reshape(h, w), g["dist"]) and same(q["rgb"].reshape(h, w, 3), g["rgb"]), what + ", shading query"
            out["shade " + view] = q
            _, planes = capture_pixels(torch, r, w, h, camera=cam)
            assert np.array_equal(planes["steps"].reshape(h, w), g["steps"] & 0xFFFF), what + ", light pass: march counts"
            assert np.array_equal(planes["id"].reshape(h, w), g["id"]) and same(planes["dist"].reshape(h, w), g["dist"]), what + ", light pass"
            out["light " + view] = planes
    finally:
        r.close()
    r = gpu.Renderer(0)
    r.want_kernel = "lol_render_spec_aa"
    try:
        x, rgb = render_aa(torch, r, sc, w, h, 2)
        assert r.kernel_name() == r.want_kernel, r.specialize_log()
        want_x, want_rgb = aa_reference(sc, name, w, h, 2)[:2]
        assert_equal_to_reference(x, rgb, want_x, want_rgb)
        out["supersampled 2x2"] = dict(xrgb=x, rgb=rgb)
    finally:
        r.close()
    return out


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", list(SCENES))
def test_the_other_families_with_the_gate_on_and_off(torch_cuda, monkeypatch, name, w, h):
    """batches, supersampled frames, ray queries, shading queries and light passes: the oracle's, and every field of every output
    the same bits with the gate on and off"""
    sc = scene_of(name)
    got = {}
    for gate in (False, True):
        set_switches(monkeypatch, name, gate)
        assert is_gated(name) == (gate and SCENES[name][2])
        got[gate] = families(torch_cuda, sc, name, w, h)
    assert set(got[False]) == set(got[True])
    for what, fields in got[False].items():
        for f, a in fields.items():
            assert same(np.asarray(a), np.asarray(got[True][what][f])), "%s %dx%d: %s: %s differs between gate off and on" % (name, w, h, what, f)
