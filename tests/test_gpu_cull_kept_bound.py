"""The culling bound kept past the march (lol_codegen.hip, SdfForm::keep; lol_kernel.h, bound_keep / taps_begin / taps_done) changes
nothing a frame holds, and nothing the frame is scheduled by: under LOL_GPU_CULL_KEEP = 0, 1 (the normal taps), 2 (once the start of
the shadow marches, measured and taken out: the bit names nothing now, the source is that of 0) and 3 (that of 1), beside
LOL_GPU_TUNING, the packed pixels, float colours, hit ids, hit-distance bits and reported march and shadow step counts are the
oracle's bit for bit (the host-libm proviso of test_gpu_parity.check_against_oracle apart) and equal among the four settings, in a
fresh frame and in the third frame of a repeated view — whose pixels are dealt to the waves by what they cost — and the table of
EXECUTED steps the pixels are dealt by (lol_gpu_testing_pixel_cost) is the same table: the kept bound changes which tests and
evaluations a turn runs, not how many turns there are.

Sizes 67x35 and 160x90: neither a multiple of the 16x4 patch of a wave; one region of 64x16 and a ragged rest, and several.
Scenes: scene4 (hooks by default); scene3 (no hooks: its kernel is what it was); a chain of smooth unions with a round box in it over
a floor, the cluster carry forced on (hooks).  Cameras: the three of tests/test_gpu_cull_update_gate.py (the scene's own, over the
seam, far) and one that looks down at the floor of scene4 just in front of the line where the blob meets it: primary rays that end
on the floor a little outside the blob, where the bound the march ends with is nearly tight at the taps — some taps of a wave are
decided by it and others fall through to the full test.

The other families that march, take the normal or march shadows on the scene's fast SDF — batches of views, supersampled frames, ray
queries, shading queries, light passes (test_gpu_cull_update_gate.families) and light updates — go through the same scenes, sizes
and settings: each is the oracle's, directly or through the frame that is, and every field of every output has the same bits under
all four settings.  The light update is the path WITHOUT a march (its hit comes from two loads, so it must see no bound at all):
after a render and a capture on the same context, every dword of its planes is the same under every setting.  The replay of the
argument is tests/test_cull_kept_bound.py."""
import os
import tempfile

import numpy as np
import pytest

import scene_shapes as C
import test_gpu_cull_update_gate as G
import test_gpu_views as V
from loltracer_amd import gpu
from test_gpu_hostile import assert_frame_is_oracle, oracle_frames_once  # noqa: F401  (the fixture)
from test_gpu_light import capture_pixels
from test_gpu_light_update import lighting_look, raw, update_args
from test_gpu_parity import gpu_render

pytestmark = pytest.mark.gpu

SIZES = G.SIZES
SCENES = G.SCENES              # name: (text or None, switches beside the mask, whether the hooks are generated when the mask allows)
MASKS = (0, 1, 2, 3)
CONTACT = ("contact", V.cam_at(-1.0, 2.0, 2.0, 0.0, -1.0, -0.8, fov=70.0))
FIELDS = G.FIELDS


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def cameras(sc):
    return G.cameras(sc) + [CONTACT]


def set_switches(monkeypatch, name, mask):
    monkeypatch.setenv("LOL_GPU_TUNING", "1")                # (the library honours A/B switches only beside this)
    monkeypatch.setenv("LOL_GPU_CULL_KEEP", str(mask))
    for k, v in SCENES[name][1].items():
        monkeypatch.setenv(k, v)


_hooks = {}


def hooks_of(name, mask):
    """which hooks the scene's own kernel, generated under the switches in the environment, carries (no device)"""
    if (name, mask) not in _hooks:
        with tempfile.TemporaryDirectory() as d:
            gpu.compile_offline(G.scene_of(name).flatten(), os.path.join(d, "s"), assume_fast=True)
            with open(os.path.join(d, "s.hip")) as f:
                src = f.read()
        _hooks[(name, mask)] = tuple(n in src for n in ("float bound_keep(", "void taps_begin(", "void taps_done("))
    return _hooks[(name, mask)]


def want_hooks(name, mask):
    return (bool(mask & 1) and SCENES[name][2],) * 3


_frames = {}


def frames(torch, monkeypatch, name, w, h, mask):
    """{view: (fresh frame, third frame of a repeated view, the table of executed steps)} under one setting, each frame the oracle's"""
    if (name, w, h, mask) in _frames:
        return _frames[(name, w, h, mask)]
    sc = G.scene_of(name)
    e = C.Hostile(name, "kept bound, mask %d" % mask, "")
    set_switches(monkeypatch, name, mask)
    assert hooks_of(name, mask) == want_hooks(name, mask)
    got = {}
    r = gpu.Renderer(0)
    r.want_kernel = "lol_render_spec"
    try:
        for view, cam in cameras(sc):
            g = gpu_render(torch, r, sc, w, h, camera=cam)
            assert "LOL_GPU_CULL_KEEP=%d" % mask in gpu.tuning_switches()
            assert_frame_is_oracle(g, e, sc, w, h, "%s, mask %d, fresh" % (view, mask), cam=cam, view=view)
            g3 = gpu_render(torch, r, sc, w, h, camera=cam, repeat=3)          # the table-dealt order
            assert r.tile_order()["order"] == "lpt"
            assert_frame_is_oracle(g3, e, sc, w, h, "%s, mask %d, third frame of a repeated view" % (view, mask), cam=cam, view=view)
            got[view] = (g, g3, r.testing_pixel_cost(w, h).copy())
    finally:
        r.close()
    _frames[(name, w, h, mask)] = got
    return got


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", list(SCENES))
def test_frames_and_costs_under_every_setting(torch_cuda, monkeypatch, name, w, h, mask):
    sc = G.scene_of(name)
    off, on = frames(torch_cuda, monkeypatch, name, w, h, 0), frames(torch_cuda, monkeypatch, name, w, h, mask)
    for view, _ in cameras(sc):
        (a, a3, cost_a), (b, b3, cost_b) = off[view], on[view]
        for f in FIELDS:
            assert G.same(a[f], b[f]) and G.same(a3[f], b3[f]), (view, f)
        assert np.array_equal(cost_a, cost_b), "%s: the pixels are dealt by another table of executed steps" % view
        if name == "scene4" and view in ("own", "over-the-seam", "contact"):
            assert {1, 2} <= set(b["id"].ravel().tolist())                     # (both objects are seen)
    if name == "scene4":
        # the camera this file adds does what it is for: most of its primary rays end on the floor (id 2), next to the blob
        ids = on["contact"][0]["id"]
        assert (ids == 2).mean() > 0.5 and (ids == 1).any()


def light_update(torch, sc, w, h):
    """a render, a capture and then an update of every light on ONE context: every dword of the planes after the update"""
    look = lighting_look(sc)
    r = gpu.Renderer(0)
    try:
        r.prepare(sc)
        assert r.kernel_name() == "lol_render_spec", r.specialize_log()
        gpu_render(torch, r, sc, w, h)
        p, _ = capture_pixels(torch, r, w, h)
        before = raw(p)
        nl = len(sc.lights())
        r.light_update_pixels_into(look, w * h, w, h, (1 << nl) - 1, 0, stream=torch.cuda.current_stream().cuda_stream, **update_args(p))
        r.sync()
        torch.cuda.synchronize()
        after = raw(p)
        p.collect()                                                            # (nothing behind the planes or between them)
        assert not np.array_equal(before["factors"], after["factors"])       # (the moved lights gave other factors)
        return after
    finally:
        r.close()


_families = {}


def families(torch, monkeypatch, name, w, h, mask):
    if (name, w, h, mask) not in _families:
        set_switches(monkeypatch, name, mask)
        sc = G.scene_of(name)
        out = G.families(torch, sc, name, w, h)
        out["light update"] = light_update(torch, sc, w, h)
        _families[(name, w, h, mask)] = out
    return _families[(name, w, h, mask)]


@pytest.mark.parametrize("mask", MASKS[1:])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", list(SCENES))
def test_the_other_families_under_every_setting(torch_cuda, monkeypatch, name, w, h, mask):
    """batches, supersampled frames, ray queries, shading queries, light passes and light updates: the oracle's, and every field of
    every output the same bits with the hooks off and under this setting"""
    off, on = families(torch_cuda, monkeypatch, name, w, h, 0), families(torch_cuda, monkeypatch, name, w, h, mask)
    assert set(off) == set(on)
    for what, fields in off.items():
        for f, a in fields.items():
            assert G.same(np.asarray(a), np.asarray(on[what][f])), "%s %dx%d: %s: %s differs between mask 0 and mask %d" % (name, w, h, what, f, mask)
