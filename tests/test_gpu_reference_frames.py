"""The device against the REFERENCE's own renderer, with no oracle in between.

tests/golden/ref_renderer_frames.npz (tests/reference_frames.py) holds the pixels naive_renderer.c's render_thread itself stored
for the example scenes, the rung and form shapes, the fuzz scenes, the degenerate inputs, the generated hostile scenes, the
exact ties and the march that ends at exactly 100, under each scene's own camera, the orbit of the family tests, the ties' three cameras and scene4's first-step cameras;
and for the hostile scenes the ids, distances and march steps composed from the reference's compiled primitives.  Here every
recorded (scene, camera) is rendered on the scene kernel and on the interpreter (the ties on all four kernels): a plain frame under
the scene's own camera, ONE lol_gpu_render_views batch for all the others.  Array equality throughout; the packed pixels under
test_gpu_sdf.py's host-libm proviso.  Fixtures only: nothing outside the repository is read.

The 8192-op trees and the 1104-op chain run on the interpreter only (tests/test_gpu_families.py pays for their compiles).
"""
import numpy as np
import pytest

import reference_frames as RF
import test_gpu_views as V
from loltracer_amd import gpu, scene as S
from test_gpu_parity import HOST_LIBM_IS_FMA_VARIANT, channels, gpu_render

pytestmark = pytest.mark.gpu

KERNELS = {1: "lol_render_spec", 3: "lol_render_spec", 0: "render_interp", 4: "render_interp"}
MODE_IDS = {1: "spec", 4: "interp", 0: "interp-plain", 3: "spec-plain"}
SCENE_KERNEL_MAX_OPS = 1100             # (chain550 has 1104 ops, the depth-12 trees 8192)


def modes_of(case):
    if case.group == "tie":
        return (1, 4, 0, 3)
    return (1, 4) if case.n_ops <= SCENE_KERNEL_MAX_OPS else (4,)


PARAMS = [pytest.param(c, m, id="%s-%s" % (c.key, MODE_IDS[m])) for c in RF.cases() for m in modes_of(c)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def assert_pixels_are_recorded(got, want, what):
    assert got.shape == want.shape, what
    if HOST_LIBM_IS_FMA_VARIANT:
        assert np.array_equal(got, want), f"{what}: {(got != want).sum()} of {got.size} pixels differ from render_thread's"
    else:
        assert np.abs(channels(got) - channels(want)).max() <= 1, what
        assert (got >> 24 == 0).all(), what


@pytest.mark.parametrize("case,specialize", PARAMS)
def test_device_renders_the_reference_frames(torch_cuda, scenes, case, specialize):
    meta, arrays = RF.load()
    entry = {m["key"]: m for m in meta["cases"]}.get(case.key)
    if entry is None:                                             # (left out by name, with the reason: tests/test_reference_renderer.py)
        assert any(e["key"] == case.key for e in meta["left_out"])
        return
    sc = scenes[case.key] if case.group == "example" else S.Scene.parse_string(case.text())
    assert entry["sha256"] == RF.sha256(case.text())
    frames, cams = arrays[case.key + "_xrgb"], arrays[case.key + "_cams"]
    w, h = case.size
    r = gpu.Renderer(0, specialize=specialize)
    try:
        r.set_view_batches(True)
        if case.group in ("hostile", "tie", "example", "exit"):
            r.want_kernel = KERNELS[specialize]
        g = gpu_render(torch_cuda, r, sc, w, h)
        assert RF.cam7(sc.camera).tobytes() == cams[0].tobytes()
        assert_pixels_are_recorded(g["xrgb"][:, :w], frames[0], f"{case.key}, own camera")
        if entry["composed"]:
            assert np.array_equal(g["id"], arrays[case.key + "_hit_id"]), "hit ids differ from the composition"
            assert np.array_equal(V.bits(g["dist"]), V.bits(arrays[case.key + "_hit_dist"])), "hit distances differ from the composition"
            assert np.array_equal(g["steps"] & 0xFFFF, arrays[case.key + "_march_steps"]), "march steps differ from the composition"
            assert not np.isnan(g["rgb"]).any()
            if HOST_LIBM_IS_FMA_VARIANT:
                assert np.array_equal(V.bits(g["rgb"]), V.bits(arrays[case.key + "_rgb"])), "float colours differ from the composition"
        if len(entry["cameras"]) > 1:
            views = [RF.camera_of(row) for row in cams[1:]]
            pitch_px, stride_px = w + 5, h * (w + 5) + 8
            b = V.render_batch(torch_cuda, r, views, w, h, pitch_px=pitch_px, stride_px=stride_px)
            assert V.untouched_outside_views(b, len(views), w, h, pitch_px, stride_px)
            for v, name in enumerate(entry["cameras"][1:]):
                assert_pixels_are_recorded(b["xrgb"][v], frames[1 + v], f"{case.key}, view {name} of the batch")
    finally:
        r.close()
