"""Every kernel family on the hostile scenes of tests/scene_shapes.py, under the library's default switches (no LOL_GPU_TUNING).

The exact shortcuts of this renderer — the culling bounds and the k-d plan, the bound carried along the ray, eval_dist and ASK_ID_ONCE,
the division skip, the fast roots with their range fall-back, the host's own first step (lol_gpu.hip, host_sdf) — are decided from
the scene's parameters.  HOSTILE holds the parameters that strain those decisions (smoothness 0, negative, 0.01 and 60 000; negative
and zero radii; coordinates of 10^4; crowds the culling plan clusters and re-orders; no light; cameras inside objects) and exact
ties, which the reference gives to the first object in file order.  tests/test_scene_shapes.py holds, on the CPU, that the scenes
are what they claim.

Every comparison is the family's own (test_gpu_parity.check_against_oracle, test_gpu_families._all_five,
test_gpu_view_blends.assert_is_reference, test_gpu_views.assert_view_is_*): array equality on bit patterns, with the host-libm
proviso of check_against_oracle; no tolerance of its own.  The oracle's frames are computed once per (scene, camera, size,
max_steps) for the whole module.
"""
import numpy as np
import pytest

import oracle_lib as O
import scene_shapes as C
import test_gpu_view_blends as VB
import test_gpu_views as V
from loltracer_amd import gpu
from test_gpu_families import _all_five
from test_gpu_parity import check_against_oracle, gpu_render

pytestmark = pytest.mark.gpu

KERNELS = {1: "lol_render_spec", 3: "lol_render_spec", 0: "render_interp", 4: "render_interp"}
FAMILY_SCENES = [e for e in C.HOSTILE if e.families]
names = lambda e: e.name                 # noqa: E731


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module", autouse=True)
def oracle_frames_once():
    """oracle_lib.render_rows, remembered: check_against_oracle asks for the same frame once per kernel and switch.  The arrays are
    handed out read-only, and oracle_lib.last_counters is what it was after the call that computed them."""
    real, memo = O.render_rows, {}

    def render_rows(scene, w, h, y0, y1, max_steps=256, camera=None, want_steps=False):
        cam = camera if camera is not None else scene.c.camera
        key = (id(scene), w, h, y0, y1, max_steps, bytes(memoryview(cam).cast("B")), want_steps)
        if key not in memo:
            out = real(scene, w, h, y0, y1, max_steps, camera=camera, want_steps=want_steps)
            for a in out:
                if a is not None:
                    a.setflags(write=False)
            memo[key] = (scene, out, O.last_counters)          # (the scene is kept: its id stays its own)
        _, out, O.last_counters = memo[key]
        return out
    O.render_rows = render_rows
    yield
    O.render_rows = real


_dist = {}


def oracle_dist(e, sc, cam, view, w, h, max_steps=256):
    """the oracle's hit distance of every pixel (check_against_oracle holds everything else a frame has)"""
    key = (e.name, view, w, h, max_steps)
    if key not in _dist:
        d = np.zeros((h, w), dtype=np.float32)
        for y in range(h):
            for x in range(w):
                d[y, x] = O.probe(sc, w, h, x, y, max_steps, camera=cam).hit_dist
        _dist[key] = d
    return _dist[key]


def assert_frame_is_oracle(g, e, sc, w, h, what, max_steps=256, cam=None, view="own"):
    """pixels, float colours, ids, march and shadow step counts (check_against_oracle) and hit distances, bit for bit"""
    try:
        check_against_oracle(g, sc, w, h, max_steps=max_steps, camera=cam)
        assert np.array_equal(V.bits(g["dist"]), V.bits(oracle_dist(e, sc, cam, view, w, h, max_steps))), "hit distances differ"
    except AssertionError as err:
        raise AssertionError(f"{e.name} ({e.purpose}) {w}x{h} {what}: {err}\n{e.text}") from err


def open_plain(e, specialize, cull=True, skips=None):
    r = gpu.Renderer(0, specialize=specialize)
    r.want_kernel = KERNELS[specialize] if e.own_kernel else "render_interp"
    r.set_cull(cull)
    if skips is not None:
        r.set_exact_skips(skips)
    return r


def test_the_library_runs_under_its_default_switches():
    import os
    assert "LOL_GPU_TUNING" not in os.environ


@pytest.mark.parametrize("specialize", [1, 4, 0, 3], ids=["spec", "interp", "interp-plain", "spec-plain"])
@pytest.mark.parametrize("e", C.HOSTILE, ids=names)
def test_plain_frame(torch_cuda, e, specialize):
    """a fresh frame; the fifth frame of a repeated view (pixels dealt to waves by cost, waves longest first); culling off; every
    shadow ray marched to the reference's own end"""
    sc, (w, h) = C.hostile_scene(e), e.size
    r = open_plain(e, specialize)
    try:
        assert_frame_is_oracle(gpu_render(torch_cuda, r, sc, w, h), e, sc, w, h, "fresh")
        g = gpu_render(torch_cuda, r, sc, w, h, repeat=5)
        assert r.tile_order()["order"] == "lpt" and r.tile_order()["decisions"] >= 1
        assert_frame_is_oracle(g, e, sc, w, h, "fifth frame of a repeated view")
        r.set_exact_skips(0)
        assert_frame_is_oracle(gpu_render(torch_cuda, r, sc, w, h), e, sc, w, h, "set_exact_skips(0)")
    finally:
        r.close()
    r = open_plain(e, specialize, cull=False)
    try:
        assert_frame_is_oracle(gpu_render(torch_cuda, r, sc, w, h), e, sc, w, h, "set_cull(False)")
    finally:
        r.close()


@pytest.mark.parametrize("specialize", [4, 1], ids=["interp4", "scene-kernel"])
@pytest.mark.parametrize("e", FAMILY_SCENES, ids=names)
def test_through_all_five(torch_cuda, e, specialize):
    """`_aa`, `_aa_list`, `_batch`, `_batch_aa` and `_batch_aa_list`; on the scene-kernel leg _all_five itself asserts that the scene got
    its own kernel (no entry of the catalogue declares that it stays on the interpreter: own_kernel)"""
    assert e.own_kernel
    some = C.HOSTILE_REFINES_SOME[C.HOSTILE.index(e)]
    try:
        _all_five(torch_cuda, "hostile-" + e.name, C.hostile_scene(e), *e.size, C.HOSTILE_CONTRAST, specialize, some=some)
    except AssertionError as err:
        raise AssertionError(f"{e.name} ({e.purpose}) failed: {err}\n{e.text}") from err


@pytest.mark.parametrize("specialize", [1, 0], ids=["scene-kernel", "interpreter"])
@pytest.mark.parametrize("e", FAMILY_SCENES, ids=names)
def test_blend(torch_cuda, e, specialize):
    """two views of two cameras each, round the scene, into a padded layout"""
    sc, (w, h) = C.hostile_scene(e), e.size
    r = VB.open_renderer(sc, specialize)
    try:
        own = bool(specialize) and e.own_kernel
        assert r.kernel_name() == ("lol_render_spec" if own else "render_interp"), r.specialize_log()
        assert r.view_blend_kernel_name(2) == VB.LIN[own], r.specialize_log()
        cams = C.cameras(sc)
        pitch_px, stride_px = w + 5, h * (w + 5) + 8
        b = VB.render_blend(torch_cuda, r, cams, 2, w, h, pitch_px=pitch_px, stride_px=stride_px)
        assert V.untouched_outside_views(b, 2, w, h, pitch_px, stride_px)
        try:
            VB.assert_is_reference(b, sc, cams, 2, e.name, w=w, h=h)
        except AssertionError as err:
            raise AssertionError(f"{err}\n{e.text}") from err
    finally:
        r.close()


def tie_cameras(sc):
    """the scene's own camera (the origin: the first step is given), the same place with x = -0.0 (taken per pixel), and a camera
    beyond the sane range (taken per pixel, the shadow marches run to their own end)"""
    given = V.copy_camera(sc.camera)
    taken = V.copy_camera(sc.camera)
    taken.point.x = -0.0
    assert np.float32(taken.point.x).view(np.uint32) == 0x80000000 and np.float32(given.point.x).view(np.uint32) == 0
    return [("given", given), ("minus-zero", taken), ("insane", V.insane_camera())]


@pytest.mark.parametrize("specialize", [1, 4, 0, 3], ids=["spec", "interp", "interp-plain", "spec-plain"])
@pytest.mark.parametrize("e", C.HOSTILE_TIES, ids=names)
def test_ties_first_step_given_and_taken(torch_cuda, e, specialize):
    """The plain kernel under each camera, and the batch kernel with the three cameras as its views (the first step is decided per
    view), with 256 steps and with ONE — where the first step's id is the pixel's id, and the colour its material's: ids, distances
    and step counts, the first step included, are the oracle's, and the batch's views are the plain frames."""
    sc, (w, h) = C.hostile_scene(e), e.size
    first = min(e.tie.tied)
    cams = tie_cameras(sc)
    r = gpu.Renderer(0, specialize=specialize)
    r2 = open_plain(e, specialize)
    try:
        r.set_view_batches(True)
        r.prepare(sc)
        assert r.kernel_name() == KERNELS[specialize], r.specialize_log()
        assert r.view_samples_kernel_name(1, -1) == KERNELS[specialize] + "_batch", r.specialize_log()
        r2.set_tile_order("rows")
        for max_steps in (256, 1):
            frames = []
            for view, cam in cams:
                g = gpu_render(torch_cuda, r2, sc, w, h, max_steps=max_steps, camera=cam)
                assert_frame_is_oracle(g, e, sc, w, h, f"plain, {view}, max_steps={max_steps}", max_steps, cam, view)
                frames.append(g)
            for g in frames[:2]:                                   # (said once more, in the test's own words: the first object wins)
                if max_steps == 1:
                    assert (g["id"] == first).all()
                elif e.tie.along_ray:
                    assert g["id"][h // 2, w // 2] == first and not (set(e.tie.tied) - {first}) & set(g["id"].ravel().tolist())
            b = V.render_batch(torch_cuda, r, [cam for _, cam in cams], w, h, max_steps=max_steps, pitch_px=w + 5, stride_px=h * (w + 5) + 8)
            assert V.untouched_outside_views(b, len(cams), w, h, w + 5, h * (w + 5) + 8)
            for v, (view, cam) in enumerate(cams):
                what = f"{e.name} batch, {view}, max_steps={max_steps}"
                V.assert_view_is_frame(b, v, frames[v], what)
                g = dict(xrgb=b["xrgb"][v], rgb=b["rgb"][v], dist=b["dist"][v], id=b["id"][v], steps=b["steps"][v], miss_skip=frames[v]["miss_skip"])
                assert_frame_is_oracle(g, e, sc, w, h, what, max_steps, cam, view)
    finally:
        r2.close()
        r.close()
