"""Views averaged over K cameras (lol_gpu_render_views_blend): every pixel IS the contract of include/lol_gpu.h restated on the CPU
oracle (tests/blend_reference.py) — packed pixels and lol_gpu_debug.rgb EQUAL, bit for bit.

Every comparison is array equality on the bit patterns.  The shapes are the smallest that can still go wrong: a frame whose sides
are no multiples of the 16 x 4 tile (37 x 11: three tiles by three, ragged in both directions) and three views (the view in the
grid's z, more than one group of cameras).  Reference frames are cached per camera for the whole module (blend_reference.linear_frame).
"""
import ctypes as C

import numpy as np
import pytest

import blend_reference as B
import scene_shapes as SH
import test_gpu_views as V
from loltracer_amd import gpu, scene as S

pytestmark = pytest.mark.gpu

W, H, N = 37, 11, 3
SENTINEL = V.SENTINEL
ERR_HIP, ERR_ARG, ERR_UNSUPPORTED = -2, -3, -5
LIN = {True: "lol_render_spec_batch_lin", False: "render_interp_batch_lin"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def shutter_groups(sc, n, k, first=0):
    """n views, each the exposure between two neighbours of an orbit of 8: n k cameras"""
    orbit = S.orbit_cameras(sc, 8)
    cams = []
    for v in range(n):
        cams += S.shutter_cameras(orbit[(first + v) % 8], orbit[(first + v + 1) % 8], k)
    return cams


def queue_blend(r, out, cams, k, max_steps=256, stream=None):
    n, w, h, pitch_px, stride_px = out["geom"]
    assert len(cams) == n * k
    r.render_blended_views_into(out["frame"].data_ptr(), cams, k, w, h, max_steps, pitch_bytes=pitch_px * 4,
                                view_stride_bytes=stride_px * 4, debug=out["dbg"], stream=stream)


def render_blend(torch, r, cams, k, w=W, h=H, max_steps=256, pitch_px=None, stride_px=None, debug=("rgb",), stream=None):
    out = V.alloc_batch(torch, len(cams) // k, w, h, pitch_px, stride_px, debug)
    torch.cuda.synchronize()                 # torch's fills run on ITS stream; the blend on the renderer's own
    queue_blend(r, out, cams, k, max_steps, stream)
    r.sync()
    return V.collect(out, *out["geom"])


def assert_is_reference(b, sc, cams, k, what, fmt=None, w=W, h=H, max_steps=256):
    px, rgb = B.render(sc, cams, k, w, h, fmt=fmt, max_steps=max_steps)
    assert np.array_equal(b["xrgb"], px), f"{what}: pixels differ from the reference"
    if "rgb" in b:
        assert np.array_equal(bits(b["rgb"]), bits(rgb)), f"{what}: rgb differs from the reference"


def open_renderer(sc, specialize=1, switch=True, wait=True):
    r = gpu.Renderer(0, specialize=specialize)
    try:
        r.set_view_blends(switch)
        r.prepare(sc, wait=wait)
    except BaseException:
        r.close()
        raise
    return r


@pytest.mark.parametrize("specialize", [1, 0], ids=["scene-kernel", "interpreter"])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_blends_equal_the_reference(torch_cuda, scenes, name, specialize):
    sc = scenes[name]
    r = open_renderer(sc, specialize)
    try:
        assert r.view_blends and r.view_blend_kernel_name(2) == LIN[bool(specialize)], r.specialize_log()
        for k in (2, 4):
            cams = shutter_groups(sc, N, k)
            b = render_blend(torch_cuda, r, cams, k)
            assert V.untouched_outside_views(b, N, W, H, W, H * W)
            assert_is_reference(b, sc, cams, k, f"{name} shutter K={k}")
        cams = S.lens_cameras(sc.camera, 6.0, 0.25, 16)
        b = render_blend(torch_cuda, r, cams, 16)
        assert_is_reference(b, sc, cams, 16, f"{name} lens K=16")
        r.set_tile_order("cols")
        cams = shutter_groups(sc, N, 8, first=3)
        b = render_blend(torch_cuda, r, cams, 8)
        assert_is_reference(b, sc, cams, 8, f"{name} shutter K=8, column order")
        # ... and without any diagnostic
        b = render_blend(torch_cuda, r, cams, 8, debug=False)
        assert_is_reference(b, sc, cams, 8, f"{name} shutter K=8, column order, no diagnostics")
    finally:
        r.close()


@pytest.mark.parametrize("specialize", [1, 0], ids=["scene-kernel", "interpreter"])
def test_equal_cameras_and_one_camera_are_the_plain_batch(torch_cuda, scenes, specialize):
    sc = scenes["scene4"]
    views = V.thirteen_cameras(sc)[:N]
    r = open_renderer(sc, specialize)
    try:
        plain = V.render_batch(torch_cuda, r, views, W, H)
        for k in (2, 4, 8, 16):
            b = render_blend(torch_cuda, r, [B.copy_camera(c) for c in views for _ in range(k)], k)
            assert np.array_equal(b["raw"], plain["raw"]), k                     # byte for byte
            assert np.array_equal(bits(b["rgb"]), bits(plain["rgb"])), k
        # one camera per view IS lol_gpu_render_views: every diagnostic
        assert r.view_blend_kernel_name(1) == r.view_samples_kernel_name(1, -1)
        one = render_blend(torch_cuda, r, views, 1, debug=True)
        assert np.array_equal(one["raw"], plain["raw"])
        for d in V.DIAGNOSTICS:
            assert np.array_equal(bits(one[d]), bits(plain[d])), d
    finally:
        r.close()


def test_a_group_may_hold_an_insane_camera(torch_cuda, scenes):
    """what a camera beyond the sane range switches off is decided per RECORD: one camera of a group with a coordinate of 10^15"""
    sc = scenes["scene4"]
    far = S.Camera()
    far.point = S.V3(1.0e15, 3.0, 2.5)
    far.direction = S.V3(-1.0, 0.0, 0.0)
    far.fov = sc.camera.fov
    for specialize in (1, 0):
        r = open_renderer(sc, specialize)
        try:
            cams = shutter_groups(sc, N, 4)
            cams[5] = far                                                        # camera 1 of view 1's four
            b = render_blend(torch_cuda, r, cams, 4)
            assert_is_reference(b, sc, cams, 4, f"insane camera in a group, specialize={specialize}")
        finally:
            r.close()


def test_padding_is_left_alone_and_the_format_is_honoured(torch_cuda, scenes):
    sc = scenes["scene4"]
    pitch_px = W + 7
    stride_px = H * pitch_px + 13
    lossy = gpu.PixelFormat(19, 10, 3, 3, 2, 3, 4, 0, 0xC0000000)                # 5-6-5 bits kept, in a 32-bit pixel with an alpha mask
    r = open_renderer(sc)
    try:
        cams = shutter_groups(sc, N, 4)
        for order in ("rows", "cols"):
            r.set_tile_order(order)
            for fmt in (None, lossy, gpu.PIXEL_FORMATS["rgba8888"]):
                r.set_pixel_format(fmt)
                b = render_blend(torch_cuda, r, cams, 4, pitch_px=pitch_px, stride_px=stride_px)
                assert V.untouched_outside_views(b, N, W, H, pitch_px, stride_px), (order, fmt)
                assert_is_reference(b, sc, cams, 4, f"padded, order={order}", fmt=fmt)
        r.set_pixel_format(None)
    finally:
        r.close()


def test_the_same_pixels_from_either_kernel(torch_cuda, scenes):
    """the scene module with the switch; the interpreter where the switch came after the upload; before and after the scene kernel"""
    sc = scenes["scene4"]
    cams = shutter_groups(sc, N, 4)
    r = open_renderer(sc)
    try:
        assert r.kernel_name() == "lol_render_spec" and r.view_blend_kernel_name(4) == LIN[True], r.specialize_log()
        assert_is_reference(render_blend(torch_cuda, r, cams, 4), sc, cams, 4, "scene module")
    finally:
        r.close()
    r = open_renderer(sc, switch=False)
    try:
        assert not r.view_blends
        r.set_view_blends(True)
        assert r.view_blends and r.kernel_name() == "lol_render_spec" and r.view_blend_kernel_name(4) == LIN[False]
        assert_is_reference(render_blend(torch_cuda, r, cams, 4), sc, cams, 4, "late switch")
        assert r.kernel_name() == "lol_render_spec"                              # frames are what they were
    finally:
        r.close()
    r = open_renderer(sc, wait=False)
    try:
        b0 = render_blend(torch_cuda, r, cams, 4)
        r.specialize_wait()
        assert r.view_blend_kernel_name(4) == LIN[True], r.specialize_log()
        assert_is_reference(b0, sc, cams, 4, "before the scene kernel")
        assert_is_reference(render_blend(torch_cuda, r, cams, 4), sc, cams, 4, "on the scene kernel")
    finally:
        r.close()


# ---- every interpreter variant and scene form of tests/scene_shapes.py, as test_gpu_families.py does for the other families
class Target:
    def __init__(self, shape, specialize, form=None):
        self.shape, self.specialize, self.form = shape, specialize, form
        self.id = form.name if form else "%s-interp%d" % (shape.name, specialize)


TARGETS = [Target(sh, mode) for sh in SH.RUNG_SHAPES for mode in (4, 0)] + [Target(f.shape, f.specialize, f) for f in SH.FORMS]


@pytest.mark.parametrize("t", TARGETS, ids=lambda t: t.id)
def test_every_rung_and_form(torch_cuda, t):
    sc, (w, h) = SH.scene_of(t.shape), t.shape.size
    r = open_renderer(sc, t.specialize)
    try:
        log = r.specialize_log()
        if t.form is None:
            assert r.interp_variant() == t.shape.rung and r.kernel_name() == "render_interp" and r.specialize_state()[0] == 0, log
        else:
            assert r.specialize_state()[0] == 2 and r.kernel_name() == "lol_render_spec", (r.specialize_state(), log)
            if t.form.second_tier:
                assert "form: SDF out of line" in log and "second tier (SDF inlined): " in log, log
            else:
                assert "form: SDF " + t.form.form in log and "second tier" not in log, log
        assert r.view_blend_kernel_name(2) == LIN[t.form is not None], log
        cams = SH.cameras(sc)                                                    # four round the scene: two views of two
        pitch_px, stride_px = w + 5, h * (w + 5) + 8
        b = render_blend(torch_cuda, r, cams, 2, w, h, pitch_px=pitch_px, stride_px=stride_px)
        assert V.untouched_outside_views(b, 2, w, h, pitch_px, stride_px)
        assert_is_reference(b, sc, cams, 2, t.id, w=w, h=h)
    finally:
        r.close()


def test_refusals_write_nothing(torch_cuda, scenes):
    sc = scenes["scene4"]
    lib = gpu.gpu_lib()
    cams = shutter_groups(sc, N, 2)
    fcs = (S.FrameCamera * gpu.MAX_VIEWS)()
    for i in range(gpu.MAX_VIEWS):
        fc = sc.frame_camera(W, H, cams[i % len(cams)])
        C.memmove(C.byref(fcs, i * C.sizeof(S.FrameCamera)), C.byref(fc), C.sizeof(S.FrameCamera))
    r = gpu.Renderer(0)
    try:
        # before an upload: what lol_gpu_render_views answers, whatever K is
        for k in (2, 3):
            assert lib.lol_gpu_render_views_blend(r._ctx, fcs, N, k, W, H, 256, C.c_void_p(8), W * 4, H * W * 4, None, None) == -4
        r.set_view_blends(True)
        r.prepare(sc)
        dev = torch_cuda.device("cuda:0")
        frame = torch_cuda.full((N * H * W + 64,), SENTINEL, dtype=torch_cuda.int32, device=dev)
        steps = torch_cuda.full((N * H * W,), SENTINEL, dtype=torch_cuda.int32, device=dev)
        torch_cuda.cuda.synchronize()

        def call(n=N, k=2, w=1, h=1, dbg=None):
            """(a 1 x 1 frame: the refusals under test are about K and the number of cameras, and whatever they might launch fits)"""
            return lib.lol_gpu_render_views_blend(r._ctx, fcs, n, k, w, h, 256, C.c_void_p(frame.data_ptr()), w * 4, h * w * 4, dbg, None)

        for k in (3, 32, 0, -2, 5, 6, 7, 12, 17):
            assert call(k=k) == ERR_ARG, k
        assert call(n=4097, k=1) == ERR_ARG
        assert call(n=2049, k=2) == ERR_ARG and call(n=1025, k=4) == ERR_ARG and call(n=257, k=16) == ERR_ARG      # n K > 4096
        assert call(n=0) == ERR_ARG
        dbg = gpu.Debug(None, None, None, steps.data_ptr())
        assert call(w=W, h=H, dbg=C.byref(dbg)) == ERR_UNSUPPORTED
        assert call(w=W, h=H, dbg=C.byref(gpu.Debug(None, steps.data_ptr(), None, None))) == ERR_UNSUPPORTED
        assert call(w=W, h=H, dbg=C.byref(gpu.Debug(None, None, steps.data_ptr(), None))) == ERR_UNSUPPORTED
        r.sync()
        torch_cuda.cuda.synchronize()
        assert bool((frame.cpu().numpy().view(np.uint32) == SENTINEL).all())
        assert bool((steps.cpu().numpy().view(np.uint32) == SENTINEL).all())
        # ... and the largest number of cameras a call takes is taken
        assert call(n=256, k=16) == 0
        r.sync()
    finally:
        r.close()


def test_a_failed_scratch_allocation_leaves_the_context_usable(torch_cuda, scenes):
    sc = scenes["scene4"]
    cams = shutter_groups(sc, N, 4)
    r = open_renderer(sc)
    try:
        out = V.alloc_batch(torch_cuda, N, W, H, debug=False)
        torch_cuda.cuda.synchronize()
        r.testing_fail_view_scratch(1)
        with pytest.raises(gpu.GpuError) as e:
            queue_blend(r, out, cams, 4)
        assert e.value.status == ERR_HIP and "scratch" in str(e.value)
        r.sync()
        assert bool((out["frame"].cpu().numpy().view(np.uint32) == SENTINEL).all())
        assert_is_reference(render_blend(torch_cuda, r, cams, 4), sc, cams, 4, "the blend after the failure")
        plain = V.render_batch(torch_cuda, r, cams[:2], W, H, debug=False)
        one, _ = B.render(sc, cams[:2], 1, W, H)
        assert np.array_equal(plain["xrgb"], one)
        dev = torch_cuda.device("cuda:0")
        frame = torch_cuda.zeros((H, W), dtype=torch_cuda.int32, device=dev)
        torch_cuda.cuda.synchronize()
        r.render_into(frame.data_ptr(), W, H, camera=cams[0])
        r.sync()
        assert np.array_equal(frame.cpu().numpy().view(np.uint32), one[0])       # the next plain frame
    finally:
        r.close()


def test_six_blends_in_flight(torch_cuda, scenes):
    """Six blends of different cameras into different destinations, queued back to back on the context's two streams with no wait
    between them: the scratch ring has 4 sets, so the fifth and sixth take a set whose blend may still be running.  One sync, then
    every one of them is its own reference.  Queued once: a correctness check, not a stress loop."""
    sc = scenes["scene4"]
    r = open_renderer(sc)
    try:
        r.set_frames_in_flight(2)
        groups = [(shutter_groups(sc, N, k, first=g), k) for g, k in enumerate((4, 2, 8, 4, 16, 2))]
        outs = [V.alloc_batch(torch_cuda, N, W, H, debug=("rgb",)) for _ in groups]
        torch_cuda.cuda.synchronize()
        for out, (cams, k) in zip(outs, groups):
            queue_blend(r, out, cams, k)
        r.sync()
        for g, (out, (cams, k)) in enumerate(zip(outs, groups)):
            V.collect(out, *out["geom"])
            assert V.untouched_outside_views(out, N, W, H, W, H * W), g
            assert_is_reference(out, sc, cams, k, f"blend {g} of six (K={k})")
    finally:
        r.close()


def test_a_blend_leaves_the_tile_order_alone(torch_cuda, scenes):
    sc = scenes["scene4"]
    r = open_renderer(sc)
    try:
        dev = torch_cuda.device("cuda:0")
        frame = torch_cuda.zeros((144, 256), dtype=torch_cuda.int32, device=dev)
        torch_cuda.cuda.synchronize()
        stream = r.next_stream()
        for _ in range(5):
            r.render_into(frame.data_ptr(), 256, 144, stream=stream)
        r.sync()
        before = r.tile_order()
        assert before["mode"] == "lpt"
        cams = shutter_groups(sc, N, 4)
        assert_is_reference(render_blend(torch_cuda, r, cams, 4, stream=stream), sc, cams, 4, "on the frames' stream")
        assert r.tile_order() == before
    finally:
        r.close()


def test_the_orbit_host_writes_blurred_frames(torch_cuda, scenes, tmp_path):
    """python -m loltracer_amd SCENE --orbit N --orbit-shutter K --size WxH -o DIR: N PPMs, view v the blend of cameras v K ... of
    scene.orbit_cameras(scene, N K); and --lens R --focus D --lens-samples K: one PPM, the blend over scene.lens_cameras."""
    import os
    import subprocess
    import sys
    scene_file = os.path.join(V.ROOT, "tests", "golden", "scenes", "scene4.lol")
    sc = scenes["scene4"]
    n, k = 3, 4
    out = tmp_path / "frames"
    cmd = [sys.executable, "-m", "loltracer_amd", scene_file, "--size", f"{W}x{H}"]
    p = subprocess.run(cmd + ["--orbit", str(n), "--orbit-shutter", str(k), "-o", str(out)], cwd=V.ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    want, _ = B.render(sc, S.orbit_cameras(sc, n * k), k, W, H)
    head = b"P6\n%d %d\n255\n" % (W, H)

    def pixels(path):
        data = open(path, "rb").read()
        assert data.startswith(head)
        rgb = np.frombuffer(data[len(head):], dtype=np.uint8).reshape(H, W, 3).astype(np.uint32)
        return rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2]

    assert sorted(os.listdir(out)) == [f"view_{v:04d}.ppm" for v in range(n)]
    for v in range(n):
        assert np.array_equal(pixels(out / f"view_{v:04d}.ppm"), want[v]), v
    one = tmp_path / "lens.ppm"
    p = subprocess.run(cmd + ["--lens", "0.25", "--focus", "6", "--lens-samples", "8", "-o", str(one)], cwd=V.ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    want, _ = B.render(sc, S.lens_cameras(sc.camera, 6.0, 0.25, 8), 8, W, H)
    assert np.array_equal(pixels(one), want[0])
    p = subprocess.run(cmd + ["--orbit-shutter", "4", "-o", str(one)], cwd=V.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert p.returncode == 1 and "--orbit" in p.stdout, p.stdout
    p = subprocess.run(cmd + ["--orbit", "2", "--lens", "0.25", "--focus", "6", "-o", str(out)], cwd=V.ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 1 and "--lens" in p.stdout, p.stdout
