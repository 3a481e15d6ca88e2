"""Supersampled blends (lol_gpu_render_views_blend_samples): every pixel IS the contract of include/lol_gpu.h restated on the CPU
oracle (tests/blend_aa_reference.py) — packed pixels and lol_gpu_debug.rgb EQUAL, bit for bit.

Every comparison is array equality on the bit patterns.  The shapes are the smallest that can still go wrong: 37 x 11 pixels, whose
sample grids (74 x 22 and 148 x 44) are ragged against the 16 x 4 tile on both axes, and three views (the view in the grid's z,
more than one group of cameras).  tests/test_blend_aa_reference.py holds the inputs, on the CPU, to telling a kernel that ignores
the samples, or all cameras but one, from a right one.  Reference means are cached per camera for the whole session
(blend_aa_reference.camera_mean).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import blend_aa_reference as BA
import blend_reference as B
import scene_shapes as SH
import test_gpu_view_blends as VB
import test_gpu_view_samples as VS
import test_gpu_views as V
from loltracer_amd import gpu, scene as S

pytestmark = pytest.mark.gpu

W, H, N = BA.W, BA.H, BA.N
SENTINEL = V.SENTINEL
ERR_HIP, ERR_ARG, ERR_NO_PROGRAM, ERR_UNSUPPORTED = -2, -3, -4, -5
AA_LIN = {True: "lol_render_spec_batch_aa_lin", False: "render_interp_batch_aa_lin"}
bits = VB.bits
shutter_groups = BA.shutter_groups


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def queue_blend(r, out, cams, k, s, max_steps=256, stream=None):
    n, w, h, pitch_px, stride_px = out["geom"]
    assert len(cams) == n * k
    r.render_blended_views_into(out["frame"].data_ptr(), cams, k, w, h, max_steps, pitch_bytes=pitch_px * 4,
                                view_stride_bytes=stride_px * 4, debug=out["dbg"], stream=stream, samples=s)


def render_blend(torch, r, cams, k, s, w=W, h=H, max_steps=256, pitch_px=None, stride_px=None, debug=("rgb",), stream=None):
    out = V.alloc_batch(torch, len(cams) // k, w, h, pitch_px, stride_px, debug)
    torch.cuda.synchronize()                 # torch's fills run on ITS stream; the blend on the renderer's own
    queue_blend(r, out, cams, k, s, max_steps, stream)
    r.sync()
    return V.collect(out, *out["geom"])


def assert_is_reference(b, sc, cams, k, s, what, fmt=None, w=W, h=H, max_steps=256):
    px, rgb = BA.render(sc, cams, k, s, w, h, fmt=fmt, max_steps=max_steps)
    assert np.array_equal(b["xrgb"], px), f"{what}: pixels differ from the reference"
    if "rgb" in b:
        assert np.array_equal(bits(b["rgb"]), bits(rgb)), f"{what}: rgb differs from the reference"


def open_renderer(sc, specialize=1, switch=True, wait=True):
    r = gpu.Renderer(0, specialize=specialize)
    try:
        r.set_view_blend_samples(switch)
        r.prepare(sc, wait=wait)
    except BaseException:
        r.close()
        raise
    return r


@pytest.mark.parametrize("specialize", [1, 0], ids=["scene-kernel", "interpreter"])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_supersampled_blends_equal_the_reference(torch_cuda, scenes, name, specialize):
    sc = scenes[name]
    r = open_renderer(sc, specialize)
    try:
        assert r.view_blend_samples, "the switch"
        cases = BA.gpu_cases(sc)
        for what, cams, k, s in cases:
            assert r.view_blend_samples_kernel_name(k, s) == AA_LIN[bool(specialize)], r.specialize_log()
            b = render_blend(torch_cuda, r, cams, k, s)
            n = len(cams) // k
            assert V.untouched_outside_views(b, n, W, H, W, H * W)
            assert_is_reference(b, sc, cams, k, s, f"{name} {what}")
        r.set_tile_order("cols")
        for what, cams, k, s in (cases[1], cases[2]):                          # K = 4 with s = 2, and K = 2 with s = 4
            b = render_blend(torch_cuda, r, cams, k, s)
            assert_is_reference(b, sc, cams, k, s, f"{name} {what}, column order")
            # ... and without any diagnostic
            b = render_blend(torch_cuda, r, cams, k, s, debug=False)
            assert_is_reference(b, sc, cams, k, s, f"{name} {what}, column order, no diagnostics")
    finally:
        r.close()


@pytest.mark.parametrize("specialize", [1, 0], ids=["scene-kernel", "interpreter"])
def test_the_three_identities(torch_cuda, scenes, specialize):
    """s = 1 IS the blend, K = 1 IS the supersampled batch, K equal cameras ARE that camera's supersampled view: byte for byte"""
    sc = scenes["scene4"]
    views = V.thirteen_cameras(sc)[:N]
    lib = gpu.gpu_lib()
    r = open_renderer(sc, specialize)
    try:
        # s = 1: lol_gpu_render_views_blend, called through the new entry point itself
        cams = shutter_groups(sc, N, 4)
        blend = VB.render_blend(torch_cuda, r, cams, 4)
        fcs = (S.FrameCamera * len(cams))()
        for i, c in enumerate(cams):
            fc = sc.frame_camera(W, H, c)
            C.memmove(C.byref(fcs, i * C.sizeof(S.FrameCamera)), C.byref(fc), C.sizeof(S.FrameCamera))
        assert r.view_blend_samples_kernel_name(4, 1) == r.view_blend_kernel_name(4)
        out = V.alloc_batch(torch_cuda, N, W, H, debug=("rgb",))
        torch_cuda.cuda.synchronize()
        assert lib.lol_gpu_render_views_blend_samples(r._ctx, fcs, N, 4, W, H, 256, 1, C.c_void_p(out["frame"].data_ptr()), W * 4, H * W * 4,
                                                      C.byref(out["dbg"]), None) == 0
        r.sync()
        one = V.collect(out, *out["geom"])
        assert np.array_equal(one["raw"], blend["raw"]) and np.array_equal(bits(one["rgb"]), bits(blend["rgb"]))
        # K = 1 with s = 1 keeps every diagnostic: lol_gpu_render_views
        out = V.alloc_batch(torch_cuda, N, W, H, debug=True)
        torch_cuda.cuda.synchronize()
        assert lib.lol_gpu_render_views_blend_samples(r._ctx, fcs, N, 1, W, H, 256, 1, C.c_void_p(out["frame"].data_ptr()), W * 4, H * W * 4,
                                                      C.byref(out["dbg"]), None) == 0
        r.sync()
        one = V.collect(out, *out["geom"])
        first = VB.render_blend(torch_cuda, r, cams[:N], 1, debug=True)
        assert np.array_equal(one["raw"], first["raw"])
        for d in V.DIAGNOSTICS:
            assert np.array_equal(bits(one[d]), bits(first[d])), d
        for s in (2, 4):
            # K = 1 with s > 1: lol_gpu_render_views_samples without a contrast
            assert r.view_blend_samples_kernel_name(1, s) == r.view_samples_kernel_name(s, -1)
            batch = VS.render_batch(torch_cuda, r, views, W, H, s, -1)
            one = render_blend(torch_cuda, r, views, 1, s)
            assert np.array_equal(one["raw"], batch["raw"]) and np.array_equal(bits(one["rgb"]), bits(batch["rgb"])), s
            # K equal cameras: the same view again, through the new kernel
            for k in (2, 4, 8, 16):
                b = render_blend(torch_cuda, r, [B.copy_camera(c) for c in views for _ in range(k)], k, s)
                assert np.array_equal(b["raw"], batch["raw"]), (s, k)
                assert np.array_equal(bits(b["rgb"]), bits(batch["rgb"])), (s, k)
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
            b = render_blend(torch_cuda, r, cams, 4, 2)
            assert_is_reference(b, sc, cams, 4, 2, f"insane camera in a group, specialize={specialize}")
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
                b = render_blend(torch_cuda, r, cams, 4, 2, pitch_px=pitch_px, stride_px=stride_px)
                assert V.untouched_outside_views(b, N, W, H, pitch_px, stride_px), (order, fmt)
                assert_is_reference(b, sc, cams, 4, 2, f"padded, order={order}", fmt=fmt)
        r.set_pixel_format(None)
    finally:
        r.close()


def test_the_same_pixels_from_either_kernel(torch_cuda, scenes):
    """the scene module with the switch; the interpreter where the switch came after the upload — and where only the blend and
    view-samples switches were set, which do not imply this one; before and after the scene kernel"""
    sc = scenes["scene4"]
    cams = shutter_groups(sc, N, 4)
    r = open_renderer(sc, switch=False)
    try:
        assert not r.view_blend_samples
        r.set_view_blend_samples(True)
        assert r.view_blend_samples and r.kernel_name() == "lol_render_spec" and r.view_blend_samples_kernel_name(4, 2) == AA_LIN[False]
        assert_is_reference(render_blend(torch_cuda, r, cams, 4, 2), sc, cams, 4, 2, "late switch")
        assert r.kernel_name() == "lol_render_spec"                              # frames are what they were
    finally:
        r.close()
    r = gpu.Renderer(0)
    try:
        r.set_view_blends(True)
        r.set_view_samples(True)
        r.prepare(sc)
        assert r.view_blend_kernel_name(4) == VB.LIN[True] and r.view_samples_kernel_name(2, -1) == "lol_render_spec_batch_aa"
        assert r.view_blend_samples_kernel_name(4, 2) == AA_LIN[False]
        assert_is_reference(render_blend(torch_cuda, r, cams, 4, 2), sc, cams, 4, 2, "the other two switches")
    finally:
        r.close()
    r = open_renderer(sc, wait=False)
    try:
        b0 = render_blend(torch_cuda, r, cams, 4, 2)
        r.specialize_wait()
        assert r.view_blend_samples_kernel_name(4, 2) == AA_LIN[True], r.specialize_log()
        assert_is_reference(b0, sc, cams, 4, 2, "before the scene kernel")
        assert_is_reference(render_blend(torch_cuda, r, cams, 4, 2), sc, cams, 4, 2, "on the scene kernel")
    finally:
        r.close()


# ---- every interpreter variant and scene form of tests/scene_shapes.py, as test_gpu_view_blends.py does for the linear family
@pytest.mark.parametrize("t", VB.TARGETS, ids=lambda t: t.id)
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
        assert r.view_blend_samples_kernel_name(2, 2) == AA_LIN[t.form is not None], log
        cams = SH.cameras(sc)                                                    # four round the scene: two views of two
        pitch_px, stride_px = w + 5, h * (w + 5) + 8
        b = render_blend(torch_cuda, r, cams, 2, 2, w, h, pitch_px=pitch_px, stride_px=stride_px)
        assert V.untouched_outside_views(b, 2, w, h, pitch_px, stride_px)
        assert_is_reference(b, sc, cams, 2, 2, t.id, w=w, h=h)
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
        # before an upload: what lol_gpu_render_views answers, whatever K is — but a bad s comes first
        for k in (2, 3):
            assert lib.lol_gpu_render_views_blend_samples(r._ctx, fcs, N, k, W, H, 256, 2, C.c_void_p(8), W * 4, H * W * 4, None, None) == ERR_NO_PROGRAM
        assert lib.lol_gpu_render_views_blend_samples(r._ctx, fcs, N, 2, W, H, 256, 3, C.c_void_p(8), W * 4, H * W * 4, None, None) == ERR_ARG
        r.set_view_blend_samples(True)
        r.prepare(sc)
        dev = torch_cuda.device("cuda:0")
        frame = torch_cuda.full((N * H * W + 64,), SENTINEL, dtype=torch_cuda.int32, device=dev)
        steps = torch_cuda.full((N * H * W,), SENTINEL, dtype=torch_cuda.int32, device=dev)
        torch_cuda.cuda.synchronize()

        def call(n=N, k=2, s=2, w=1, h=1, dbg=None, pitch=None, stride=None):
            """(a 1 x 1 frame unless the refusal under test is about the size: whatever it might launch fits)"""
            pitch = w * 4 if pitch is None else pitch
            return lib.lol_gpu_render_views_blend_samples(r._ctx, fcs, n, k, w, h, 256, s, C.c_void_p(frame.data_ptr()), pitch,
                                                          h * pitch if stride is None else stride, dbg, None)

        for s in (0, 3, 8, -1, 5, 16):
            assert call(s=s) == ERR_ARG, s
        for k in (3, 32, 0, -2, 5, 6, 7, 12, 17):
            assert call(k=k) == ERR_ARG, k
        assert call(n=4097, k=1) == ERR_ARG
        assert call(n=2049, k=2) == ERR_ARG and call(n=1025, k=4) == ERR_ARG and call(n=257, k=16) == ERR_ARG      # n K > 4096
        assert call(n=0) == ERR_ARG
        assert call(w=W, h=H, pitch=W * 4 - 4) == ERR_ARG and call(w=W, h=H, stride=(H - 1) * W * 4) == ERR_ARG      # the batch's geometry
        for d in (gpu.Debug(None, None, None, steps.data_ptr()), gpu.Debug(None, steps.data_ptr(), None, None),
                  gpu.Debug(None, None, steps.data_ptr(), None)):
            assert call(w=W, h=H, dbg=C.byref(d)) == ERR_UNSUPPORTED                       # K > 1 and s > 1
            assert call(w=W, h=H, k=1, dbg=C.byref(d)) == ERR_UNSUPPORTED                  # s > 1 alone
            assert call(w=W, h=H, s=1, dbg=C.byref(d)) == ERR_UNSUPPORTED                  # K > 1 alone
        # A sample grid of more than 65535 tiles along an axis, and more than 2^32 - 1 lanes over all the sample grids.  Both are
        # refused before anything is allocated or launched: the destination such a call names is never touched, so it need not exist.
        assert call(w=1, h=65536, s=4) == ERR_ARG                                          # 4 * 65536 / 4 = 65536 tiles in y
        assert call(w=262144, h=1, s=4) == ERR_ARG                                         # 4 * 262144 / 16 = 65536 tiles in x
        assert call(n=64, k=16, w=2048, h=1024, s=2) == ERR_ARG                            # 1024 cameras x 4096 x 2048 samples = 2^33
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
            queue_blend(r, out, cams, 4, 2)
        assert e.value.status == ERR_HIP and "scratch" in str(e.value)
        r.sync()
        assert bool((out["frame"].cpu().numpy().view(np.uint32) == SENTINEL).all())
        assert_is_reference(render_blend(torch_cuda, r, cams, 4, 2), sc, cams, 4, 2, "the supersampled blend after the failure")
    finally:
        r.close()


def test_six_supersampled_blends_in_flight(torch_cuda, scenes):
    """Six supersampled blends of different cameras into different destinations, queued back to back on the context's two streams
    with no wait between them: the scratch ring has 4 sets, so the fifth and sixth take a set whose blend may still be running.  One
    sync, then every one of them is its own reference.  Queued once: a correctness check, not a stress loop."""
    sc = scenes["scene4"]
    r = open_renderer(sc)
    try:
        r.set_frames_in_flight(2)
        shapes = ((4, 2), (2, 2), (2, 4), (4, 2), (2, 2), (2, 4))
        groups = [(shutter_groups(sc, N, k, first=g % 2), k, s) for g, (k, s) in enumerate(shapes)]
        outs = [V.alloc_batch(torch_cuda, N, W, H, debug=("rgb",)) for _ in groups]
        torch_cuda.cuda.synchronize()
        for out, (cams, k, s) in zip(outs, groups):
            queue_blend(r, out, cams, k, s)
        r.sync()
        for g, (out, (cams, k, s)) in enumerate(zip(outs, groups)):
            V.collect(out, *out["geom"])
            assert V.untouched_outside_views(out, N, W, H, W, H * W), g
            assert_is_reference(out, sc, cams, k, s, f"blend {g} of six (K={k}, s={s})")
    finally:
        r.close()


def test_a_supersampled_blend_leaves_the_tile_order_alone(torch_cuda, scenes):
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
        assert_is_reference(render_blend(torch_cuda, r, cams, 4, 2, stream=stream), sc, cams, 4, 2, "on the frames' stream")
        assert r.tile_order() == before
        assert r.samples == 1 and r.adaptive_samples == -1                       # neither read nor changed
    finally:
        r.close()


def test_the_hosts_write_supersampled_blurred_frames(torch_cuda, scenes, tmp_path):
    """python -m loltracer_amd SCENE --orbit N --orbit-shutter K --orbit-samples S: N PPMs, view v the supersampled blend of cameras
    v K ... of scene.orbit_cameras(scene, N K); --lens R --focus D --lens-samples K --samples S: one PPM; a shutter with
    --orbit-adaptive, and a lens with --adaptive, stay refused."""
    scene_file = os.path.join(V.ROOT, "tests", "golden", "scenes", "scene4.lol")
    sc = scenes["scene4"]
    n, k, s = 3, 4, 2
    out = tmp_path / "frames"
    cmd = [sys.executable, "-m", "loltracer_amd", scene_file, "--size", f"{W}x{H}"]

    def run(*more):
        return subprocess.run(cmd + list(more), cwd=V.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)

    p = run("--orbit", str(n), "--orbit-shutter", str(k), "--orbit-samples", str(s), "-o", str(out))
    assert p.returncode == 0, p.stdout
    want, _ = BA.render(sc, S.orbit_cameras(sc, n * k), k, s, W, H)
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
    p = run("--lens", "0.25", "--focus", "6", "--lens-samples", "8", "--samples", str(s), "-o", str(one))
    assert p.returncode == 0, p.stdout
    want, _ = BA.render(sc, S.lens_cameras(sc.camera, 6.0, 0.25, 8), 8, s, W, H)
    assert np.array_equal(pixels(one), want[0])
    p = run("--orbit", str(n), "--orbit-shutter", str(k), "--orbit-samples", str(s), "--orbit-adaptive", "16", "-o", str(out))
    assert p.returncode == 1 and "--orbit-adaptive" in p.stdout, p.stdout
    p = run("--lens", "0.25", "--focus", "6", "--samples", str(s), "--adaptive", "16", "-o", str(one))
    assert p.returncode == 1 and "--adaptive" in p.stdout, p.stdout
