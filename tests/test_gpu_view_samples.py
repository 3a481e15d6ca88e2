"""Supersampled batches of views (lol_gpu_render_views_samples): view v of a batch with s x s samples and contrast T IS the frame
lol_gpu_render_device renders under cams[v] on a context with set_samples(s) / set_adaptive_samples(T) — packed pixels and float
colours EQUAL, bit for bit — and both are the CPU oracle's frame (tests/aa_reference.py, tests/adaptive_reference.py).

Every comparison is array equality on the bit patterns.  The scene's own kernels (lol_gpu_set_view_samples before the upload) and
the interpreter's are both held to it, and which of the two a batch ran is asked of the library (lol_gpu_view_samples_kernel_name:
the test the launch itself makes), not assumed.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aa_reference as A
import adaptive_reference as D
import oracle_lib as O
from loltracer_amd import gpu, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7B0B5
ERR_HIP, ERR_ARG, ERR_NO_PROGRAM, ERR_UNSUPPORTED = -2, -3, -4, -5
K = 16
# views of S.orbit_cameras(scene, 16) that, says the oracle, refine SOME but not all of their pixels at contrast 16 in scene4 and
# in scene.lol, at 64 x 36 and at 50 x 23 (asserted where they are used); view 7 refines none in either: an empty list in the
# middle of a batch
SOME_BUT_NOT_ALL = (1, 5, 11)
NONE_REFINED = 7
RGB565_IN_32 = gpu.PixelFormat(11, 5, 0, 3, 2, 3, 4, 0, 0xFF000000)      # lossy: the unrefined pixels of an adaptive batch lose bits too


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cam_at(x, y, z, dx, dy, dz, fov=90.0):
    cam = S.Camera()
    cam.point = S.V3(x, y, z)
    d = np.array([dx, dy, dz], dtype=np.float32)
    n = np.float32(1.0) / np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1]) + np.float32(d[2] * d[2]), dtype=np.float32)
    cam.direction = S.V3(*(float(np.float32(v * n)) for v in d))
    cam.fov = float(np.float32(np.float32(fov) / np.float32(180) * np.pi))
    return cam


def insane_camera():
    cam = S.Camera()
    cam.point = S.V3(1.0e16, 3.0, 2.5)
    cam.direction = S.V3(-1.0, 0.0, 0.0)
    cam.fov = float(np.float32(np.float32(60.0) / np.float32(180) * np.pi))
    return cam


def alloc(torch, k, w, h, pitch_px=None, stride_px=None, rgb=True):
    pitch_px = pitch_px or w
    stride_px = stride_px or h * pitch_px
    dev = torch.device("cuda:0")
    out = dict(frame=torch.full((k * stride_px,), SENTINEL, dtype=torch.int32, device=dev), geom=(k, w, h, pitch_px, stride_px))
    out["rgb_t"] = torch.zeros((k, h, w, 3), dtype=torch.float32, device=dev) if rgb else None
    out["dbg"] = gpu.Debug(out["rgb_t"].data_ptr(), None, None, None) if rgb else None
    return out


def queue(r, out, cams, s, T, stream=None, max_steps=256):
    k, w, h, pitch_px, stride_px = out["geom"]
    assert len(cams) == k
    r.render_views_into(out["frame"].data_ptr(), cams, w, h, max_steps, pitch_bytes=pitch_px * 4, view_stride_bytes=stride_px * 4,
                        debug=out["dbg"], stream=stream, samples=s, adaptive=T)


def collect(out):
    k, w, h, pitch_px, stride_px = out["geom"]
    raw = out["frame"].cpu().numpy().view(np.uint32)
    out["raw"] = raw
    out["xrgb"] = np.stack([np.stack([raw[v * stride_px + y * pitch_px:v * stride_px + y * pitch_px + w] for y in range(h)]) for v in range(k)])
    if out["rgb_t"] is not None:
        out["rgb"] = out["rgb_t"].cpu().numpy()
    inside = np.zeros(raw.shape, dtype=bool)
    for v in range(k):
        for y in range(h):
            inside[v * stride_px + y * pitch_px:v * stride_px + y * pitch_px + w] = True
    out["outside_untouched"] = bool((raw[~inside] == SENTINEL).all())
    return out


def render_batch(torch, r, cams, w, h, s, T, pitch_px=None, stride_px=None, rgb=True, stream=None, max_steps=256):
    out = alloc(torch, len(cams), w, h, pitch_px, stride_px, rgb)
    torch.cuda.synchronize()                 # torch's fills run on ITS stream; the batch on the renderer's own
    queue(r, out, cams, s, T, stream, max_steps)
    r.sync()
    return collect(out)


def render_single(torch, r2, cam, w, h, s, T, max_steps=256):
    """the frame of set_samples(s) / set_adaptive_samples(T) under `cam`, by lol_gpu_render_device"""
    r2.set_samples(s)
    r2.set_adaptive_samples(T)
    dev = torch.device("cuda:0")
    frame = torch.full((h, w), SENTINEL, dtype=torch.int32, device=dev)
    rgb = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    r2.render_into(frame.data_ptr(), w, h, max_steps, camera=cam, debug=gpu.Debug(rgb.data_ptr(), None, None, None))
    r2.sync()
    return dict(xrgb=frame.cpu().numpy().view(np.uint32), rgb=rgb.cpu().numpy())


_oracle = {}


def oracle(name, sc, v, cam, w, h, s, T, fmt=None, fmt_name=None):
    """(packed, rgb, mask or None) of the oracle's frame; the s x s frame is computed once per (scene, view, size, s, format)"""
    full_key = (name, v, w, h, s, fmt_name)
    if full_key not in _oracle:
        _oracle[full_key] = A.render(sc, w, h, s, fmt=fmt, camera=cam)
    full = _oracle[full_key]
    if T < 0:
        return full[0], full[1], None
    key = full_key + (T,)
    if key not in _oracle:
        _oracle[key] = D.render(sc, w, h, s, T, fmt=fmt, camera=cam, full=full)
    return _oracle[key]


def make_pair(specialize, sc, switch=True):
    """the renderer under test (the switch on before prepare, which waits for the scene compiler) and a second context for the
    single frames.  Which kernels the batches run is asked of the library."""
    r = gpu.Renderer(0, specialize=specialize)
    if switch:
        r.set_view_samples(True)
    r.prepare(sc)
    r2 = gpu.Renderer(0, specialize=specialize)
    r2.prepare(sc)
    assert_kernels(r, bool(specialize) and switch)
    return r, r2


def assert_kernels(r, own):
    """the scene's own kernels (the module is there: settled, and it was compiled with the switch) or the interpreter's"""
    if own:
        assert r.view_samples and r.specialize_state()[0] == 2 and r.kernel_name() == "lol_render_spec", r.specialize_log()
    want = ("lol_render_spec_batch_aa", "lol_render_spec_batch_aa_list", "lol_render_spec_batch") if own else \
           ("render_interp_batch_aa", "render_interp_batch_aa_list", None)
    for s in (2, 4):
        assert r.view_samples_kernel_name(s, -1) == want[0] and r.view_samples_kernel_name(s, 16) == want[1], r.specialize_log()
    if want[2]:
        assert r.view_samples_kernel_name(1, -1) == want[2]


def assert_view(b, v, g, what):
    assert np.array_equal(b["xrgb"][v], g["xrgb"]), f"{what}: pixels differ from the single frame"
    assert np.array_equal(bits(b["rgb"][v]), bits(g["rgb"])), f"{what}: rgb differs from the single frame"


@pytest.mark.parametrize("specialize", [1, 0], ids=["scene-kernel", "interpreter"])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_views_equal_single_frames_and_the_oracle(torch_cuda, scenes, name, specialize):
    sc = scenes[name]
    cams = S.orbit_cameras(sc, K)
    r, r2 = make_pair(specialize, sc)
    try:
        for (w, h) in ((64, 36), (50, 23)):
            for s in (2, 4):
                for T in (-1, 0, 16):
                    b = render_batch(torch_cuda, r, cams, w, h, s, T)
                    assert b["outside_untouched"]
                    refined = 0
                    for v in range(K):
                        what = f"{name} {w}x{h} s={s} T={T} view {v}"
                        assert_view(b, v, render_single(torch_cuda, r2, cams[v], w, h, s, T), what)
                        ox, orgb, m = oracle(name, sc, v, cams[v], w, h, s, T)
                        assert np.array_equal(b["xrgb"][v], ox), f"{what}: pixels differ from the oracle"
                        assert np.array_equal(bits(b["rgb"][v]), bits(orgb)), f"{what}: rgb differs from the oracle"
                        if T == 16:
                            if v in SOME_BUT_NOT_ALL:
                                assert 0 < int(m.sum()) < w * h, what
                            if v == NONE_REFINED:
                                assert int(m.sum()) == 0, what
                        refined += int(m.sum()) if m is not None else 0
                    if T >= 0:
                        assert r.views_refined() == refined, (name, w, h, s, T)
        assert_kernels(r, bool(specialize))
    finally:
        r.close()
        r2.close()


@pytest.mark.parametrize("specialize", [1, 0], ids=["scene-kernel", "interpreter"])
def test_a_batch_may_mix_any_cameras(torch_cuda, scenes, specialize):
    """a sane camera, one beyond 10^15 (the plain pipeline, the list with v_div_fixup), one with a -0 coordinate and one inside an
    object (no first step given), then sane ones again: each view equals its single frame"""
    sc = scenes["scene4"]
    orbit = S.orbit_cameras(sc, K)
    cams = [orbit[1], insane_camera(), cam_at(-0.0, 6.0, 3.0, 0.0, -0.5, -1.0), cam_at(0.0, 1.0, -6.0, 0.0, 0.0, -1.0),
            cam_at(-2.0, 6.0, 3.0, 0.2, -0.5, -1.0), orbit[11]]
    r, r2 = make_pair(specialize, sc)
    try:
        for order in ("rows", "cols"):
            r.set_tile_order(order)
            for (w, h) in ((61, 37),):
                for s in (2, 4):
                    for T in (-1, 8):
                        b = render_batch(torch_cuda, r, cams, w, h, s, T)
                        assert b["outside_untouched"]
                        for v, cam in enumerate(cams):
                            assert_view(b, v, render_single(torch_cuda, r2, cam, w, h, s, T), f"{order} s={s} T={T} view {v}")
    finally:
        r.close()
        r2.close()


@pytest.mark.parametrize("specialize", [1, 0], ids=["scene-kernel", "interpreter"])
def test_lossy_format_and_padded_layout(torch_cuda, scenes, specialize):
    """RGB565's shifts and losses in a 32-bit pixel, a padded pitch and a padded view stride over a sentinel: every pixel inside the
    views is written (refined or not), nothing outside them; pixels equal the single frames and the oracle."""
    sc = scenes["scene4"]
    orbit = S.orbit_cameras(sc, K)
    idx = [1, NONE_REFINED, 5, 11, 0]
    cams = [orbit[i] for i in idx]
    w, h, pitch_px = 50, 23, 64
    stride_px = h * pitch_px + 40
    r, r2 = make_pair(specialize, sc)
    try:
        for fmt, fmt_name in ((RGB565_IN_32, "rgb565-in-32"), (None, None)):
            r.set_pixel_format(fmt)
            r2.set_pixel_format(fmt)
            for s, T in ((2, -1), (2, 16), (4, 16), (4, 0)):
                b = render_batch(torch_cuda, r, cams, w, h, s, T, pitch_px=pitch_px, stride_px=stride_px)
                assert b["outside_untouched"], (fmt_name, s, T)
                if fmt is not None:                      # (the sentinel has bits no pixel of this format has)
                    assert ((b["xrgb"] & 0xFFFF0000) == 0xFF000000).all(), (fmt_name, s, T)
                for v, i in enumerate(idx):
                    what = f"{fmt_name} s={s} T={T} view {v}"
                    assert_view(b, v, render_single(torch_cuda, r2, cams[v], w, h, s, T), what)
                    ox, orgb, m = oracle("scene4", sc, i, cams[v], w, h, s, T, fmt=fmt, fmt_name=fmt_name)
                    assert np.array_equal(b["xrgb"][v], ox) and np.array_equal(bits(b["rgb"][v]), bits(orgb)), what
                    if T == 16 and i in SOME_BUT_NOT_ALL:
                        assert 0 < int(m.sum()) < w * h
                # without the diagnostic colour: the same pixels
                b2 = render_batch(torch_cuda, r, cams, w, h, s, T, pitch_px=pitch_px, stride_px=stride_px, rgb=False)
                assert np.array_equal(b2["raw"], b["raw"]), (fmt_name, s, T)
    finally:
        r.close()
        r2.close()


def test_one_sample_is_render_views(torch_cuda, scenes):
    """samples == 1 is lol_gpu_render_views whatever contrast says, with hit_dist, hit_id and steps — and whatever the context's own
    lol_gpu_set_samples says: the new call does not read it (and does not change it)."""
    sc = scenes["scene4"]
    cams = S.orbit_cameras(sc, 5)
    w, h = 61, 37
    r = gpu.Renderer(0)
    r.set_view_samples(True)
    r.prepare(sc)
    try:
        dev = torch_cuda.device("cuda:0")

        def run(samples_call, **kw):
            t = dict(frame=torch_cuda.full((5, h, w), SENTINEL, dtype=torch_cuda.int32, device=dev),
                     rgb=torch_cuda.zeros((5, h, w, 3), dtype=torch_cuda.float32, device=dev),
                     dist=torch_cuda.zeros((5, h, w), dtype=torch_cuda.float32, device=dev),
                     id=torch_cuda.zeros((5, h, w), dtype=torch_cuda.int32, device=dev),
                     steps=torch_cuda.zeros((5, h, w), dtype=torch_cuda.int32, device=dev))
            torch_cuda.cuda.synchronize()
            dbg = gpu.Debug(t["rgb"].data_ptr(), t["dist"].data_ptr(), t["id"].data_ptr(), t["steps"].data_ptr())
            if samples_call:
                fcs = (S.FrameCamera * 5)(*[sc.frame_camera(w, h, c) for c in cams])
                st = gpu.gpu_lib().lol_gpu_render_views_samples(r._ctx, fcs, 5, w, h, 256, 1, kw["contrast"], C.c_void_p(t["frame"].data_ptr()),
                                                                w * 4, h * w * 4, C.byref(dbg), None)
                assert st == 0, st
            else:
                r.render_views_into(t["frame"].data_ptr(), cams, w, h, debug=dbg)
            r.sync()
            return {k: bits(a.cpu().numpy()) for k, a in t.items()}

        want = run(False)
        assert (want["steps"] != 0).any() and (want["id"] != 0).any()
        for contrast in (-1, 16):
            got = run(True, contrast=contrast)
            for k in want:
                assert np.array_equal(got[k], want[k]), (contrast, k)
        r.set_samples(4)
        r.set_adaptive_samples(3)
        got = run(True, contrast=-1)
        for k in want:
            assert np.array_equal(got[k], want[k]), ("context at 4 samples", k)
        b = render_batch(torch_cuda, r, cams, w, h, 2, -1)
        assert r.samples == 4 and r.adaptive_samples == 3
        r2 = gpu.Renderer(0)
        r2.prepare(sc)
        try:
            for v in range(5):
                assert_view(b, v, render_single(torch_cuda, r2, cams[v], w, h, 2, -1), f"context at 4 samples, batch at 2, view {v}")
        finally:
            r2.close()
    finally:
        r.close()


def test_refusals_write_nothing(torch_cuda, scenes):
    sc = scenes["scene4"]
    w, h = 64, 36
    cams = S.orbit_cameras(sc, 2)
    fcs = (S.FrameCamera * 2)(*[sc.frame_camera(w, h, c) for c in cams])
    lib = gpu.gpu_lib()
    r = gpu.Renderer(0)
    try:
        dev = torch_cuda.device("cuda:0")
        frame = torch_cuda.full((2 * h * w + 64,), SENTINEL, dtype=torch_cuda.int32, device=dev)
        diag = torch_cuda.full((2 * h * w * 3,), SENTINEL, dtype=torch_cuda.int32, device=dev)
        torch_cuda.cuda.synchronize()

        def call(n=2, pitch=w * 4, stride=h * w * 4, width=w, height=h, s=2, T=-1, dbg=None, cam=fcs, dst=True):
            return lib.lol_gpu_render_views_samples(r._ctx, cam, n, width, height, 256, s, T, C.c_void_p(frame.data_ptr()) if dst else None,
                                                    pitch, stride, dbg, None)

        assert call() == ERR_NO_PROGRAM and call(T=16) == ERR_NO_PROGRAM and call(s=1) == ERR_NO_PROGRAM
        r.set_view_samples(True)
        r.prepare(sc)
        before = r.tile_order()
        for T in (-1, 16):
            for s in (0, 3, 8, -2):
                assert call(s=s, T=T) == ERR_ARG, (s, T)
            assert call(n=0, T=T) == ERR_ARG and call(n=-1, T=T) == ERR_ARG and call(n=gpu.MAX_VIEWS + 1, T=T) == ERR_ARG
            assert call(pitch=w * 4 - 4, T=T) == ERR_ARG and call(pitch=w * 4 + 2, T=T) == ERR_ARG
            assert call(stride=h * w * 4 - 4, T=T) == ERR_ARG and call(stride=h * w * 4 + 2, T=T) == ERR_ARG
            assert call(width=0, T=T) == ERR_ARG and call(cam=None, T=T) == ERR_ARG and call(dst=False, T=T) == ERR_ARG
            # hit_dist, hit_id, steps: no single value for a supersampled pixel
            for which in range(1, 4):
                ptrs = [diag.data_ptr() if i in (0, which) else None for i in range(4)]
                assert call(T=T, dbg=C.byref(gpu.Debug(*ptrs))) == ERR_UNSUPPORTED, (T, which)
        for s in (2, 4):
            assert call(s=s, T=-2) == ERR_ARG and call(s=s, T=256) == ERR_ARG
        assert call(s=1, T=256) == ERR_ARG
        # the sample grid: more than 65535 tiles on an axis (s w / 16, s h / 4); the launch counted in SAMPLES (1024 x 1024 views:
        # 2^20 pixels, 2^24 samples at s = 4, so 256 views are 2^32 lanes — while their pixels alone would fit)
        big_w = 65535 * 16 // 2 + 16
        assert call(n=1, width=big_w, height=1, pitch=big_w * 4, stride=big_w * 4) == ERR_ARG
        big_h = 65535 * 4 // 4 + 4
        assert call(n=1, width=1, height=big_h, pitch=4, stride=big_h * 4, s=4) == ERR_ARG
        assert call(n=256, width=1024, height=1024, pitch=4096, stride=4096 * 1024, s=4) == ERR_ARG
        assert call(n=256, width=1024, height=1024, pitch=4096, stride=4096 * 1024, s=4, T=16) == ERR_ARG
        # adaptive batches: the pixel table's fields, s w <= 65536 and s h <= 32768
        assert call(n=1, width=32768 + 16, height=1, pitch=(32768 + 16) * 4, stride=(32768 + 16) * 4, s=2, T=0) == ERR_ARG
        assert call(n=1, width=1, height=8192 + 4, pitch=4, stride=(8192 + 4) * 4, s=4, T=0) == ERR_ARG
        r.sync()
        torch_cuda.cuda.synchronize()
        assert bool((frame.cpu().numpy().view(np.uint32) == SENTINEL).all())
        assert bool((diag.cpu().numpy().view(np.uint32) == SENTINEL).all())
        # a scratch allocation that fails: LOL_GPU_ERR_HIP, nothing written, and the context still renders
        r.testing_fail_view_scratch(1)
        assert call(T=16) == ERR_HIP and "scratch" in gpu.gpu_lib().lol_gpu_error(r._ctx).decode()
        r.sync()
        assert bool((frame.cpu().numpy().view(np.uint32) == SENTINEL).all())
        # ... and the next valid calls work, full and adaptive; the scheduling state of plain frames is what it was
        for T in (16, -1):
            assert call(T=T) == 0
            r.sync()
            got = frame.cpu().numpy().view(np.uint32)
            for v in range(2):
                ox, _, _ = oracle("scene4-orbit2", sc, v, cams[v], w, h, 2, T)
                assert np.array_equal(got[v * h * w:(v + 1) * h * w].reshape(h, w), ox), (T, v)
            assert bool((got[2 * h * w:] == SENTINEL).all())
        assert r.tile_order() == before
    finally:
        r.close()


def test_a_batch_leaves_scheduling_alone(torch_cuda, scenes):
    """A repeated view under longest-first until the library has sorted it; a full and an adaptive supersampled batch; the tile-order
    state is what it was and the next plain frame of that view still comes from the tables, and equals the oracle."""
    sc = scenes["scene4"]
    w, h = 256, 144
    r = gpu.Renderer(0)
    r.set_view_samples(True)
    r.prepare(sc)
    try:
        assert r.tile_order()["mode"] == "lpt"
        dev = torch_cuda.device("cuda:0")
        frame = torch_cuda.zeros((h, w), dtype=torch_cuda.int32, device=dev)
        torch_cuda.cuda.synchronize()
        stream = r.next_stream()
        for _ in range(5):
            r.render_into(frame.data_ptr(), w, h, stream=stream)
        r.sync()
        before = r.tile_order()
        assert before["order"] == "lpt" and before["decisions"] >= 1 and not before["deciding"], before
        cams = S.orbit_cameras(sc, K)
        for T in (-1, 16):
            b = render_batch(torch_cuda, r, [cams[i] for i in SOME_BUT_NOT_ALL], 64, 36, 2, T, stream=stream)
            for v, i in enumerate(SOME_BUT_NOT_ALL):
                assert np.array_equal(b["xrgb"][v], oracle("scene4", sc, i, cams[i], 64, 36, 2, T)[0]), (T, v)
            assert r.tile_order() == before
        frame.zero_()
        torch_cuda.cuda.synchronize()
        r.render_into(frame.data_ptr(), w, h, stream=stream)
        r.sync()
        after = r.tile_order()
        assert after["order"] == "lpt" and not after["deciding"] and after["decisions"] == before["decisions"], (before, after)
        ox, _, _ = O.render_rows(sc, w, h, 0, h)
        assert np.array_equal(frame.cpu().numpy().view(np.uint32), ox)
    finally:
        r.close()


def test_batches_in_flight_on_two_streams(torch_cuda, scenes):
    """Ten batches of different cameras, sizes of s and contrasts queued back to back with NO wait between them, over two streams:
    every destination is allocated and filled first, torch is synchronised once, then the calls follow each other and only then the
    renderer is waited for.  Seven of them are adaptive and the scratch ring has 4 sets, so from the fifth adaptive batch on a batch
    takes a set whose previous batch may still be running — and each must still render ITS cameras.  Queued once: a correctness
    check, not a stress loop."""
    sc = scenes["scene4"]
    w, h = 64, 36
    orbit = S.orbit_cameras(sc, K)
    plans = [(2, 16), (4, 16), (2, -1), (2, 0), (4, 16), (2, 16), (4, -1), (4, 0), (2, 16), (4, -1)]
    assert sum(1 for _, T in plans if T >= 0) > 4
    index = [[(g + 3 * v) % K for v in range(5)] for g in range(len(plans))]
    r = gpu.Renderer(0)
    r.set_view_samples(True)
    r.prepare(sc)
    try:
        r.set_frames_in_flight(2)
        outs = [alloc(torch_cuda, 5, w, h) for _ in plans]
        torch_cuda.cuda.synchronize()
        for out, idx, (s, T) in zip(outs, index, plans):
            queue(r, out, [orbit[i] for i in idx], s, T)
        r.sync()
        for g, (out, idx, (s, T)) in enumerate(zip(outs, index, plans)):
            collect(out)
            assert out["outside_untouched"]
            for v, i in enumerate(idx):
                ox, orgb, _ = oracle("scene4", sc, i, orbit[i], w, h, s, T)
                assert np.array_equal(out["xrgb"][v], ox) and np.array_equal(bits(out["rgb"][v]), bits(orgb)), f"batch {g} (s={s} T={T}) view {v}"
    finally:
        r.close()


def test_the_scratch_grows_at_the_wrap_of_its_ring(torch_cuda, scenes):
    """Five adaptive batches (s = 2, T = 16) queued back to back with NO wait between them, over two streams.  The first four hold 2
    views of 16 x 8 and fill the ring of scratch sets; the fifth holds 3 views of 32 x 16, so it takes set 0 again and must GROW it
    while the first batch, which classified its pixels there, may still be in flight.  Every pixel of every batch is the adaptive
    reference's, and views_refined() afterwards is the reference's count for the fifth batch: the ring's last set is the one that
    grew.  Queued once."""
    sc = scenes["scene4"]
    orbit = S.orbit_cameras(sc, K)
    s, T = 2, 16
    plans = [(16, 8, [0, 1]), (16, 8, [2, 3]), (16, 8, [4, 5]), (16, 8, [6, 8]), (32, 16, list(SOME_BUT_NOT_ALL))]
    r = gpu.Renderer(0)
    r.set_view_samples(True)
    r.prepare(sc)
    try:
        r.set_frames_in_flight(2)
        outs = [alloc(torch_cuda, len(idx), w, h, pitch_px=w + 3, stride_px=h * (w + 3) + 5) for w, h, idx in plans]
        torch_cuda.cuda.synchronize()
        for out, (w, h, idx) in zip(outs, plans):
            queue(r, out, [orbit[i] for i in idx], s, T)
        r.sync()
        for g, (out, (w, h, idx)) in enumerate(zip(outs, plans)):
            collect(out)
            assert out["outside_untouched"], f"batch {g}"
            refined = 0
            for v, i in enumerate(idx):
                ox, orgb, m = oracle("scene4", sc, i, orbit[i], w, h, s, T)
                assert np.array_equal(out["xrgb"][v], ox) and np.array_equal(bits(out["rgb"][v]), bits(orgb)), f"batch {g} view {v}"
                refined += int(m.sum())
        assert 0 < refined < 3 * 32 * 16                         # (of the fifth batch: the loop's last)
        assert r.views_refined() == refined
    finally:
        r.close()


def test_late_switch_and_tiering(torch_cuda, scenes):
    """The switch set after the upload: the module has none of the new kernels, batches run on the interpreter's, same pixels (and
    frames keep the scene's kernel).  The switch on, one batch before specialize_wait() and one after: same pixels from whichever
    kernel was there, and after the wait it IS the scene's."""
    sc = scenes["scene4"]
    w, h = 50, 23
    orbit = S.orbit_cameras(sc, K)
    idx = [1, NONE_REFINED, 5, 11]
    cams = [orbit[i] for i in idx]

    def check(b, s, T, what):
        for v, i in enumerate(idx):
            ox, orgb, _ = oracle("scene4", sc, i, orbit[i], w, h, s, T)
            assert np.array_equal(b["xrgb"][v], ox) and np.array_equal(bits(b["rgb"][v]), bits(orgb)), f"{what} s={s} T={T} view {v}"

    r = gpu.Renderer(0)
    r.prepare(sc)
    try:
        assert not r.view_samples
        r.set_view_samples(True)
        assert r.view_samples
        assert_kernels(r, False)
        for s, T in ((2, -1), (4, 16)):
            check(render_batch(torch_cuda, r, cams, w, h, s, T), s, T, "late switch")
        assert r.kernel_name() == "lol_render_spec"
    finally:
        r.close()
    r = gpu.Renderer(0)
    r.set_view_samples(True)
    r.prepare(sc, wait=False)
    try:
        for s, T in ((2, 16), (4, -1)):
            check(render_batch(torch_cuda, r, cams, w, h, s, T), s, T, "before the scene kernel")
        r.specialize_wait()
        assert_kernels(r, True)
        for s, T in ((2, 16), (4, -1)):
            check(render_batch(torch_cuda, r, cams, w, h, s, T), s, T, "on the scene kernel")
    finally:
        r.close()


def test_the_orbit_host_supersamples(torch_cuda, scenes, tmp_path):
    """python -m loltracer_amd SCENE --orbit K --orbit-samples N [--orbit-adaptive T]: K PPMs from one supersampled batch, each the
    oracle's frame under scene.orbit_cameras(scene, K)[v]."""
    scene_file = os.path.join(ROOT, "tests", "golden", "scenes", "scene4.lol")
    k, w, h = 4, 64, 36
    sc = scenes["scene4"]
    cams = S.orbit_cameras(sc, k)
    for extra, (s, T) in ((["--orbit-samples", "2"], (2, -1)), (["--orbit-samples", "2", "--orbit-adaptive", "8"], (2, 8))):
        out = tmp_path / ("views_%d" % T)
        cmd = [sys.executable, "-m", "loltracer_amd", scene_file, "--orbit", str(k), "--size", f"{w}x{h}", "-o", str(out)] + extra
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0, p.stdout
        assert sorted(os.listdir(out)) == [f"view_{v:04d}.ppm" for v in range(k)]
        for v in range(k):
            data = open(out / f"view_{v:04d}.ppm", "rb").read()
            head = b"P6\n%d %d\n255\n" % (w, h)
            assert data.startswith(head)
            rgb = np.frombuffer(data[len(head):], dtype=np.uint8).reshape(h, w, 3).astype(np.uint32)
            ox, _, _ = oracle("scene4-orbit4", sc, v, cams[v], w, h, s, T)
            assert np.array_equal(rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2], ox), (extra, v)
    # options the host cannot honour are refused, not ignored
    base = [sys.executable, "-m", "loltracer_amd", scene_file, "--size", f"{w}x{h}"]
    for cmd in (base + ["--orbit-samples", "2"], base + ["--orbit", "4", "-o", str(tmp_path / "x"), "--orbit-samples", "2", "--orbit-adaptive", "300"]):
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 1 and "--orbit" in p.stdout, (cmd, p.stdout)
