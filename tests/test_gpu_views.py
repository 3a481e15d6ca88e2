"""Batches of views (lol_gpu_render_views): view v of a batch IS the frame lol_gpu_render_device renders under cams[v] in a fixed
tile order — pixels, float colours, hit distances, ids and both step counts EQUAL, bit for bit — and both are the CPU oracle's.

Every comparison is array equality on the bit patterns.  The oracle (tests/oracle_lib.py) gives packed pixels, float colours and
ids per frame (render_rows) and the hit distance per pixel (probe): all of them are held against every pixel of every view.  The
step counts are held against the single-frame render (whose counts tests/test_gpu_parity.py holds against the oracle's under each
skip mask).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from loltracer_amd import gpu, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402  (orbit_camera: the flagship workload's camera path)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7B0B5
ERR_ARG, ERR_NO_PROGRAM, ERR_UNSUPPORTED = -3, -4, -5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def cam_at(x, y, z, dx, dy, dz, fov=90.0):
    cam = S.Camera()
    cam.point = S.V3(x, y, z)
    d = np.array([dx, dy, dz], dtype=np.float32)
    n = np.float32(1.0) / np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1]) + np.float32(d[2] * d[2]), dtype=np.float32)
    cam.direction = S.V3(*(float(np.float32(v * n)) for v in d))
    cam.fov = float(np.float32(np.float32(fov) / np.float32(180) * np.pi))
    return cam


def insane_camera():
    """the camera of test_gpu_parity.test_camera_beyond_the_sane_range: 10^16 away, not camera_sane"""
    cam = S.Camera()
    cam.point = S.V3(1.0e16, 3.0, 2.5)
    cam.direction = S.V3(-1.0, 0.0, 0.0)
    cam.fov = float(np.float32(np.float32(60.0) / np.float32(180) * np.pi))
    return cam


def copy_camera(c):
    out = S.Camera()
    C.memmove(C.byref(out), C.byref(c), C.sizeof(S.Camera))
    return out


def thirteen_cameras(sc):
    """A spread of the orbit, the scene's own camera, a camera beyond the sane range in the MIDDLE, and the cameras of
    test_gpu_parity.test_first_step_is_given_or_taken (the first step given, and declined for each reason there is)."""
    return [
        bench.orbit_camera(0, 256), bench.orbit_camera(37, 256), bench.orbit_camera(91, 256),
        copy_camera(sc.camera),
        cam_at(-2.0, 6.0, 3.0, 0.2, -0.5, -1.0),          # the first step is given
        cam_at(-0.0, 6.0, 3.0, 0.0, -0.5, -1.0),          # x = -0: taken per pixel
        insane_camera(),                                  # index 6 of 13: the middle
        cam_at(0.0, 1.0, -6.0, 0.0, 0.0, -1.0),           # inside scene4's blob: the first step ends the march
        cam_at(0.0, -0.9995, 3.0, 0.0, 0.1, -1.0),        # 0.0005 above scene4's floor
        cam_at(0.0, 150.0, 0.0, 0.0, -1.0, -0.01),        # the first step overshoots MAX_DIST
        cam_at(0.0, 99.0, 0.0, 0.0, -1.0, -0.01),         # dist == MAX_DIST after one step
        bench.orbit_camera(128, 256), bench.orbit_camera(200, 256),
    ]


def pick(cams, k):
    """which of the thirteen a batch of k holds (by index)"""
    return {1: [3], 2: [1, 6], 13: list(range(13))}[k]


_oracle_cache = {}


def oracle_view(name, sc, idx, cam, w, h, max_steps=256):
    key = (name, idx, w, h, max_steps)
    if key not in _oracle_cache:
        ox, orgb, osteps = O.render_rows(sc, w, h, 0, h, max_steps, camera=cam, want_steps=True)
        dist = np.zeros((h, w), dtype=np.float32)
        for y in range(h):
            for x in range(w):
                dist[y, x] = O.probe(sc, w, h, x, y, max_steps, camera=cam).hit_dist
        _oracle_cache[key] = dict(xrgb=ox, rgb=orgb, id=osteps[..., 2].astype(np.uint32), dist=dist)
    return _oracle_cache[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


DIAGNOSTICS = ("rgb", "dist", "id", "steps")


def alloc_batch(torch, k, w, h, pitch_px=None, stride_px=None, debug=True):
    """The sentinel-filled destination and the diagnostics asked for (debug: True = all four, False = none, or a tuple of names of
    DIAGNOSTICS) of a batch of k views; filled on torch's stream: synchronise torch before the batch is queued."""
    pitch_px = pitch_px or w
    stride_px = stride_px or h * pitch_px
    dev = torch.device("cuda:0")
    out = dict(frame=torch.full((max(1, k) * stride_px,), SENTINEL, dtype=torch.int32, device=dev), geom=(k, w, h, pitch_px, stride_px))
    want = DIAGNOSTICS if debug is True else () if debug is False else tuple(debug)
    shapes = dict(rgb=((k, h, w, 3), torch.float32), dist=((k, h, w), torch.float32), id=((k, h, w), torch.int32),
                  steps=((k, h, w), torch.int32))
    for name in want:
        out[name + "_t"] = torch.zeros(shapes[name][0], dtype=shapes[name][1], device=dev)
    ptr = [out[n + "_t"].data_ptr() if n in want else None for n in DIAGNOSTICS]
    out["dbg"] = gpu.Debug(*ptr) if want else None
    return out


def queue_batch(r, out, cams, max_steps=256, stream=None):
    k, w, h, pitch_px, stride_px = out["geom"]
    assert len(cams) == k
    r.render_views_into(out["frame"].data_ptr(), cams, w, h, max_steps, pitch_bytes=pitch_px * 4, view_stride_bytes=stride_px * 4,
                        debug=out["dbg"], stream=stream)


def render_batch(torch, r, cams, w, h, max_steps=256, pitch_px=None, stride_px=None, debug=True, stream=None):
    """One batch, waited for → dict of [K, h, w(, 3)] arrays (+ 'raw': the whole destination)."""
    out = alloc_batch(torch, len(cams), w, h, pitch_px, stride_px, debug)
    torch.cuda.synchronize()                 # torch's fills run on ITS stream; the batch on the renderer's own
    queue_batch(r, out, cams, max_steps, stream)
    r.sync()
    return collect(out, *out["geom"])


def collect(out, k, w, h, pitch_px, stride_px):
    raw = out["frame"].cpu().numpy().view(np.uint32)
    out["raw"] = raw
    views = np.zeros((k, h, w), dtype=np.uint32)
    for v in range(k):
        for y in range(h):
            o = v * stride_px + y * pitch_px
            views[v, y] = raw[o:o + w]
    out["xrgb"] = views
    for name in DIAGNOSTICS:
        if name + "_t" in out:
            a = out[name + "_t"].cpu().numpy()
            out[name] = a.view(np.uint32) if name in ("id", "steps") else a
    return out


def untouched_outside_views(out, k, w, h, pitch_px, stride_px):
    mask = np.ones(out["raw"].shape, dtype=bool)
    for v in range(k):
        for y in range(h):
            o = v * stride_px + y * pitch_px
            mask[o:o + w] = False
    return bool((out["raw"][mask] == SENTINEL).all())


def render_single(torch, r, cam, w, h, max_steps=256):
    dev = torch.device("cuda:0")
    frame = torch.zeros((h, w), dtype=torch.int32, device=dev)
    rgb = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    dist = torch.zeros((h, w), dtype=torch.float32, device=dev)
    hid = torch.zeros((h, w), dtype=torch.int32, device=dev)
    steps = torch.zeros((h, w), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    r.render_into(frame.data_ptr(), w, h, max_steps, camera=cam,
                  debug=gpu.Debug(rgb.data_ptr(), dist.data_ptr(), hid.data_ptr(), steps.data_ptr()))
    r.sync()
    return dict(xrgb=frame.cpu().numpy().view(np.uint32), rgb=rgb.cpu().numpy(), dist=dist.cpu().numpy(),
                id=hid.cpu().numpy().view(np.uint32), steps=steps.cpu().numpy().view(np.uint32))


def assert_view_is_frame(b, v, g, what):
    assert np.array_equal(b["xrgb"][v], g["xrgb"]), f"{what}: pixels differ from the single frame"
    assert np.array_equal(bits(b["rgb"][v]), bits(g["rgb"])), f"{what}: rgb differs from the single frame"
    assert np.array_equal(b["id"][v], g["id"]), f"{what}: hit ids differ from the single frame"
    assert np.array_equal(bits(b["dist"][v]), bits(g["dist"])), f"{what}: hit distances differ from the single frame"
    assert np.array_equal(b["steps"][v] & 0xFFFF, g["steps"] & 0xFFFF), f"{what}: march steps differ from the single frame"
    assert np.array_equal(b["steps"][v] >> 16, g["steps"] >> 16), f"{what}: shadow steps differ from the single frame"


def assert_view_is_oracle(b, v, o, what):
    assert np.array_equal(b["xrgb"][v], o["xrgb"]), f"{what}: pixels differ from the oracle"
    assert np.array_equal(bits(b["rgb"][v]), bits(o["rgb"])), f"{what}: rgb differs from the oracle"
    assert np.array_equal(b["id"][v], o["id"]), f"{what}: hit ids differ from the oracle"
    assert np.array_equal(bits(b["dist"][v]), bits(o["dist"])), f"{what}: hit distances differ from the oracle"


def make_pair(specialize, sc, switch=True):
    """the renderer under test (batch switch on before prepare) and a second one for single frames in row order"""
    r = gpu.Renderer(0, specialize=specialize)
    r.set_view_batches(switch)
    r.prepare(sc)
    r2 = gpu.Renderer(0, specialize=specialize)
    r2.set_tile_order("rows")
    r2.prepare(sc)
    want = "lol_render_spec" if specialize else "render_interp"
    assert r.kernel_name() == want and r2.kernel_name() == want, r.specialize_log()
    return r, r2


@pytest.mark.parametrize("specialize", [1, 0], ids=["scene-kernel", "interpreter"])
@pytest.mark.parametrize("name", ["scene", "scene2", "scene3", "scene4"])
def test_views_equal_single_frames_and_the_oracle(torch_cuda, scenes, name, specialize):
    sc = scenes[name]
    cams = thirteen_cameras(sc)
    r, r2 = make_pair(specialize, sc)
    try:
        for skips in (7, 0):
            r.set_exact_skips(skips)
            r2.set_exact_skips(skips)
            for (w, h) in ((64, 36), (61, 37), (128, 128)):
                singles = {}
                for k in (1, 2, 13):
                    idx = pick(cams, k)
                    b = render_batch(torch_cuda, r, [cams[i] for i in idx], w, h)
                    assert untouched_outside_views(b, k, w, h, w, h * w)
                    for v, i in enumerate(idx):
                        what = f"{name} {w}x{h} K={k} view {v} (camera {i}) skips={skips}"
                        if i not in singles:
                            singles[i] = render_single(torch_cuda, r2, cams[i], w, h)
                        assert_view_is_frame(b, v, singles[i], what)
                        assert_view_is_oracle(b, v, oracle_view(name, sc, i, cams[i], w, h), what)
                # The batches above ask for the step counts: on the scene kernel they run lol_render_spec_batch_steps.  What a
                # production host runs is the non-counting lol_render_spec_batch: pixels alone, and each diagnostic alone.
                idx = pick(cams, 13)
                for debug in (False, ("id",), ("dist",), ("rgb",), ("steps",)):
                    b = render_batch(torch_cuda, r, [cams[i] for i in idx], w, h, debug=debug)
                    assert untouched_outside_views(b, 13, w, h, w, h * w)
                    for v, i in enumerate(idx):
                        o = oracle_view(name, sc, i, cams[i], w, h)
                        what = f"{name} {w}x{h} diagnostics={debug} view {v} (camera {i}) skips={skips}"
                        assert np.array_equal(b["xrgb"][v], o["xrgb"]), what
                        for d in (debug or ()):
                            want = singles[i]["steps"] if d == "steps" else o[d]
                            assert np.array_equal(bits(b[d][v]), bits(want)), f"{what}: {d}"
    finally:
        r.close()
        r2.close()


@pytest.mark.parametrize("specialize", [1, 0], ids=["scene-kernel", "interpreter"])
def test_layout_padding_formats_and_column_order(torch_cuda, scenes, specialize):
    """Padded pitch and padded view stride over a sentinel: nothing outside the views' w x h pixels is written; the five pixel
    formats of test_gpu_boundary.py; LOL_GPU_TILES_COLS."""
    sc = scenes["scene4"]
    cams = thirteen_cameras(sc)
    idx = [0, 6, 3, 12, 4]
    batch = [cams[i] for i in idx]
    w, h, pitch_px = 61, 37, 80
    stride_px = h * pitch_px + 24
    r = gpu.Renderer(0, specialize=specialize)
    r.set_view_batches(True)
    r.prepare(sc)
    try:
        for order in ("rows", "cols"):
            r.set_tile_order(order)
            for fmt_name in ("xrgb8888", "argb8888", "bgrx8888", "rgba8888", "abgr8888"):
                f = gpu.PIXEL_FORMATS[fmt_name]
                r.set_pixel_format(fmt_name)
                b = render_batch(torch_cuda, r, batch, w, h, pitch_px=pitch_px, stride_px=stride_px)
                assert untouched_outside_views(b, len(batch), w, h, pitch_px, stride_px), (order, fmt_name)
                O.set_pixel_format(f)
                try:
                    for v, i in enumerate(idx):
                        want, _, _ = O.render_rows(sc, w, h, 0, h, camera=cams[i])
                        assert np.array_equal(b["xrgb"][v], want), (order, fmt_name, v)
                finally:
                    O.set_pixel_format(None)
                for v, i in enumerate(idx):           # the diagnostics are dense whatever the pitch
                    o = oracle_view("scene4", sc, i, cams[i], w, h)
                    assert np.array_equal(bits(b["rgb"][v]), bits(o["rgb"])) and np.array_equal(b["id"][v], o["id"])
                    assert np.array_equal(bits(b["dist"][v]), bits(o["dist"]))
            r.set_pixel_format(None)
        # no diagnostics at all (the non-counting kernel), same layout
        r.set_tile_order("rows")
        b = render_batch(torch_cuda, r, batch, w, h, pitch_px=pitch_px, stride_px=stride_px, debug=False)
        assert untouched_outside_views(b, len(batch), w, h, pitch_px, stride_px)
        for v, i in enumerate(idx):
            assert np.array_equal(b["xrgb"][v], oracle_view("scene4", sc, i, cams[i], w, h)["xrgb"])
    finally:
        r.close()


def test_one_big_batch(torch_cuda, scenes):
    """256 orbit views of scene4 at 128 x 128 in one launch: every view against its single-frame render, a dozen also against the
    oracle."""
    sc = scenes["scene4"]
    k, w, h = 256, 128, 128
    cams = [bench.orbit_camera(i, 256) for i in range(k)]
    r, r2 = make_pair(1, sc)
    try:
        b = render_batch(torch_cuda, r, cams, w, h)
        assert untouched_outside_views(b, k, w, h, w, h * w)
        for v in range(k):
            assert_view_is_frame(b, v, render_single(torch_cuda, r2, cams[v], w, h), f"view {v}")
        for v in range(5, k, 22):                # 12 views
            assert_view_is_oracle(b, v, oracle_view("scene4-orbit", sc, v, cams[v], w, h), f"view {v}")
    finally:
        r.close()
        r2.close()


def test_a_batch_leaves_scheduling_alone(torch_cuda, scenes):
    """A repeated view under longest-first until the library has sorted it; a batch; the next plain frame of that view still comes
    from the tables — no trial, no new sort: it is the view's sixth frame, and the tables are sorted before its fourth and every
    16th — and equals the oracle."""
    sc = scenes["scene4"]
    w, h = 256, 144
    r = gpu.Renderer(0)
    r.set_view_batches(True)
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
        idx = (3, 77, 150)
        cams = [bench.orbit_camera(i, 256) for i in idx]
        b = render_batch(torch_cuda, r, cams, 64, 36, stream=stream)
        for v in range(3):
            assert_view_is_oracle(b, v, oracle_view("scene4-orbit", sc, idx[v], cams[v], 64, 36), f"view {v}")
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
    """Batches of different cameras queued back to back with NO wait between them, over two streams: every destination is
    allocated and filled first, torch is synchronised once, then the calls follow each other and only then the renderer is waited
    for.  The first two run side by side on the two streams, the third behind the first, and so on for 14 batches: the ring of view
    records has 8 sets, so from the ninth on a batch takes a set whose previous batch may still be running, and each batch must
    still render ITS cameras.  A correctness check, queued once, not a stress loop."""
    sc = scenes["scene4"]
    w, h = 128, 128
    n_batches = 3 + 11
    per = 8
    # batch g holds orbit frames g, g + 14, g + 28, ...: no two batches share a camera
    index = [[g + n_batches * v for v in range(per)] for g in range(n_batches)]
    groups = [[bench.orbit_camera(i, 256) for i in idx] for idx in index]
    r = gpu.Renderer(0)
    r.set_view_batches(True)
    r.prepare(sc)
    try:
        r.set_frames_in_flight(2)
        outs = [alloc_batch(torch_cuda, per, w, h) for _ in groups]
        torch_cuda.cuda.synchronize()
        for out, cams in zip(outs, groups):
            queue_batch(r, out, cams)
        r.sync()
        for g, (out, cams) in enumerate(zip(outs, groups)):
            collect(out, *out["geom"])
            assert untouched_outside_views(out, per, w, h, w, h * w)
            for v, cam in enumerate(cams):
                assert_view_is_oracle(out, v, oracle_view("scene4-orbit", sc, index[g][v], cam, w, h), f"batch {g} view {v}")
    finally:
        r.close()


def test_the_view_records_grow_at_the_wrap_of_their_ring(torch_cuda, scenes):
    """Nine batches queued back to back with NO wait between them, over two streams.  The first eight hold 2 views each and fill the
    ring of view records, whose sets hold 64 views at least; the ninth holds 65 — one past that floor —, so it takes set 0 again and
    must GROW it while the first batch, which read its records from there, may still be in flight.  Every view of every batch is
    the oracle's frame of ITS camera (no two views share one), and nothing is written outside the views.  Queued once."""
    sc = scenes["scene4"]
    w, h = 16, 8
    sizes = [2] * 8 + [65]
    index, at = [], 0
    for k in sizes:
        index.append(list(range(at, at + k)))
        at += k
    groups = [[bench.orbit_camera(i, 256) for i in idx] for idx in index]
    r = gpu.Renderer(0)
    r.set_view_batches(True)
    r.prepare(sc)
    try:
        r.set_frames_in_flight(2)
        pitch_px, stride_px = w + 3, h * (w + 3) + 5           # padding after every row and every view: it keeps its sentinel
        outs = [alloc_batch(torch_cuda, len(cams), w, h, pitch_px, stride_px) for cams in groups]
        torch_cuda.cuda.synchronize()
        for out, cams in zip(outs, groups):
            queue_batch(r, out, cams)
        r.sync()
        for g, (out, cams) in enumerate(zip(outs, groups)):
            collect(out, *out["geom"])
            assert untouched_outside_views(out, len(cams), w, h, pitch_px, stride_px), f"batch {g}"
            for v, cam in enumerate(cams):
                assert_view_is_oracle(out, v, oracle_view("scene4-orbit", sc, index[g][v], cam, w, h), f"batch {g} view {v}")
    finally:
        r.close()


def test_the_orbit_host_writes_one_ppm_per_view(torch_cuda, scenes, tmp_path):
    """python -m loltracer_amd SCENE --orbit K --size WxH -o DIR: K PPMs from one batch, each the oracle's frame under
    scene.orbit_cameras(scene, K)[v]; options a batch cannot honour are refused, not ignored."""
    import subprocess
    scene_file = os.path.join(ROOT, "tests", "golden", "scenes", "scene4.lol")
    k, w, h = 5, 64, 36
    out = tmp_path / "views"
    cmd = [sys.executable, "-m", "loltracer_amd", scene_file, "--orbit", str(k), "--size", f"{w}x{h}", "-o", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    sc = scenes["scene4"]
    cams = S.orbit_cameras(sc, k)
    assert sorted(os.listdir(out)) == [f"view_{v:04d}.ppm" for v in range(k)]
    for v in range(k):
        data = open(out / f"view_{v:04d}.ppm", "rb").read()
        head = b"P6\n%d %d\n255\n" % (w, h)
        assert data.startswith(head)
        rgb = np.frombuffer(data[len(head):], dtype=np.uint8).reshape(h, w, 3).astype(np.uint32)
        ox, _, _ = O.render_rows(sc, w, h, 0, h, camera=cams[v])
        assert np.array_equal(rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2], ox), v
    for extra in (["--frames", "2"], ["--samples", "2"], ["--adaptive", "8"]):
        p = subprocess.run(cmd + extra, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 1 and "--orbit" in p.stdout, (extra, p.stdout)


def test_refusals_write_nothing(torch_cuda, scenes):
    sc = scenes["scene4"]
    w, h = 64, 36
    cams = [bench.orbit_camera(i, 256) for i in (0, 50)]
    fcs = (S.FrameCamera * 2)(*[sc.frame_camera(w, h, c) for c in cams])
    lib = gpu.gpu_lib()
    r = gpu.Renderer(0)
    try:
        dev = torch_cuda.device("cuda:0")
        frame = torch_cuda.full((2 * h * w + 64,), SENTINEL, dtype=torch_cuda.int32, device=dev)
        torch_cuda.cuda.synchronize()

        def call(n=2, pitch=w * 4, stride=h * w * 4, width=w):
            return lib.lol_gpu_render_views(r._ctx, fcs, n, width, h, 256, C.c_void_p(frame.data_ptr()), pitch, stride, None, None)

        assert call() == ERR_NO_PROGRAM
        r.set_view_batches(True)
        r.prepare(sc)
        for s in (2, 4):
            r.set_samples(s)
            assert call() == ERR_UNSUPPORTED
        r.set_samples(1)
        assert call(n=0) == ERR_ARG and call(n=-1) == ERR_ARG and call(n=gpu.MAX_VIEWS + 1) == ERR_ARG
        assert call(pitch=w * 4 - 4) == ERR_ARG and call(pitch=w * 4 + 2) == ERR_ARG
        assert call(stride=h * w * 4 - 4) == ERR_ARG and call(stride=h * w * 4 + 2) == ERR_ARG
        assert call(width=0) == ERR_ARG
        assert lib.lol_gpu_render_views(r._ctx, None, 2, w, h, 256, C.c_void_p(frame.data_ptr()), w * 4, h * w * 4, None, None) == ERR_ARG
        assert lib.lol_gpu_render_views(r._ctx, fcs, 2, w, h, 256, None, w * 4, h * w * 4, None, None) == ERR_ARG
        r.sync()
        torch_cuda.cuda.synchronize()
        assert bool((frame.cpu().numpy().view(np.uint32) == SENTINEL).all())
        # ... and the next valid call works
        assert call() == 0
        r.sync()
        got = frame.cpu().numpy().view(np.uint32)
        for v in range(2):
            o = oracle_view("scene4-orbit", sc, (0, 50)[v], cams[v], w, h)
            assert np.array_equal(got[v * h * w:(v + 1) * h * w].reshape(h, w), o["xrgb"])
        assert bool((got[2 * h * w:] == SENTINEL).all())
    finally:
        r.close()


def test_late_switch_and_tiering(torch_cuda, scenes):
    """The switch set after the upload: batches run on render_interp_batch, same pixels.  The switch on, one batch before
    specialize_wait() and one after: same pixels from whichever kernel was there."""
    sc = scenes["scene4"]
    w, h = 61, 37
    cams = thirteen_cameras(sc)
    idx = [0, 6, 4, 12]
    batch = [cams[i] for i in idx]
    # (a) late: the module has no batch kernel
    r = gpu.Renderer(0)
    r.prepare(sc)
    try:
        assert not r.view_batches
        r.set_view_batches(True)
        assert r.view_batches
        b = render_batch(torch_cuda, r, batch, w, h)
        for v, i in enumerate(idx):
            assert_view_is_oracle(b, v, oracle_view("scene4", sc, i, cams[i], w, h), f"late switch, view {v}")
        assert r.kernel_name() == "lol_render_spec"          # frames are what they were
    finally:
        r.close()
    # (b) tiering: before the scene kernel is there, and after
    r = gpu.Renderer(0)
    r.set_view_batches(True)
    r.prepare(sc, wait=False)
    try:
        b0 = render_batch(torch_cuda, r, batch, w, h)
        r.specialize_wait()
        assert r.kernel_name() == "lol_render_spec", r.specialize_log()
        b1 = render_batch(torch_cuda, r, batch, w, h)
        for v, i in enumerate(idx):
            o = oracle_view("scene4", sc, i, cams[i], w, h)
            assert_view_is_oracle(b0, v, o, f"before the scene kernel, view {v}")
            assert_view_is_oracle(b1, v, o, f"on the scene kernel, view {v}")
            assert np.array_equal(b0["steps"][v], b1["steps"][v])
    finally:
        r.close()
