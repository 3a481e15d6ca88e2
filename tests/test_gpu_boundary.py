"""The boundary the reference's host sees: surf->pixels is HOST memory of whatever size and pixel
format the window has this frame (main.c:157,182-187; renderer.h:17-22).

  - colorf_to_pixfmt maps through the SURFACE's format: the kernel's pack equals SDL_MapRGB's definition, computed
    here in numpy from the float colours, for XRGB / ARGB / BGRX / RGBA / ABGR; palettised and 16-bit are refused;
  - the surface is never registered with the device: it may be freed and mapped again at the same address;
  - the surface may change size between frames, with frames in flight: nothing is ever written beyond a surface;
  - a rejected scene upload leaves the previous scene rendering.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from loltracer_amd import gpu, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "loltracer_amd", "lib", "lol_headless")
SCENE4 = os.path.join(ROOT, "tests", "golden", "scenes", "scene4.lol")
SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "scene.lol")


def sdl_map_rgb(rgb: np.ndarray, f: gpu.PixelFormat) -> np.ndarray:
    """colorf_to_pixfmt (renderer.h:17-22): Uint8 channel = colorf * 255 (float multiply, truncation), then
    SDL_MapRGB for a non-palettised format: (r >> Rloss) << Rshift | (g >> Gloss) << Gshift | (b >> Bloss) << Bshift | Amask."""
    ch = (rgb.astype(np.float32) * np.float32(255.0)).astype(np.uint32) & 0xFF
    r, g, b = ch[..., 0], ch[..., 1], ch[..., 2]
    return ((r >> f.r_loss) << f.r_shift | (g >> f.g_loss) << f.g_shift | (b >> f.b_loss) << f.b_shift | f.a_mask).astype(np.uint32)


def test_pixel_format_struct_matches_the_header():
    assert C.sizeof(gpu.PixelFormat) == 12 and C.sizeof(gpu.Rows) == 12


def test_oracle_packs_through_the_surface_format(scenes):
    """The checker's own pack against SDL_MapRGB's definition (CPU only)."""
    sc = scenes["scene4"]
    try:
        for name in ("xrgb8888", "argb8888", "bgrx8888", "rgba8888", "abgr8888"):
            f = gpu.PIXEL_FORMATS[name]
            O.set_pixel_format(f)
            px, rgb, _ = O.render_rows(sc, 48, 32, 0, 32)
            assert np.array_equal(px, sdl_map_rgb(rgb, f)), name
    finally:
        O.set_pixel_format(None)
    px, rgb, _ = O.render_rows(sc, 48, 32, 0, 32)
    ch = (rgb * np.float32(255)).astype(np.uint32)
    assert np.array_equal(px, ch[..., 0] << 16 | ch[..., 1] << 8 | ch[..., 2])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.gpu
@pytest.mark.parametrize("specialize", [1, 0])
def test_device_packs_like_sdl_map_rgb(torch_cuda, scenes, specialize):
    torch = torch_cuda
    w, h = 96, 64
    for scene_name in ("scene4", "scene"):
        sc = scenes[scene_name]
        r = gpu.Renderer(0, specialize=specialize)
        r.prepare(sc)
        _, orgb, _ = O.render_rows(sc, w, h, 0, h)
        for name in ("xrgb8888", "argb8888", "bgrx8888", "rgba8888", "abgr8888"):
            f = gpu.PIXEL_FORMATS[name]
            r.set_pixel_format(name)
            frame = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()                 # torch's fills run on ITS stream; the frame on the renderer's own
            r.render_into(frame.data_ptr(), w, h, debug=gpu.Debug(rgb.data_ptr(), None, None, None))
            r.sync()
            got = frame.cpu().numpy().view(np.uint32)
            # integer-exact against the definition applied to the device's own float colours ...
            assert np.array_equal(got, sdl_map_rgb(rgb.cpu().numpy(), f)), (scene_name, name)
            # ... and against the oracle packing through the same format
            O.set_pixel_format(f)
            try:
                want, _, _ = O.render_rows(sc, w, h, 0, h)
            finally:
                O.set_pixel_format(None)
            assert np.array_equal(got, want), (scene_name, name)
            if f.a_mask:
                assert np.all(got & f.a_mask == f.a_mask)
        # formats the reference's Uint32 store cannot express are refused, loudly, and change nothing
        for bad in ("rgb565", "index8"):
            with pytest.raises(gpu.GpuError) as e:
                r.set_pixel_format(bad)
            assert e.value.status == -5
        frame = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.render_into(frame.data_ptr(), w, h)
        r.sync()
        assert np.array_equal(frame.cpu().numpy().view(np.uint32), want)         # still ABGR, the last accepted format
        r.set_pixel_format(None)
        r.close()


@pytest.mark.gpu
def test_host_surface_pitches_and_padding(torch_cuda, scenes):
    """lol_gpu_render_host: odd sizes, padded and unaligned pitches; padding untouched; one context, sizes going up and down."""
    sc = scenes["scene4"]
    r = gpu.Renderer(0)
    r.prepare(sc)
    for (w, h, pitch) in ((200, 120, 203 * 4), (97, 61, 97 * 4), (640, 360, 700 * 4), (33, 7, 33 * 4 + 2), (320, 517, 320 * 4),
                          (1280, 720, 1280 * 4 + 6), (64, 40, 256)):
        want, _, _ = O.render(sc, w, h, threads=4)
        buf = np.full(h * pitch + 64, 0xA5, dtype=np.uint8)
        r.render_host(buf.ctypes.data, w, h, pitch_bytes=pitch)
        rows = np.stack([buf[y * pitch:y * pitch + w * 4].view(np.uint32) for y in range(h)])
        assert np.array_equal(rows, want), (w, h)
        for y in range(h):                                   # row padding and the tail are untouched
            assert np.all(buf[y * pitch + w * 4:(y + 1) * pitch] == 0xA5)
        assert np.all(buf[h * pitch:] == 0xA5)
    r.close()


REMAP_SCRIPT = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import oracle_lib as O
from loltracer_amd import gpu, scene as S
libc = C.CDLL(None, use_errno=True)
libc.mmap.restype = C.c_void_p
libc.mmap.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_long]
libc.munmap.argtypes = [C.c_void_p, C.c_size_t]
PROT_RW, MAP_PRIVATE, MAP_ANON, MAP_FIXED_NOREPLACE = 3, 2, 0x20, 0x100000
sc = S.Scene.parse_file({scene!r})
r = gpu.Renderer(0)
r.prepare(sc)
w, h = 512, 256
size = w * h * 4
addr = libc.mmap(None, size, PROT_RW, MAP_PRIVATE | MAP_ANON, -1, 0)
for (ww, hh) in ((w, h), (w, h), (w // 2, h // 2), (w, h)):
    r.render_host(addr, ww, hh, pitch_bytes=ww * 4)
    got = np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint32)), shape=(hh * ww,)).reshape(hh, ww).copy()
    assert np.array_equal(got, O.render(sc, ww, hh, threads=4)[0]), (ww, hh)
    assert libc.munmap(addr, size) == 0                      # the host drops the surface ...
    again = libc.mmap(addr, size, PROT_RW, MAP_PRIVATE | MAP_ANON | MAP_FIXED_NOREPLACE, -1, 0)
    assert again == addr, "could not map the same address again"      # ... and gets fresh zero pages at the same address
    assert not np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint32)), shape=(h * w,)).any()
r.close()
print("remap ok")
"""


@pytest.mark.gpu
def test_surface_freed_and_mapped_again_at_the_same_address(tmp_path):
    """SDL frees the window surface on a resize and allocates a new one (main.c:182); the allocator may hand out the
    SAME address for new pages.  The library remembers nothing about the surface between frames and never registers it
    with the device, so the new pages get the frame: map, render, unmap, map again at that very address, render, for a
    same-size and a smaller surface.  (Round 3 first pinned surfaces by address and had the kernel store into them: this
    very case aborted the process, which is why that route is gone — lol_gpu.hip, lol_gpu_render_host.)  Runs in a process
    of its own."""
    import sys
    p = subprocess.run([sys.executable, "-c", REMAP_SCRIPT.format(root=ROOT, scene=SCENE4)], capture_output=True, text=True, timeout=180)
    assert p.returncode == 0 and "remap ok" in p.stdout, p.stderr[-2000:]


@pytest.mark.gpu
def test_frames_in_flight_survive_a_resize(torch_cuda, scenes):
    """a frame queued at one size must never be copied into a surface of another size."""
    sc = scenes["scene4"]
    r = gpu.Renderer(0)
    r.prepare(sc)
    sizes = [(200, 120), (96, 54), (320, 200), (320, 200), (64, 40)]
    want = {s: O.render(sc, s[0], s[1], threads=4)[0] for s in set(sizes)}
    # two frames of DIFFERENT sizes in flight, each ended into a surface of its own size
    r.render_host_begin(*sizes[0])
    for i in range(len(sizes)):
        if i + 1 < len(sizes):
            r.render_host_begin(*sizes[i + 1])
        w, h = sizes[i]
        assert r.render_host_pending_size() == (w, h)
        # a surface of the NEXT size is refused and stays untouched, the frame stays queued
        other = sizes[(i + 1) % len(sizes)]
        if other != (w, h):
            guard = np.full((other[1], other[0]), 0x5A5A5A5A, dtype=np.uint32)
            pending = r.render_host_pending()
            with pytest.raises(gpu.GpuError):
                r.render_host_end(guard.ctypes.data, other[0] * 4, other[0], other[1])
            assert np.all(guard == 0x5A5A5A5A) and r.render_host_pending() == pending
        surf = np.zeros((h, w), dtype=np.uint32)
        r.render_host_end(surf.ctypes.data, w * 4, w, h)
        assert np.array_equal(surf, want[(w, h)]), sizes[i]
    assert r.render_host_pending() == 0 and r.render_host_pending_size() == (0, 0)
    # discard drops what is queued; the pipeline works again afterwards
    r.render_host_begin(200, 120); r.render_host_begin(96, 54)
    r.render_host_discard()
    assert r.render_host_pending() == 0
    r.render_host_begin(64, 40)
    surf = np.zeros((40, 64), dtype=np.uint32)
    r.render_host_end(surf.ctypes.data, 256, 64, 40)
    assert np.array_equal(surf, want[(64, 40)])
    r.close()


def read_frames(prefix, n):
    out = []
    for i in range(n):
        data = open(f"{prefix}{i:04d}.raw", "rb").read()
        assert data[:4] == b"LOLF"
        w, h = struct.unpack("<ii", data[4:12])
        out.append(np.frombuffer(data[12:], dtype=np.uint32).reshape(h, w))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--pipeline"], ["--devices", "0", "--parts-per-device", "3"], ["--pipeline", "--tile-columns"],
                                   ["--pipeline-depth", "3"], ["--pipeline-depth", "4"]])
def test_c_host_resizes_between_frames(tmp_path, scenes, flags):
    """main.c:182-187 through render_thread: grow, shrink, grow again on ONE context; every surface the host sees equals
    the oracle's frame of that size (static camera, so the pipelined mode's one-frame lag shows the same picture)."""
    script = "320x180,320x180,1280x720,97x61,97x61,640x480,33x7,320x180"
    sizes = [tuple(int(v) for v in s.split("x")) for s in script.split(",")]
    prefix = str(tmp_path / "f")
    p = subprocess.run([HOST, "3", SCENE4, "--resize-script", script, "--dump-frames", prefix] + flags,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "hip_renderer" not in p.stderr, p.stderr
    n = len(sizes) + (1 if "--pipeline" in flags else 0) + (int(flags[1]) - 1 if flags[:1] == ["--pipeline-depth"] else 0)
    frames = read_frames(prefix, n)
    want = {s: O.render(scenes["scene4"], s[0], s[1], threads=4)[0] for s in set(sizes)}
    for i, f in enumerate(frames):
        s = sizes[min(i, len(sizes) - 1)]
        assert f.shape == (s[1], s[0])
        assert np.array_equal(f, want[s]), (i, s, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["argb8888", "bgrx8888", "rgba8888", "abgr8888"])
def test_c_host_honours_the_surface_format(tmp_path, scenes, name):
    prefix = str(tmp_path / "f")
    w, h = 160, 90
    p = subprocess.run([HOST, "2", SCENE4, "--size", f"{w}x{h}", "--format", name, "--dump-frames", prefix],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "hip_renderer" not in p.stderr, p.stderr
    _, rgb, _ = O.render_rows(scenes["scene4"], w, h, 0, h)
    assert np.array_equal(read_frames(prefix, 1)[0], sdl_map_rgb(rgb, gpu.PIXEL_FORMATS[name]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rgb565", "index8"])
def test_c_host_refuses_other_surface_formats(tmp_path, name):
    prefix = str(tmp_path / "f")
    p = subprocess.run([HOST, "2", SCENE4, "--size", "64x36", "--frames", "2", "--format", name, "--dump-frames", prefix],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0
    assert p.stderr.count("hip_renderer:") == 1 and "supported" in p.stderr      # reported once, not per frame
    assert not np.any(read_frames(prefix, 2)[1])                                  # nothing was written


@pytest.mark.gpu
@pytest.mark.parametrize("specialize", [1, 0])
def test_rejected_upload_leaves_the_previous_scene_rendering(torch_cuda, scenes, specialize, monkeypatch):
    """lol_gpu_upload_program is all-or-nothing."""
    torch = torch_cuda
    w, h = 128, 72
    a, b = scenes["scene4"], scenes["scene"]
    want_a, want_b = O.render(a, w, h, threads=4)[0], O.render(b, w, h, threads=4)[0]
    r = gpu.Renderer(0, specialize=specialize)
    r.prepare(a)

    def frame():
        t = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.render_into(t.data_ptr(), w, h, camera=cam)
        r.sync()
        return t.cpu().numpy().view(np.uint32)
    cam = a.c.camera
    assert np.array_equal(frame(), want_a)
    # 1. malformed programs (stack underflow, bad material index, too many ops)
    for breaker in ("smin", "material", "n_ops"):
        bad = b.flatten()
        if breaker == "smin":
            bad.ops[0].op = S.OP_SMIN
        elif breaker == "material":
            bad.root_material[0] = 9999
        else:
            bad.n_ops = S.LOL_MAX_OPS + 1              # beyond the sanity cap: taken for corruption (the table is not read)
        with pytest.raises(gpu.GpuError):
            r._check(r._lib.lol_gpu_upload_program(r._ctx, C.byref(bad)))
        assert np.array_equal(frame(), want_a), breaker
    # 2. a device-side failure in the middle of the upload (injected)
    r.testing_fail_uploads(1)                                      # include/lol_gpu_testing.h
    with pytest.raises(gpu.GpuError):
        r._check(r._lib.lol_gpu_upload_program(r._ctx, C.byref(b.flatten())))
    assert np.array_equal(frame(), want_a)
    assert r.kernel_name() == ("lol_render_spec" if specialize else "render_interp")
    # 3. a good upload switches over
    r.prepare(b)
    cam = b.c.camera
    assert np.array_equal(frame(), want_b)
    r.close()


@pytest.mark.gpu
def test_kernel_key_names_the_code(torch_cuda, scenes, tmp_path):
    r = gpu.Renderer(0)
    r.prepare(scenes["scene4"])
    k4 = r.kernel_key()
    r.prepare(scenes["scene"])
    k1 = r.kernel_key()
    r.prepare(scenes["scene4"])
    assert len(k4) == 16 and k4 != k1 and r.kernel_key() == k4
    ri = gpu.Renderer(0, specialize=0)
    ri.prepare(scenes["scene4"])
    i4 = ri.kernel_key()
    assert len(i4) == 16 and i4 != k4
    # the interpreter's key names this build AND the uploaded macro-op lists (what render_interp executes depends on both)
    ri.prepare(scenes["scene"])
    assert ri.kernel_key() != i4
    ri.prepare(scenes["scene4"])
    assert ri.kernel_key() == i4
    rf = gpu.Renderer(0, specialize=4)                   # interpreter + proven fast paths: other records, other key
    rf.prepare(scenes["scene4"])
    assert rf.kernel_name() == "render_interp" and rf.kernel_key() != i4
    # a scene kernel's key is gpu.code_key of its code object — what the device loads of it: a context without the proven shortcuts
    # (which need a device to prove them) runs the module compile_offline makes in this process
    rp = gpu.Renderer(0, specialize=3)
    rp.prepare(scenes["scene4"])
    base = str(tmp_path / "scene4")
    gpu.compile_offline(scenes["scene4"].flatten(), base)
    with open(base + ".co", "rb") as f:
        assert rp.kernel_name() == "lol_render_spec" and rp.kernel_key() == gpu.code_key(f.read()) != k4
    r.close(); ri.close(); rf.close(); rp.close()


ROCTX_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
import numpy as np
from loltracer_amd import gpu, scene as S
lib = gpu.gpu_lib()
before = lib.lol_gpu_roctx_ranges()
r = gpu.Renderer(0)
r.prepare(S.Scene.parse_file({scene!r}))
buf = np.zeros((36, 64), dtype=np.uint32)
for _ in range(3):
    r.render_host(buf.ctypes.data, 64, 36)
print("ranges", before, lib.lol_gpu_roctx_ranges(), int(buf.any()))
"""


@pytest.mark.gpu
def test_roctx_ranges_mark_every_frame_when_asked_for():
    """LOL_GPU_ROCTX=1 (the counterpart of the reference's -j/--jitdump aid): the roctx library resolves and
    every frame launch pushes a range; without the variable nothing is loaded and nothing is pushed."""
    import sys
    for env_value, want in (("1", 3), (None, 0)):
        env = {k: v for k, v in os.environ.items() if k != "LOL_GPU_ROCTX"}
        if env_value:
            env["LOL_GPU_ROCTX"] = env_value
        p = subprocess.run([sys.executable, "-c", ROCTX_SCRIPT.format(root=ROOT, scene=SCENE4)], env=env, capture_output=True,
                           text=True, timeout=180)
        assert p.returncode == 0, p.stderr[-2000:]
        assert f"ranges 0 {want} 1" in p.stdout, (p.stdout, p.stderr[-500:])


def _union_tree_scene(depth, seed=11):
    """one object: a balanced smooth-union tree of 2^depth spheres (2^(depth+1) ops) — seconds of hipRTC"""
    rng = np.random.default_rng(seed)

    def tree(d):
        if d == 0:
            return "sphere { point = (%.3f, %.3f, %.3f), radius = %.3f }" % (*(rng.normal(size=3) * [4, 2, 3] + [0, 0, -9]), rng.uniform(0.2, 0.8))
        return "smooth_union { smoothness = 0.5, a = %s, b = %s }" % (tree(d - 1), tree(d - 1))
    return S.Scene.parse_string(
        "materials { { shininess = 2, diffuse = (0,0,0), specular = (0,0,0), ambient = (.02,.02,.02) },"
        " { shininess = 8, diffuse = (.5,.5,.5), specular = (.2,.2,.2), ambient = (.1,.1,.1) } }\n"
        "scene { camera { point = (0, 1, 4), direction = (0, -0.1, -1), fov = 100 },"
        " point_light { point = (0,9,0), diffuse_intensity = (2,2,2), specular_intensity = (2,2,2) }, "
        + tree(depth).replace("{", "{ material = #1,", 1) + " }")


@pytest.mark.gpu
def test_tiered_start_up(torch_cuda, scenes, monkeypatch, tmp_path):
    """render_prepare returns at once (naive_renderer.c:242-244; the JIT's takes milliseconds, tracing_jit_renderer.dasc:416-434):
    lol_gpu_upload_program commits the tables and comes back while hipRTC compiles the scene's kernel on a host thread; frames
    render on the interpreter meanwhile and the first frame after the compiler has finished runs the scene's kernel — the
    same frame, bit for bit.  A 1024-op scene (seconds of hipRTC) with the code-object caches out of the way — a size that gets
    its kernel in two tiers: interpreter -> SDF out of line -> SDF inlined."""
    import time
    torch = torch_cuda
    monkeypatch.setenv("LOL_GPU_CACHE_DIR", "")                  # no disk cache: the compiler really runs
    sc = _union_tree_scene(9, seed=int(time.time()) % 100000)      # (a scene no earlier test of this process has compiled)
    assert sc.flatten().n_ops == 1024
    w, h = 96, 54
    want, _, _ = O.render(sc, w, h, threads=4)
    r = gpu.Renderer(0)
    t0 = time.perf_counter()
    r.prepare(sc, wait=False)
    prepare_ms = (time.perf_counter() - t0) * 1e3
    state, _ = r.specialize_state()
    assert state == 1 and r.kernel_name() == "render_interp"      # compiling; the interpreter is what renders now
    assert prepare_ms < 250, prepare_ms                            # (50 ms is the aim, measured in profiles/r4_startup.json; this bound only catches a blocking compile)
    buf = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    frames_on_interp = 0
    last = None
    deadline = time.perf_counter() + 120
    while r.kernel_name() == "render_interp" and time.perf_counter() < deadline:
        buf.zero_()
        r.render_into(buf.data_ptr(), w, h)
        r.sync()
        if r.kernel_name() == "render_interp":
            frames_on_interp += 1
        last = buf.cpu().numpy().view(np.uint32).copy()
        assert np.array_equal(last, want)
    assert frames_on_interp >= 1, "the compiler finished before a single frame could be rendered?"
    # A scene of this size gets TWO kernels (round 5): the one with the SDF out of line is in use now (hipRTC delivers it 3 - 6
    # times sooner), the one with the SDF inlined — a third faster — is being compiled behind it (state 5; 6 once it waits for
    # the next frame boundary)
    assert r.kernel_name() == "lol_render_spec" and r.specialize_state()[0] in (5, 6) and r.specialize_state()[1] > 100
    key_first = r.kernel_key()
    # `last` was the first frame of the scene's own kernel; the frame before it came from the interpreter: identical (checked above)
    frames_on_first = 0
    deadline = time.perf_counter() + 180
    while r.specialize_state()[0] in (5, 6) and time.perf_counter() < deadline:
        buf.zero_()
        r.render_into(buf.data_ptr(), w, h)
        r.sync()
        frames_on_first += r.kernel_key() == key_first
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), want)
    assert frames_on_first >= 1 and r.specialize_state()[0] == 2 and r.kernel_key() != key_first       # the second kernel took over at a frame boundary
    assert "second tier" in r.specialize_log()
    for _ in range(6):                                    # ... and the repeated view is scheduled afresh on it (its tables are another kernel's)
        buf.zero_()
        r.render_into(buf.data_ptr(), w, h)
        r.sync()
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), want)
    # a second context, same scene: both code objects are in the process's cache, the compiler's threads are done at once
    r2 = gpu.Renderer(0)
    t0 = time.perf_counter()
    r2.prepare(sc, wait=False)
    r2.specialize_wait()
    assert (time.perf_counter() - t0) < 1.0 and r2.kernel_name() == "lol_render_spec" and r2.kernel_key() == r.kernel_key()
    r2.close()
    r.close()


@pytest.mark.gpu
def test_uploads_while_the_scene_compiler_runs(torch_cuda, scenes, monkeypatch):
    """A scene uploaded while the previous one is still being compiled replaces it — its frames at once (interpreter), its own
    kernel later; the abandoned run's result is never used.  A REFUSED upload during a compile leaves scene and compile alone.
    Destroying a context with the compiler at work waits for the thread instead of leaving it behind."""
    import time
    torch = torch_cuda
    monkeypatch.setenv("LOL_GPU_CACHE_DIR", "")
    big = _union_tree_scene(9, seed=int(time.time()) % 100000 + 7)
    small = scenes["scene4"]
    w, h = 64, 36
    want_big, _, _ = O.render(big, w, h, threads=4)
    want_small, _, _ = O.render(small, w, h, threads=4)
    r = gpu.Renderer(0)
    buf = torch.zeros((h, w), dtype=torch.int32, device="cuda")

    def frame(cam):
        buf.zero_()
        r.render_into(buf.data_ptr(), w, h, camera=cam)
        r.sync()
        return buf.cpu().numpy().view(np.uint32)
    r.prepare(big, wait=False)
    assert r.specialize_state()[0] == 1
    assert np.array_equal(frame(big.c.camera), want_big)
    # refused upload (malformed) while compiling: nothing changes
    bad = small.flatten()
    bad.root_material[0] = 9999
    with pytest.raises(gpu.GpuError):
        r._check(r._lib.lol_gpu_upload_program(r._ctx, C.byref(bad)))
    assert r.specialize_state()[0] in (1, 3) and np.array_equal(frame(big.c.camera), want_big)
    # a good upload replaces the scene; the run for `big` is abandoned
    r.prepare(small, wait=False)
    assert np.array_equal(frame(small.c.camera), want_small)
    r.specialize_wait()
    assert r.kernel_name() == "lol_render_spec" and np.array_equal(frame(small.c.camera), want_small)
    key_small = r.kernel_key()
    rs = gpu.Renderer(0)
    rs.prepare(small)
    assert rs.kernel_key() == key_small                        # the kernel in use is scene4's, not the abandoned tree's
    rs.close()
    # close with a compile in flight
    r.prepare(_union_tree_scene(9, seed=int(time.time()) % 100000 + 13), wait=False)
    assert r.specialize_state()[0] == 1
    t0 = time.perf_counter()
    r.close()
    assert time.perf_counter() - t0 < 60
