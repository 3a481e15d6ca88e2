"""Adaptive supersampling on the GPU (lol_gpu_set_adaptive_samples): every packed pixel and every lol_gpu_debug.rgb float of an
adaptive frame equals the CPU restatement of the contract (tests/adaptive_reference.py: the oracle's plain frame, the mask of its
ids and 8-bit channels, aa_reference's s x s pixel where it is set) — on the interpreter and on the scene's own kernel, through
every way a frame leaves the library.  And what adaptive frames must refuse or leave alone."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import aa_reference as A
import adaptive_reference as R
import oracle_lib as O
from loltracer_amd import gpu

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -3, -5             # include/lol_gpu.h
SENTINEL = 0x55AA55
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 32 bits per pixel that drop low bits of every channel: the mask must read the channels before the format's loss
LOSSY = gpu.PixelFormat(16, 8, 0, 2, 1, 3, 4, 0, 0xFF000000)


def _host_has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return False


# glibc picks its FMA build of powf on x86-64 CPUs with FMA; that is the variant the device code restates (test_gpu_parity.py)
HOST_LIBM_IS_FMA_VARIANT = _host_has_fma()

_full, _adaptive = {}, {}


def full_reference(sc, key, w, h, s, fmt=None):
    k = (key, w, h, s, None if fmt is None else bytes(fmt))
    if k not in _full:
        _full[k] = A.render(sc, w, h, s, fmt=fmt)
    return _full[k]


def reference(sc, key, w, h, s, T, fmt=None):
    """(packed, rgb, mask) of the adaptive frame"""
    k = (key, w, h, s, T, None if fmt is None else bytes(fmt))
    if k not in _adaptive:
        _adaptive[k] = R.render(sc, w, h, s, T, fmt=fmt, full=full_reference(sc, key, w, h, s, fmt))
    return _adaptive[k]


def assert_equal_to_reference(xrgb, rgb, want_x, want_rgb):
    if HOST_LIBM_IS_FMA_VARIANT:
        assert np.array_equal(xrgb, want_x), f"{int((xrgb != want_x).sum())} packed pixels differ"
        if rgb is not None:
            assert np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)), "colours after gamma are not bit-identical"
    else:                                     # (another host libm's powf may move a channel by one step: test_gpu_parity.py)
        d = np.abs(((xrgb[..., None] >> np.array([16, 8, 0], dtype=np.uint32)) & 0xFF).astype(np.int32)
                   - ((want_x[..., None] >> np.array([16, 8, 0], dtype=np.uint32)) & 0xFF).astype(np.int32))
        assert d.max() <= 1
        if rgb is not None:
            assert np.abs(rgb - want_rgb).max() <= 1e-4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module", params=[1, 4], ids=["spec", "interp"])
def renderer(torch_cuda, request):
    """the scene's own kernel (samples set before the upload: its module carries lol_render_spec_aa_list) and the interpreter"""
    r = gpu.Renderer(0, specialize=request.param)
    r.want_kernel = "lol_render_spec_aa_list" if request.param == 1 else "render_interp_aa_list"
    yield r
    r.close()


def render_adaptive(torch, r, sc, w, h, s, T, rows=None, pitch_px=None, want_rgb=True, prepare=True, max_steps=256):
    if prepare:
        r.set_samples(s)
        r.set_adaptive_samples(T)
        r.prepare(sc)
    assert r.samples == s and r.adaptive_samples == T
    pitch_px = pitch_px or w
    frame = torch.full((h, pitch_px), SENTINEL, dtype=torch.int32, device="cuda:0")
    rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0") if want_rgb else None
    dbg = gpu.Debug(rgb.data_ptr(), None, None, None) if want_rgb else None
    torch.cuda.synchronize()
    r.render_into(frame.data_ptr(), w, h, max_steps, rows=rows, pitch_bytes=pitch_px * 4, debug=dbg,
                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x = frame.cpu().numpy().view(np.uint32)
    assert (x[:, w:] == SENTINEL).all(), "written beyond the row"
    return x[:, :w], (rgb.cpu().numpy() if want_rgb else None)


def assert_inputs_tell_the_feature_apart(sc, key, w, h, s, want_x, m):
    """T = 16: 'never refine' and 'always refine' must both fail on this input (the issue's conditions, on the reference alone)"""
    plain_x, _, _ = O.render(sc, w, h)
    full_x, _ = full_reference(sc, key, w, h, s)
    share, vs_plain, vs_full = float(m.mean()), int((want_x != plain_x).sum()), int((want_x != full_x).sum())
    print(f"{key} {w}x{h} s={s}: refined share {share:.3f}, {vs_plain} pixels differ from P, {vs_full} from the full frame")
    assert 0.02 <= share <= 0.90
    assert vs_plain >= 10
    assert vs_full >= 10


@pytest.mark.parametrize("T", [0, 16, 255])
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("w,h", [(61, 37), (97, 53)])
@pytest.mark.parametrize("name", ["scene", "scene2", "scene3", "scene4"])
def test_frame_equals_the_reference(torch_cuda, renderer, scenes, name, w, h, s, T):
    sc = scenes[name]
    want_x, want_rgb, m = reference(sc, name, w, h, s, T)
    if T == 16:
        assert_inputs_tell_the_feature_apart(sc, name, w, h, s, want_x, m)
    x, rgb = render_adaptive(torch_cuda, renderer, sc, w, h, s, T)
    assert renderer.kernel_name() == renderer.want_kernel, renderer.specialize_log()
    assert renderer.adaptive_refined() == int(m.sum())
    assert_equal_to_reference(x, rgb, want_x, want_rgb)


@pytest.mark.parametrize("fmt", ["argb8888", "lossy"])
def test_pixel_formats(torch_cuda, renderer, scenes, fmt):
    sc = scenes["scene4"]
    f = LOSSY if fmt == "lossy" else gpu.PIXEL_FORMATS[fmt]
    renderer.set_pixel_format(f)
    try:
        x, rgb = render_adaptive(torch_cuda, renderer, sc, 61, 37, 2, 16)
    finally:
        renderer.set_pixel_format(None)
    want_x, want_rgb, _ = reference(sc, "scene4", 61, 37, 2, 16, fmt=f)
    assert_equal_to_reference(x, rgb, want_x, want_rgb)


def test_render_host_with_a_padded_pitch(torch_cuda, scenes):
    sc = scenes["scene4"]
    w, h, s, T, pad = 61, 37, 4, 16, 7
    r = gpu.Renderer(0)
    r.set_samples(s)
    r.set_adaptive_samples(T)
    r.prepare(sc)
    surf = np.full((h, w + pad), SENTINEL, dtype=np.uint32)
    r.render_host(surf.ctypes.data, w, h, pitch_bytes=(w + pad) * 4)
    assert r.kernel_name() == "lol_render_spec_aa_list"
    r.close()
    assert (surf[:, w:] == SENTINEL).all()
    want_x, _, _ = reference(sc, "scene4", w, h, s, T)
    assert_equal_to_reference(surf[:, :w], None, want_x, None)


def test_frames_in_flight_keep_their_setting(torch_cuda, scenes):
    """render_host_begin / _end, two frames in flight, the contrast changed between the begins: each frame has its own"""
    sc = scenes["scene3"]
    w, h, s = 61, 37, 2
    r = gpu.Renderer(0)
    r.set_samples(s)
    r.set_adaptive_samples(16)
    r.prepare(sc)
    r.render_host_begin(w, h)
    r.set_adaptive_samples(255)
    r.render_host_begin(w, h)
    r.set_adaptive_samples(-1)                # (after both begins: changes neither)
    assert r.render_host_pending() == 2
    out = []
    for _ in range(2):
        surf = np.zeros((h, w), dtype=np.uint32)
        r.render_host_end(surf.ctypes.data, w * 4, w, h)
        out.append(surf)
    r.close()
    assert_equal_to_reference(out[0], None, reference(sc, "scene3", w, h, s, 16)[0], None)
    assert_equal_to_reference(out[1], None, reference(sc, "scene3", w, h, s, 255)[0], None)


def test_four_frames_in_flight_on_the_library_streams(torch_cuda, scenes):
    """four streams, four scratch sets reused in turn: eight frames of alternating contrast, each checked"""
    torch = torch_cuda
    sc = scenes["scene2"]
    w, h, s = 61, 37, 2
    r = gpu.Renderer(0)
    r.set_frames_in_flight(4)
    r.set_samples(s)
    r.set_adaptive_samples(0)
    r.prepare(sc)
    frames = [torch.zeros((h, w), dtype=torch.int32, device="cuda:0") for _ in range(8)]
    torch.cuda.synchronize()
    for i, f in enumerate(frames):
        r.set_adaptive_samples((0, 16, 255)[i % 3])
        r.render_into(f.data_ptr(), w, h)
    r.sync()
    r.close()
    for i, f in enumerate(frames):
        assert_equal_to_reference(f.cpu().numpy().view(np.uint32), None, reference(sc, "scene2", w, h, s, (0, 16, 255)[i % 3])[0], None)


def test_adaptive_set_after_the_upload_renders_on_the_interpreter(torch_cuda, scenes):
    sc = scenes["scene4"]
    r = gpu.Renderer(0)
    r.prepare(sc)
    assert r.kernel_name() == "lol_render_spec"
    r.set_samples(2)
    r.set_adaptive_samples(16)
    assert r.kernel_name() == "render_interp_aa_list"
    x, rgb = render_adaptive(torch_cuda, r, sc, 61, 37, 2, 16, prepare=False)
    want_x, want_rgb, m = reference(sc, "scene4", 61, 37, 2, 16)
    assert r.adaptive_refined() == int(m.sum())
    assert_equal_to_reference(x, rgb, want_x, want_rgb)
    r.set_adaptive_samples(-1)
    assert r.kernel_name() == "render_interp_aa"
    r.close()


def test_one_sample_per_pixel_is_the_plain_frame(torch_cuda, scenes):
    sc = scenes["scene"]
    w, h = 61, 37
    r = gpu.Renderer(0)
    r.set_adaptive_samples(0)
    r.prepare(sc)
    x, rgb = render_adaptive(torch_cuda, r, sc, w, h, 1, 0, prepare=False)
    assert r.kernel_name() == "lol_render_spec"
    r.close()
    want_x, want_rgb, _ = O.render(sc, w, h, want_rgb=True)
    assert_equal_to_reference(x, rgb, want_x, want_rgb)


def test_plain_frames_after_adaptive_ones(torch_cuda, scenes):
    """longest-first scheduling goes on under a still camera as if the adaptive frames had not been there"""
    torch = torch_cuda
    sc = scenes["scene4"]
    w, h = 200, 120
    r = gpu.Renderer(0)
    r.set_samples(2)
    r.prepare(sc)
    frame = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(3):
        r.set_samples(1)
        r.render_into(frame.data_ptr(), w, h)
    r.sync()
    before = r.tile_order()["decisions"]
    r.set_adaptive_samples(16)
    for _ in range(3):
        r.set_samples(2)
        r.render_into(frame.data_ptr(), w, h)
    r.sync()
    assert r.tile_order()["decisions"] == before
    r.set_samples(1)
    for _ in range(3):
        r.render_into(frame.data_ptr(), w, h)
    r.sync()
    info = r.tile_order()
    assert info["order"] == "lpt" and info["decisions"] > before, info
    got = frame.cpu().numpy().view(np.uint32)
    r.close()
    want, _, _ = O.render(sc, w, h, threads=4)
    assert_equal_to_reference(got, None, want, None)


def test_refusals_write_nothing(torch_cuda, scenes):
    """partitioned frames, hit_dist / hit_id / steps, and bad contrasts are refused; nothing is written"""
    torch = torch_cuda
    sc = scenes["scene4"]
    w, h = 32, 16
    r = gpu.Renderer(0)
    r.set_samples(2)
    r.set_adaptive_samples(16)
    r.prepare(sc)
    frame = torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda:0")
    f32 = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda:0")
    u32 = torch.full((h, w), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for rows in (gpu.Rows.equal(4, 2, 0), gpu.Rows.equal(4, 2, 1), gpu.Rows(8, 16, 0)):
        with pytest.raises(gpu.GpuError) as e:
            r.render_into(frame.data_ptr(), w, h, rows=rows)
        assert e.value.status == ERR_UNSUPPORTED
    for dbg in (gpu.Debug(None, None, u32.data_ptr(), None), gpu.Debug(None, None, None, u32.data_ptr()),
                gpu.Debug(None, f32.data_ptr(), None, None)):
        with pytest.raises(gpu.GpuError) as e:
            r.render_into(frame.data_ptr(), w, h, debug=dbg)
        assert e.value.status == ERR_UNSUPPORTED
    r.sync()
    assert (frame.cpu().numpy() == SENTINEL).all() and (u32.cpu().numpy() == 7).all() and (f32.cpu().numpy() == 7.0).all()
    for bad in (-2, 256, 1000, -100):
        with pytest.raises(gpu.GpuError) as e:
            r.set_adaptive_samples(bad)
        assert e.value.status == ERR_ARG
        assert r.adaptive_samples == 16
    r.set_adaptive_samples(-1)
    assert r.adaptive_samples == -1
    r.close()
    fresh = gpu.Renderer(0)
    with pytest.raises(gpu.GpuError) as e:
        fresh.adaptive_refined()                        # no adaptive frame yet
    assert e.value.status == ERR_ARG
    fresh.close()


def _headless(args, timeout=180):
    host = os.path.join(os.path.dirname(gpu.__file__), "lib", "lol_headless")
    return subprocess.run([host] + args, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("flags", [[], ["--pipeline"], ["--tile-columns"]])
def test_c_host_adaptive_flag(tmp_path, scenes, flags):
    """hip_renderer.c's --adaptive T through lol_headless (render_thread as main.c calls it, its padded surface pitch)"""
    scene = os.path.join(ROOT, "tests", "golden", "scenes", "scene4.lol")
    w, h, prefix = 61, 37, str(tmp_path / "f")
    p = _headless(["2", scene, "--size", f"{w}x{h}", "--frames", "2", "--samples", "2", "--adaptive", "16",
                   "--dump-frames", prefix] + flags)
    assert p.returncode == 0 and "hip_renderer" not in p.stderr, p.stderr
    want_x, _, _ = reference(scenes["scene4"], "scene4", w, h, 2, 16)
    for i in range(2):
        data = open(f"{prefix}{i:04d}.raw", "rb").read()
        assert data[:4] == b"LOLF" and struct.unpack("<ii", data[4:12]) == (w, h)
        assert_equal_to_reference(np.frombuffer(data[12:], dtype=np.uint32).reshape(h, w), None, want_x, None)


def test_c_host_refuses_adaptive_with_devices(tmp_path):
    scene = os.path.join(ROOT, "tests", "golden", "scenes", "scene4.lol")
    p = _headless(["2", scene, "--size", "61x37", "--frames", "1", "--samples", "2", "--adaptive", "16", "--devices", "0",
                   "--dump-frames", str(tmp_path / "f")])
    assert "--adaptive is refused with --devices" in p.stderr, p.stderr


def test_python_cli_adaptive_flag(tmp_path, scenes):
    out = str(tmp_path / "f.ppm")
    w, h = 61, 37
    p = subprocess.run([sys.executable, "-m", "loltracer_amd", os.path.join(ROOT, "tests", "golden", "scenes", "scene4.lol"),
                        "--size", f"{w}x{h}", "--samples", "4", "--adaptive", "16", "-o", out],
                       capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    assert "lol_render_spec_aa_list" in p.stdout
    data = open(out, "rb").read()
    header = b"P6\n%d %d\n255\n" % (w, h)
    assert data.startswith(header)
    rgb = np.frombuffer(data[len(header):], dtype=np.uint8).reshape(h, w, 3).astype(np.uint32)
    got = rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2]
    assert_equal_to_reference(got, None, reference(scenes["scene4"], "scene4", w, h, 4, 16)[0], None)


def test_full_size_frame_on_sampled_rows(torch_cuda, scenes):
    sc = scenes["scene4"]
    w, h, s, T = 1920, 1080, 2, 16
    r = gpu.Renderer(0)
    x, rgb = render_adaptive(torch_cuda, r, sc, w, h, s, T)
    assert r.kernel_name() == "lol_render_spec_aa_list"
    n = r.adaptive_refined()
    r.close()
    assert 0 < n < w * h
    rows = [0, 1, 333, 539, 540, 1078, 1079]
    want_x, want_rgb, m = R.render(sc, w, h, s, T, rows=rows)
    assert m.any() and (~m).any()
    assert_equal_to_reference(x[rows], rgb[rows], want_x, want_rgb)
