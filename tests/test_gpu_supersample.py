"""Supersampling on the GPU (lol_gpu_set_samples): every packed pixel and every lol_gpu_debug.rgb float of an s x s frame equals
the CPU restatement of the contract (tests/aa_reference.py: the reference's s w x s h frame, averaged in a fixed order) — on the
interpreter and on the scene's own kernel, at frame sizes that are not multiples of the tile, through every way a frame leaves the
library.  And what supersampling must leave alone: plain frames after it, the longest-first schedule, the diagnostics it cannot
give."""
import numpy as np
import pytest

import aa_reference as A
import oracle_lib as O
from loltracer_amd import gpu, scene as S

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -3, -5             # include/lol_gpu.h
SENTINEL = 0x55AA55


def _host_has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return False


# glibc picks its FMA build of powf on x86-64 CPUs with FMA; that is the variant the device code restates (test_gpu_parity.py)
HOST_LIBM_IS_FMA_VARIANT = _host_has_fma()

_refs = {}


def reference(sc, key, w, h, s, rows=None, fmt=None):
    k = (key, w, h, s, None if rows is None else tuple(rows), None if fmt is None else bytes(fmt))
    if k not in _refs:
        _refs[k] = A.render(sc, w, h, s, rows=rows, fmt=fmt)
    return _refs[k]


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
    """the scene's own kernel (uploaded after set_samples: its module carries lol_render_spec_aa) and the interpreter"""
    r = gpu.Renderer(0, specialize=request.param)
    r.want_kernel = "lol_render_spec_aa" if request.param == 1 else "render_interp_aa"
    yield r
    r.close()


def render_aa(torch, r, sc, w, h, s, rows=None, pitch_px=None, want_rgb=True, prepare=True, max_steps=256):
    if prepare:
        r.set_samples(s)
        r.prepare(sc)
    assert r.samples == s
    n_rows = gpu.part_rows(h, rows)
    pitch_px = pitch_px or w
    frame = torch.full((n_rows, pitch_px), SENTINEL, dtype=torch.int32, device="cuda:0")
    rgb = torch.zeros((n_rows, w, 3), dtype=torch.float32, device="cuda:0") if want_rgb else None
    dbg = gpu.Debug(rgb.data_ptr(), None, None, None) if want_rgb else None
    torch.cuda.synchronize()
    r.render_into(frame.data_ptr(), w, h, max_steps, rows=rows, pitch_bytes=pitch_px * 4, debug=dbg,
                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x = frame.cpu().numpy().view(np.uint32)
    assert (x[:, w:] == SENTINEL).all(), "written beyond the row"
    return x[:, :w], (rgb.cpu().numpy() if want_rgb else None)


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("w,h", [(61, 37), (97, 53)])
@pytest.mark.parametrize("name", ["scene", "scene2", "scene3", "scene4"])
def test_frame_equals_the_reference(torch_cuda, renderer, scenes, name, w, h, s):
    sc = scenes[name]
    x, rgb = render_aa(torch_cuda, renderer, sc, w, h, s)
    assert renderer.kernel_name() == renderer.want_kernel, renderer.specialize_log()
    assert_equal_to_reference(x, rgb, *reference(sc, name, w, h, s))


@pytest.mark.parametrize("fmt", ["argb8888", "bgrx8888"])
def test_pixel_formats(torch_cuda, renderer, scenes, fmt):
    sc = scenes["scene4"]
    f = gpu.PIXEL_FORMATS[fmt]
    renderer.set_pixel_format(fmt)
    try:
        x, rgb = render_aa(torch_cuda, renderer, sc, 61, 37, 2)
    finally:
        renderer.set_pixel_format(None)
    assert_equal_to_reference(x, rgb, *reference(sc, "scene4", 61, 37, 2, fmt=f))


def test_row_partition(torch_cuda, renderer, scenes):
    """three parts with bands of 5 rows, assembled by lol_gpu_part_frame_row: the whole frame"""
    sc = scenes["scene2"]
    w, h, s = 61, 37, 2
    want_x, want_rgb = reference(sc, "scene2", w, h, s)
    renderer.set_samples(s)
    renderer.prepare(sc)
    seen = np.zeros(h, dtype=bool)
    for part in range(3):
        rows = gpu.Rows.equal(5, 3, part)
        x, rgb = render_aa(torch_cuda, renderer, sc, w, h, s, rows=rows, prepare=False)
        lib = gpu.gpu_lib()
        fr = [lib.lol_gpu_part_frame_row(h, rows, i) for i in range(x.shape[0])]
        assert all(0 <= y < h for y in fr)
        seen[fr] = True
        assert_equal_to_reference(x, rgb, want_x[fr], want_rgb[fr])
    assert seen.all()


@pytest.mark.parametrize("order", ["cols", "rows"])
def test_fixed_tile_orders(torch_cuda, renderer, scenes, order):
    """under LOL_GPU_TILES_COLS the sample grid's launch is transposed and store_pixel_aa finds its tile through tile_of_block"""
    sc = scenes["scene"]
    renderer.set_tile_order(order)
    try:
        for s in (2, 4):
            x, rgb = render_aa(torch_cuda, renderer, sc, 97, 53, s)
            assert renderer.kernel_name() == renderer.want_kernel
            assert_equal_to_reference(x, rgb, *reference(sc, "scene", 97, 53, s))
    finally:
        renderer.set_tile_order("lpt")


@pytest.mark.parametrize("flags", [[], ["--pipeline"], ["--devices", "0", "--parts-per-device", "3"], ["--tile-columns"]])
def test_c_host_samples_flag(tmp_path, scenes, flags):
    """hip_renderer.c's --samples N through lol_headless (render_thread as main.c calls it, its padded surface pitch)"""
    import os
    import struct
    import subprocess
    host = os.path.join(os.path.dirname(gpu.__file__), "lib", "lol_headless")
    scene = os.path.join(os.path.dirname(os.path.dirname(gpu.__file__)), "tests", "golden", "scenes", "scene4.lol")
    w, h, prefix = 61, 37, str(tmp_path / "f")
    p = subprocess.run([host, "2", scene, "--size", f"{w}x{h}", "--frames", "2", "--samples", "2", "--dump-frames", prefix] + flags,
                       capture_output=True, text=True, timeout=180)
    assert p.returncode == 0 and "hip_renderer" not in p.stderr, p.stderr
    want = reference(scenes["scene4"], "scene4", w, h, 2)
    for i in range(2):
        data = open(f"{prefix}{i:04d}.raw", "rb").read()
        assert data[:4] == b"LOLF" and struct.unpack("<ii", data[4:12]) == (w, h)
        assert_equal_to_reference(np.frombuffer(data[12:], dtype=np.uint32).reshape(h, w), None, *want)


def test_python_cli_samples_flag(tmp_path, scenes):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(gpu.__file__))
    out = str(tmp_path / "f.ppm")
    w, h = 61, 37
    p = subprocess.run([sys.executable, "-m", "loltracer_amd", os.path.join(root, "tests", "golden", "scenes", "scene4.lol"),
                        "--size", f"{w}x{h}", "--samples", "4", "-o", out], capture_output=True, text=True, timeout=180, cwd=root)
    assert p.returncode == 0, p.stderr
    assert "lol_render_spec_aa" in p.stdout
    data = open(out, "rb").read()
    header = b"P6\n%d %d\n255\n" % (w, h)
    assert data.startswith(header)
    rgb = np.frombuffer(data[len(header):], dtype=np.uint8).reshape(h, w, 3).astype(np.uint32)
    got = rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2]
    assert_equal_to_reference(got, None, *reference(scenes["scene4"], "scene4", w, h, 4))


def test_render_host_with_a_padded_pitch(torch_cuda, scenes):
    sc = scenes["scene4"]
    w, h, s, pad = 61, 37, 4, 7
    r = gpu.Renderer(0)
    r.set_samples(s)
    r.prepare(sc)
    surf = np.full((h, w + pad), SENTINEL, dtype=np.uint32)
    r.render_host(surf.ctypes.data, w, h, pitch_bytes=(w + pad) * 4)
    assert r.kernel_name() == "lol_render_spec_aa"
    r.close()
    assert (surf[:, w:] == SENTINEL).all()
    assert_equal_to_reference(surf[:, :w], None, *reference(sc, "scene4", w, h, s))


def test_frames_in_flight_keep_their_samples(torch_cuda, scenes):
    """render_host_begin / _end, two frames in flight, s changed between the begins: each frame is delivered with its own s"""
    sc = scenes["scene3"]
    w, h = 61, 37
    r = gpu.Renderer(0)
    r.set_samples(2)
    r.prepare(sc)
    r.render_host_begin(w, h)
    r.set_samples(4)
    r.render_host_begin(w, h)
    r.set_samples(1)                          # (after both begins: changes neither)
    assert r.render_host_pending() == 2
    out = []
    for _ in range(2):
        surf = np.zeros((h, w), dtype=np.uint32)
        r.render_host_end(surf.ctypes.data, w * 4, w, h)
        out.append(surf)
    r.close()
    assert_equal_to_reference(out[0], None, *reference(sc, "scene3", w, h, 2))
    assert_equal_to_reference(out[1], None, *reference(sc, "scene3", w, h, 4))


def test_multi_renderer_parts(torch_cuda, scenes):
    """one device, three parts: bands are output rows, the exchange moves pixels as before"""
    sc = scenes["scene4"]
    w, h, s = 97, 53, 2
    m = gpu.MultiRenderer([0])
    m.set_parts_per_device(3)
    m.set_samples(s)
    m.prepare(sc)
    surf = np.zeros((h, w), dtype=np.uint32)
    m.render_host(surf.ctypes.data, w, h)
    dev = torch_cuda.zeros((h, w), dtype=torch_cuda.int32, device="cuda:0")
    m.render_into(dev.data_ptr(), w, h)
    m.sync()
    m.close()
    want = reference(sc, "scene4", w, h, s)
    assert_equal_to_reference(surf, None, *want)
    assert_equal_to_reference(dev.cpu().numpy().view(np.uint32), None, *want)


def _union_tree_scene(depth, seed=3):
    """one object: a balanced smooth-union tree of 2^depth spheres (2^(depth+1) ops)"""
    rng = np.random.default_rng(seed)

    def tree(d):
        if d == 0:
            return "sphere { point = (%.3f, %.3f, %.3f), radius = %.3f }" % (*(rng.normal(size=3) * [3, 1.5, 2] + [0, 0, -8]), rng.uniform(0.3, 0.9))
        return "smooth_union { smoothness = 0.5, a = %s, b = %s }" % (tree(d - 1), tree(d - 1))
    return S.Scene.parse_string(
        "materials { { shininess = 2, diffuse = (0,0,0), specular = (0,0,0), ambient = (.02,.02,.02) },"
        " { shininess = 8, diffuse = (.5,.5,.5), specular = (.2,.2,.2), ambient = (.1,.1,.1) } }\n"
        "scene { camera { point = (0, 1, 4), direction = (0, -0.1, -1), fov = 100 },"
        " point_light { point = (0,9,0), diffuse_intensity = (2,2,2), specular_intensity = (2,2,2) }, "
        + tree(depth).replace("{", "{ material = #1,", 1) + " }")


@pytest.mark.parametrize("specialize,form", [(5, "out of line"), (1, "inlined")])
def test_mid_size_scene_on_both_tiers(torch_cuda, specialize, form):
    """257 ... 1024 ops: the first tier (SDF out of line; specialize 5 keeps it) and the second (SDF inlined) both carry the
    supersampling kernel"""
    sc = _union_tree_scene(8)
    assert 257 <= sc.flatten().n_ops <= 1024
    r = gpu.Renderer(0, specialize=specialize)
    x, rgb = render_aa(torch_cuda, r, sc, 37, 23, 2)
    assert r.kernel_name() == "lol_render_spec_aa", r.specialize_log()
    assert r.specialize_state()[0] == 2
    r.close()
    assert_equal_to_reference(x, rgb, *reference(sc, "tree8", 37, 23, 2))


def _many_tables_scene(seed=9):
    """lights + materials + objects beyond what a block stages in LDS (lol_kernel.h, TABLES_GLOBAL)"""
    rng = np.random.default_rng(seed)
    f3 = lambda v: "(%.3f, %.3f, %.3f)" % tuple(v)
    mats = ["{ shininess = 2, diffuse = (0,0,0), specular = (0,0,0), ambient = (.02,.02,.03) }"]
    mats += ["{ shininess = 8, diffuse = %s, specular = %s, ambient = %s }" % (f3(rng.uniform(.1, .6, 3)), f3(rng.uniform(0, .4, 3)),
                                                                            f3(rng.uniform(0, .3, 3))) for _ in range(39)]
    comps = ["ambient { color = (.1,.1,.1) }", "camera { point = (0, 4, 6), direction = (0, -0.35, -1), fov = 110 }"]
    comps += ["point_light { point = %s, diffuse_intensity = %s, specular_intensity = %s }" % (
        f3(rng.normal(size=3) * [12, 1, 12] + [0, 10, -10]), f3(rng.uniform(.02, .08, 3)), f3(rng.uniform(0, .05, 3))) for _ in range(60)]
    comps.append("plane { material = #1, y = -1 }")
    comps += ["sphere { material = #%d, point = %s, radius = %.3f }" % (1 + i % 39, f3(rng.uniform([-20, -.5, -30], [20, 2, 2])),
                                                                       rng.uniform(.15, .7)) for i in range(99)]
    return S.Scene.parse_string("materials { %s }\nscene { %s }\n" % (",\n".join(mats), ",\n".join(comps)))


@pytest.mark.parametrize("specialize,name", [(1, "lol_render_spec_aa"), (4, "render_interp_aa")])
def test_tables_in_global_memory(torch_cuda, specialize, name):
    sc = _many_tables_scene()
    p = sc.flatten()
    assert p.n_lights * 9 + p.n_materials * 10 + p.n_roots > 1024
    r = gpu.Renderer(0, specialize=specialize)
    x, rgb = render_aa(torch_cuda, r, sc, 29, 19, 2)
    assert r.kernel_name() == name, r.specialize_log()
    r.close()
    assert_equal_to_reference(x, rgb, *reference(sc, "tables", 29, 19, 2))


def test_full_size_frame_on_sampled_rows(torch_cuda, scenes):
    sc = scenes["scene4"]
    w, h, s = 1920, 1080, 2
    r = gpu.Renderer(0)
    x, rgb = render_aa(torch_cuda, r, sc, w, h, s)
    assert r.kernel_name() == "lol_render_spec_aa"
    r.close()
    rows = [0, 1, 333, 539, 540, 1078, 1079]
    assert_equal_to_reference(x[rows], rgb[rows], *reference(sc, "scene4", w, h, s, rows=rows))


def test_samples_set_after_the_upload_render_on_the_interpreter(torch_cuda, scenes):
    """set_samples after prepare(): the next frame is supersampled, by render_interp_aa until the next upload"""
    sc = scenes["scene4"]
    r = gpu.Renderer(0)
    r.prepare(sc)
    assert r.kernel_name() == "lol_render_spec"
    plain_key = r.kernel_key()
    r.set_samples(2)
    assert r.kernel_name() == "render_interp_aa" and r.kernel_key() != plain_key
    x, rgb = render_aa(torch_cuda, r, sc, 61, 37, 2, prepare=False)
    assert_equal_to_reference(x, rgb, *reference(sc, "scene4", 61, 37, 2))
    r.set_samples(1)
    assert r.kernel_name() == "lol_render_spec" and r.kernel_key() == plain_key
    r.close()


def test_plain_frames_after_supersampled_ones(torch_cuda, scenes):
    """s = 1 after s = 2 frames is the oracle's frame, and longest-first scheduling goes on sorting under a still camera as if
    the supersampled frames had not been there"""
    torch = torch_cuda
    sc = scenes["scene4"]
    w, h = 200, 120
    r = gpu.Renderer(0)
    r.set_samples(2)
    r.prepare(sc)
    frame = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()                  # (the fill runs on torch's stream, the frames on the library's own)
    for _ in range(3):
        r.set_samples(1)
        r.render_into(frame.data_ptr(), w, h)
    r.sync()
    before = r.tile_order()["decisions"]
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
    assert r.kernel_name() == "lol_render_spec"
    got = frame.cpu().numpy().view(np.uint32)
    r.close()
    want, _, _ = O.render(sc, w, h, threads=4)
    assert_equal_to_reference(got, None, want, None)       # (bit for bit on an FMA host, else within one step per channel)


def test_diagnostics_without_a_single_value_are_refused(torch_cuda, scenes):
    torch = torch_cuda
    sc = scenes["scene4"]
    w, h = 32, 16
    r = gpu.Renderer(0)
    r.set_samples(2)
    r.prepare(sc)
    frame = torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda:0")
    f32 = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda:0")
    u32 = torch.full((h, w), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for dbg in (gpu.Debug(None, None, u32.data_ptr(), None), gpu.Debug(None, None, None, u32.data_ptr()),
                gpu.Debug(None, f32.data_ptr(), None, None)):
        with pytest.raises(gpu.GpuError) as e:
            r.render_into(frame.data_ptr(), w, h, debug=dbg)
        assert e.value.status == ERR_UNSUPPORTED
    r.sync()
    assert (frame.cpu().numpy() == SENTINEL).all() and (u32.cpu().numpy() == 7).all() and (f32.cpu().numpy() == 7.0).all()
    # the same requests with one sample per pixel are served
    r.set_samples(1)
    r.render_into(frame.data_ptr(), w, h, debug=gpu.Debug(None, f32.data_ptr(), u32.data_ptr(), None))
    r.sync()
    assert (frame.cpu().numpy() != SENTINEL).all()
    r.close()


def test_set_samples_refuses_other_values(torch_cuda):
    r = gpu.Renderer(0)
    assert r.samples == 1
    r.set_samples(4)
    for bad in (0, 3, 5, 8, -2):
        with pytest.raises(gpu.GpuError) as e:
            r.set_samples(bad)
        assert e.value.status == ERR_ARG
        assert r.samples == 4
    r.set_samples(2)
    assert r.samples == 2
    r.close()
    m = gpu.MultiRenderer([0])
    for bad in (0, 3):
        with pytest.raises(gpu.GpuError) as e:
            m.set_samples(bad)
        assert e.value.status == ERR_ARG
    m.close()
