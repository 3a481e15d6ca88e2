"""Supersampled scene views (lol_gpu_render_scene_views_samples): every pixel IS the contract of include/lol_gpu.h restated on the CPU
oracle (tests/scene_view_samples_reference.py) — packed pixels and lol_gpu_debug.rgb EQUAL, bit for bit — and, with K = 1, the
frame a fresh context with lol_gpu_set_samples(s) renders after uploading that record's scene.

The three arms of tests/test_gpu_scene_views.py: the interpreter's kernels in plain arithmetic (specialize=0), the interpreter's
kernels with the upload's proven fast paths (specialize=4), and the structure module made with set_scene_view_samples (the kernels'
names checked after specialize_wait).  Frames are 33 x 17 with max_steps 256: sample grids of 66 x 34 and 132 x 68, ragged against
the 16 x 4 tile in x for both s and in y for s = 2.  tests/test_scene_view_samples_reference.py holds the inputs, on the CPU, to
telling a kernel that ignores s, the record's scene or all records but one from a right one.  Reference means and fresh contexts'
frames are cached for the whole module and shared between the arms.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_view_samples_reference as R
import test_gpu_scene_views as SV
import test_gpu_views as V
from loltracer_amd import gpu, scene as S

pytestmark = pytest.mark.gpu

W, H, MAX_STEPS = R.W, R.H, R.MAX_STEPS
PITCH, STRIDE = W + 3, H * (W + 3) + 5                   # a pitch and a view stride larger than the frame
ERR_ARG, ERR_UNSUPPORTED = -3, -5
ARMS = SV.ARMS
NAMES = R.NAMES
KERNEL = {"interpreter": ("render_interp_scene_batch_aa", "render_interp_scene_batch_aa_lin"),
          "interpreter-fast": ("render_interp_scene_batch_aa", "render_interp_scene_batch_aa_lin"),
          "structure-module": ("lol_render_param_batch_aa", "lol_render_param_batch_aa_lin")}
bits = V.bits
_kept = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def open_renderer(sc, arm, wait=True):
    r = gpu.Renderer(0, specialize=SV.SPECIALIZE[arm])
    try:
        r.set_scene_view_samples(arm == "structure-module")
        assert r.scene_view_samples == (arm == "structure-module") and not r.scene_views      # (it brings the module, not the other getter)
        r.prepare(sc, wait=wait)
        if wait:
            assert r.scene_views_state() == (2 if arm == "structure-module" else 0), r.specialize_log()
            for s in (2, 4):
                assert (r.scene_view_samples_kernel_name(1, s), r.scene_view_samples_kernel_name(4, s)) == KERNEL[arm]
            assert (r.scene_view_samples_kernel_name(1, 1), r.scene_view_samples_kernel_name(4, 1)) == SV.KERNEL[arm]
    except BaseException:
        r.close()
        raise
    return r


def queue(r, out, cams, scs, k, s, stream=None):
    n, w, h, pitch_px, stride_px = out["geom"]
    assert len(scs) == len(cams) == n * k
    r.render_scene_views_into(out["frame"].data_ptr(), cams, scs, w, h, k, MAX_STEPS, pitch_bytes=pitch_px * 4,
                              view_stride_bytes=stride_px * 4, debug=out["dbg"], stream=stream, samples=s)


def render(torch, r, cams, scs, k, s, debug=("rgb",), pitch_px=None, stride_px=None, w=W, h=H):
    out = V.alloc_batch(torch, len(scs) // k, w, h, pitch_px, stride_px, debug)
    torch.cuda.synchronize()                 # torch's fills run on ITS stream; the call on the renderer's own
    queue(r, out, cams, scs, k, s)
    r.sync()
    return V.collect(out, *out["geom"])


def assert_is_reference(b, scs, cams, k, s, what, w=W, h=H):
    px, rgb = R.render(scs, cams, k, s, w, h, max_steps=MAX_STEPS)
    assert np.array_equal(b["xrgb"], px), f"{what}: pixels differ from the reference"
    assert np.array_equal(bits(b["rgb"]), bits(rgb)), f"{what}: rgb differs from the reference"


def supersampled_frame(torch, r, cam, s):
    """(xrgb, rgb) of the frame `r` renders under `cam` with set_samples(s); the setting is put back"""
    dev = torch.device("cuda:0")
    frame = torch.zeros((H, W), dtype=torch.int32, device=dev)
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    r.set_samples(s)
    try:
        r.render_into(frame.data_ptr(), W, H, MAX_STEPS, camera=cam, debug=gpu.Debug(rgb.data_ptr(), None, None, None))
        r.sync()
    finally:
        r.set_samples(1)
    return frame.cpu().numpy().view(np.uint32), rgb.cpu().numpy()


def fresh_frame(torch, sc, cam, s, key):
    """... of a fresh context that uploaded `sc` (cached: every arm asks)"""
    if key not in _kept:
        r = gpu.Renderer(0, specialize=False)
        try:
            r.prepare(sc)
            _kept[key] = supersampled_frame(torch, r, cam, s)
        finally:
            r.close()
    return _kept[key]


@pytest.mark.parametrize("s", R.SINGLE_SAMPLES)
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name", NAMES + ("tables-global",))
def test_three_views_are_three_supersampled_frames_of_three_scenes(torch_cuda, scenes, name, arm, s):
    scs, cams = R.single_case(scenes, name)
    r = open_renderer(SV.base_scene(scenes, name), arm)
    try:
        b = render(torch_cuda, r, cams, scs, 1, s, pitch_px=PITCH, stride_px=STRIDE)
        assert V.untouched_outside_views(b, 3, W, H, PITCH, STRIDE)
        assert_is_reference(b, scs, cams, 1, s, f"{name} s={s} ({arm})")
        for v in range(3):
            px, rgb = fresh_frame(torch_cuda, scs[v], cams[v], s, ("fresh", name, v, s))
            assert np.array_equal(b["xrgb"][v], px) and np.array_equal(bits(b["rgb"][v]), bits(rgb)), f"{name} view {v} s={s} ({arm})"
    finally:
        r.close()


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name", NAMES)
def test_supersampled_blends_over_moving_objects_equal_the_reference(torch_cuda, scenes, name, arm):
    r = open_renderer(SV.base_scene(scenes, name), arm)
    try:
        for k, s in R.BLENDS:
            scs, cams = R.blend_case(scenes, name, k)
            b = render(torch_cuda, r, cams, scs, k, s, pitch_px=PITCH, stride_px=STRIDE)
            assert V.untouched_outside_views(b, 2, W, H, PITCH, STRIDE)
            assert_is_reference(b, scs, cams, k, s, f"{name} K={k} s={s} ({arm})")
        # hit_dist, hit_id and steps: refused whenever s > 1 or K > 1, and nothing is written
        scs1, cams1 = R.single_case(scenes, name)
        scs2, cams2 = R.blend_case(scenes, name, 2)
        for items, cameras, k, s, n in ((scs2, cams2, 2, 2, 2), (scs1, cams1, 1, 2, 3), (scs1, cams1, 1, 4, 3)):
            for d in ("dist", "id", "steps"):
                out = V.alloc_batch(torch_cuda, n, W, H, None, None, (d,))
                torch_cuda.cuda.synchronize()
                with pytest.raises(gpu.GpuError) as e:
                    queue(r, out, cameras, items, k, s)
                assert e.value.status == ERR_UNSUPPORTED, (k, s, d)
                r.sync()
                got = V.collect(out, *out["geom"])
                assert (got["raw"] == V.SENTINEL).all() and not bits(got[d]).any(), (k, s, d)
    finally:
        r.close()


def call_entry_point(r, sc, out, cams, scs, k, s):
    """lol_gpu_render_scene_views_samples itself (Renderer.render_scene_views_into takes the older entry point for samples = 1)"""
    n, w, h, pitch_px, stride_px = out["geom"]
    keep = [x.flatten() for x in scs]
    progs = (S.Program * len(scs))()
    fcs = (S.FrameCamera * len(scs))()
    for i, (p, c) in enumerate(zip(keep, cams)):
        C.memmove(C.byref(progs, i * C.sizeof(S.Program)), C.byref(p), C.sizeof(S.Program))
        fc = sc.frame_camera(w, h, c)
        C.memmove(C.byref(fcs, i * C.sizeof(S.FrameCamera)), C.byref(fc), C.sizeof(S.FrameCamera))
    dbg = C.byref(out["dbg"]) if out["dbg"] is not None else None
    return gpu.gpu_lib().lol_gpu_render_scene_views_samples(r._ctx, fcs, progs, n, k, w, h, MAX_STEPS, s, C.c_void_p(out["frame"].data_ptr()),
                                                            pitch_px * 4, stride_px * 4, dbg, None)


@pytest.mark.parametrize("arm", ARMS)
def test_one_sample_is_the_scene_views_call(torch_cuda, scenes, arm):
    base = scenes["scene4"]
    scs, cams = R.single_case(scenes, "scene4")
    r = open_renderer(base, arm)
    try:
        plain = SV.render(torch_cuda, r, cams, scs)                             # all four diagnostics
        out = V.alloc_batch(torch_cuda, 3, W, H, None, None, True)
        torch_cuda.cuda.synchronize()
        assert call_entry_point(r, base, out, cams, scs, 1, 1) == 0
        r.sync()
        one = V.collect(out, *out["geom"])
        assert np.array_equal(one["raw"], plain["raw"])
        for d in V.DIAGNOSTICS:
            assert np.array_equal(bits(one[d]), bits(plain[d])), d
        scs2, cams2 = R.blend_case(scenes, "scene4", 2)
        blend = SV.render(torch_cuda, r, cams2, scs2, 2, debug=("rgb",))
        out = V.alloc_batch(torch_cuda, 2, W, H, None, None, ("rgb",))
        torch_cuda.cuda.synchronize()
        assert call_entry_point(r, base, out, cams2, scs2, 2, 1) == 0
        r.sync()
        one = V.collect(out, *out["geom"])
        assert np.array_equal(one["raw"], blend["raw"]) and np.array_equal(bits(one["rgb"]), bits(blend["rgb"]))
    finally:
        r.close()


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name", NAMES)
def test_the_uploaded_scene_in_every_record_is_the_supersampled_blend(torch_cuda, scenes, name, arm):
    base = SV.base_scene(scenes, name)
    orbit = S.orbit_cameras(base, 8)
    r = open_renderer(base, arm)
    try:
        for k, s in ((2, 2), (1, 4)):
            cams = []
            for v in range(2):
                cams += S.shutter_cameras(orbit[v], orbit[v + 1], k) if k > 1 else [orbit[v]]
            out = V.alloc_batch(torch_cuda, 2, W, H, None, None, ("rgb",))
            torch_cuda.cuda.synchronize()
            r.render_blended_views_into(out["frame"].data_ptr(), cams, k, W, H, MAX_STEPS, debug=out["dbg"], samples=s)
            r.sync()
            blend = V.collect(out, *out["geom"])
            b = render(torch_cuda, r, cams, [base] * len(cams), k, s)
            assert np.array_equal(b["raw"], blend["raw"]) and np.array_equal(bits(b["rgb"]), bits(blend["rgb"])), (k, s)
    finally:
        r.close()


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name", NAMES)
def test_a_hostile_record_is_its_own_business(torch_cuda, scenes, name, arm):
    base = SV.base_scene(scenes, name)
    sane, cams = R.single_case(scenes, name)
    bad, insane = SV.hostile_scene(scenes, name), _kept.setdefault("insane", V.insane_camera())
    scs = [sane[0], bad, sane[1], sane[2], sane[2]]
    all_cams = [cams[0], cams[1], cams[1], insane, cams[2]]
    r = open_renderer(base, arm)
    try:
        b = render(torch_cuda, r, all_cams, scs, 1, 2)
        alone = render(torch_cuda, r, cams, sane, 1, 2)
        for v, u in ((0, 0), (2, 1), (4, 2)):
            assert np.array_equal(b["xrgb"][v], alone["xrgb"][u]) and np.array_equal(bits(b["rgb"][v]), bits(alone["rgb"][u])), (v, u)
        for v in (1, 3):
            px, rgb = R.render([scs[v]], [all_cams[v]], 1, 2, W, H, max_steps=MAX_STEPS)
            assert np.array_equal(b["xrgb"][v], px[0]), f"{name} hostile view {v} ({arm})"
            assert np.array_equal(b["rgb"][v], rgb[0], equal_nan=True), f"{name} hostile view {v} ({arm})"      # (a NaN is a NaN)
        # ... and in a blend: the group with the hostile record is the reference's, the other group is what it is without it
        k = 2
        scs2, cams2 = [sane[0], bad, sane[1], sane[2]], [cams[0], cams[1], cams[1], cams[2]]
        b2 = render(torch_cuda, r, cams2, scs2, k, 2)
        px, rgb = R.render(scs2, cams2, k, 2, W, H, max_steps=MAX_STEPS)
        assert np.array_equal(b2["xrgb"], px) and np.array_equal(b2["rgb"], rgb, equal_nan=True), f"{name} hostile blend ({arm})"
    finally:
        r.close()


@pytest.mark.parametrize("arm", ARMS)
def test_the_context_is_left_as_it_was(torch_cuda, scenes, arm):
    base = scenes["scene4"]
    scs, cams = R.single_case(scenes, "scene4")
    r = open_renderer(base, arm)
    other = gpu.Renderer(0, specialize=SV.SPECIALIZE[arm])
    try:
        other.prepare(base)                                                      # the same scene without the switch
        assert other.kernel_key() == r.kernel_key() and other.kernel_name() == r.kernel_name()
        for _ in range(3):                                                       # (a repeated view: the tile-order state has something to lose)
            before = V.render_single(torch_cuda, r, cams[1], W, H, MAX_STEPS)
        before_aa = supersampled_frame(torch_cuda, r, cams[1], 2)
        key, order, name, samples = r.kernel_key(), r.tile_order(), r.kernel_name(), r.samples
        render(torch_cuda, r, cams, scs, 1, 2)
        render(torch_cuda, r, cams + cams[:1], scs + scs[:1], 2, 4)
        assert (r.kernel_key(), r.tile_order(), r.kernel_name(), r.samples) == (key, order, name, samples)
        after = V.render_single(torch_cuda, r, cams[1], W, H, MAX_STEPS)
        for d in ("xrgb",) + V.DIAGNOSTICS:
            assert np.array_equal(bits(after[d]), bits(before[d])), d
        after_aa = supersampled_frame(torch_cuda, r, cams[1], 2)
        assert np.array_equal(after_aa[0], before_aa[0]) and np.array_equal(bits(after_aa[1]), bits(before_aa[1]))
    finally:
        other.close()
        r.close()


@pytest.mark.parametrize("arm", ARMS)
def test_refusals_write_nothing_and_leave_the_context_usable(torch_cuda, scenes, arm):
    base = scenes["scene4"]
    scs, cams = R.single_case(scenes, "scene4")
    progs = [sc.flatten() for sc in scs]
    r = open_renderer(base, arm)
    try:
        dev = torch_cuda.device("cuda:0")
        frame = torch_cuda.full((3 * H * W,), SV.PATTERN, dtype=torch_cuda.int32, device=dev)
        torch_cuda.cuda.synchronize()

        def refused(cameras, items, k, s, status):
            with pytest.raises(gpu.GpuError) as e:
                r.render_scene_views_into(frame.data_ptr(), cameras, items, W, H, k, MAX_STEPS, samples=s)
            assert e.value.status == status, e.value
            r.sync()
            assert (frame.cpu().numpy().view(np.uint32) == SV.PATTERN).all()

        refused(cams, progs, 1, 3, ERR_ARG)                                      # s outside the set
        refused(cams, progs, 3, 3, ERR_ARG)                                      # ... which is checked first
        for s in (2, 4):
            refused(cams, progs, 3, s, ERR_ARG)                                  # K outside the set
            for what in ("opcode", "n_lights"):                                  # a scene of another structure, anywhere in the list
                for at in (0, 2):
                    items = list(progs)
                    items[at] = SV.changed_program(progs[at], what)
                    refused(cams, items, 1, s, ERR_ARG)
        # a sample grid of more than 65535 tiles along an axis (nothing is touched: refused before any launch)
        with pytest.raises(gpu.GpuError) as e:
            r.render_scene_views_into(frame.data_ptr(), cams[:1], progs[:1], 300000, 1, 1, MAX_STEPS, pitch_bytes=1200000,
                                      view_stride_bytes=1200000, samples=4)
        assert e.value.status == ERR_ARG
        r.sync()
        assert (frame.cpu().numpy().view(np.uint32) == SV.PATTERN).all()
        # ... and the context still renders
        b = render(torch_cuda, r, cams, scs, 1, 2)
        assert_is_reference(b, scs, cams, 1, 2, f"after the refusals ({arm})")
    finally:
        r.close()


@pytest.mark.parametrize("streams", (1, 4), ids=("one-stream", "four-streams"))
@pytest.mark.parametrize("arm", ARMS)
def test_ten_calls_back_to_back(torch_cuda, scenes, arm, streams):
    """Ten calls with NO wait between them, supersampled blends (K = 2, s = 2) alternating with plain blends of scene views: the
    record ring has 8 sets, the scratch ring both kinds share has 4.  Every result is its own reference.  16 x 8 pixels, two views."""
    base = scenes["scene4"]
    w, h, k = 16, 8, 2
    moved = SV.moving(scenes, "scene4", 6, k)                                  # 12 scenes: four for a call, three different calls
    cam = _kept.setdefault("base-camera", V.copy_camera(base.camera))
    calls = [(moved[4 * (i % 3):4 * (i % 3) + 4], 2 if i % 2 == 0 else 1) for i in range(10)]
    r = open_renderer(base, arm)
    try:
        r.set_frames_in_flight(streams)
        outs = [V.alloc_batch(torch_cuda, 2, w, h, w + 3, h * (w + 3) + 5, ("rgb",)) for _ in calls]
        torch_cuda.cuda.synchronize()
        for out, (scs, s) in zip(outs, calls):
            queue(r, out, [cam] * 4, scs, k, s)
        r.sync()
        for i, (out, (scs, s)) in enumerate(zip(outs, calls)):
            b = V.collect(out, *out["geom"])
            assert_is_reference(b, scs, [cam] * 4, k, s, f"call {i} s={s} ({arm})", w, h)
            assert V.untouched_outside_views(b, 2, w, h, w + 3, h * (w + 3) + 5), f"call {i}"
    finally:
        r.close()


def test_a_call_before_the_structure_module_is_loaded(torch_cuda, scenes):
    """a context that asked for the module renders from the first call on: on the interpreter's kernels while the module is being
    compiled, on the module once a call's boundary or specialize_wait has loaded it — the same frames"""
    base = scenes["scene4"]
    scs, cams = R.single_case(scenes, "scene4")
    r = open_renderer(base, "structure-module", wait=False)
    try:
        assert r.scene_view_samples and r.scene_views_state() == 1              # nothing is loaded outside a boundary
        names = set()
        for _ in range(2):
            b = render(torch_cuda, r, cams, scs, 1, 2)
            names.add(r.scene_view_samples_kernel_name(1, 2))
            assert_is_reference(b, scs, cams, 1, 2, f"({r.scene_view_samples_kernel_name(1, 2)})")
        r.specialize_wait()
        assert r.scene_views_state() == 2, r.specialize_log()
        assert (r.scene_view_samples_kernel_name(1, 2), r.scene_view_samples_kernel_name(2, 4)) == KERNEL["structure-module"]
        assert (r.scene_views_kernel_name(1), r.scene_views_kernel_name(2)) == SV.KERNEL["structure-module"]      # it brings set_scene_views
        b = render(torch_cuda, r, cams, scs, 1, 2)
        assert_is_reference(b, scs, cams, 1, 2, "after the wait")
        assert names <= {KERNEL["interpreter"][0], KERNEL["structure-module"][0]}
    finally:
        r.close()


def test_a_module_without_the_switch_leaves_supersampled_calls_to_the_interpreter(torch_cuda, scenes):
    """set_scene_views alone: the structure module has two kernels, which render s = 1; s > 1 runs on the interpreter's — same bits"""
    base = scenes["scene4"]
    scs, cams = R.single_case(scenes, "scene4")
    r = SV.open_renderer(base, "structure-module")
    try:
        assert not r.scene_view_samples
        assert (r.scene_view_samples_kernel_name(1, 2), r.scene_view_samples_kernel_name(2, 2)) == KERNEL["interpreter"]
        assert r.scene_view_samples_kernel_name(1, 1) == SV.KERNEL["structure-module"][0]
        b = render(torch_cuda, r, cams, scs, 1, 2)
        assert_is_reference(b, scs, cams, 1, 2, "a structure module without the supersampled kernels")
    finally:
        r.close()


def read_ppm(path, w, h):
    data = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert data.startswith(head)
    rgb = np.frombuffer(data[len(head):], dtype=np.uint8).reshape(h, w, 3).astype(np.uint32)
    return rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2]


def test_the_tween_host_supersamples(torch_cuda, scenes, tmp_path):
    """python -m loltracer_amd A.lol --tween B.lol --frames 2 --tween-samples 2 [--tween-shutter 2] -o DIR writes the frames of
    render_scene_views_into(..., samples=2) over scene.tween's scenes; --samples beside --tween stays refused"""
    root = V.ROOT
    a_file = os.path.join(root, "tests", "golden", "scenes", "scene4.lol")
    text = open(a_file).read()
    assert "point\t\t= (0, 1, -6)" in text
    b_file = str(tmp_path / "b.lol")
    with open(b_file, "w") as f:
        f.write(text.replace("point\t\t= (0, 1, -6)", "point\t\t= (1.5, 2, -5)"))
    a, other = scenes["scene4"], S.Scene.parse_file(b_file)
    w, h, n = 32, 16, 2
    r = gpu.Renderer(0)
    try:
        r.prepare(a)
        for k in (1, 2):
            out_dir = tmp_path / ("frames_k%d" % k)
            cmd = [sys.executable, "-m", "loltracer_amd", a_file, "--tween", b_file, "--frames", str(n), "--tween-samples", "2",
                   "--size", f"{w}x{h}", "-o", str(out_dir)] + (["--tween-shutter", "2"] if k > 1 else [])
            p = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            assert p.returncode == 0 and "2x2 samples per pixel" in p.stdout and "_aa" in p.stdout, p.stdout
            scs = [S.tween(a, other, t) for f in range(n) for t in S.shutter_times(f, n, k)]
            b = render(torch_cuda, r, [a.camera] * len(scs), scs, k, 2, debug=False, w=w, h=h)
            assert sorted(os.listdir(out_dir)) == [f"frame_{f:04d}.ppm" for f in range(n)]
            for f in range(n):
                assert np.array_equal(read_ppm(out_dir / f"frame_{f:04d}.ppm", w, h), b["xrgb"][f] & 0xFFFFFF), (k, f)
            assert not np.array_equal(b["xrgb"][0], b["xrgb"][1])
        p = subprocess.run(cmd + ["--samples", "2"], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 1 and "--tween" in p.stdout, p.stdout
    finally:
        r.close()
