"""Relit averaged pixels on the device: lol_gpu_light_views (a loop of light_interp launches) held to lol_gpu_light_pixels, and
lol_gpu_relight_views (relight_views) held to the host composition of lol_gpu_relight's leaves (tests/light_views_reference.py, which
tests/test_light_views_reference.py holds to the oracle) and to the supersampled frames and blends of contexts that uploaded the look.

Every comparison is ray_reference.same_bits: equality of bit patterns, two NaNs counting as the same; no tolerance.  Sizes: 13 x 5 (one
partial block) and 37 x 11 (more than one block, neither side a multiple of the 16 x 4 patch).  The captures are made once per (scene,
mode, shape) for the whole module and left unchanged: a look changes no plane.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import blend_aa_reference as BA
import light_views_reference as LV
import ray_reference as R
import scene_shapes as SH
import test_gpu_views as V
from loltracer_amd import gpu
from loltracer_amd import scene as S
from loltracer_amd.__main__ import main as cli_main
from test_gpu_light import (FACTORS, LOOK_TEXT, RELIT, SENTINEL, Colours, Planes, assert_same, capture_pixels, forbidden_looks,
                            open_renderer, refusal, relight, restore, scene_with_lights)
from test_gpu_shades import LOSSY, frame, stream_of
from test_light_reference import looks_of

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (4, 1), (1, 2), (1, 16), (2, 4), (4, 2)]      # (s, K)
SIZES = {1: (13, 5), 3: (37, 11)}                               # by n_views
MODES = {"default": 1, "interp": 4}                             # lol_gpu_set_specialize
LENS_FOCUS, LENS_RADIUS = 6.0, 0.25


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def cameras_of(sc, n_views, k):
    """n_views K cameras: one view is the scene's camera or a lens round it, three views are neighbours of an orbit or exposures
    between them"""
    if n_views == 1:
        return S.lens_cameras(sc.camera, LENS_FOCUS, LENS_RADIUS, k)
    if k == 1:
        return S.orbit_cameras(sc, 8)[:n_views]
    return BA.shutter_groups(sc, n_views, k)


def capture_views(torch, r, cams, k, w, h, s, stride=0, stream="torch", max_steps=256):
    """the planes of lol_gpu_light_views over all N leaves, with their sentinel padding"""
    p = Planes(torch, len(cams) * s * s * w * h, len(r.scene.lights()), stride)
    torch.cuda.synchronize()
    r.light_views_into(cams, k, w, h, s, max_steps, stream=stream_of(torch, stream), **p.args())
    r.sync()
    torch.cuda.synchronize()
    return p


def relight_views(torch, r, look, p, n_views, k, w, h, s, want=RELIT, stream="torch"):
    c = Colours(torch, n_views * w * h, want)
    torch.cuda.synchronize()
    r.relight_views_into(look, n_views, k, w, h, s, stream=stream_of(torch, stream), **p.relight_args(), **c.args())
    r.sync()
    torch.cuda.synchronize()
    return c.collect()


def composed(torch, r, look, p, n_views, k, w, h, s, fmt=None):
    """the contract on the host: tree means of plain lol_gpu_relight's rgb_linear over the same planes, then powf and pack"""
    leaves = relight(torch, r, look, p, want=("rgb_linear",))["rgb_linear"]
    return LV.finish(LV.resolve(leaves, n_views, k, w, h, s), fmt)


def rendered(torch, r2, cams, k, w, h, s):
    """dict(rgb, pixel), dense over [view, y, x], of the views a context renders: frames after set_samples(s) for K = 1, else
    render_blended_views_into(..., samples=s)"""
    n = len(cams) // k
    if k == 1:
        r2.set_samples(s)
        try:
            fs = [frame(torch, r2, w, h, camera=c, planes=False) for c in cams]
        finally:
            r2.set_samples(1)
        return dict(rgb=np.concatenate([f["rgb"] for f in fs]), pixel=np.concatenate([f["pixel"] for f in fs]))
    out = V.alloc_batch(torch, n, w, h, debug=("rgb",))
    torch.cuda.synchronize()
    r2.render_blended_views_into(out["frame"].data_ptr(), cams, k, w, h, debug=out["dbg"], samples=s)
    r2.sync()
    got = V.collect(out, *out["geom"])
    return dict(rgb=np.ascontiguousarray(got["rgb"].reshape(-1, 3)), pixel=np.ascontiguousarray(got["xrgb"].ravel()))


class Captures:
    """the capturing renderer of each (scene, mode) and its captures, made once and shared by the tests of this module"""

    def __init__(self, torch, scenes):
        self.torch, self.scenes, self.r, self.p = torch, scenes, {}, {}

    def renderer(self, name, mode):
        if (name, mode) not in self.r:
            self.r[name, mode] = open_renderer(self.scenes[name], MODES[mode])
        return self.r[name, mode]

    def planes(self, name, mode, n_views, s, k):
        key = (name, mode, n_views, s, k)
        if key not in self.p:
            w, h = SIZES[n_views]
            cams = cameras_of(self.scenes[name], n_views, k)
            self.p[key] = (cams, capture_views(self.torch, self.renderer(name, mode), cams, k, w, h, s))
        return self.p[key]

    def close(self):
        for r in self.r.values():
            r.close()


@pytest.fixture(scope="module")
def captures(torch_cuda, scenes):
    c = Captures(torch_cuda, scenes)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------------------ 1. the capture's layout
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_the_capture_is_one_light_pixels_call_per_camera(torch_cuda, scenes, name, mode):
    """record r = v K + k is lol_gpu_light_pixels of the s w x s h frame under cams[r], r s^2 w h elements into planes whose lights
    are `light_stride` apart; nothing behind a plane, between two planes or behind the last is written (Planes.collect)"""
    sc, n_views = scenes[name], 2
    r = open_renderer(sc, MODES[mode])
    try:
        for (w, h), shapes in (((13, 5), [(s, k) for s in (1, 2, 4) for k in (1, 2)]), ((37, 11), [(2, 2)])):
            for s, k in shapes:
                cams = BA.shutter_groups(sc, n_views, k) if k > 1 else S.orbit_cameras(sc, 8)[1:1 + n_views]
                per = s * s * w * h
                for stride in (len(cams) * per + 7, 0):
                    got = capture_views(torch_cuda, r, cams, k, w, h, s, stride=stride).collect()
                    for i, cam in enumerate(cams):
                        _, one = capture_pixels(torch_cuda, r, s * w, s * h, camera=cam)
                        part = {f: got[f][i * per:(i + 1) * per] for f in got}
                        assert_same(part, one, ("id", "dist", "steps") + FACTORS + ("shadow_steps",),
                                    f"{name} {mode} {w}x{h} s={s} K={k} stride={stride}: record {i}")
    finally:
        r.close()


# -------------------------------------------------------------------------------------------------- 2. the resolve against composition
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_the_resolve_is_the_tree_mean_of_relit_leaves(torch_cuda, scenes, captures, name, mode):
    """rgb_linear is aa_reference.tree_mean, over the samples and then over the cameras, of plain lol_gpu_relight's rgb_linear over the
    same planes; rgb and pixel follow from it by oracle_lib.powf and aa_reference.pack; each output alone is its column"""
    sc = scenes[name]
    r = captures.renderer(name, mode)
    looks = looks_of(sc)
    for n_views in (1, 3):
        w, h = SIZES[n_views]
        for s, k in SHAPES:
            _, p = captures.planes(name, mode, n_views, s, k)
            for what, look in [("own", None), looks[0], looks[4]]:
                got = relight_views(torch_cuda, r, look, p, n_views, k, w, h, s)
                assert_same(got, composed(torch_cuda, r, look, p, n_views, k, w, h, s), RELIT, f"{name} {mode} n={n_views} s={s} K={k} {what}")
    for f in RELIT:
        alone = relight_views(torch_cuda, r, look, p, n_views, k, w, h, s, want=(f,))
        assert set(alone) == {f}
        assert_same(alone, got, (f,), f"{f} alone")


def test_a_light_stride_between_the_planes(torch_cuda, scenes):
    """planes whose lights are more than N apart resolve as dense ones do, and nothing of them is written"""
    sc, (w, h), (s, k, n_views) = scenes["scene4"], (37, 11), (2, 2, 2)
    cams = BA.shutter_groups(sc, n_views, k)
    r = open_renderer(sc, 1)
    try:
        dense = capture_views(torch_cuda, r, cams, k, w, h, s)
        wide = capture_views(torch_cuda, r, cams, k, w, h, s, stride=dense.n + 77)
        look = looks_of(sc)[1][1]
        before = wide.collect()
        assert_same(relight_views(torch_cuda, r, look, wide, n_views, k, w, h, s), relight_views(torch_cuda, r, look, dense, n_views, k, w, h, s),
                    RELIT, "strided planes")
        assert_same(wide.collect(), before, ("id",) + FACTORS, "the planes after a resolve")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------- 3. end to end
@pytest.mark.parametrize("which", range(6), ids=lambda k: "abcde-"[k])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_relit_views_are_the_views_of_a_context_that_uploaded_the_look(torch_cuda, scenes, captures, name, mode, which):
    """every look of looks_of (the NaN and infinite ones included) and look = None, every shape, one view and three: rgb and pixel are
    the supersampled frame (K = 1) or the blend (K > 1) of a context that uploaded the look"""
    sc = scenes[name]
    what, look = ("own", None) if which == 5 else looks_of(sc)[which]
    r = captures.renderer(name, mode)
    r2 = open_renderer(sc if look is None else look, MODES[mode])
    try:
        for n_views in (1, 3):
            w, h = SIZES[n_views]
            for s, k in SHAPES:
                cams, p = captures.planes(name, mode, n_views, s, k)
                got = relight_views(torch_cuda, r, look, p, n_views, k, w, h, s)
                assert_same(got, rendered(torch_cuda, r2, cams, k, w, h, s), ("rgb", "pixel"), f"{name} {mode} {what} n={n_views} s={s} K={k}")
    finally:
        r2.close()


# ------------------------------------------------------------------------------------------------------------------- 4. forwarding
def test_one_sample_and_one_camera_is_relight(torch_cuda, scenes):
    sc, (w, h), n_views = scenes["scene4"], (37, 11), 3
    cams = S.orbit_cameras(sc, 8)[:n_views]
    r = open_renderer(sc, 1)
    try:
        p = capture_views(torch_cuda, r, cams, 1, w, h, 1)
        for what, look in [("own", None)] + looks_of(sc):
            assert_same(relight_views(torch_cuda, r, look, p, n_views, 1, w, h, 1), relight(torch_cuda, r, look, p), RELIT, what)
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 5. tables in global memory, three lights
@pytest.mark.parametrize("case", ["three-lights", "tree2-tables"])
def test_light_counts_and_large_tables(torch_cuda, case):
    sc = SH.scene_of(SH.RUNG["tree2-tables"]) if case == "tree2-tables" else scene_with_lights(3)
    nl, nm = len(sc.lights()), len(sc.materials())
    look = sc.with_look(lights=[((.2, .9, .4), (.7, .1, .5))] * nl, materials=[((.1, .2, .3), (.3, .2, .1), (.4, .4, .1))] * nm, ambient=(.6, .5, .4))
    (w, h), n_views = (13, 5), 2
    r, r2 = open_renderer(sc, 1), open_renderer(look, 1)
    try:
        assert r.interp_variant()[1] == (case == "tree2-tables")        # the tables read from global memory, or staged
        for s, k in ((2, 2), (4, 1), (1, 4)):
            cams = S.lens_cameras(sc.camera, LENS_FOCUS, LENS_RADIUS, k) + S.lens_cameras(sc.camera, LENS_FOCUS / 2, LENS_RADIUS, k)
            p = capture_views(torch_cuda, r, cams, k, w, h, s)
            for what, lk, ctx in (("own", None, r), ("look", look, r2)):
                got = relight_views(torch_cuda, r, lk, p, n_views, k, w, h, s)
                assert_same(got, composed(torch_cuda, r, lk, p, n_views, k, w, h, s), RELIT, f"{case} s={s} K={k} {what}: composition")
                assert_same(got, rendered(torch_cuda, ctx, cams, k, w, h, s), ("rgb", "pixel"), f"{case} s={s} K={k} {what}: rendered")
    finally:
        r2.close()
        r.close()


# ------------------------------------------------------------------------------------------------------------------ 6. pixel formats
def test_a_lossy_pixel_format(torch_cuda, scenes):
    sc, (w, h), n_views = scenes["scene4"], (37, 11), 1
    what, look = looks_of(sc)[1]
    r, r2 = open_renderer(sc, 1), open_renderer(look, 1)
    try:
        r.set_pixel_format(LOSSY)
        r2.set_pixel_format(LOSSY)
        for s, k in ((2, 1), (2, 4)):
            cams = cameras_of(sc, n_views, k)
            p = capture_views(torch_cuda, r, cams, k, w, h, s)
            got = relight_views(torch_cuda, r, look, p, n_views, k, w, h, s)
            assert_same(got, composed(torch_cuda, r, look, p, n_views, k, w, h, s, fmt=LOSSY), RELIT, f"lossy s={s} K={k}: composition")
            assert_same(got, rendered(torch_cuda, r2, cams, k, w, h, s), ("rgb", "pixel"), f"lossy s={s} K={k}: rendered")
            assert (got["pixel"] & 0xFF000000 == 0xFF000000).all()
    finally:
        r2.close()
        r.close()


# ------------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(torch_cuda, scenes):
    """every line of the header's list returns its status with nothing written, and a plain frame afterwards is the frame before"""
    sc, (w, h), (s, k, n_views) = scenes["scene4"], (13, 5), (2, 2, 1)
    N = n_views * k * s * s * w * h
    cams = cameras_of(sc, n_views, k)
    fcs = (S.FrameCamera * len(cams))(*[sc.frame_camera(w, h, c) for c in cams])
    p, c = Planes(torch_cuda, N, 2), Colours(torch_cuda, n_views * w * h)
    a, ra, ca = p.args(), p.relight_args(), c.args()
    lib = gpu.gpu_lib()
    torch_cuda.cuda.synchronize()

    def passes(**kw):
        v = dict(a, **kw)
        return gpu.LightPasses(v["factors_ptr"] or None, v["light_stride"], v["id_ptr"] or None, v["dist_ptr"] or None, v["steps_ptr"] or None)

    relit = gpu.Relit(*(ca[f + "_ptr"] for f in RELIT))

    def light(ctx, cams=fcs, n=n_views, k=k, w=w, h=h, s=s, max_steps=256, out=True, **kw):
        return lib.lol_gpu_light_views(ctx, cams, n, k, w, h, s, max_steps, passes(**kw) if out else None, None)

    def resolve(ctx, n=n_views, k=k, w=w, h=h, s=s, planes=True, out=relit, **kw):
        return lib.lol_gpu_relight_views(ctx, None, passes(**kw) if planes else None, n, k, w, h, s, out, None)

    empty = gpu.Renderer(0)
    try:
        assert light(empty._ctx) == -4 and resolve(empty._ctx) == -4                       # no program uploaded
        assert resolve(empty._ctx, k=1, s=1) == -4                                         # ... through the forwarded call too
        assert light(empty._ctx, k=3) == -3 and resolve(empty._ctx, s=3) == -3             # a bad argument first
        assert light(empty._ctx, k=2) == -4                                                # ... and K and s before the program
    finally:
        empty.close()
    r = open_renderer(sc, 1)
    try:
        first = frame(torch_cuda, r, 37, 11)
        order = r.tile_order()
        assert light(None) == -3 and resolve(None) == -3                                   # no context
        for call in (light, resolve):
            for bad in (0, 3, 5, 6, 12, 17, 32, -1):
                assert call(r._ctx, k=bad) == -3, ("K", bad)
            for bad in (0, 3, 8, 16, -2):
                assert call(r._ctx, s=bad) == -3, ("s", bad)
            assert call(r._ctx, n=0) == -3 and call(r._ctx, n=-1) == -3 and call(r._ctx, w=0) == -3 and call(r._ctx, h=0) == -3
            assert call(r._ctx, n=4096, k=16, s=4, w=1024, h=1024) == -3                   # N = 2^44
            assert call(r._ctx, n=2 ** 31 - 1, k=16, s=4, w=2 ** 31 - 1, h=2 ** 31 - 1) == -3      # ... beyond 64 bits
            assert call(r._ctx, n=1, k=1, s=1, w=65536, h=65536) == -3                     # N = 2^32
            assert call(r._ctx, id_ptr=0) == -3                                            # no hit_id
            assert call(r._ctx, factors_ptr=0) == -3                                       # no factors, two lights
            assert call(r._ctx, factors_ptr=a["factors_ptr"] + 4) == -3                    # misaligned
            assert call(r._ctx, light_stride=N - 1) == -3 and call(r._ctx, light_stride=s * s * w * h) == -3     # 0 < stride < N
        assert light(r._ctx, cams=None) == -3                                              # no cameras
        assert light(r._ctx, max_steps=-1) == -3
        assert light(r._ctx, out=False) == -3                                              # no lol_gpu_light_passes
        assert resolve(r._ctx, planes=False) == -3 and resolve(r._ctx, out=None) == -3
        assert resolve(r._ctx, out=gpu.Relit(None, None, None)) == -3                      # all three outputs NULL
        assert refusal(lambda: r.relight_views_into(None, n_views, k, w, h, s, **ra)) == (-3, "relight: no output")
        assert refusal(lambda: r.light_views_into(cams + cams[:1], 3, w, h, s, **a)) == (-3, "relit views: cams_per_view must be 1, 2, 4, 8 or 16")
        with pytest.raises(ValueError):
            r.light_views_into(cams[:1], 2, w, h, s, **a)                                  # not a whole number of views
        for what, prog in forbidden_looks(sc):                                             # what a look may not differ in
            try:
                assert refusal(lambda: r.relight_views_into(prog, n_views, k, w, h, s, **ra, **ca)) == (-3, LOOK_TEXT[what]), what
            finally:
                restore(what, prog)
        r.sync()
        torch_cuda.cuda.synchronize()
        assert p.untouched() and c.untouched()
        # the context stays usable: the call that was refused in every way above now passes, and a frame is the frame it was
        assert light(r._ctx) == 0 and resolve(r._ctx) == 0
        r.sync()
        torch_cuda.cuda.synchronize()
        assert not c.untouched()
        second = frame(torch_cuda, r, 37, 11)
        for f in first:
            assert R.same_bits(first[f], second[f]).all(), f
        assert r.tile_order()["mode"] == order["mode"] == "lpt"
    finally:
        r.close()


# --------------------------------------------------------------------------------------------------------------------- 8. streams
def test_streams(torch_cuda, scenes):
    """a torch stream, the context's own (NULL) and LOL_GPU_STREAM_DEFAULT; twenty relights back to back on two streams, more than
    the ring of looks has sets; and the tile order's record is what it was"""
    sc, (w, h), (s, k, n_views) = scenes["scene4"], (37, 11), (2, 2, 3)
    cams = cameras_of(sc, n_views, k)
    looks = [l for _, l in looks_of(sc)]
    r = open_renderer(sc, 1)
    try:
        frame(torch_cuda, r, w, h)
        order = r.tile_order()
        base = capture_views(torch_cuda, r, cams, k, w, h, s)
        want_planes = base.collect()
        wants = [relight_views(torch_cuda, r, l, base, n_views, k, w, h, s) for l in looks]
        for stream in (0, None):
            p = capture_views(torch_cuda, r, cams, k, w, h, s, stream=stream)
            assert_same(p.collect(), want_planes, ("id", "dist", "steps") + FACTORS, f"capture on stream {stream}")
            assert_same(relight_views(torch_cuda, r, looks[0], p, n_views, k, w, h, s, stream=stream), wants[0], RELIT, f"resolve on stream {stream}")
        streams = [torch_cuda.cuda.Stream(), torch_cuda.cuda.Stream()]
        planes = [Planes(torch_cuda, base.n, 2) for _ in streams]
        colours = [[Colours(torch_cuda, n_views * w * h) for _ in range(2 * len(looks))] for _ in streams]
        torch_cuda.cuda.synchronize()
        for st, p in zip(streams, planes):
            r.light_views_into(cams, k, w, h, s, stream=st.cuda_stream, **p.args())
        for i in range(2 * len(looks)):                                      # 2 x 10 resolves, alternating between the streams
            for st, p, cs in zip(streams, planes, colours):
                r.relight_views_into(looks[i % len(looks)], n_views, k, w, h, s, stream=st.cuda_stream, **p.relight_args(), **cs[i].args())
        for st in streams:
            st.synchronize()
        for j, (p, cs) in enumerate(zip(planes, colours)):
            assert_same(p.collect(), want_planes, ("id", "dist", "steps") + FACTORS, f"stream {j} of two")
            for i, c in enumerate(cs):
                assert_same(c.collect(), wants[i % len(looks)], RELIT, f"stream {j} of two, resolve {i}")
        assert r.tile_order() == order
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------------- 9. CLI
def test_averaged_relights_through_the_cli(torch_cuda, scenes, tmp_path, capsys):
    """SCENE.lol --relight LOOK.lol ... with --samples S, and with --lens R --focus D --lens-samples K [--samples S]: the bytes LOOK.lol
    with the same flags and without --relight writes; --adaptive stays refused"""
    w, h = 37, 11
    path = os.path.join(SH.SCENES_DIR, "scene4.lol")
    text = open(path).read()
    a = re.sub(r"diffuse_intensity\s*=\s*\([^)]*\)", "diffuse_intensity = (0.9, 0.3, 0.2)", text)
    b = re.sub(r"specular_intensity\s*=\s*\([^)]*\)", "specular_intensity = (0.1, 0.9, 0.4)", text)
    assert a != text and b != text
    files = []
    for name, t in (("a.lol", a), ("b.lol", b)):
        files.append(str(tmp_path / name))
        with open(files[-1], "w") as f:
            f.write(t)
    plain = str(tmp_path / "plain.ppm")
    assert cli_main([files[0], "--size", f"{w}x{h}", "-o", plain]) == 0
    for j, flags in enumerate((["--samples", "2"], ["--lens", "0.25", "--focus", "6", "--lens-samples", "4"],
                               ["--lens", "0.25", "--focus", "6", "--lens-samples", "2", "--samples", "4"])):
        out = str(tmp_path / f"looks{j}")
        capsys.readouterr()
        assert cli_main([path, "--relight", files[0], files[1], "--size", f"{w}x{h}", "-o", out] + flags) == 0
        assert "relight_views" in capsys.readouterr().out
        for i, f in enumerate(files):
            single = str(tmp_path / f"single{j}_{i}.ppm")
            assert cli_main([f, "--size", f"{w}x{h}", "-o", single] + flags) == 0
            got = open(os.path.join(out, f"look_{i:04d}.ppm"), "rb").read()
            assert got == open(single, "rb").read(), (flags, f)
            assert i or got != open(plain, "rb").read(), flags             # (an averaged frame, not the plain one)
    assert cli_main([path, "--relight", files[0], "--samples", "2", "--adaptive", "16", "--size", f"{w}x{h}", "-o", str(tmp_path / "no")]) == 1
    assert not os.path.exists(str(tmp_path / "no"))
