"""Light passes and relighting on the device: lol_gpu_light_rays / lol_gpu_light_pixels (light_interp) held to tests/light_reference.py,
and lol_gpu_relight (relight_rays) held to the shading queries and frames of contexts that uploaded the look, and to light_reference.relit.

Every comparison is ray_reference.same_bits: equality of bit patterns, two NaNs counting as the same; no tolerance.  The reference of
a ray is computed once per (scene, max_steps) for the whole module.  The settled-shadow exit shortens shadow marches, so shadow_steps
is compared after set_exact_skips(0) alone; every factor either way.
"""
import os
import re

import numpy as np
import pytest

import light_reference as LR
import ray_reference as R
import scene_shapes as C
import shade_reference as SR
from loltracer_amd import gpu
from loltracer_amd import scene as S
from loltracer_amd.__main__ import main as cli_main
from test_gpu_shades import LOSSY, all_pixels, frame, refusal, shade_rays, stream_of
from test_light_reference import looks_of

pytestmark = pytest.mark.gpu

SEED = 20261018
SENTINEL = 0x5A5A5A5A
PAD = 67                                 # elements behind the last element of every plane: more than a wave
MODES = {"default": 1, "interp": 4, "interp-plain": 0}       # lol_gpu_set_specialize
FACTORS = ("shadow", "di", "si")
RELIT = ("rgb_linear", "rgb", "pixel")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_lists = {}


def ray_list(sc):
    """shade_reference.shade_ray_set, and behind it camera rays of larger frames until the reference holds every population the
    hostile looks need: an escaped ray, a hit with di == 0 for some light, one with shadow == 0, one with 0 < shadow < 1"""
    if id(sc) in _lists:
        return _lists[id(sc)][1]
    rays = np.array(SR.shade_ray_set(sc, SEED))
    nl = len(sc.lights())

    def lacking(ref):
        hit = ref["id"] != 0
        have = [(~hit).any()] + ([(ref["di"][hit] == 0).any(), (ref["shadow"][hit] == 0).any(),
                                  ((ref["shadow"][hit] > 0) & (ref["shadow"][hit] < 1)).any()] if nl else [])
        return [k for k, h in enumerate(have) if not h]

    for w, h in ((37, 11), (64, 36), (128, 72)):
        if not lacking(LR.reference(sc, rays)):
            break
        more = R.camera_rays(sc, w, h)
        ref = LR.reference(sc, more)
        hit = ref["id"] != 0
        partial = hit & ((ref["shadow"] > 0) & (ref["shadow"] < 1)).any(axis=1)
        dark = hit & (ref["shadow"] == 0).any(axis=1)
        back = hit & (ref["di"] == 0).any(axis=1)
        pick = np.concatenate([np.flatnonzero(m)[:5] for m in (partial, dark, back, ~hit)])
        rays = np.concatenate([rays, more[pick]])
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    assert not lacking(LR.reference(sc, rays)), "the list lacks a population the hostile looks need"
    rays.setflags(write=False)
    _lists[id(sc)] = (sc, rays)
    return rays


class Planes:
    """the planes of a capture of n rays under nl lights, SENTINEL everywhere before the call: factors [nl * stride + PAD] x 16 bytes,
    id / dist / steps [n + PAD]"""

    def __init__(self, torch, n, nl, stride=0, optional=True):
        dev = torch.device("cuda:0")
        self.n, self.nl, self.stride = n, nl, stride
        s = stride or n
        self.factors = torch.full(((nl * s + PAD) * 4,), SENTINEL, dtype=torch.int32, device=dev) if nl else None
        self.t = {f: torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=dev) for f in (("id", "dist", "steps") if optional else ("id",))}

    def args(self):
        return dict(factors_ptr=self.factors.data_ptr() if self.factors is not None else 0, light_stride=self.stride,
                    **{f + "_ptr": (self.t[f].data_ptr() if f in self.t else 0) for f in ("id", "dist", "steps")})

    def relight_args(self):
        a = self.args()
        return dict(factors_ptr=a["factors_ptr"], id_ptr=a["id_ptr"], light_stride=self.stride)

    def collect(self):
        """dict(shadow, di, si [n, nl] f32, shadow_steps [n, nl] u32, id, dist, steps); asserts that nothing behind element n - 1 of
        any plane, and nothing in the gap between two lights' planes, was written"""
        n, nl, s = self.n, self.nl, self.stride or self.n
        out = {}
        for f, t in self.t.items():
            a = t.cpu().numpy().view(np.uint32)
            assert (a[n:] == SENTINEL).all(), f"{f}: written beyond element n - 1"
            out[f] = a[:n].view(np.float32) if f == "dist" else a[:n]
        if nl:
            a = self.factors.cpu().numpy().view(np.uint32).reshape(-1, 4)
            for l in range(nl):
                assert (a[l * s + n:(l + 1) * s] == SENTINEL).all(), f"light {l}: the gap behind its plane was written"
            assert (a[nl * s:] == SENTINEL).all(), "written behind the last plane"
            body = np.stack([a[l * s:l * s + n] for l in range(nl)], axis=1)            # [n, nl, 4]
            for k, f in enumerate(FACTORS):
                out[f] = np.ascontiguousarray(body[:, :, k]).view(np.float32)
            out["shadow_steps"] = np.ascontiguousarray(body[:, :, 3])
        return out

    def untouched(self):
        ts = list(self.t.values()) + ([self.factors] if self.factors is not None else [])
        return all((t.cpu().numpy().view(np.uint32) == SENTINEL).all() for t in ts)


class Colours:
    """the three outputs of a relight of n elements, each with PAD elements of SENTINEL behind"""

    def __init__(self, torch, n, want=RELIT):
        dev = torch.device("cuda:0")
        self.n = n
        self.t = {f: torch.full(((n + PAD) * (1 if f == "pixel" else 3),), SENTINEL, dtype=torch.int32, device=dev) for f in want}

    def args(self):
        return {f + "_ptr": (self.t[f].data_ptr() if f in self.t else 0) for f in RELIT}

    def collect(self):
        out = {}
        for f, t in self.t.items():
            a = t.cpu().numpy().view(np.uint32)
            k = 1 if f == "pixel" else 3
            assert (a[self.n * k:] == SENTINEL).all(), f"{f}: written beyond element n - 1"
            out[f] = a[:self.n * k] if f == "pixel" else a[:self.n * k].view(np.float32).reshape(-1, 3)
        return out

    def untouched(self):
        return all((t.cpu().numpy().view(np.uint32) == SENTINEL).all() for t in self.t.values())


def capture(torch, r, rays, n=None, stride=0, max_steps=256, stream="torch"):
    """(planes, what they hold) of the first n rays through lol_gpu_light_rays; the ray buffer must come back as it went"""
    n = len(rays) if n is None else n
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
    p = Planes(torch, n, len(r.scene.lights()), stride)
    torch.cuda.synchronize()
    r.light_rays_into(d_rays.data_ptr(), n, max_steps, stream=stream_of(torch, stream), **p.args())
    r.sync()
    torch.cuda.synchronize()
    assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), np.ascontiguousarray(rays).view(np.uint32)), "the ray buffer was written"
    return p, p.collect()


def capture_pixels(torch, r, w, h, xy=None, camera=None, max_steps=256):
    n = w * h if xy is None else len(xy)
    d_xy = None if xy is None else torch.from_numpy(np.ascontiguousarray(xy, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")
    p = Planes(torch, n, len(r.scene.lights()))
    torch.cuda.synchronize()
    r.light_pixels_into(n, w, h, max_steps, xy_ptr=0 if d_xy is None else d_xy.data_ptr(), camera=camera,
                        stream=torch.cuda.current_stream().cuda_stream, **p.args())
    r.sync()
    torch.cuda.synchronize()
    return p, p.collect()


def relight(torch, r, look, p, want=RELIT, stream="torch"):
    c = Colours(torch, p.n, want)
    torch.cuda.synchronize()
    r.relight_into(look, p.n, stream=stream_of(torch, stream), **p.relight_args(), **c.args())
    r.sync()
    torch.cuda.synchronize()
    return c.collect()


def assert_same(got, want, fields, what):
    for f in fields:
        ok = R.same_bits(got[f], want[f])
        if not ok.all():
            i = int(np.flatnonzero(~ok.reshape(len(ok), -1).all(axis=1))[0])
            raise AssertionError(f"{what}: {f} differs for {int((~ok.reshape(len(ok), -1).all(axis=1)).sum())} elements; first: [{i}] = {got[f][i]!r}, expected {want[f][i]!r}")


def assert_factors(got, ref, n, what, exact):
    want = {f: ref[f][:n] for f in ref}
    fields = ("id", "dist", "steps") + ((FACTORS + (("shadow_steps",) if exact else ())) if ref["shadow"].shape[1] else ())
    assert_same(got, want, fields, what)


def open_renderer(sc, specialize):
    r = gpu.Renderer(0, specialize=specialize)
    try:
        r.prepare(sc)
    except BaseException:
        r.close()
        raise
    return r


# ---------------------------------------------------------------------------------------------------------------- 1. the factors
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_factors_are_the_reference(torch_cuda, scenes, name, mode):
    sc = scenes[name]
    rays = ray_list(sc)
    ref = LR.reference(sc, rays)
    r = open_renderer(sc, MODES[mode])
    try:
        assert r.miss_skip_active() == 7                        # the context's skips are on: the capture must not take the first two
        for exact in (False, True):
            r.set_exact_skips(0 if exact else 7)
            for n in (1, 63, 64, 65, len(rays)):
                for stride in (0, n + 7):
                    _, got = capture(torch_cuda, r, rays, n, stride)
                    assert_factors(got, ref, n, f"{name} {mode} exact={exact} n={n} stride={stride}", exact)
        r.set_exact_skips(7)
        perm = np.random.default_rng(SEED + 1).permutation(len(rays))
        _, got = capture(torch_cuda, r, rays[perm])
        assert_factors(got, {f: ref[f][perm] for f in ref}, len(rays), f"{name} {mode} permuted", False)
    finally:
        r.close()


def test_max_steps_and_optional_planes(torch_cuda, scenes):
    sc = scenes["scene4"]
    rays = ray_list(sc)[:130]
    r = open_renderer(sc, 1)
    try:
        r.set_exact_skips(0)
        for max_steps in (0, 1, 7):
            _, got = capture(torch_cuda, r, rays, max_steps=max_steps)
            assert_factors(got, LR.reference(sc, rays, max_steps), len(rays), f"max_steps={max_steps}", True)
        # hit_dist and march_steps are optional: without them the others are what they were
        d_rays = torch_cuda.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
        p = Planes(torch_cuda, 65, 2, optional=False)
        r.light_rays_into(d_rays.data_ptr(), 65, stream=torch_cuda.cuda.current_stream().cuda_stream, **p.args())
        r.sync()
        torch_cuda.cuda.synchronize()
        got = p.collect()
        want = LR.reference(sc, rays)
        assert_same(got, {f: want[f][:65] for f in want}, ("id",) + FACTORS + ("shadow_steps",), "id and factors alone")
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the identity
@pytest.mark.parametrize("mode", ["default", "interp"])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_relight_without_a_look_is_the_shading_query(torch_cuda, scenes, name, mode):
    sc = scenes[name]
    rays = ray_list(sc)
    r = open_renderer(sc, MODES[mode])
    try:
        for fmt in (None, LOSSY):
            r.set_pixel_format(fmt)
            for stride in (0, len(rays) + 7):
                p, _ = capture(torch_cuda, r, rays, stride=stride)
                got = relight(torch_cuda, r, None, p)
                want = shade_rays(torch_cuda, r, rays, want=RELIT)
                assert_same(got, want, RELIT, f"{name} {mode} fmt={'lossy' if fmt else 'xrgb'} stride={stride}")
        # ... and each output alone is its column
        for f in RELIT:
            alone = relight(torch_cuda, r, None, p, want=(f,))
            assert set(alone) == {f}
            assert_same(alone, got, (f,), f"{f} alone")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------- 3. the looks
@pytest.mark.parametrize("k", range(5), ids=lambda k: "abcde"[k])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_looks(torch_cuda, scenes, name, k):
    """relight(look) over planes captured under the scene IS the shading query of a context that uploaded the look, and
    light_reference.relit of the reference's factors"""
    sc = scenes[name]
    rays = ray_list(sc)
    what, look = looks_of(sc)[k]
    r, r2 = open_renderer(sc, 1), open_renderer(look, 1)
    try:
        p, got_f = capture(torch_cuda, r, rays)
        got = relight(torch_cuda, r, look, p)
        assert_same(got, shade_rays(torch_cuda, r2, rays, want=RELIT), RELIT, f"{name} {what}: against a context that uploaded the look")
        assert_same(got, LR.relit_reference(LR.reference(sc, rays), look), RELIT, f"{name} {what}: against light_reference.relit")
        # a ready Program is taken as a Scene is, and the capturing context's own colours are what they were
        again = relight(torch_cuda, r, look.flatten(), p, want=("pixel",))
        assert_same(again, got, ("pixel",), "a Program for a look")
        assert_same(relight(torch_cuda, r, None, p), shade_rays(torch_cuda, r, rays, want=RELIT), RELIT, "the own look after another")
    finally:
        r2.close()
        r.close()


# -------------------------------------------------------------------------------------------------------------- 4. all the pixels
@pytest.mark.parametrize("mode", ["default", "interp"])
@pytest.mark.parametrize("w,h", [(13, 5), (37, 11)])
def test_all_pixels_are_the_frame(torch_cuda, scenes, w, h, mode):
    sc = scenes["scene4"]
    what, look = looks_of(sc)[0]
    r, r2 = open_renderer(sc, MODES[mode]), open_renderer(look, MODES[mode])
    try:
        p, got = capture_pixels(torch_cuda, r, w, h)
        own = frame(torch_cuda, r, w, h)
        assert_same(dict(id=got["id"], dist=got["dist"], steps=got["steps"]), dict(own, steps=own["steps"] & 0xFFFF), ("id", "dist", "steps"),
                    f"{w}x{h} {mode}: the planes against the frame's")
        ref = LR.reference(sc, R.camera_rays(sc, w, h))
        assert_factors(got, ref, w * h, f"{w}x{h} {mode}: the factors", False)
        assert_same(relight(torch_cuda, r, None, p, want=("rgb", "pixel")), own, ("rgb", "pixel"), f"{w}x{h} {mode}: the own frame")
        assert_same(relight(torch_cuda, r, look, p, want=("rgb", "pixel")), frame(torch_cuda, r2, w, h), ("rgb", "pixel"),
                    f"{w}x{h} {mode}: the frame of look {what}")
        # the list of all pixels is the form without a list
        _, listed = capture_pixels(torch_cuda, r, w, h, xy=all_pixels(w, h))
        assert_same(listed, got, ("id", "dist", "steps") + FACTORS, f"{w}x{h} {mode}: a list of every pixel")
        some = all_pixels(w, h)[::3][:66]
        _, part = capture_pixels(torch_cuda, r, w, h, xy=some)
        idx = some[:, 1].astype(np.int64) * w + some[:, 0]
        assert_same(part, {f: got[f][idx] for f in got}, ("id", "dist", "steps") + FACTORS, f"{w}x{h} {mode}: a list of some pixels")
    finally:
        r2.close()
        r.close()


# -------------------------------------------------------------------------------------------------- 5. light counts, large tables
def scene_with_lights(n):
    return next(sc for sc in C.fuzz_scenes() if len(sc.lights()) == n)


@pytest.mark.parametrize("case", ["no-lights", "three-lights", "tree2-tables"])
def test_light_counts_and_large_tables(torch_cuda, case):
    sc = C.scene_of(C.RUNG["tree2-tables"]) if case == "tree2-tables" else scene_with_lights(0 if case == "no-lights" else 3)
    nl, nm = len(sc.lights()), len(sc.materials())
    rays = R.ray_set(sc, SEED, "ae")
    ref = LR.reference(sc, rays)
    look = sc.with_look(lights=[((.2, .9, .4), (.7, .1, .5))] * nl, materials=[((.1, .2, .3), (.3, .2, .1), (.4, .4, .1))] * nm, ambient=(.6, .5, .4))
    r, r2 = open_renderer(sc, 1), open_renderer(look, 1)
    try:
        assert r.interp_variant()[1] == (case == "tree2-tables")        # the tables read from global memory, or staged
        r.set_exact_skips(0)
        p, got = capture(torch_cuda, r, rays, stride=len(rays) + 7)
        assert (p.factors is None) == (nl == 0)
        assert_factors(got, ref, len(rays), case, True)
        assert_same(relight(torch_cuda, r, None, p), shade_rays(torch_cuda, r, rays, want=RELIT), RELIT, f"{case}: the own look")
        got = relight(torch_cuda, r, look, p)
        assert_same(got, shade_rays(torch_cuda, r2, rays, want=RELIT), RELIT, f"{case}: a look")
        assert_same(got, LR.relit_reference(ref, look), RELIT, f"{case}: a look against relit")
    finally:
        r2.close()
        r.close()


# ------------------------------------------------------------------------------------------------------------ 6. degenerate scenes
@pytest.mark.parametrize("mode", ["default", "interp"])
@pytest.mark.parametrize("name", C.DEGENERATE_NAMES)
def test_degenerate_scenes(torch_cuda, name, mode):
    sc = C.degenerate_scenes()[C.DEGENERATE_NAMES.index(name)]
    w, h = 13, 7
    rays = R.camera_rays(sc, w, h)
    ref = LR.reference(sc, rays)
    r = open_renderer(sc, MODES[mode])
    try:
        for exact in (False, True):
            r.set_exact_skips(0 if exact else 7)
            for n, stride in ((65, 0), (len(rays), len(rays) + 7)):
                p, got = capture(torch_cuda, r, rays, n, stride)
                assert_factors(got, ref, n, f"{name} {mode} exact={exact} n={n}", exact)
            assert_same(relight(torch_cuda, r, None, p), shade_rays(torch_cuda, r, rays, want=RELIT), RELIT, f"{name} {mode} exact={exact}: identity")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------- 7. refusals
# what lol_gpu_error() says after each refusal of test_refusals: the text is part of what a host sees
REFUSAL_TEXT = {
    "no program": "no scene program uploaded",
    "no list": "light passes: no list",
    "max_steps or n": "light passes: max_steps < 0 or more than 2^32 - 1 rays",
    "geometry": "light passes: no camera or bad frame geometry",
    "not all pixels": "light passes: no list of pixels, and n is not w * h",
    "no hit_id": "light passes: no hit_id plane",
    "no factors": "light passes: no factors, and the program has lights",
    "misaligned": "light passes: factors must be 16-byte aligned",
    "stride": "light passes: light_stride is neither 0 nor at least n",
    "relight: no output": "relight: no output",
    "relight: n": "relight: more than 2^32 - 1 elements",
}
# ... and after each look of forbidden_looks, by its name there
LOOK_TEXT = {
    "f[]": "relight: the look differs from the uploaded program in an op (opcode, id or a number): capture again",
    "light point": "relight: the look moves a light: capture again",
    "shininess": "relight: the look changes a shininess: capture again",
    "root_material": "relight: the look gives an object another material: capture again",
    "a count": "relight: the look differs from the uploaded program in a count (ops, lights, materials, roots, max_stack)",
    "NULL materials": "relight: malformed look: a table is missing",
    "root_material out of range": "relight: material index out of range in the look",
}


def test_refusals(torch_cuda, scenes):
    """every line of the header's list, with nothing written; the status, the text of lol_gpu_error() and the ORDER of the refusals"""
    sc = scenes["scene4"]
    rays = ray_list(sc)[:64]
    d_rays = torch_cuda.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
    d_xy = torch_cuda.zeros(128, dtype=torch_cuda.int32, device="cuda:0")
    p, c = Planes(torch_cuda, 64, 2), Colours(torch_cuda, 64)
    a, ra, ca = p.args(), p.relight_args(), c.args()
    lib = gpu.gpu_lib()
    fc = sc.frame_camera(8, 8)
    T = REFUSAL_TEXT
    torch_cuda.cuda.synchronize()

    def passes(**kw):
        v = dict(a, **kw)
        return gpu.LightPasses(v["factors_ptr"] or None, v["light_stride"], v["id_ptr"] or None, v["dist_ptr"] or None, v["steps_ptr"] or None)

    relit = gpu.Relit(*(ca[f + "_ptr"] for f in RELIT))
    empty = gpu.Renderer(0)
    try:
        assert refusal(lambda: empty.light_rays_into(d_rays.data_ptr(), 64, **a)) == (-4, T["no program"])
        assert refusal(lambda: empty.light_rays_into(d_rays.data_ptr(), 64, -1, **a)) == (-3, T["max_steps or n"])        # a bad argument first
        assert lib.lol_gpu_light_pixels(empty._ctx, fc, 8, 8, 256, None, 64, passes(), None) == -4
        assert lib.lol_gpu_relight(empty._ctx, None, passes(), 64, relit, None) == -4
        # the order, without a program: a list of pixels asks for the program BEFORE the camera and the frame's geometry
        assert lib.lol_gpu_light_pixels(empty._ctx, fc, 0, 8, 256, d_xy.data_ptr(), 64, passes(), None) == -4
        assert lib.lol_gpu_light_pixels(empty._ctx, None, 8, 8, 256, d_xy.data_ptr(), 64, passes(), None) == -4
        assert lib.lol_gpu_light_pixels(empty._ctx, fc, 8, 8, -1, d_xy.data_ptr(), 64, passes(), None) == -3
        assert lib.lol_gpu_light_rays(empty._ctx, d_rays.data_ptr(), 64, -1, passes(), None) == -3
    finally:
        empty.close()
    r = open_renderer(sc, 1)
    try:
        assert lib.lol_gpu_light_rays(None, d_rays.data_ptr(), 64, 256, passes(), None) == -3            # no context
        assert lib.lol_gpu_light_pixels(None, fc, 8, 8, 256, None, 64, passes(), None) == -3
        assert lib.lol_gpu_relight(None, None, passes(), 64, relit, None) == -3
        assert refusal(lambda: r.light_rays_into(0, 64, **a)) == (-3, T["no list"])                                       # no rays
        assert lib.lol_gpu_light_rays(r._ctx, d_rays.data_ptr(), 64, 256, None, None) == -3              # no lol_gpu_light_passes
        assert lib.lol_gpu_relight(r._ctx, None, None, 64, relit, None) == -3
        assert lib.lol_gpu_relight(r._ctx, None, passes(), 64, None, None) == -3                         # no lol_gpu_relit
        assert refusal(lambda: r.light_rays_into(d_rays.data_ptr(), 64, **dict(a, id_ptr=0))) == (-3, T["no hit_id"])     # no hit_id
        assert refusal(lambda: r.relight_into(None, 64, **dict(ra, id_ptr=0), **ca)) == (-3, T["no hit_id"])
        assert refusal(lambda: r.light_rays_into(d_rays.data_ptr(), 64, **dict(a, factors_ptr=0))) == (-3, T["no factors"])       # no factors, two lights
        assert refusal(lambda: r.relight_into(None, 64, **dict(ra, factors_ptr=0), **ca)) == (-3, T["no factors"])
        assert refusal(lambda: r.light_rays_into(d_rays.data_ptr(), 64, **dict(a, factors_ptr=a["factors_ptr"] + 4))) == (-3, T["misaligned"])
        assert refusal(lambda: r.light_rays_into(d_rays.data_ptr(), 64, **dict(a, light_stride=63))) == (-3, T["stride"])
        assert refusal(lambda: r.relight_into(None, 64, **dict(ra, light_stride=63), **ca)) == (-3, T["stride"])
        assert refusal(lambda: r.relight_into(None, 64, **ra)) == (-3, T["relight: no output"])                           # all three outputs NULL
        assert refusal(lambda: r.light_rays_into(d_rays.data_ptr(), 64, -1, **a)) == (-3, T["max_steps or n"])            # max_steps < 0
        assert refusal(lambda: r.light_rays_into(d_rays.data_ptr(), 1 << 32, **a)) == (-3, T["max_steps or n"])           # n > 2^32 - 1
        assert refusal(lambda: r.relight_into(None, 1 << 32, **ra, **ca)) == (-3, T["relight: n"])
        assert refusal(lambda: r.light_pixels_into(64, 0, 8, frame_camera=fc, xy_ptr=d_xy.data_ptr(), **a)) == (-3, T["geometry"])
        assert refusal(lambda: r.light_pixels_into(64, 8, 0, frame_camera=fc, xy_ptr=d_xy.data_ptr(), **a)) == (-3, T["geometry"])
        assert refusal(lambda: r.light_pixels_into(64, 8, 8, -1, xy_ptr=d_xy.data_ptr(), **a)) == (-3, T["max_steps or n"])
        assert lib.lol_gpu_light_pixels(r._ctx, None, 8, 8, 256, d_xy.data_ptr(), 64, passes(), None) == -3      # no camera
        assert lib.lol_gpu_light_pixels(r._ctx, None, 8, 8, 256, d_xy.data_ptr(), 0, passes(), None) == -3       # ... with n = 0 too
        assert refusal(lambda: r.light_pixels_into(63, 8, 8, **a)) == (-3, T["not all pixels"])                           # no list, and n != w h
        # n = 0: fine, with no list at all, and nothing launched
        r.light_rays_into(0, 0, **a)
        r.light_pixels_into(0, 8, 8, xy_ptr=d_xy.data_ptr(), **a)
        r.relight_into(None, 0, **ra, **ca)
        r.sync()
        torch_cuda.cuda.synchronize()
        assert p.untouched() and c.untouched()
        assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), rays.view(np.uint32))
    finally:
        r.close()


def forbidden_looks(sc):
    """(what, program) pairs: the scene with ONE thing changed that a look may not change"""
    def changed(edit):
        c = sc.clone()
        edit(c.c)
        return c

    def first_sphere(c):
        return next(c.nodes[i] for i in range(c.n_nodes) if c.nodes[i].type == S.NODE_SPHERE)

    root = sc.roots()[0]
    out = [("f[]", changed(lambda c: setattr(first_sphere(c), "radius", first_sphere(c).radius * 1.5)).flatten()),
           ("light point", changed(lambda c: setattr(c.lights[0].point, "x", c.lights[0].point.x + 1)).flatten()),
           ("shininess", changed(lambda c: setattr(c.materials[1], "shininess", c.materials[1].shininess + 1)).flatten()),
           ("root_material", changed(lambda c: setattr(c.nodes[root], "material", (c.nodes[root].material + 1) % c.n_materials)).flatten())]
    fewer = sc.flatten()
    fewer.n_lights -= 1                                       # a count (the tables are the scene's own: nothing beyond them is named)
    out.append(("a count", fewer))
    no_table = sc.flatten()
    keep = no_table.materials
    no_table.materials = type(keep)()                         # a NULL table that a count speaks of
    no_table._keep = keep
    out.append(("NULL materials", no_table))
    wild = sc.flatten()
    wild.root_material[0] = wild.n_materials                  # a root_material out of range
    out.append(("root_material out of range", wild))
    return out


def restore(what, prog):
    if what == "NULL materials":
        prog.materials = prog._keep                           # (so that lol_program_free releases what flatten allocated)


@pytest.mark.parametrize("mode", ["default", "interp"])
def test_forbidden_looks_and_the_frame_after(torch_cuda, scenes, mode):
    """each look that differs in one forbidden thing is refused with nothing written, the context stays usable, and a frame after the
    three calls is the frame it would have been"""
    sc, (w, h) = scenes["scene4"], (37, 11)
    rays = ray_list(sc)[:130]
    r, alone = open_renderer(sc, MODES[mode]), open_renderer(sc, MODES[mode])
    try:
        assert r.tile_order()["mode"] == "lpt"
        first = frame(torch_cuda, r, w, h)
        p, _ = capture(torch_cuda, r, rays)
        want = relight(torch_cuda, r, None, p)
        c = Colours(torch_cuda, p.n)
        for what, prog in forbidden_looks(sc):
            try:
                assert refusal(lambda: r.relight_into(prog, p.n, **p.relight_args(), **c.args())) == (-3, LOOK_TEXT[what]), what
            finally:
                restore(what, prog)
            r.sync()
            assert c.untouched(), what
            assert_same(relight(torch_cuda, r, None, p), want, RELIT, f"after the refused look ({what})")
        pp, _ = capture_pixels(torch_cuda, r, w, h)
        relit = relight(torch_cuda, r, looks_of(sc)[1][1], pp)
        assert not np.array_equal(relit["pixel"], first["pixel"])
        second = frame(torch_cuda, r, w, h)
        for f in first:
            assert R.same_bits(first[f], second[f]).all(), f
        for _ in range(2):
            other = frame(torch_cuda, alone, w, h)
        assert np.array_equal(other["pixel"], second["pixel"]) and np.array_equal(other["steps"], second["steps"])
        assert r.tile_order()["mode"] == alone.tile_order()["mode"] == "lpt"
    finally:
        alone.close()
        r.close()


# --------------------------------------------------------------------------------------------------------------------- 8. streams
def test_streams(torch_cuda, scenes):
    """LOL_GPU_STREAM_DEFAULT, the context's own (NULL), and two torch streams with a capture and relights in flight on each: more
    relights in flight than the ring of looks has sets"""
    sc = scenes["scene4"]
    rays = ray_list(sc)
    ref = LR.reference(sc, rays)
    looks = [l for _, l in looks_of(sc)]
    wants = [LR.relit_reference(ref, l) for l in looks]
    r = open_renderer(sc, 1)
    try:
        for stream in (0, None):
            p, got = capture(torch_cuda, r, rays, stream=stream)
            assert_factors(got, ref, len(rays), f"stream {stream}", False)
            assert_same(relight(torch_cuda, r, looks[0], p, stream=stream), wants[0], RELIT, f"relight on stream {stream}")
        d_rays = torch_cuda.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
        streams = [torch_cuda.cuda.Stream(), torch_cuda.cuda.Stream()]
        planes = [Planes(torch_cuda, len(rays), 2) for _ in streams]
        colours = [[Colours(torch_cuda, len(rays)) for _ in range(2 * len(looks))] for _ in streams]
        torch_cuda.cuda.synchronize()
        for s, p in zip(streams, planes):
            r.light_rays_into(d_rays.data_ptr(), len(rays), stream=s.cuda_stream, **p.args())
        for k in range(2 * len(looks)):                                      # 2 x 10 relights, alternating between the streams
            for s, p, cs in zip(streams, planes, colours):
                r.relight_into(looks[k % len(looks)], len(rays), stream=s.cuda_stream, **p.relight_args(), **cs[k].args())
        for s in streams:
            s.synchronize()
        for j, (p, cs) in enumerate(zip(planes, colours)):
            assert_factors(p.collect(), ref, len(rays), f"stream {j} of two", False)
            for k, c in enumerate(cs):
                assert_same(c.collect(), wants[k % len(looks)], RELIT, f"stream {j} of two, relight {k}")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------------- 9. CLI
def test_relight_through_the_cli(torch_cuda, scenes, tmp_path, capsys):
    """python -m loltracer_amd scene4.lol --relight A.lol B.lol -o DIR: the bytes of rendering each look's scene; a look whose
    geometry differs is refused with its first difference"""
    w, h = 37, 11
    path = os.path.join(C.SCENES_DIR, "scene4.lol")
    text = open(path).read()
    # two looks as files — other diffuse intensities, other specular intensities — and a scene that is no look: a sphere has grown
    a = re.sub(r"diffuse_intensity\s*=\s*\([^)]*\)", "diffuse_intensity = (0.9, 0.3, 0.2)", text)
    b = re.sub(r"specular_intensity\s*=\s*\([^)]*\)", "specular_intensity = (0.1, 0.9, 0.4)", text)
    moved = re.sub(r"radius\s*=\s*[0-9.]+", "radius = 0.77", text, count=1)
    assert a != text and b != text and moved != text
    files = []
    for name, t in (("a.lol", a), ("b.lol", b), ("moved.lol", moved)):
        files.append(str(tmp_path / name))
        with open(files[-1], "w") as f:
            f.write(t)
    out = str(tmp_path / "looks")
    assert cli_main([path, "--relight", files[0], files[1], "--size", f"{w}x{h}", "-o", out]) == 0
    assert "light_interp" in capsys.readouterr().out
    for i, f in enumerate(files[:2]):
        single = str(tmp_path / f"single{i}.ppm")
        assert cli_main([f, "--size", f"{w}x{h}", "-o", single]) == 0
        assert open(os.path.join(out, f"look_{i:04d}.ppm"), "rb").read() == open(single, "rb").read(), f
    capsys.readouterr()
    assert cli_main([path, "--relight", files[0], files[2], "--size", f"{w}x{h}", "-o", str(tmp_path / "refused")]) == 1
    err = capsys.readouterr().err
    assert "moved.lol" in err and "differs in a number" in err and not os.path.exists(str(tmp_path / "refused"))
    assert cli_main([path, "--relight", files[0], "--size", f"{w}x{h}"]) == 1                # no -o: nowhere to write
