"""Shading queries on the device: lol_gpu_shade_rays and lol_gpu_shade_pixels, on the scene kernel (lol_shade_spec) and on the
interpreter (shade_interp), held to tests/shade_reference.py (arbitrary rays) and to the pixels and debug planes of a frame (pixels).

Every comparison is ray_reference.same_bits: equality of bit patterns, two NaNs counting as the same; no tolerance.  The reference of
a ray is computed once per (scene, max_steps) for the whole module, whatever list the ray comes in.  With the exact skips on
(the default) the shadow steps really marched are fewer than the reference's, so the high half of `steps` is compared with all skips
off alone; everything else either way.
"""
import os

import numpy as np
import pytest

import aa_reference as A
import oracle_lib as O
import ray_reference as R
import scene_shapes as C
import shade_reference as SR
import test_gpu_views as V
from loltracer_amd import gpu
from loltracer_amd import scene as S
from loltracer_amd.__main__ import main as cli_main
from test_gpu_families import FORMS, INTERP
from test_gpu_hostile import tie_cameras

pytestmark = pytest.mark.gpu

SEED = 20261018
SENTINEL = 0x5A5A5A5A                    # what every output holds before a query (as a float: 1.5e16, no answer of any ray here)
PAD = 67                                 # elements behind element n - 1 of every output: more than a wave
FIELDS = SR.FIELDS
WIDE = ("rgb_linear", "rgb")             # three floats per ray
FLOATS = WIDE + ("dist",)
MODES = {"spec": 1, "interp": 4, "interp-plain": 0, "spec-plain": 3}           # lol_gpu_set_specialize
SHADE = {1: "lol_shade_spec", 3: "lol_shade_spec", 4: "shade_interp", 0: "shade_interp"}
FRAME = {1: "lol_render_spec", 3: "lol_render_spec", 4: "render_interp", 0: "render_interp"}
LOSSY = gpu.PixelFormat(11, 5, 0, 3, 2, 3, 4, 0, 0xFF000000)                   # channels that lose bits, and an alpha mask
ids = lambda t: t.id                     # noqa: E731


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def open_renderer(sc, specialize, queries=True, wait=True):
    r = gpu.Renderer(0, specialize=specialize)
    try:
        r.set_shade_queries(queries)
        assert r.shade_queries == bool(queries)
        r.prepare(sc, wait=wait)
        if wait:
            assert r.shade_kernel_name() == (SHADE[specialize] if queries else "shade_interp"), r.specialize_log()
            assert r.kernel_name() == FRAME[specialize], r.specialize_log()
    except BaseException:
        r.close()
        raise
    return r


class Outputs:
    """the six outputs of a query of n rays, each n + PAD elements of SENTINEL on the device, or absent"""

    def __init__(self, torch, n, want=FIELDS):
        dev = torch.device("cuda:0")
        self.n, self.t = n, {}
        for f in want:
            self.t[f] = torch.full(((n + PAD) * (3 if f in WIDE else 1),), SENTINEL, dtype=torch.int32, device=dev)

    def ptrs(self):
        return {f + "_ptr": (self.t[f].data_ptr() if f in self.t else 0) for f in FIELDS}

    def collect(self):
        """{field: the first n elements}; asserts that nothing behind them was written"""
        out = {}
        for f, t in self.t.items():
            a = t.cpu().numpy().view(np.uint32)
            k = 3 if f in WIDE else 1
            assert (a[self.n * k:] == SENTINEL).all(), f"{f}: written beyond element n - 1"
            a = a[:self.n * k]
            out[f] = a.view(np.float32).reshape(-1, 3) if f in WIDE else a.view(np.float32) if f == "dist" else a
        return out

    def untouched(self):
        return all((t.cpu().numpy().view(np.uint32) == SENTINEL).all() for t in self.t.values())


def stream_of(torch, stream):
    return torch.cuda.current_stream().cuda_stream if stream == "torch" else stream


def shade_rays(torch, r, rays, n=None, max_steps=256, want=FIELDS, stream="torch"):
    """the first n rays of `rays` through lol_gpu_shade_rays; the ray buffer must come back as it went"""
    n = len(rays) if n is None else n
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
    out = Outputs(torch, n, want)
    torch.cuda.synchronize()
    r.shade_rays_into(d_rays.data_ptr(), n, max_steps, stream=stream_of(torch, stream), **out.ptrs())
    r.sync()
    torch.cuda.synchronize()
    assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), np.ascontiguousarray(rays).view(np.uint32)), "the ray buffer was written"
    return out.collect()


def shade_pixels(torch, r, xy, w, h, camera=None, max_steps=256, want=FIELDS, stream="torch"):
    xy = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
    d_xy = torch.from_numpy(xy.view(np.int32).copy()).to("cuda:0")
    out = Outputs(torch, len(xy), want)
    torch.cuda.synchronize()
    r.shade_pixels_into(d_xy.data_ptr(), len(xy), w, h, max_steps, camera=camera, stream=stream_of(torch, stream), **out.ptrs())
    r.sync()
    torch.cuda.synchronize()
    assert np.array_equal(d_xy.cpu().numpy().view(np.uint32), xy), "the pixel list was written"
    return out.collect()


def assert_is_reference(got, want, what, rays=None, march_steps_only=False):
    bad = SR.differing(got, want, fields=tuple(got), march_steps_only=march_steps_only)
    if bad:
        f, i = bad[0]
        ray = "" if rays is None else f" ray {rays[i].tolist()}"
        g, w = (hex(int(v[f][i])) if f in ("pixel", "steps") else repr(v[f][i]) for v in (got, want))
        raise AssertionError(f"{what}: {len(bad)} (field, ray) pairs differ; first: {f}[{i}] = {g}, reference {w}{ray}")


def take(ref, idx, fields=FIELDS):
    return {f: ref[f][idx] for f in fields}


def all_pixels(w, h):
    return np.array([(x, y) for y in range(h) for x in range(w)], np.uint32)


def both_ways(torch, r, rays, want, what, **kw):
    """all six outputs with every skip off, everything but the shadow steps with the default skips"""
    r.set_miss_skip(False)
    assert r.miss_skip_active() == 0
    assert_is_reference(shade_rays(torch, r, rays, **kw), want, what + ", skips off", rays)
    r.set_miss_skip(True)
    assert_is_reference(shade_rays(torch, r, rays, **kw), want, what + ", default skips", rays, march_steps_only=True)


# ------------------------------------------------------------------------------------------------ lists of arbitrary rays
@pytest.mark.parametrize("mode", ["spec", "interp", "interp-plain", "spec-plain"])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_ray_set(torch_cuda, scenes, name, mode):
    """every kind of ray of shade_ray_set — the specials among ordinary rays, a wave of escaped rays alone, a wave that mixes escaped
    rays and hits — and the same list in a seeded permutation: a ray's answer does not depend on its wave-mates"""
    sc = scenes[name]
    rays = SR.shade_ray_set(sc, SEED)
    want = SR.reference(sc, rays)
    assert 0 < int((want["id"] == 0).sum()) < len(rays) and np.isinf(want["dist"]).any()
    assert (want["shadow"][want["id"] != 0] == 0).any() and (want["shadow"][want["id"] != 0] == 1).any()
    r = open_renderer(sc, MODES[mode])
    try:
        assert r.miss_skip_active() == 7                                    # both scenes qualify for every exact skip
        both_ways(torch_cuda, r, rays, take(want, slice(None)), f"{name} {mode}")
        perm = np.random.default_rng(SEED + 1).permutation(len(rays))
        got = shade_rays(torch_cuda, r, rays[perm])
        assert_is_reference(got, take(want, perm), f"{name} {mode} permuted", rays[perm], march_steps_only=True)
    finally:
        r.close()


@pytest.mark.parametrize("mode", ["spec", "interp"])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_prefixes_and_single_outputs(torch_cuda, scenes, name, mode):
    """n = 1, 63, 64, 65: nothing beyond element n - 1 is written (Outputs.collect) and the rays are only read (shade_rays); each
    output pointer alone, the others NULL, is its column of the full run"""
    sc = scenes[name]
    rays = SR.shade_ray_set(sc, SEED)
    want = SR.reference(sc, rays)
    r = open_renderer(sc, MODES[mode])
    try:
        r.set_miss_skip(False)
        for n in (1, 63, 64, 65):
            assert_is_reference(shade_rays(torch_cuda, r, rays, n=n), take(want, slice(0, n)), f"{name} {mode} n={n}", rays)
        for f in FIELDS:
            got = shade_rays(torch_cuda, r, rays, n=65, want=(f,))
            assert set(got) == {f}
            assert_is_reference(got, {f: want[f][:65]}, f"{name} {mode} {f} alone", rays)
    finally:
        r.close()


@pytest.mark.parametrize("mode", ["spec", "interp"])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_max_steps(torch_cuda, scenes, name, mode):
    sc = scenes[name]
    rays = SR.shade_ray_set(sc, SEED)[:130]
    r = open_renderer(sc, MODES[mode])
    try:
        for max_steps in (0, 1, 7):
            want = SR.reference(sc, rays, max_steps)
            assert int((want["steps"] & 0xFFFF).max()) == max_steps
            both_ways(torch_cuda, r, rays, take(want, slice(None)), f"{name} {mode} max_steps={max_steps}", max_steps=max_steps)
    finally:
        r.close()


@pytest.mark.parametrize("t", INTERP + FORMS, ids=ids)
def test_rungs_and_forms(torch_cuda, t):
    """one shape per rung of the interpreter's ladder, with and without the fast paths, and one per form of the scene compiler — the
    large tables read from global memory and both tiers of the 284-op scene among them: the camera rays of a 13 x 5 frame with the
    specials among them.  The library says which kernel ran, and that is held to what the case was written for."""
    sc = C.scene_of(t.shape)
    rays = R.ray_set(sc, SEED, "ae")
    want = SR.reference(sc, rays)
    r = gpu.Renderer(0, specialize=t.specialize)
    try:
        r.set_shade_queries(True)
        r.prepare(sc)
        t.assert_identity(r, families=False)
        name = "lol_shade_spec" if t.own else "shade_interp"
        assert r.shade_kernel_name() == name, r.specialize_log()
        both_ways(torch_cuda, r, rays, take(want, slice(None)), t.id)
        assert r.shade_kernel_name() == name
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------- lists of pixels
def frame(torch, r, w, h, camera=None, max_steps=256, rgb=True, planes=True):
    """a frame of lol_gpu_render_device with its debug planes: dict(pixel, rgb, dist, id, steps), row-major"""
    dev = torch.device("cuda:0")
    px = torch.full((h, w), 0x55AA55, dtype=torch.int32, device=dev)
    t = dict(rgb=torch.zeros((h, w, 3), dtype=torch.float32, device=dev), dist=torch.zeros((h, w), dtype=torch.float32, device=dev),
             id=torch.zeros((h, w), dtype=torch.int32, device=dev), steps=torch.zeros((h, w), dtype=torch.int32, device=dev))
    dbg = gpu.Debug(t["rgb"].data_ptr() if rgb else None, *((t[f].data_ptr() if planes else None) for f in ("dist", "id", "steps")))
    torch.cuda.synchronize()
    r.render_into(px.data_ptr(), w, h, max_steps, camera=camera, debug=dbg, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = dict(pixel=px.cpu().numpy().view(np.uint32).ravel(), rgb=t["rgb"].cpu().numpy().reshape(-1, 3), dist=t["dist"].cpu().numpy().ravel(),
               id=t["id"].cpu().numpy().view(np.uint32).ravel(), steps=t["steps"].cpu().numpy().view(np.uint32).ravel())
    return out


def frame_cameras(sc):
    minus_zero = V.copy_camera(sc.camera)
    minus_zero.point.x = -0.0
    return [("own", V.copy_camera(sc.camera)), ("orbit1", C.cameras(sc)[1]), ("minus-zero", minus_zero), ("insane", V.insane_camera())]


@pytest.mark.parametrize("mode", ["spec", "interp"])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_pixels_are_the_frame(torch_cuda, scenes, name, mode):
    """every pixel of a 13 x 5 and of a 16 x 9 frame: pixel, rgb, dist, id and steps ARE the frame's pixels and debug planes under
    the same camera, skips and pixel format — the first step given by the host and taken per pixel, a camera beyond the sane range —
    and with the skips off all six outputs are shade()'s for those rays"""
    sc = scenes[name]
    r, r2 = open_renderer(sc, MODES[mode]), gpu.Renderer(0, specialize=MODES[mode])
    try:
        r2.prepare(sc)
        for (w, h), fmt in (((13, 5), None), ((16, 9), LOSSY)):
            xy = all_pixels(w, h)
            for q in (r, r2):
                q.set_pixel_format(fmt)
            for view, cam in frame_cameras(sc):
                for skips in (True, False):
                    for q in (r, r2):
                        q.set_miss_skip(skips)
                    what = f"{name} {mode} {w}x{h} {view} skips={skips}"
                    got = shade_pixels(torch_cuda, r, xy, w, h, camera=cam)
                    want = frame(torch_cuda, r2, w, h, camera=cam)
                    assert_is_reference(take(got, slice(None), tuple(want)), want, what + " against the frame")
                    if not skips and view in ("own", "orbit1"):
                        ref = SR.reference(sc, R.camera_rays(sc, w, h, cam), fmt=fmt)
                        assert_is_reference(got, take(ref, slice(None)), what + " against shade()")
    finally:
        r2.close()
        r.close()


def test_pixels_outside_the_frame(torch_cuda, scenes):
    """coordinates are not inspected: a pair outside the frame gives the ray the reference's formula gives (the oracle's probe takes
    any x, y), shaded as shade() shades it"""
    sc, (w, h) = scenes["scene4"], (13, 5)
    outside = np.array([(w, 0), (0, h), (w + 5, h + 3), (0xFFFFFFFF, 2), (3, 0xFFFFFFFE)], np.uint32)      # (the last two: -1 and -2 as int)
    signed = [tuple(int(v) - (1 << 32) if v >= 1 << 31 else int(v) for v in p) for p in outside.astype(np.int64)]
    ro = sc.camera.point.tuple()
    rays = np.array([ro + tuple(O.probe(sc, w, h, x, y, 1).rd) for x, y in signed], np.float32)
    r = open_renderer(sc, MODES["spec"])
    try:
        r.set_miss_skip(False)
        assert_is_reference(shade_pixels(torch_cuda, r, outside, w, h), take(SR.reference(sc, rays), slice(None)), "pixels outside the frame")
    finally:
        r.close()


@pytest.mark.parametrize("mode", ["spec", "interp"])
def test_sample_rays_are_the_leaves_of_a_supersampled_pixel(torch_cuda, scenes, mode):
    """rgb_linear of pixels (2 x + i, 2 y + j) of the 16 x 8 frame, summed on the host in the tree of lol_gpu_set_samples and put
    through the host's powf, is lol_gpu_debug.rgb of the 8 x 4 frame under set_samples(2)"""
    sc, (w, h), s = scenes["scene4"], (8, 4), 2
    r = open_renderer(sc, MODES[mode])
    try:
        xy = np.array([(s * x + i, s * y + j) for y in range(h) for x in range(w) for j in range(s) for i in range(s)], np.uint32)
        leaves = shade_pixels(torch_cuda, r, xy, s * w, s * h, want=("rgb_linear",))["rgb_linear"].reshape(h * w, s * s, 3)
        mean = A.tree_mean(leaves)
        post = O.powf(mean, np.full(mean.shape, A.GAMMA, dtype=np.float32))
        r.set_samples(s)
        aa = frame(torch_cuda, r, w, h, planes=False)
        assert R.same_bits(post, aa["rgb"]).all()
        assert np.array_equal(A.pack(post), aa["pixel"])
        r.set_samples(1)
    finally:
        r.close()


DEGENERATE_SIZE = (13, 7)


@pytest.mark.parametrize("mode", ["spec", "interp"])
@pytest.mark.parametrize("name", C.DEGENERATE_NAMES)
def test_degenerate_scenes(torch_cuda, name, mode):
    sc = C.degenerate_scenes()[C.DEGENERATE_NAMES.index(name)]
    w, h = DEGENERATE_SIZE
    want = SR.reference(sc, R.camera_rays(sc, w, h))
    r = gpu.Renderer(0, specialize=MODES[mode])
    try:
        r.set_shade_queries(True)
        r.prepare(sc)
        for skips in (False, True):
            r.set_miss_skip(skips)
            got = shade_pixels(torch_cuda, r, all_pixels(w, h), w, h)
            assert_is_reference(got, take(want, slice(None)), f"{name} {mode} skips={skips}", march_steps_only=skips)
    finally:
        r.close()


@pytest.mark.parametrize("mode", ["spec", "interp"])
@pytest.mark.parametrize("e", C.HOSTILE_TIES, ids=lambda e: e.name)
def test_ties_go_to_the_first_object(torch_cuda, e, mode):
    """exact ties: the hit is the first object's and so is the material the colour is made of — with the first step given by the
    host, taken per pixel (a -0 in the origin), with 256 steps and with ONE, where the first step's id is the ray's"""
    sc = C.hostile_scene(e)
    w, h = DEGENERATE_SIZE
    first = min(e.tie.tied)
    r = open_renderer(sc, MODES[mode])
    try:
        r.set_miss_skip(False)
        for max_steps in (256, 1):
            for view, cam in tie_cameras(sc)[:2]:
                want = SR.reference(sc, R.camera_rays(sc, w, h, cam), max_steps)
                got = shade_pixels(torch_cuda, r, all_pixels(w, h), w, h, camera=cam, max_steps=max_steps)
                assert_is_reference(got, take(want, slice(None)), f"{e.name} {mode} {view} max_steps={max_steps}")
                if max_steps == 1:
                    assert (got["id"] == first).all()
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------ the context around it
def test_tiers_and_the_switch(torch_cuda, scenes):
    """a query before the scene kernel is there and one after: same bits, and the name goes from shade_interp to lol_shade_spec.
    Without the switch it stays shade_interp, and the module is the parent's: the same kernel_key as a context that never heard of
    shading queries"""
    sc = scenes["scene4"]
    rays = SR.shade_ray_set(sc, SEED)
    want = take(SR.reference(sc, rays), slice(None))
    r = open_renderer(sc, 1, wait=False)
    try:
        assert r.shade_kernel_name() == "shade_interp"                # nothing has taken over yet: no frame boundary, no query
        before = shade_rays(torch_cuda, r, rays)
        r.specialize_wait()
        assert r.shade_kernel_name() == "lol_shade_spec" and r.kernel_name() == "lol_render_spec", r.specialize_log()
        assert_is_reference(before, want, "before the scene kernel", rays, march_steps_only=True)
        assert_is_reference(shade_rays(torch_cuda, r, rays), want, "on the scene kernel", rays, march_steps_only=True)
        key_with = r.kernel_key()
    finally:
        r.close()
    off, plain = open_renderer(sc, 1, queries=False), gpu.Renderer(0, specialize=1)
    try:
        plain.prepare(sc)
        assert off.shade_kernel_name() == "shade_interp" and off.kernel_name() == "lol_render_spec"
        assert off.kernel_key() == plain.kernel_key() != key_with
        assert_is_reference(shade_rays(torch_cuda, off, rays), want, "without the switch", rays, march_steps_only=True)
        assert off.shade_kernel_name() == "shade_interp"
    finally:
        off.close()
        plain.close()


@pytest.mark.parametrize("mode", ["spec", "interp"])
def test_a_frame_after_a_query_is_the_frame_it_would_have_been(torch_cuda, scenes, mode):
    """frame, queries of both kinds, frame under a still camera in the default tile order (longest tiles first): the two frames are
    equal, the query is the frame, and the second frame is that of a context that rendered the two frames alone"""
    sc, (w, h) = scenes["scene4"], (37, 11)
    r, alone = open_renderer(sc, MODES[mode]), gpu.Renderer(0, specialize=MODES[mode])
    try:
        alone.prepare(sc)
        assert r.tile_order()["mode"] == "lpt"
        a = frame(torch_cuda, r, w, h)
        got = shade_pixels(torch_cuda, r, all_pixels(w, h), w, h)
        shade_rays(torch_cuda, r, SR.shade_ray_set(sc, SEED), n=130)
        b = frame(torch_cuda, r, w, h)
        for f in a:
            assert R.same_bits(a[f], b[f]).all(), f
        assert_is_reference(take(got, slice(None), tuple(a)), a, "the query against the frame before it")
        for _ in range(2):
            c = frame(torch_cuda, alone, w, h)
        assert np.array_equal(c["pixel"], b["pixel"]) and np.array_equal(c["steps"], b["steps"])
        assert r.tile_order()["mode"] == alone.tile_order()["mode"] == "lpt"
    finally:
        alone.close()
        r.close()


def refusal(call):
    """(status, text) of the GpuError that `call` raises: the text is what lol_gpu_error() returned, which GpuError puts behind the
    status's name"""
    with pytest.raises(gpu.GpuError) as e:
        call()
    st = e.value.status
    head = f"lol_gpu: {gpu._STATUS.get(st, st)}: "
    assert str(e.value).startswith(head), str(e.value)
    return st, str(e.value)[len(head):]


# what lol_gpu_error() says after each refusal of test_refusals: the text is part of what a host sees
REFUSAL_TEXT = {
    "no program": "no scene program uploaded",
    "no list": "shading query: no list",
    "no output": "shading query: no output",
    "max_steps or n": "shading query: max_steps < 0 or more than 2^32 - 1 rays",
    "geometry": "shading query: no camera or bad frame geometry",
}


def test_refusals(torch_cuda, scenes):
    """what the header says, with nothing written; the status, the text of lol_gpu_error() and the ORDER of the refusals"""
    sc = scenes["scene4"]
    rays = SR.shade_ray_set(sc, SEED)[:64]
    d_rays = torch_cuda.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
    d_xy = torch_cuda.zeros(128, dtype=torch_cuda.int32, device="cuda:0")
    out = Outputs(torch_cuda, 64)
    lib = gpu.gpu_lib()
    T = REFUSAL_TEXT
    torch_cuda.cuda.synchronize()

    def shades():
        return gpu.Shades(*(out.ptrs()[f + "_ptr"] for f in FIELDS))

    empty = gpu.Renderer(0)
    try:
        assert refusal(lambda: empty.shade_rays_into(d_rays.data_ptr(), 64, **out.ptrs())) == (-4, T["no program"])
        assert refusal(lambda: empty.shade_rays_into(d_rays.data_ptr(), 64, -1, **out.ptrs())) == (-3, T["max_steps or n"])      # a bad argument first
        fc = sc.frame_camera(8, 8)
        assert lib.lol_gpu_shade_pixels(empty._ctx, fc, 8, 8, 256, d_xy.data_ptr(), 64, shades(), None) == -4
        # the order, without a program: a list of pixels asks for the program BEFORE the camera and the frame's geometry
        assert lib.lol_gpu_shade_pixels(empty._ctx, fc, 0, 8, 256, d_xy.data_ptr(), 64, shades(), None) == -4
        assert lib.lol_gpu_shade_pixels(empty._ctx, None, 8, 8, 256, d_xy.data_ptr(), 64, shades(), None) == -4
        assert lib.lol_gpu_shade_pixels(empty._ctx, fc, 8, 8, -1, d_xy.data_ptr(), 64, shades(), None) == -3
        assert lib.lol_gpu_shade_rays(empty._ctx, d_rays.data_ptr(), 64, -1, shades(), None) == -3
    finally:
        empty.close()
    r = open_renderer(sc, 1)
    try:
        fc = sc.frame_camera(8, 8)
        assert lib.lol_gpu_shade_rays(None, d_rays.data_ptr(), 64, 256, shades(), None) == -3            # no context
        assert refusal(lambda: r.shade_rays_into(0, 64, **out.ptrs())) == (-3, T["no list"])                              # no rays
        assert refusal(lambda: r.shade_rays_into(d_rays.data_ptr(), 64)) == (-3, T["no output"])                          # all six outputs NULL
        assert lib.lol_gpu_shade_rays(r._ctx, d_rays.data_ptr(), 64, 256, None, None) == -3              # no lol_gpu_shades
        assert refusal(lambda: r.shade_rays_into(d_rays.data_ptr(), 64, -1, **out.ptrs())) == (-3, T["max_steps or n"])   # max_steps < 0
        assert refusal(lambda: r.shade_rays_into(d_rays.data_ptr(), 1 << 32, **out.ptrs())) == (-3, T["max_steps or n"])  # n > 2^32 - 1
        assert refusal(lambda: r.shade_pixels_into(0, 64, 8, 8, **out.ptrs())) == (-3, T["no list"])
        assert refusal(lambda: r.shade_pixels_into(d_xy.data_ptr(), 64, 0, 8, frame_camera=fc, **out.ptrs())) == (-3, T["geometry"])
        assert refusal(lambda: r.shade_pixels_into(d_xy.data_ptr(), 64, 8, 0, frame_camera=fc, **out.ptrs())) == (-3, T["geometry"])
        assert refusal(lambda: r.shade_pixels_into(d_xy.data_ptr(), 64, 8, 8, -1, **out.ptrs())) == (-3, T["max_steps or n"])
        assert refusal(lambda: r.shade_pixels_into(d_xy.data_ptr(), 64, 8, 8)) == (-3, T["no output"])
        assert lib.lol_gpu_shade_pixels(r._ctx, None, 8, 8, 256, d_xy.data_ptr(), 64, shades(), None) == -3      # no camera
        assert lib.lol_gpu_shade_pixels(r._ctx, None, 8, 8, 256, d_xy.data_ptr(), 0, shades(), None) == -3       # ... with n = 0 too
        # n = 0: fine, with no list at all, and nothing launched
        r.shade_rays_into(0, 0, **out.ptrs())
        r.shade_pixels_into(0, 0, 8, 8, **out.ptrs())
        r.sync()
        torch_cuda.cuda.synchronize()
        assert out.untouched()
        assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), rays.view(np.uint32))
    finally:
        r.close()


def test_streams(torch_cuda, scenes):
    """LOL_GPU_STREAM_DEFAULT, the context's own (NULL), and two torch streams with a query in flight on each: the same answers"""
    sc = scenes["scene"]
    rays = SR.shade_ray_set(sc, SEED)
    want = take(SR.reference(sc, rays), slice(None))
    r = open_renderer(sc, 1)
    try:
        assert_is_reference(shade_rays(torch_cuda, r, rays, stream=0), want, "LOL_GPU_STREAM_DEFAULT", rays, march_steps_only=True)
        assert_is_reference(shade_rays(torch_cuda, r, rays, stream=None), want, "the context's own stream", rays, march_steps_only=True)
        d_rays = torch_cuda.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
        s1, s2 = torch_cuda.cuda.Stream(), torch_cuda.cuda.Stream()
        o1, o2 = Outputs(torch_cuda, len(rays)), Outputs(torch_cuda, len(rays))
        torch_cuda.cuda.synchronize()
        r.shade_rays_into(d_rays.data_ptr(), len(rays), stream=s1.cuda_stream, **o1.ptrs())
        r.shade_rays_into(d_rays.data_ptr(), len(rays), stream=s2.cuda_stream, **o2.ptrs())
        s1.synchronize()
        s2.synchronize()
        assert_is_reference(o1.collect(), want, "the first of two streams", rays, march_steps_only=True)
        assert_is_reference(o2.collect(), want, "the second of two streams", rays, march_steps_only=True)
    finally:
        r.close()


def test_panorama_through_the_cli(torch_cuda, scenes, tmp_path, capsys):
    """python -m loltracer_amd scene4.lol --panorama 8x4: one shading query over scene.panorama_rays, the reference's colours"""
    w, h = 8, 4
    path = os.path.join(C.SCENES_DIR, "scene4.lol")
    out = str(tmp_path / "pano.ppm")
    assert cli_main([path, "--panorama", f"{w}x{h}", "-o", out]) == 0
    assert "[lol_shade_spec]" in capsys.readouterr().out
    with open(out, "rb") as f:
        data = f.read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert data.startswith(head) and len(data) == len(head) + 3 * w * h
    got = np.frombuffer(data[len(head):], np.uint8).reshape(-1, 3)
    sc = scenes["scene4"]
    px = SR.reference(sc, S.panorama_rays(sc.camera, w, h))["pixel"]
    assert np.array_equal(got, np.stack([px >> 16 & 0xFF, px >> 8 & 0xFF, px & 0xFF], axis=-1).astype(np.uint8))
    assert cli_main([path, "--panorama", f"{w}x{h}"]) == 1                    # no -o: nowhere to write
