"""Ray queries on the device: lol_gpu_trace_rays, lol_gpu_trace_pixels and lol_gpu_pick, on the scene kernel (lol_trace_spec) and on
the interpreter (trace_interp), held to tests/ray_reference.py (arbitrary rays), to the oracle's probe and to the debug planes of a
frame (pixels).

Every comparison is ray_reference.same_bits: equality of bit patterns, two NaNs counting as the same; no tolerance.  The reference of
a ray is computed once per (scene, max_steps) for the whole module, whatever list the ray comes in.
"""
import numpy as np
import pytest

import oracle_lib as O
import ray_reference as R
import scene_shapes as C
import test_gpu_views as V
from loltracer_amd import gpu
from test_gpu_families import FORMS, INTERP
from test_gpu_hostile import tie_cameras
from test_gpu_parity import gpu_render
from test_gpu_shades import refusal

pytestmark = pytest.mark.gpu

SEED = 20261018
SENTINEL = 0x5A5A5A5A                    # what every output holds before a query (as a float: 1.5e16, no answer of any ray here)
PAD = 67                                 # elements behind element n - 1 of every output: more than a wave
FIELDS = ("dist", "id", "steps", "normal")
MODES = {"spec": 1, "interp": 4, "interp-plain": 0, "spec-plain": 3}           # lol_gpu_set_specialize
TRACE = {1: "lol_trace_spec", 3: "lol_trace_spec", 4: "trace_interp", 0: "trace_interp"}
FRAME = {1: "lol_render_spec", 3: "lol_render_spec", 4: "render_interp", 0: "render_interp"}
ids = lambda t: t.id                     # noqa: E731


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def open_renderer(sc, specialize, queries=True, wait=True):
    r = gpu.Renderer(0, specialize=specialize)
    try:
        r.set_ray_queries(queries)
        assert r.ray_queries == bool(queries)
        r.prepare(sc, wait=wait)
        if wait:
            assert r.trace_kernel_name() == (TRACE[specialize] if queries else "trace_interp"), r.specialize_log()
            assert r.kernel_name() == FRAME[specialize], r.specialize_log()
    except BaseException:
        r.close()
        raise
    return r


class Outputs:
    """the four outputs of a query of n rays, each n + PAD elements of SENTINEL on the device, or absent"""

    def __init__(self, torch, n, want=FIELDS):
        dev = torch.device("cuda:0")
        self.n, self.t = n, {}
        for f in want:
            k = 3 if f == "normal" else 1
            self.t[f] = torch.full(((n + PAD) * k,), SENTINEL, dtype=torch.int32, device=dev)

    def ptrs(self):
        return {f + "_ptr": (self.t[f].data_ptr() if f in self.t else 0) for f in FIELDS}

    def collect(self):
        """{field: the first n elements}; asserts that nothing behind them was written"""
        out = {}
        for f, t in self.t.items():
            a = t.cpu().numpy().view(np.uint32)
            k = 3 if f == "normal" else 1
            assert (a[self.n * k:] == SENTINEL).all(), f"{f}: written beyond element n - 1"
            a = a[:self.n * k]
            out[f] = a.view(np.float32).reshape(-1, 3) if f == "normal" else a.view(np.float32) if f == "dist" else a
        return out

    def untouched(self):
        return all((t.cpu().numpy().view(np.uint32) == SENTINEL).all() for t in self.t.values())


def stream_of(torch, stream):
    return torch.cuda.current_stream().cuda_stream if stream == "torch" else stream


def trace_rays(torch, r, rays, n=None, max_steps=256, want=FIELDS, stream="torch"):
    """the first n rays of `rays` through lol_gpu_trace_rays; the ray buffer must come back as it went"""
    n = len(rays) if n is None else n
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
    out = Outputs(torch, n, want)
    torch.cuda.synchronize()
    r.trace_rays_into(d_rays.data_ptr(), n, max_steps, stream=stream_of(torch, stream), **out.ptrs())
    r.sync()
    torch.cuda.synchronize()
    assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), np.ascontiguousarray(rays).view(np.uint32)), "the ray buffer was written"
    return out.collect()


def trace_pixels(torch, r, xy, w, h, camera=None, max_steps=256, want=FIELDS, stream="torch"):
    xy = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
    d_xy = torch.from_numpy(xy.view(np.int32).copy()).to("cuda:0")
    out = Outputs(torch, len(xy), want)
    torch.cuda.synchronize()
    r.trace_pixels_into(d_xy.data_ptr(), len(xy), w, h, max_steps, camera=camera, stream=stream_of(torch, stream), **out.ptrs())
    r.sync()
    torch.cuda.synchronize()
    assert np.array_equal(d_xy.cpu().numpy().view(np.uint32), xy), "the pixel list was written"
    return out.collect()


def assert_is_reference(got, want, what, rays=None):
    bad = R.differing(got, want, fields=tuple(got))
    if bad:
        f, i = bad[0]
        ray = "" if rays is None else f" ray {rays[i].tolist()}"
        raise AssertionError(f"{what}: {len(bad)} (field, ray) pairs differ; first: {f}[{i}] = {got[f][i]!r}, reference {want[f][i]!r}{ray}")


def take(ref, idx):
    return {f: ref[f][idx] for f in ref}


_probe = {}


def probe_frame(key, sc, w, h, cam, max_steps=256):
    """the oracle's probe of every pixel of a frame, row-major, in the outputs' layout; once per key for the module"""
    key = (key, w, h, max_steps)
    if key not in _probe:
        n = w * h
        ref = dict(dist=np.zeros(n, np.float32), id=np.zeros(n, np.uint32), steps=np.zeros(n, np.uint32), normal=np.zeros((n, 3), np.float32))
        for y in range(h):
            for x in range(w):
                p = O.probe(sc, w, h, x, y, max_steps, camera=cam)
                ref["dist"][y * w + x], ref["id"][y * w + x], ref["steps"][y * w + x] = p.hit_dist, p.hit_id, p.march_steps
                ref["normal"][y * w + x] = tuple(p.normal)
        _probe[key] = ref
    return _probe[key]


def all_pixels(w, h):
    return np.array([(x, y) for y in range(h) for x in range(w)], np.uint32)


# ------------------------------------------------------------------------------------------------ lists of arbitrary rays
@pytest.mark.parametrize("mode", ["spec", "interp", "interp-plain", "spec-plain"])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_ray_set(torch_cuda, scenes, name, mode):
    """scene4 asks for the id at every step, scene.lol once (ASK_ID_ONCE): every kind of ray of ray_set, the specials among ordinary
    rays, and the same list in a seeded permutation — a ray's answer does not depend on its wave-mates"""
    sc = scenes[name]
    rays = R.ray_set(sc, SEED)
    want = R.reference(sc, rays)
    # the set has hits, misses and rays whose answer is not finite (a NaN or inf component: dist inf, normal NaN)
    assert 0 < int((want["id"] == 0).sum()) < len(rays) and np.isinf(want["dist"]).any() and np.isnan(want["normal"]).any()
    r = open_renderer(sc, MODES[mode])
    try:
        assert_is_reference(trace_rays(torch_cuda, r, rays), want, f"{name} {mode}", rays)
        perm = np.random.default_rng(SEED + 1).permutation(len(rays))
        assert_is_reference(trace_rays(torch_cuda, r, rays[perm]), take(want, perm), f"{name} {mode} permuted", rays[perm])
    finally:
        r.close()


@pytest.mark.parametrize("mode", ["spec", "interp"])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_prefixes_and_single_outputs(torch_cuda, scenes, name, mode):
    """n = 1, 63, 64, 65, 130: nothing beyond element n - 1 is written (Outputs.collect) and the rays are only read (trace_rays); each
    output pointer alone, the others NULL, is its column of the full run — for scene.lol that is the id asked for once with no
    normal wanted"""
    sc = scenes[name]
    rays = R.ray_set(sc, SEED)
    want = R.reference(sc, rays)
    r = open_renderer(sc, MODES[mode])
    try:
        for n in (1, 63, 64, 65, 130):
            assert_is_reference(trace_rays(torch_cuda, r, rays, n=n), take(want, slice(0, n)), f"{name} {mode} n={n}", rays)
        for f in FIELDS:
            got = trace_rays(torch_cuda, r, rays, n=130, want=(f,))
            assert set(got) == {f}
            assert_is_reference(got, {f: want[f][:130]}, f"{name} {mode} {f} alone", rays)
    finally:
        r.close()


@pytest.mark.parametrize("mode", ["spec", "interp"])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_max_steps(torch_cuda, scenes, name, mode):
    sc = scenes[name]
    rays = R.ray_set(sc, SEED)[:130]
    r = open_renderer(sc, MODES[mode])
    try:
        for max_steps in C.MAX_STEPS:
            want = R.reference(sc, rays, max_steps)
            assert int(want["steps"].max()) <= max_steps and (max_steps > 7 or int(want["steps"].max()) == max_steps)
            if max_steps == 0:
                assert not want["dist"].view(np.uint32).any() and not want["id"].any()
            assert_is_reference(trace_rays(torch_cuda, r, rays, max_steps=max_steps), want, f"{name} {mode} max_steps={max_steps}", rays)
    finally:
        r.close()


@pytest.mark.parametrize("t", INTERP + FORMS, ids=ids)
def test_rungs_and_forms(torch_cuda, t):
    """one shape per rung of the interpreter's ladder, with and without the fast paths, and one per form of the scene compiler: 130
    rays of kinds (a) - (c).  The library says which kernel ran, and that is held to what the case was written for."""
    assert {u.shape.rung[0] for u in INTERP} == {1, 3, 7, 11, 63}      # trace_interp's five stack classes (it reads no tables) all have a case
    sc = C.scene_of(t.shape)
    rays = np.resize(R.ray_set(sc, SEED, "abc"), (130, 6))          # (a sparse scene has few hits to start (b) and (c) from: its rays repeat)
    want = R.reference(sc, rays)
    r = gpu.Renderer(0, specialize=t.specialize)
    try:
        r.set_ray_queries(True)
        r.prepare(sc)
        t.assert_identity(r, families=False)
        assert r.trace_kernel_name() == ("lol_trace_spec" if t.own else "trace_interp"), r.specialize_log()
        assert_is_reference(trace_rays(torch_cuda, r, rays), want, t.id, rays)
        assert r.trace_kernel_name() == ("lol_trace_spec" if t.own else "trace_interp")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------- lists of pixels
DEGENERATE = ("no-objects", "inside-a-sphere", "inf-squared-length", "zero-squared-length")
SMALL = (13, 7)                          # odd both ways: the central ray is a pixel's


@pytest.mark.parametrize("mode", ["spec", "interp"])
@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_scenes(torch_cuda, name, mode):
    sc = C.degenerate_scenes()[C.DEGENERATE_NAMES.index(name)]
    w, h = SMALL
    r = gpu.Renderer(0, specialize=MODES[mode])
    try:
        r.set_ray_queries(True)
        r.prepare(sc)
        got = trace_pixels(torch_cuda, r, all_pixels(w, h), w, h)
        assert_is_reference(got, probe_frame(("degenerate", name), sc, w, h, None), f"{name} {mode}")
    finally:
        r.close()


@pytest.mark.parametrize("mode", ["spec", "interp"])
@pytest.mark.parametrize("e", C.HOSTILE_TIES, ids=lambda e: e.name)
def test_ties_go_to_the_first_object(torch_cuda, e, mode):
    """the first step given by the host, taken per pixel (a -0 in the origin) and under a camera beyond the sane range, with 256 steps
    and with ONE, where the first step's id is the ray's"""
    sc = C.hostile_scene(e)
    w, h = SMALL
    first = min(e.tie.tied)
    r = open_renderer(sc, MODES[mode])
    try:
        for max_steps in (256, 1):
            for view, cam in tie_cameras(sc):
                got = trace_pixels(torch_cuda, r, all_pixels(w, h), w, h, camera=cam, max_steps=max_steps)
                assert_is_reference(got, probe_frame((e.name, view), sc, w, h, cam, max_steps), f"{e.name} {mode} {view} max_steps={max_steps}")
                if view != "insane" and max_steps == 1:
                    assert (got["id"] == first).all()
                elif view != "insane" and e.tie.along_ray:
                    assert got["id"][(h // 2) * w + w // 2] == first and not (set(e.tie.tied) - {first}) & set(got["id"].tolist())
    finally:
        r.close()


def frame_cameras(sc):
    orbit = C.cameras(sc)
    minus_zero = V.copy_camera(sc.camera)
    minus_zero.point.x = -0.0
    return [("own", V.copy_camera(sc.camera)), ("orbit1", orbit[1]), ("orbit2", orbit[2]), ("insane", V.insane_camera()), ("minus-zero", minus_zero)]


@pytest.mark.parametrize("mode", ["spec", "interp"])
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_pixels_are_the_frame_and_the_oracle(torch_cuda, scenes, name, mode):
    """every pixel of a 37 x 11 frame, row-major and shuffled: dist, id and steps ARE the debug planes of lol_gpu_render_device under
    that camera, and all four outputs the oracle's probe"""
    sc, (w, h) = scenes[name], (37, 11)
    xy = all_pixels(w, h)
    perm = np.random.default_rng(SEED + 2).permutation(len(xy))
    r = open_renderer(sc, MODES[mode])
    r2 = gpu.Renderer(0, specialize=MODES[mode])
    try:
        for view, cam in frame_cameras(sc):
            what = f"{name} {mode} {view}"
            g = gpu_render(torch_cuda, r2, sc, w, h, camera=cam)
            got = trace_pixels(torch_cuda, r, xy, w, h, camera=cam)
            planes = dict(dist=g["dist"].ravel(), id=g["id"].ravel(), steps=(g["steps"] & 0xFFFF).ravel())
            assert_is_reference({f: got[f] for f in planes}, planes, what + " against the frame's planes")
            want = probe_frame((name, view), sc, w, h, cam)
            assert_is_reference(got, want, what + " against the oracle")
            assert_is_reference(trace_pixels(torch_cuda, r, xy[perm], w, h, camera=cam), take(want, perm), what + " shuffled")
    finally:
        r2.close()
        r.close()


def test_pixels_outside_the_frame_and_sample_rays(torch_cuda, scenes):
    """coordinates are not inspected: a pair outside the frame gives the ray the reference's formula gives (the oracle's probe takes
    any x, y); and pixel (s x + i, s y + j) of the s w x s h frame is sample (i, j) of pixel (x, y)"""
    sc, (w, h) = scenes["scene4"], (13, 7)
    outside = np.array([(w, 0), (0, h), (w + 5, h + 3), (0xFFFFFFFF, 2), (3, 0xFFFFFFFE)], np.uint32)      # (the last two: -1 and -2 as int)
    r = open_renderer(sc, MODES["spec"])
    try:
        got = trace_pixels(torch_cuda, r, outside, w, h)
        for i, (x, y) in enumerate(outside.astype(np.int64)):
            x, y = (int(v) - (1 << 32) if v >= 1 << 31 else int(v) for v in (x, y))
            p = O.probe(sc, w, h, x, y, 256)
            want = dict(dist=np.array([p.hit_dist], np.float32), id=np.array([p.hit_id], np.uint32), steps=np.array([p.march_steps], np.uint32),
                        normal=np.array([tuple(p.normal)], np.float32))
            assert_is_reference(take(got, slice(i, i + 1)), want, f"pixel ({x}, {y}) outside the frame")
        s = 2
        got = trace_pixels(torch_cuda, r, all_pixels(s * w, s * h), s * w, s * h)
        assert_is_reference(got, probe_frame(("scene4", "samples"), sc, s * w, s * h, None), "the sample rays of s = 2")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------ the context around it
def test_tiers_and_the_switch(torch_cuda, scenes):
    """a query before the scene kernel is there and one after: same bits, and the name goes from trace_interp to lol_trace_spec.
    Without the switch it stays trace_interp, and the module is the parent's: the same kernel_key as a context that never heard of
    queries"""
    sc = scenes["scene4"]
    rays = R.ray_set(sc, SEED)
    want = R.reference(sc, rays)
    r = open_renderer(sc, 1, wait=False)
    try:
        assert r.trace_kernel_name() == "trace_interp"                # nothing has taken over yet: no frame boundary, no query
        before = trace_rays(torch_cuda, r, rays)
        r.specialize_wait()
        assert r.trace_kernel_name() == "lol_trace_spec" and r.kernel_name() == "lol_render_spec", r.specialize_log()
        assert_is_reference(before, want, "before the scene kernel", rays)
        assert_is_reference(trace_rays(torch_cuda, r, rays), want, "on the scene kernel", rays)
        key_with = r.kernel_key()
    finally:
        r.close()
    off, plain = open_renderer(sc, 1, queries=False), gpu.Renderer(0, specialize=1)
    try:
        plain.prepare(sc)
        assert off.trace_kernel_name() == "trace_interp" and off.kernel_name() == "lol_render_spec"
        assert off.kernel_key() == plain.kernel_key() != key_with
        assert_is_reference(trace_rays(torch_cuda, off, rays), want, "without the switch", rays)
        assert off.trace_kernel_name() == "trace_interp"
    finally:
        off.close()
        plain.close()


def render(torch, r, w, h, steps=True):
    dev = torch.device("cuda:0")
    frame = torch.full((h, w), 0x55AA55, dtype=torch.int32, device=dev)
    dist, hid, st = (torch.zeros((h, w), dtype=dt, device=dev) for dt in (torch.float32, torch.int32, torch.int32))
    torch.cuda.synchronize()
    r.render_into(frame.data_ptr(), w, h, debug=gpu.Debug(None, dist.data_ptr(), hid.data_ptr(), st.data_ptr()),
                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [a.cpu().numpy().view(np.uint32) for a in (frame, dist, hid, st)]


@pytest.mark.parametrize("mode", ["spec", "interp"])
def test_a_frame_after_a_query_is_the_frame_it_would_have_been(torch_cuda, scenes, mode):
    """frame, query, pick, frame under a still camera in the default tile order: the two frames are equal, and equal to the second
    frame of a context that rendered the two frames alone; pick is the matching element of trace_pixels"""
    sc, (w, h) = scenes["scene4"], (37, 11)
    r, alone = open_renderer(sc, MODES[mode]), gpu.Renderer(0, specialize=MODES[mode])
    try:
        alone.prepare(sc)
        assert r.tile_order()["mode"] == "lpt"
        a = render(torch_cuda, r, w, h)
        got = trace_pixels(torch_cuda, r, all_pixels(w, h), w, h)
        for x, y in ((0, 0), (w - 1, h - 1), (w // 2, h // 2), (5, 3)):
            p = r.pick(x, y, w, h)
            i = y * w + x
            one = dict(dist=np.array([p["dist"]], np.float32), id=np.array([p["id"]], np.uint32), steps=np.array([p["steps"]], np.uint32),
                       normal=np.array([p["normal"]], np.float32))
            assert_is_reference(one, take(got, slice(i, i + 1)), f"pick({x}, {y})")
        b = render(torch_cuda, r, w, h)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
        assert np.array_equal(a[1], got["dist"].view(np.uint32).reshape(h, w)) and np.array_equal(a[2], got["id"].reshape(h, w))
        # ... and the second frame is that of a context that rendered the two frames alone
        for _ in range(2):
            c = render(torch_cuda, alone, w, h)
        assert np.array_equal(c[0], b[0])
        assert r.tile_order()["mode"] == alone.tile_order()["mode"] == "lpt"
    finally:
        alone.close()
        r.close()


# what lol_gpu_error() says after each refusal of test_refusals: the text is part of what a host sees
REFUSAL_TEXT = {
    "no program": "no scene program uploaded",
    "no list": "ray query: no list",
    "no output": "ray query: no output",
    "max_steps or n": "ray query: max_steps < 0 or more than 2^32 - 1 rays",
    "geometry": "ray query: no camera or bad frame geometry",
    "pick outside": "pick: the pixel lies outside the frame",
    "pick geometry": "pick: no camera, no output or bad frame geometry",
}


def test_refusals(torch_cuda, scenes):
    """what the header says, with nothing written; the status, the text of lol_gpu_error() and the ORDER of the refusals"""
    sc = scenes["scene4"]
    rays = R.ray_set(sc, SEED)[:64]
    d_rays = torch_cuda.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
    d_xy = torch_cuda.zeros(128, dtype=torch_cuda.int32, device="cuda:0")
    out = Outputs(torch_cuda, 64)
    lib = gpu.gpu_lib()
    T = REFUSAL_TEXT
    torch_cuda.cuda.synchronize()

    empty = gpu.Renderer(0)
    try:
        assert refusal(lambda: empty.trace_rays_into(d_rays.data_ptr(), 64, **out.ptrs())) == (-4, T["no program"])
        assert refusal(lambda: empty.trace_rays_into(d_rays.data_ptr(), 64, -1, **out.ptrs())) == (-3, T["max_steps or n"])      # a bad argument first
        fc = sc.frame_camera(8, 8)
        hits = gpu.Hits(*(out.ptrs()[f + "_ptr"] for f in FIELDS))
        assert lib.lol_gpu_trace_pixels(empty._ctx, fc, 8, 8, 256, d_xy.data_ptr(), 64, hits, None) == -4
        hit = gpu.Hit()
        assert lib.lol_gpu_pick(empty._ctx, fc, 8, 8, 256, 0, 0, hit) == -4
        # the order, without a program: a list of pixels asks for the program BEFORE the camera and the frame's geometry, a pick after
        assert lib.lol_gpu_trace_pixels(empty._ctx, fc, 0, 8, 256, d_xy.data_ptr(), 64, hits, None) == -4
        assert lib.lol_gpu_trace_pixels(empty._ctx, None, 8, 8, 256, d_xy.data_ptr(), 64, hits, None) == -4
        assert lib.lol_gpu_trace_pixels(empty._ctx, fc, 8, 8, -1, d_xy.data_ptr(), 64, hits, None) == -3
        assert lib.lol_gpu_trace_rays(empty._ctx, d_rays.data_ptr(), 64, -1, hits, None) == -3
        assert lib.lol_gpu_pick(empty._ctx, fc, 0, 8, 256, 0, 0, hit) == -3
    finally:
        empty.close()
    r = open_renderer(sc, 1)
    try:
        fc = sc.frame_camera(8, 8)
        hits = gpu.Hits(*(out.ptrs()[f + "_ptr"] for f in FIELDS))
        assert refusal(lambda: r.trace_rays_into(0, 64, **out.ptrs())) == (-3, T["no list"])                              # no rays
        assert refusal(lambda: r.trace_rays_into(d_rays.data_ptr(), 64)) == (-3, T["no output"])                          # all four outputs NULL
        assert lib.lol_gpu_trace_rays(r._ctx, d_rays.data_ptr(), 64, 256, None, None) == -3              # no lol_gpu_hits
        assert refusal(lambda: r.trace_rays_into(d_rays.data_ptr(), 64, -1, **out.ptrs())) == (-3, T["max_steps or n"])   # max_steps < 0
        assert refusal(lambda: r.trace_rays_into(d_rays.data_ptr(), 1 << 32, **out.ptrs())) == (-3, T["max_steps or n"])  # n > 2^32 - 1
        assert refusal(lambda: r.trace_pixels_into(0, 64, 8, 8, **out.ptrs())) == (-3, T["no list"])
        assert refusal(lambda: r.trace_pixels_into(d_xy.data_ptr(), 64, 0, 8, frame_camera=fc, **out.ptrs())) == (-3, T["geometry"])
        assert refusal(lambda: r.trace_pixels_into(d_xy.data_ptr(), 64, 8, 0, frame_camera=fc, **out.ptrs())) == (-3, T["geometry"])
        assert refusal(lambda: r.trace_pixels_into(d_xy.data_ptr(), 64, 8, 8, -1, **out.ptrs())) == (-3, T["max_steps or n"])
        assert lib.lol_gpu_trace_pixels(r._ctx, None, 8, 8, 256, d_xy.data_ptr(), 64, hits, None) == -3  # no camera
        assert lib.lol_gpu_trace_pixels(r._ctx, None, 8, 8, 256, d_xy.data_ptr(), 0, hits, None) == -3   # ... with n = 0 too
        for x, y in ((-1, 0), (0, -1), (8, 0), (0, 8)):
            assert refusal(lambda: r.pick(x, y, 8, 8)) == (-3, T["pick outside"])
        assert refusal(lambda: r.pick(0, 0, 8, 8, max_steps=-1)) == (-3, T["pick geometry"])
        assert lib.lol_gpu_pick(r._ctx, fc, 8, 8, 256, 0, 0, None) == -3
        # n = 0: fine, with no list at all, and nothing launched
        r.trace_rays_into(0, 0, **out.ptrs())
        r.trace_pixels_into(0, 0, 8, 8, **out.ptrs())
        r.sync()
        torch_cuda.cuda.synchronize()
        assert out.untouched()
        assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), rays.view(np.uint32))
    finally:
        r.close()


def test_streams(torch_cuda, scenes):
    """LOL_GPU_STREAM_DEFAULT, a torch stream, and the context's own (NULL): the same answers"""
    sc = scenes["scene"]
    rays = R.ray_set(sc, SEED)
    want = R.reference(sc, rays)
    r = open_renderer(sc, 1)
    try:
        assert_is_reference(trace_rays(torch_cuda, r, rays, stream=0), want, "LOL_GPU_STREAM_DEFAULT", rays)      # (0 is passed on as the legacy default stream)
        assert_is_reference(trace_rays(torch_cuda, r, rays, stream=None), want, "the context's own stream", rays)
        s = torch_cuda.cuda.Stream()
        with torch_cuda.cuda.stream(s):
            got = trace_rays(torch_cuda, r, rays, stream=s.cuda_stream)
        assert_is_reference(got, want, "a torch stream", rays)
    finally:
        r.close()
