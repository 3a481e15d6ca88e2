"""Scene queries on the device (lol_gpu_trace_scene_rays, lol_gpu_trace_scene_pixels, lol_gpu_shade_scene_rays,
lol_gpu_shade_scene_pixels): element (r, i) of a call IS what the single-scene query answers for that ray on a context that uploaded
scenes[r] — and so tests/ray_reference.py's and tests/shade_reference.py's answer on that record's own Scene, and, for shaded pixels,
frame r of render_scene_views_into.

Every comparison is ray_reference.same_bits: equality of bit patterns, two NaNs counting as the same; no tolerance.  The one latitude
of the header is kept as it stands there: for a list of RAYS with the exact skips on, the shadow steps (the high half of `steps`) are
compared with the single-scene query after set_exact_skips(0) alone; for pixels all 32 bits are compared either way.  Against the CPU
reference the shadow steps are compared with every skip off, as in tests/test_gpu_shades.py.

The records: scene4, scene4 with the sphere at (0, 1, -6) moved to (1.5, 2, -5), and scene4 with a diffuse colour on material #0, so
that the miss skip holds in two records and not in the third.  What the inputs must show — some rays hit and some escape in every
record, the records differ where a kernel that read the wrong record would not — is asserted on the CPU references before the device
is looked at (`refs`).  The answers of the fresh single-scene contexts are computed once per list for the module.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ray_reference as R
import scene_shapes as C
import shade_reference as SR
import test_gpu_rays as TR
import test_gpu_shades as TS
import test_gpu_views as V
from loltracer_amd import gpu
from loltracer_amd import scene as S
from loltracer_amd.__main__ import axis_cosine, pick_line
from test_gpu_families import INTERP

pytestmark = pytest.mark.gpu

SEED = 20261021
N = 70                                   # rays per record of a list: one full wave and a tail of six lanes
W, H = 33, 16                            # 528 pixels: eight full waves and a tail of 16 lanes
GAP = 5                                  # elements between the lists of two records where every record brings its own
KINDS = ("trace", "shade")
HELP = {"trace": TR, "shade": TS}
REF = {"trace": R, "shade": SR}
ERR_ARG, ERR_NO_PROGRAM = -3, -4
ids = lambda t: t.id                     # noqa: E731


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_kept = {}


def records(scenes):
    """the three records"""
    if "records" not in _kept:
        base = scenes["scene4"]
        moved, lit = base.clone(), base.clone()
        sphere = next(i for i in range(base.c.n_nodes)
                      if base.c.nodes[i].type == S.NODE_SPHERE and base.c.nodes[i].point.tuple() == (0.0, 1.0, -6.0))
        moved.c.nodes[sphere].point.x, moved.c.nodes[sphere].point.y, moved.c.nodes[sphere].point.z = 1.5, 2.0, -5.0
        lit.c.materials[0].diffuse.x, lit.c.materials[0].diffuse.y, lit.c.materials[0].diffuse.z = 0.375, 0.25, 0.125
        _kept["records"] = [base, moved, lit]
    return _kept["records"]


def pick_rays(pool, offset):
    """N rays of a ray set: the eight special rays, each inside the list, among ordinary rays taken from `pool` at even distances
    from `offset` on"""
    specials = R.special_rays(pool[0, :3], pool[0, 3:])
    ordinary = np.array([r for r in pool if np.isfinite(r).all()], np.float32)
    step = max(1, len(ordinary) // (N - len(specials)))
    rays = list(ordinary[(offset + step * np.arange(N - len(specials))) % len(ordinary)])
    for at, s in zip((3, 11, 19, 27, 35, 43, 65, 67), specials):               # six inside the full wave, two inside the tail
        rays.insert(at + offset % 3, s)
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    assert rays.shape == (N, 6)
    return rays


def ray_lists(scenes, kind):
    """(the list every record may share, one list per record): N rays each, of ray_set / shade_ray_set on the base scene"""
    key = ("lists", kind)
    if key not in _kept:
        base = records(scenes)[0]
        pool = R.ray_set(base, SEED) if kind == "trace" else SR.shade_ray_set(base, SEED)
        own = [pick_rays(pool, 1 + 17 * r) for r in range(3)]
        assert not np.array_equal(own[0].view(np.uint32), own[1].view(np.uint32)) and not np.array_equal(own[1].view(np.uint32), own[2].view(np.uint32))
        _kept[key] = (pick_rays(pool, 0), own)
    return _kept[key]


def all_pixels():
    return TR.all_pixels(W, H)


@pytest.fixture(scope="module")
def refs(scenes):
    """the CPU references of every record on the shared list, on its own list and on the frame's pixels — and what the inputs must
    show, asserted here, before any test looks at the device"""
    if "refs" in _kept:
        return _kept["refs"]
    scs = records(scenes)
    out = {}
    for kind in KINDS:
        shared, own = ray_lists(scenes, kind)
        frame_rays = [R.camera_rays(sc, W, H) for sc in scs]
        out[kind] = dict(shared=[REF[kind].reference(sc, shared) for sc in scs], own=[REF[kind].reference(sc, own[r]) for r, sc in enumerate(scs)],
                         pixels=[REF[kind].reference(sc, frame_rays[r]) for r, sc in enumerate(scs)])
        for what in ("shared", "own", "pixels"):
            for r in range(3):
                hit = out[kind][what][r]["id"] != 0
                assert hit.any() and (~hit).any(), f"{kind} {what}: record {r} needs rays that hit and rays that escape"
    for what in ("shared", "pixels"):
        t, s = out["trace"][what], out["shade"][what]
        assert (~R.same_bits(t[0]["dist"], t[1]["dist"])).any(), f"{what}: records 0 and 1 differ in no dist"
        assert (s[0]["pixel"] != s[1]["pixel"]).any(), f"{what}: records 0 and 1 differ in no pixel"
        escaped = (s[0]["id"] == 0) & (s[2]["id"] == 0)
        assert (~R.same_bits(s[0]["rgb_linear"], s[2]["rgb_linear"]).all(axis=1) & escaped).any(), f"{what}: no escaped ray of record 2 has another colour"
        assert R.same_bits(t[0]["dist"], t[2]["dist"]).all()                     # (the third record moves nothing)
    _kept["refs"] = out
    return out


def open_fresh(sc, specialize=4):
    """a context that uploaded `sc`: the interpreter with the upload's proven fast paths (no scene compiler to wait for)"""
    r = gpu.Renderer(0, specialize=specialize)
    try:
        r.prepare(sc)
    except BaseException:
        r.close()
        raise
    return r


def single(torch, kind, sc, key, skips, rays=None, xy=None, size=None, camera=None, specialize=4, max_steps=256):
    """what a fresh context that uploaded `sc` answers (cached per `key`)"""
    key = ("single", kind, key, skips, specialize, max_steps)
    if key not in _kept:
        r = open_fresh(sc, specialize)
        try:
            r.set_exact_skips(skips)
            if rays is not None:
                _kept[key] = (HELP[kind].trace_rays if kind == "trace" else HELP[kind].shade_rays)(torch, r, rays, max_steps=max_steps)
            else:
                fn = HELP[kind].trace_pixels if kind == "trace" else HELP[kind].shade_pixels
                _kept[key] = fn(torch, r, xy, *size, camera=camera, max_steps=max_steps)
        finally:
            r.close()
    return _kept[key]


def scene_query(torch, r, kind, scs, n, rays=None, xy=None, stride=0, size=None, cameras=None, want=None, max_steps=256, stream="torch"):
    """one scene query over len(scs) records of n elements; `rays` / `xy`: the WHOLE device list (every record's, gaps included), which
    must come back as it went.  -> per record, {field: n elements}; nothing behind element R n - 1 may be written"""
    H_ = HELP[kind]
    want = H_.FIELDS if want is None else want
    host = np.ascontiguousarray(rays if rays is not None else xy)
    d_list = torch.from_numpy(host.view(np.int32).copy()).to("cuda:0")
    out = H_.Outputs(torch, len(scs) * n, want)
    torch.cuda.synchronize()
    s = H_.stream_of(torch, stream)
    if rays is not None:
        fn = r.trace_scene_rays_into if kind == "trace" else r.shade_scene_rays_into
        fn(scs, d_list.data_ptr(), n, stride, max_steps, stream=s, **out.ptrs())
    else:
        fn = r.trace_scene_pixels_into if kind == "trace" else r.shade_scene_pixels_into
        fn(scs, d_list.data_ptr(), n, *size, stride, max_steps, stream=s, cameras=cameras, **out.ptrs())
    r.sync()
    torch.cuda.synchronize()
    assert np.array_equal(d_list.cpu().numpy().view(np.uint32), host.view(np.uint32)), "the list was written"
    return split(out.collect(), len(scs), n)


def split(flat, n_records, n):
    return [{f: a[r * n:(r + 1) * n] for f, a in flat.items()} for r in range(n_records)]


def assert_same(kind, got, want, what, march_steps_only=False, fields=None):
    fields = tuple(f for f in got if f in want) if fields is None else fields
    if kind == "trace":
        bad = R.differing(got, want, fields=fields)
    else:
        bad = SR.differing(got, want, fields=fields, march_steps_only=march_steps_only)
    if bad:
        f, i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} (field, ray) pairs differ; first: {f}[{i}] = {got[f][i]!r}, expected {want[f][i]!r}")


def with_gaps(lists, stride, fill):
    """the lists of the records, `stride` elements apart, `fill` between them"""
    n, width = lists[0].shape
    buf = np.full(((len(lists) - 1) * stride + n, width), fill, lists[0].dtype)
    for r, a in enumerate(lists):
        buf[r * stride:r * stride + n] = a
    return buf


# ----------------------------------------------------------------------------------------------------------------- lists of pixels
@pytest.mark.parametrize("skips", [7, 0], ids=["default-skips", "skips-off"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_pixel_of_three_records(torch_cuda, scenes, refs, kind, skips):
    """all 33 x 16 pixels under each record's own scene: the single-scene query of a context that uploaded the record (every field,
    all 32 bits of `steps`), the CPU reference on the record's Scene and, shaded, frame r of render_scene_views_into with its planes"""
    scs = records(scenes)
    xy = all_pixels()
    r = open_fresh(scs[0])
    try:
        r.set_exact_skips(skips)
        assert r.miss_skip_active() == skips
        got = scene_query(torch_cuda, r, kind, scs, len(xy), xy=xy, size=(W, H))
        if kind == "shade":
            out = V.alloc_batch(torch_cuda, 3, W, H)
            torch_cuda.cuda.synchronize()
            r.render_scene_views_into(out["frame"].data_ptr(), None, scs, W, H, debug=out["dbg"])
            r.sync()
            frames = V.collect(out, *out["geom"])
        for rec, sc in enumerate(scs):
            what = f"{kind} pixels, record {rec}, skips {skips}"
            assert_same(kind, got[rec], single(torch_cuda, kind, sc, ("pixels", rec), skips, xy=xy, size=(W, H)), what + ": the fresh context")
            want = refs[kind]["pixels"][rec]
            assert_same(kind, got[rec], want, what + ": the CPU reference", march_steps_only=skips != 0, fields=tuple(got[rec]))
            if kind == "shade":
                frame = dict(pixel=frames["xrgb"][rec].ravel(), rgb=frames["rgb"][rec].reshape(-1, 3), dist=frames["dist"][rec].ravel(),
                             id=frames["id"][rec].ravel(), steps=frames["steps"][rec].ravel())
                assert_same(kind, got[rec], frame, what + ": the frame of render_scene_views_into")
    finally:
        r.close()


@pytest.mark.parametrize("kind", KINDS)
def test_pixels_under_each_records_own_camera(torch_cuda, scenes, kind):
    """four records, four cameras — the scene's own, one of the orbit, one with x = -0 (no first step from the host), one beyond the
    sane range (no fast SDF, no settled exit) — and lists of their own, a gap between them: the first step, the list and the flags
    are each record's own"""
    scs = records(scenes) + [records(scenes)[1]]
    cams = [c for _, c in TS.frame_cameras(scs[0])]
    w, h = 13, 5
    xy = TR.all_pixels(w, h)
    lists = [np.roll(xy, 7 * rec, axis=0) for rec in range(4)]
    buf = with_gaps(lists, len(xy) + GAP, 0x7FFFFFF0)
    r = open_fresh(scs[0])
    try:
        got = scene_query(torch_cuda, r, kind, scs, len(xy), xy=buf, stride=len(xy) + GAP, size=(w, h), cameras=cams)
        for rec, sc in enumerate(scs):
            want = single(torch_cuda, kind, sc, ("cameras", rec), 7, xy=lists[rec], size=(w, h), camera=cams[rec])
            assert_same(kind, got[rec], want, f"{kind} pixels, record {rec} under its own camera")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------- lists of rays
@pytest.mark.parametrize("lists", ["shared", "own"])
@pytest.mark.parametrize("kind", KINDS)
def test_ray_lists_of_three_records(torch_cuda, scenes, refs, kind, lists):
    """70 rays per record, the special rays among them: one list for every record (list_stride = 0), and a list per record of other
    rays, a gap of NaN rays between them"""
    scs = records(scenes)
    shared, own = ray_lists(scenes, kind)
    per_record = [shared] * 3 if lists == "shared" else own
    buf, stride = (shared, 0) if lists == "shared" else (with_gaps(own, N + GAP, np.float32(np.nan)), N + GAP)
    r = open_fresh(scs[0])
    try:
        for skips in (0, 7):
            r.set_exact_skips(skips)
            got = scene_query(torch_cuda, r, kind, scs, N, rays=buf, stride=stride)
            for rec, sc in enumerate(scs):
                what = f"{kind} rays ({lists}), record {rec}, skips {skips}"
                want = single(torch_cuda, kind, sc, (lists, rec), skips, rays=per_record[rec])
                assert_same(kind, got[rec], want, what + ": the fresh context", march_steps_only=skips != 0)       # the header's latitude
                assert_same(kind, got[rec], refs[kind][lists][rec], what + ": the CPU reference", march_steps_only=skips != 0, fields=tuple(got[rec]))
    finally:
        r.close()


def second_record(sc):
    """a scene of `sc`'s structure with its first solid moved and grown, a light moved and the ambient colour changed"""
    key = ("second", id(sc))
    if key not in _kept:
        b = sc.clone()
        solid = next(i for i in range(sc.c.n_nodes) if sc.c.nodes[i].type in (S.NODE_SPHERE, S.NODE_BOX))
        b.c.nodes[solid].point.x += 0.375
        b.c.nodes[solid].radius = b.c.nodes[solid].radius * 1.25 + 0.0625
        b.c.lights[0].point.y += 1.0
        b.c.ambient_color.x += 0.125
        _kept[key] = (sc, b)
    return _kept[key][1]


@pytest.mark.parametrize("t", INTERP, ids=ids)
def test_every_instantiation(torch_cuda, t):
    """one scene per rung of the interpreter's ladder, in plain arithmetic (specialize 0) and with the proven root (specialize 4): two
    records of 70 rays each, both kinds of query, held to the single-scene query of a context that uploaded the record"""
    base = C.scene_of(t.shape)
    scs = [base, second_record(base)]
    rays = R.ray_set(base, TR.SEED, "ae")[:N]
    assert len(rays) == N and np.isnan(rays).any() and np.isinf(rays).any()        # specials are among them
    r = open_fresh(base, t.specialize)
    try:
        assert r.interp_variant() == t.shape.rung and r.interp_fast_paths()[0] == (3 if t.specialize == 4 else 0)
        for kind in KINDS:
            got = scene_query(torch_cuda, r, kind, scs, N, rays=rays)
            answers = []
            for rec, sc in enumerate(scs):
                want = single(torch_cuda, kind, sc, ("rung", t.shape.name, rec), 7, rays=rays, specialize=t.specialize)
                assert_same(kind, got[rec], want, f"{t.id} {kind}, record {rec}", march_steps_only=True)
                answers.append(want["dist"])
            assert not R.same_bits(*answers).all(), f"{t.id}: the two records answer alike"
    finally:
        r.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_centre_is_its_records_business_alone(torch_cuda, scenes, kind):
    scs = records(scenes)
    if "nan" not in _kept:
        bad = scs[0].clone()
        sphere = next(i for i in range(bad.c.n_nodes) if bad.c.nodes[i].type == S.NODE_SPHERE)
        bad.c.nodes[sphere].point.y = float("nan")
        _kept["nan"] = bad
    three = [scs[0], _kept["nan"], scs[1]]
    shared, _ = ray_lists(scenes, kind)
    r = open_fresh(scs[0])
    try:
        got = scene_query(torch_cuda, r, kind, three, N, rays=shared)
        clean = scene_query(torch_cuda, r, kind, [scs[0], scs[1]], N, rays=shared)
        assert_same(kind, got[0], clean[0], f"{kind}: the clean record before the NaN one")
        assert_same(kind, got[2], clean[1], f"{kind}: the clean record behind the NaN one")
        assert_same(kind, got[1], single(torch_cuda, kind, three[1], ("nan", 0), 7, rays=shared), f"{kind}: the NaN record", march_steps_only=True)
        assert_same(kind, got[0], single(torch_cuda, kind, scs[0], ("shared", 0), 7, rays=shared), f"{kind}: record 0", march_steps_only=True)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------ refusals, state, streams
def test_refusals(torch_cuda, scenes):
    """the refusals in the header's order, each with nothing written; n = 0; and another structure, a missing table and a material
    out of range in lol_gpu_render_scene_views' words"""
    scs = records(scenes)
    shared, _ = ray_lists(scenes, "trace")
    d_rays = torch_cuda.from_numpy(shared.copy()).to("cuda:0")
    d_xy = torch_cuda.zeros(2 * N, dtype=torch_cuda.int32, device="cuda:0")
    hits_out, shades_out = TR.Outputs(torch_cuda, 3 * N), TS.Outputs(torch_cuda, 3 * N)
    torch_cuda.cuda.synchronize()
    lib = gpu.gpu_lib()
    progs = [sc.flatten() for sc in scs]
    arr = (S.Program * 3)(*progs)
    cams = (S.FrameCamera * 3)(*[sc.frame_camera(8, 8) for sc in scs])
    hits = gpu.Hits(*(hits_out.ptrs()[f + "_ptr"] for f in TR.FIELDS))
    shades = gpu.Shades(*(shades_out.ptrs()[f + "_ptr"] for f in TS.FIELDS))
    rays, xy = d_rays.data_ptr(), d_xy.data_ptr()
    refusal = TS.refusal

    empty = gpu.Renderer(0)
    try:    # without a program: a bad argument first, then the program, and only then the records
        assert lib.lol_gpu_trace_scene_rays(empty._ctx, arr, 3, rays, N, 0, -1, hits, None) == ERR_ARG
        assert lib.lol_gpu_trace_scene_rays(empty._ctx, None, 0, rays, N, 1, 256, hits, None) == ERR_NO_PROGRAM
        assert lib.lol_gpu_shade_scene_pixels(empty._ctx, None, None, 0, 0, 8, 256, xy, N, 1, shades, None) == ERR_NO_PROGRAM
    finally:
        empty.close()

    r = open_fresh(scs[0])
    try:
        ctx = r._ctx
        for who, out, rays_fn, pixels_fn, ptrs in (
                ("scene ray query", hits, lib.lol_gpu_trace_scene_rays, lib.lol_gpu_trace_scene_pixels, hits_out.ptrs()),
                ("scene shading query", shades, lib.lol_gpu_shade_scene_rays, lib.lol_gpu_shade_scene_pixels, shades_out.ptrs())):
            into = r.trace_scene_rays_into if out is hits else r.shade_scene_rays_into
            pixels_into = r.trace_scene_pixels_into if out is hits else r.shade_scene_pixels_into
            # 1. the list query's own, in its order — each beats everything behind it
            assert rays_fn(None, arr, 3, rays, N, 0, 256, out, None) == ERR_ARG
            assert refusal(lambda: into(scs, 0, N, 1, -1)) == (ERR_ARG, who + ": no list")
            assert refusal(lambda: into(scs, rays, N, 1, -1)) == (ERR_ARG, who + ": no output")
            assert rays_fn(ctx, None, 0, rays, N, 1, -1, None, None) == ERR_ARG and r._lib.lol_gpu_error(ctx).decode() == who + ": no output"
            assert refusal(lambda: into(scs, rays, N, 1, -1, **ptrs)) == (ERR_ARG, who + ": max_steps < 0 or more than 2^32 - 1 rays")
            assert refusal(lambda: into(scs, rays, 1 << 32, 1, **ptrs)) == (ERR_ARG, who + ": max_steps < 0 or more than 2^32 - 1 rays")
            assert pixels_fn(ctx, None, None, 0, 0, 8, 256, xy, N, 1, out, None) == ERR_ARG
            assert r._lib.lol_gpu_error(ctx).decode() == who + ": no camera or bad frame geometry"
            assert pixels_fn(ctx, cams, arr, 3, 8, 0, 256, xy, 0, 0, out, None) == ERR_ARG                       # ... with n = 0 too
            # 2. the records and their lists, in the header's order
            assert rays_fn(ctx, None, 0, rays, N, 1, 256, out, None) == ERR_ARG and r._lib.lol_gpu_error(ctx).decode() == who + ": no scenes"
            for n_scenes in (0, -1, gpu.MAX_VIEWS + 1):
                assert rays_fn(ctx, arr, n_scenes, rays, N, 1, 256, out, None) == ERR_ARG
                assert r._lib.lol_gpu_error(ctx).decode() == who + ": the number of scenes is not in 1 ... LOL_GPU_MAX_VIEWS"
            assert pixels_fn(ctx, None, arr, 3, 8, 8, 256, xy, N, 1, out, None) == ERR_ARG and r._lib.lol_gpu_error(ctx).decode() == who + ": no cameras"
            for stride in (1, N - 1):
                assert refusal(lambda: into(scs, rays, N, stride, **ptrs)) == (ERR_ARG, who + ": list_stride is neither 0 nor at least n")
            assert refusal(lambda: into(scs, rays, (1 << 32) // 3 + 1, 0, **ptrs)) == (ERR_ARG, who + ": more than 2^32 - 1 rays over all scenes")
            assert refusal(lambda: into(scs + [scenes["scene"]], rays, N - 1, 1, **ptrs)) == (ERR_ARG, who + ": list_stride is neither 0 nor at least n")
            # 3. the scenes, in lol_gpu_render_scene_views' words
            assert refusal(lambda: into(scs + [scenes["scene"]], rays, N, 0, **ptrs)) == (
                ERR_ARG, "a view's scene has not the uploaded program's structure (counts, opcodes, ids)")
            broken = (S.Program * 2)(progs[0], progs[1])
            broken[1].materials = None
            assert rays_fn(ctx, broken, 2, rays, N, 0, 256, out, None) == ERR_ARG
            assert r._lib.lol_gpu_error(ctx).decode() == "malformed scene of a view: a table is missing"
            roots = (type(progs[1].root_material.contents) * progs[1].n_roots)(*[progs[1].root_material[i] for i in range(progs[1].n_roots)])
            roots[0] = progs[1].n_materials
            broken = (S.Program * 2)(progs[0], progs[1])
            broken[1].root_material = roots
            assert rays_fn(ctx, broken, 2, rays, N, 0, 256, out, None) == ERR_ARG
            assert r._lib.lol_gpu_error(ctx).decode() == "material index out of range in a view's scene"
            # n = 0: fine behind every refusal, with no list at all, and nothing launched
            into(scs, 0, 0, 0, **ptrs)
            pixels_into(scs, 0, 0, 8, 8, 0, **ptrs)
            assert refusal(lambda: into(scs + [scenes["scene"]], 0, 0, 0, **ptrs))[0] == ERR_ARG
        r.sync()
        torch_cuda.cuda.synchronize()
        assert hits_out.untouched() and shades_out.untouched()
        assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), shared.view(np.uint32))
        # the context stays usable
        got = scene_query(torch_cuda, r, "trace", scs, N, rays=shared)
        assert_same("trace", got[1], single(torch_cuda, "trace", scs[1], ("shared", 1), 7, rays=shared), "after the refusals")
    finally:
        r.close()


def test_the_context_is_what_it_was(torch_cuda, scenes):
    """frame, scene queries of all four kinds, frame — on a DEFAULT context, its scene kernels loaded and both query switches set: the
    frames are equal, kernel_key, the tile order and the kernels' names are what they were, and the interpreter answered (same bits)"""
    scs = records(scenes)
    shared, _ = ray_lists(scenes, "shade")
    xy = TR.all_pixels(13, 5)
    r = gpu.Renderer(0)
    try:
        r.set_ray_queries(True)
        r.set_shade_queries(True)
        r.prepare(scs[0])
        names = (r.kernel_name(), r.trace_kernel_name(), r.shade_kernel_name())
        assert names == ("lol_render_spec", "lol_trace_spec", "lol_shade_spec"), r.specialize_log()
        a = TS.frame(torch_cuda, r, 37, 11)
        key, order = r.kernel_key(), r.tile_order()
        for kind in KINDS:
            got = scene_query(torch_cuda, r, kind, scs, N, rays=shared)
            assert_same(kind, got[2], single(torch_cuda, kind, scs[2], ("state", 2), 7, rays=shared), f"{kind} rays on a default context", march_steps_only=True)
            got = scene_query(torch_cuda, r, kind, scs, len(xy), xy=xy, size=(13, 5))
            assert_same(kind, got[1], single(torch_cuda, kind, scs[1], ("state", 1), 7, xy=xy, size=(13, 5)), f"{kind} pixels on a default context")
        assert (r.kernel_name(), r.trace_kernel_name(), r.shade_kernel_name()) == names
        assert r.kernel_key() == key and r.tile_order() == order and order["mode"] == "lpt"
        b = TS.frame(torch_cuda, r, 37, 11)
        for f in a:
            assert R.same_bits(a[f], b[f]).all(), f
        assert r.kernel_key() == key
    finally:
        r.close()


def test_two_streams_and_the_special_handles(torch_cuda, scenes):
    """LOL_GPU_STREAM_DEFAULT, the context's own stream, and two torch streams with a call in flight on each and no wait between
    them — ten calls in all through the ring of 8 sets"""
    scs = records(scenes)
    shared, _ = ray_lists(scenes, "shade")
    want = [single(torch_cuda, "shade", sc, ("shared", rec), 7, rays=shared) for rec, sc in enumerate(scs)]
    r = open_fresh(scs[0])
    try:
        for stream in (0, None):
            got = scene_query(torch_cuda, r, "shade", scs, N, rays=shared, stream=stream)
            for rec in range(3):
                assert_same("shade", got[rec], want[rec], f"stream {stream}, record {rec}", march_steps_only=True)
        s1, s2 = torch_cuda.cuda.Stream(), torch_cuda.cuda.Stream()
        d_rays = torch_cuda.from_numpy(shared.view(np.int32).copy()).to("cuda:0")
        outs = [TS.Outputs(torch_cuda, 3 * N) for _ in range(8)]
        torch_cuda.cuda.synchronize()
        for i, out in enumerate(outs):                                           # (nothing waits between the calls)
            r.shade_scene_rays_into(scs, d_rays.data_ptr(), N, 0, stream=(s1, s2)[i % 2].cuda_stream, **out.ptrs())
        s1.synchronize()
        s2.synchronize()
        for i, out in enumerate(outs):
            got = split(out.collect(), 3, N)
            for rec in range(3):
                assert_same("shade", got[rec], want[rec], f"call {i} of two streams, record {rec}", march_steps_only=True)
    finally:
        r.close()


# --------------------------------------------------------------------------------------------------------------------------- the CLI
def tween_files(tmp_path):
    a_file = os.path.join(V.ROOT, "tests", "golden", "scenes", "scene4.lol")
    text = open(a_file).read()
    assert "point\t\t= (0, 1, -6)" in text
    b_file = str(tmp_path / "b.lol")
    with open(b_file, "w") as f:
        f.write(text.replace("point\t\t= (0, 1, -6)", "point\t\t= (1.5, 2, -5)"))
    return a_file, b_file


def run_cli(args):
    return subprocess.run([sys.executable, "-m", "loltracer_amd"] + args, cwd=V.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                          timeout=300)


def test_the_tween_host_picks_and_pulls_focus(torch_cuda, scenes, tmp_path):
    """A.lol --tween B.lol --frames 3 --pick X,Y prints what pick_scenes returns, one line per frame, without -o; with --lens R
    --focus-at X,Y --lens-samples 2 it writes the frames of render_scene_views_into under each frame's own lens cameras"""
    a_file, b_file = tween_files(tmp_path)
    a, other = scenes["scene4"], S.Scene.parse_file(b_file)
    w, h, n, k, x, y, radius = 32, 16, 3, 2, 17, 4, 0.0625
    scs = [S.tween(a, other, t) for f in range(n) for t in S.shutter_times(f, n, 1)]
    r = open_fresh(a)
    try:
        picks = r.pick_scenes(scs, x, y, w, h, cameras=[a.camera] * n)
        for f, sc in enumerate(scs):                                             # pick_scenes IS pick on a context that uploaded the frame's scene
            fresh = open_fresh(sc)
            try:
                assert picks[f] == fresh.pick(x, y, w, h, camera=a.camera), f
            finally:
                fresh.close()
        assert len({p["dist"] for p in picks}) == n and all(p["id"] != 0 for p in picks)      # the object moves under the pixel
        p = run_cli([a_file, "--tween", b_file, "--frames", str(n), "--size", f"{w}x{h}", "--pick", f"{x},{y}"])
        assert p.returncode == 0, p.stdout
        assert [line for line in p.stdout.splitlines() if line.startswith("pick ")] == [pick_line(x, y, q) for q in picks], p.stdout

        out_dir = tmp_path / "frames"
        p = run_cli([a_file, "--tween", b_file, "--frames", str(n), "--size", f"{w}x{h}", "--lens", str(radius), "--focus-at", f"{x},{y}",
                     "--lens-samples", str(k), "-o", str(out_dir)])
        assert p.returncode == 0, p.stdout
        cosine = axis_cosine(a, w, h, x, y)
        cams = [c for f in range(n) for c in S.lens_cameras(a.camera, picks[f]["dist"] * cosine, radius, k)]
        out = V.alloc_batch(torch_cuda, n, w, h, None, None, False)
        torch_cuda.cuda.synchronize()
        r.render_scene_views_into(out["frame"].data_ptr(), cams, [scs[f] for f in range(n) for _ in range(k)], w, h, k)
        r.sync()
        frames = V.collect(out, *out["geom"])["xrgb"]
        assert sorted(os.listdir(out_dir)) == [f"frame_{f:04d}.ppm" for f in range(n)]
        from test_gpu_scene_view_samples import read_ppm
        for f in range(n):
            assert np.array_equal(read_ppm(out_dir / f"frame_{f:04d}.ppm", w, h), frames[f] & 0xFFFFFF), f
        assert not np.array_equal(frames[0], frames[n - 1])
        # what stays refused: the shutter beside the lens, --samples beside --tween, a focus pixel whose ray escapes names its frame
        p = run_cli([a_file, "--tween", b_file, "--frames", "2", "--size", f"{w}x{h}", "--lens", str(radius), "--focus-at", f"{x},{y}",
                     "--tween-shutter", "2", "-o", str(out_dir)])
        assert p.returncode == 1 and "--tween-shutter" in p.stdout, p.stdout
        p = run_cli([a_file, "--tween", b_file, "--frames", "2", "--size", f"{w}x{h}", "--pick", f"{x},{y}", "--samples", "2"])
        assert p.returncode == 1 and "--tween" in p.stdout, p.stdout
        assert r.pick_scenes(scs[:1], 0, 0, w, h, cameras=[a.camera])[0]["id"] == 0
        p = run_cli([a_file, "--tween", b_file, "--frames", "2", "--size", f"{w}x{h}", "--lens", str(radius), "--focus-at", "0,0", "-o", str(out_dir)])
        assert p.returncode == 1 and "in frame 0" in p.stdout and "hits nothing" in p.stdout, p.stdout
    finally:
        r.close()
