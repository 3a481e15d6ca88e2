"""Scene light passes on the device (lol_gpu_light_scene_rays, lol_gpu_light_scene_pixels, lol_gpu_relight_scenes): element (r, i) of a
capture IS what light_rays_into / light_pixels_into writes for that ray on a context that uploaded scenes[r] — and so
tests/light_reference.py's answer on that record's own Scene —, and element (r, i) of a relight IS relight_into's on such a context
under looks[r] — and so the shading query and the frame of the looks' scenes.

Every comparison is ray_reference.same_bits: equality of bit patterns, two NaNs counting as the same; no tolerance.  The one latitude
of the header is kept as it stands there: for a LIST of rays with the settled-shadow exit on, shadow_steps is compared with the
single-scene capture after set_exact_skips(0) alone; for pixels all 16 bytes of a factor are compared either way.  Against the CPU
reference shadow_steps is compared with every skip off, as in tests/test_gpu_light.py.

Shapes and records are those of tests/test_gpu_scene_queries.py: scene4, scene4 with a sphere moved, scene4 with a diffuse colour on
material #0 (the record that makes the cleared skips matter: its escaped rays are no longer black); 33 x 16 pixels; lists of 70 rays
with the eight special rays.  What the inputs must show is asserted on the CPU reference before the device is looked at (`refs`).
"""
import os

import numpy as np
import pytest

import light_reference as LR
import ray_reference as R
import scene_shapes as C
import test_gpu_light_views as LV
import test_gpu_rays as TR
import test_gpu_scene_queries as SQ
import test_gpu_shades as TS
import test_gpu_views as V
from loltracer_amd import gpu
from loltracer_amd import scene as S
from loltracer_amd.__main__ import look_of
from test_gpu_families import INTERP
from test_gpu_light import FACTORS, RELIT, SENTINEL, Colours, Planes, assert_same, capture, capture_pixels, relight
from test_gpu_scene_queries import GAP, H, N, W, open_fresh, records, split, with_gaps

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NO_PROGRAM = -3, -4
MARCH = ("id", "dist", "steps")
ids = lambda t: t.id                     # noqa: E731
_kept = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def ray_lists(scenes):
    """(the list every record may share, one list per record) of tests/test_gpu_scene_queries.py's shading lists"""
    return SQ.ray_lists(scenes, "shade")


def fields(shadow_steps):
    return MARCH + FACTORS + (("shadow_steps",) if shadow_steps else ())


@pytest.fixture(scope="module")
def refs(scenes):
    """the CPU references of every record on the shared list, on its own list and on the frame's pixels — and what the inputs must
    show, asserted here, before any test looks at the device"""
    if "refs" in _kept:
        return _kept["refs"]
    scs = records(scenes)
    shared, own = ray_lists(scenes)
    out = dict(shared=[LR.reference(sc, shared) for sc in scs], own=[LR.reference(sc, own[r]) for r, sc in enumerate(scs)],
               pixels=[LR.reference(sc, R.camera_rays(sc, W, H)) for sc in scs])
    for what, per_record in out.items():
        for r, ref in enumerate(per_record):
            hit = ref["id"] != 0
            assert hit.any() and (~hit).any(), f"{what}: record {r} needs rays that hit and rays that escape"
    for what in ("shared", "pixels"):
        a, b, c = out[what]
        assert any((~R.same_bits(a[f], b[f])).any() for f in FACTORS), f"{what}: records 0 and 1 differ in no factor"
        escaped = (a["id"] == 0) & (c["id"] == 0)
        relit_a, relit_c = LR.relit_reference(a, scs[0]), LR.relit_reference(c, scs[2])
        assert ((relit_a["pixel"] != relit_c["pixel"]) & escaped).any(), f"{what}: no escaped ray of record 2 has another relit pixel"
    _kept["refs"] = out
    return out


def scene_capture(torch, r, scs, n, rays=None, xy=None, stride=0, size=None, cameras=None, light_stride=0, max_steps=256, stream="torch"):
    """one capture over len(scs) records of n elements.  `rays` / `xy`: the WHOLE device list (every record's, gaps included), which must
    come back as it went; neither: every pixel of the size frame.  -> (the planes, per record {field: n elements}); Planes.collect
    asserts that nothing behind element N - 1 of any plane, and nothing between two lights' planes, was written"""
    host = None if rays is None and xy is None else np.ascontiguousarray(rays if rays is not None else xy)
    d_list = None if host is None else torch.from_numpy(host.view(np.int32).copy()).to("cuda:0")
    p = Planes(torch, len(scs) * n, len(r.scene.lights()), light_stride)
    torch.cuda.synchronize()
    s = TS.stream_of(torch, stream)
    if rays is not None:
        r.light_scene_rays_into(scs, d_list.data_ptr(), n, stride, max_steps, stream=s, **p.args())
    else:
        r.light_scene_pixels_into(scs, n, *size, stride, max_steps, xy_ptr=0 if d_list is None else d_list.data_ptr(), stream=s,
                                  cameras=cameras, **p.args())
    r.sync()
    torch.cuda.synchronize()
    if host is not None:
        assert np.array_equal(d_list.cpu().numpy().view(np.uint32), host.view(np.uint32)), "the list was written"
    return p, split(p.collect(), len(scs), n)


def single(torch, sc, key, skips, rays=None, xy=None, size=None, camera=None, specialize=4, all_pixels=False):
    """what light_rays_into / light_pixels_into writes on a fresh context that uploaded `sc` (cached per `key`)"""
    key = ("single", key, skips, specialize)
    if key not in _kept:
        r = open_fresh(sc, specialize)
        try:
            r.set_exact_skips(skips)
            if rays is not None:
                _kept[key] = capture(torch, r, rays)[1]
            else:
                _kept[key] = capture_pixels(torch, r, *size, xy=None if all_pixels else xy, camera=camera)[1]
        finally:
            r.close()
    return _kept[key]


def scene_relight(torch, r, scs, looks, p, n, want=RELIT, stream="torch"):
    """-> per record {field: n elements} of one relight_scenes_into over the planes `p`"""
    c = Colours(torch, len(scs) * n, want)
    torch.cuda.synchronize()
    r.relight_scenes_into(scs, looks, n, stream=TS.stream_of(torch, stream), **p.relight_args(), **c.args())
    r.sync()
    torch.cuda.synchronize()
    return split(c.collect(), len(scs), n)


# --------------------------------------------------------------------------------------------------------------------- the capture
@pytest.mark.parametrize("skips", [7, 0], ids=["default-skips", "skips-off"])
def test_every_pixel_of_three_records(torch_cuda, scenes, refs, skips):
    """all 33 x 16 pixels under each record's own scene, with no list and as a list of pixels: the capture of a context that uploaded
    the record (all 16 bytes of every factor, whatever the skips) and the CPU reference on the record's Scene; the planes a
    light_stride apart with canaries between them"""
    scs = records(scenes)
    xy = SQ.all_pixels()
    n = W * H
    r = open_fresh(scs[0])
    try:
        r.set_exact_skips(skips)
        assert r.miss_skip_active() == skips
        _, whole = scene_capture(torch_cuda, r, scs, n, size=(W, H))
        _, listed = scene_capture(torch_cuda, r, scs, n, xy=xy, size=(W, H), light_stride=3 * n + 37)
        for rec, sc in enumerate(scs):
            what = f"pixels, record {rec}, skips {skips}"
            fresh = single(torch_cuda, sc, ("pixels", rec), skips, size=(W, H), all_pixels=True)
            assert_same(whole[rec], fresh, fields(True), what + ": no list, the fresh context")
            assert_same(listed[rec], fresh, fields(True), what + ": a list of pixels, the fresh context")
            assert_same(whole[rec], refs["pixels"][rec], fields(skips == 0), what + ": the CPU reference")
    finally:
        r.close()


@pytest.mark.parametrize("lists", ["shared", "own"])
def test_ray_lists_of_three_records(torch_cuda, scenes, refs, lists):
    """70 rays per record, the special rays among them: one list for every record (list_stride = 0), and a list per record of other
    rays, a gap of NaN rays between them; a light_stride beyond N"""
    scs = records(scenes)
    shared, own = ray_lists(scenes)
    per_record = [shared] * 3 if lists == "shared" else own
    buf, stride = (shared, 0) if lists == "shared" else (with_gaps(own, N + GAP, np.float32(np.nan)), N + GAP)
    r = open_fresh(scs[0])
    try:
        for skips in (0, 7):
            r.set_exact_skips(skips)
            _, got = scene_capture(torch_cuda, r, scs, N, rays=buf, stride=stride, light_stride=0 if skips else 3 * N + 5)
            for rec, sc in enumerate(scs):
                what = f"rays ({lists}), record {rec}, skips {skips}"
                fresh = single(torch_cuda, sc, (lists, rec), skips, rays=per_record[rec])
                assert_same(got[rec], fresh, fields(skips == 0), what + ": the fresh context")                  # the header's latitude
                assert_same(got[rec], refs[lists][rec], fields(skips == 0), what + ": the CPU reference")
    finally:
        r.close()


def test_pixels_under_each_records_own_camera(torch_cuda, scenes):
    """four records, four cameras — the scene's own, one of the orbit, one with x = -0 (no first step from the host), one beyond the
    sane range (no fast SDF, no settled exit) — and lists of their own, a gap between them"""
    scs = records(scenes) + [records(scenes)[1]]
    cams = [c for _, c in TS.frame_cameras(scs[0])]
    w, h = 13, 5
    xy = TR.all_pixels(w, h)
    lists = [np.roll(xy, 7 * rec, axis=0) for rec in range(4)]
    buf = with_gaps(lists, len(xy) + GAP, 0x7FFFFFF0)
    r = open_fresh(scs[0])
    try:
        _, got = scene_capture(torch_cuda, r, scs, len(xy), xy=buf, stride=len(xy) + GAP, size=(w, h), cameras=cams)
        _, whole = scene_capture(torch_cuda, r, scs, len(xy), size=(w, h), cameras=cams)
        for rec, sc in enumerate(scs):
            fresh = single(torch_cuda, sc, ("cameras", rec), 7, xy=lists[rec], size=(w, h), camera=cams[rec])
            assert_same(got[rec], fresh, fields(True), f"record {rec} under its own camera")
            in_order = {f: np.roll(a, -7 * rec, axis=0) for f, a in fresh.items()}       # pixel y w + x is element (y w + x + 7 rec) % n of the list
            assert_same(whole[rec], in_order, fields(True), f"record {rec} under its own camera, every pixel")
    finally:
        r.close()


@pytest.mark.parametrize("t", INTERP, ids=ids)
def test_every_instantiation(torch_cuda, t):
    """one scene per rung of the interpreter's ladder, in plain arithmetic (specialize 0) and with the proven root (specialize 4): two
    records of 70 rays each, capture and relight, held to a context that uploaded the record"""
    base = C.scene_of(t.shape)
    scs = [base, SQ.second_record(base)]
    rays = R.ray_set(base, TR.SEED, "ae")[:N]
    assert len(rays) == N and np.isnan(rays).any() and np.isinf(rays).any()        # specials are among them
    r = open_fresh(base, t.specialize)
    try:
        assert r.interp_variant() == t.shape.rung and r.interp_fast_paths()[0] == (3 if t.specialize == 4 else 0)
        p, got = scene_capture(torch_cuda, r, scs, N, rays=rays)
        lit = scene_relight(torch_cuda, r, scs, None, p, N)
        answers = []
        for rec, sc in enumerate(scs):
            fresh = open_fresh(sc, t.specialize)
            try:
                fp, want = capture(torch_cuda, fresh, rays)
                assert_same(got[rec], want, fields(False), f"{t.id}, record {rec}")
                assert_same(lit[rec], relight(torch_cuda, fresh, None, fp), RELIT, f"{t.id}, record {rec}: relit")
            finally:
                fresh.close()
            answers.append(want["dist"])
        assert not R.same_bits(*answers).all(), f"{t.id}: the two records answer alike"
    finally:
        r.close()


def test_a_nan_centre_is_its_records_business_alone(torch_cuda, scenes):
    scs = records(scenes)
    bad = scs[0].clone()
    sphere = next(i for i in range(bad.c.n_nodes) if bad.c.nodes[i].type == S.NODE_SPHERE)
    bad.c.nodes[sphere].point.y = float("nan")
    three = [scs[0], bad, scs[1]]
    shared, _ = ray_lists(scenes)
    r = open_fresh(scs[0])
    try:
        _, got = scene_capture(torch_cuda, r, three, N, rays=shared)
        _, clean = scene_capture(torch_cuda, r, [scs[0], scs[1]], N, rays=shared)
        assert_same(got[0], clean[0], fields(True), "the clean record before the NaN one")
        assert_same(got[2], clean[1], fields(True), "the clean record behind the NaN one")
        assert_same(got[1], single(torch_cuda, bad, ("nan", 0), 7, rays=shared), fields(False), "the NaN record")
        assert_same(got[0], single(torch_cuda, scs[0], ("shared", 0), 7, rays=shared), fields(False), "record 0")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------- equal scenes: light views
def test_equal_scenes_are_light_views(torch_cuda, scenes):
    """2 views x K = 2 cameras, s = 2, at 9 x 5, every record the uploaded scene: the planes of light_views_into, byte for byte, in
    one launch; relight_views_into of them is render_blended_views_into(..., samples=2)"""
    sc = scenes["scene4"]
    n_views, k, w, h, s = 2, 2, 9, 5, 2
    cams = LV.cameras_of(sc, n_views, k)
    per = s * s * w * h
    r = open_fresh(sc)
    try:
        loop = LV.capture_views(torch_cuda, r, cams, k, w, h, s)
        frame_cams = [sc.frame_camera(w, h, c) for c in cams]                       # (the same bits for w x h and s w x s h: the header)
        one, _ = scene_capture(torch_cuda, r, [sc] * len(cams), per, size=(s * w, s * h), cameras=frame_cams)
        assert np.array_equal(loop.factors.cpu().numpy(), one.factors.cpu().numpy())
        for f in loop.t:
            assert np.array_equal(loop.t[f].cpu().numpy(), one.t[f].cpu().numpy()), f
        got = LV.relight_views(torch_cuda, r, None, one, n_views, k, w, h, s)
        assert_same(got, LV.rendered(torch_cuda, r, cams, k, w, h, s), ("rgb", "pixel"), "relit views of the one-launch capture")
    finally:
        r.close()


# ----------------------------------------------------------------------------------------------------------------------- the relight
def record_looks(scs):
    nan, inf = float("nan"), float("inf")
    nl, nm = len(scs[0].lights()), len(scs[0].materials())
    return [scs[0].with_look(lights=[((nan, .5, .25), (inf, 1., 2.))] + [None] * (nl - 1)),
            scs[1].with_look(materials=[((.3, .5, .7), (.6, .4, .2), (.2, .1, .3))] + [None] * (nm - 1)),
            scs[2].with_look(lights=[None] * (nl - 1) + [((.9, .2, .1), (.1, .8, .3))], ambient=(.35, .15, .6))]


def test_relight_with_per_record_looks(torch_cuda, scenes):
    """every pixel of three records under three looks — one with a NaN diffuse and an infinite specular intensity, one that gives
    material #0 a colour, one tinted: relight_into on a fresh context per record, shade_scene_pixels_into(looks), and the packed pixels
    of frame r of render_scene_views_into(looks); looks=None: the shading query on the scenes themselves"""
    scs = records(scenes)
    looks = record_looks(scs)
    xy = SQ.all_pixels()
    n = W * H
    r = open_fresh(scs[0])
    try:
        p, _ = scene_capture(torch_cuda, r, scs, n, size=(W, H), light_stride=3 * n + 11)
        got = scene_relight(torch_cuda, r, scs, looks, p, n)
        own = scene_relight(torch_cuda, r, scs, None, p, n)
        shaded = SQ.scene_query(torch_cuda, r, "shade", looks, n, xy=xy, size=(W, H))
        shaded_own = SQ.scene_query(torch_cuda, r, "shade", scs, n, xy=xy, size=(W, H))
        out = V.alloc_batch(torch_cuda, 3, W, H)
        torch_cuda.cuda.synchronize()
        r.render_scene_views_into(out["frame"].data_ptr(), None, looks, W, H, debug=out["dbg"])
        r.sync()
        frames = V.collect(out, *out["geom"])
        for rec, sc in enumerate(scs):
            fresh = open_fresh(sc)
            try:
                fp, _ = capture_pixels(torch_cuda, fresh, W, H)
                assert_same(got[rec], relight(torch_cuda, fresh, looks[rec], fp), RELIT, f"record {rec}: relight_into on a fresh context")
            finally:
                fresh.close()
            assert_same(got[rec], shaded[rec], RELIT, f"record {rec}: shade_scene_pixels_into(looks)")
            assert_same(got[rec], dict(pixel=frames["xrgb"][rec].ravel(), rgb=frames["rgb"][rec].reshape(-1, 3)), ("pixel", "rgb"),
                        f"record {rec}: frame {rec} of render_scene_views_into(looks)")
            assert_same(own[rec], shaded_own[rec], RELIT, f"record {rec}: looks=None")
        assert not R.same_bits(got[0]["rgb_linear"], own[0]["rgb_linear"]).all() and np.isnan(looks[0].lights()[0].diffuse_intensity.x)
    finally:
        r.close()


def test_relit_ray_lists_are_the_shading_query_of_the_looks(torch_cuda, scenes):
    """... and over a captured list of rays: shade_scene_rays_into on `looks`"""
    scs = records(scenes)
    looks = record_looks(scs)
    shared, _ = ray_lists(scenes)
    r = open_fresh(scs[0])
    try:
        p, _ = scene_capture(torch_cuda, r, scs, N, rays=shared)
        got = scene_relight(torch_cuda, r, scs, looks, p, N)
        shaded = SQ.scene_query(torch_cuda, r, "shade", looks, N, rays=shared)
        for rec in range(3):
            assert_same(got[rec], shaded[rec], RELIT, f"record {rec}: shade_scene_rays_into(looks)")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------ refusals, state, streams
def test_refusals(torch_cuda, scenes):
    """the refusals in the header's order, each with nothing written; n = 0; a look that moves a light in record 1 alone is named"""
    scs = records(scenes)
    shared, _ = ray_lists(scenes)
    d_rays = torch_cuda.from_numpy(shared.copy()).to("cuda:0")
    d_xy = torch_cuda.zeros(2 * N, dtype=torch_cuda.int32, device="cuda:0")
    nl = len(scs[0].lights())
    planes, colours = Planes(torch_cuda, 3 * N, nl), Colours(torch_cuda, 3 * N)
    torch_cuda.cuda.synchronize()
    lib = gpu.gpu_lib()
    progs = [sc.flatten() for sc in scs]
    arr = (S.Program * 3)(*progs)
    cams = (S.FrameCamera * 3)(*[sc.frame_camera(8, 8) for sc in scs])
    a = planes.args()
    out = gpu.LightPasses(a["factors_ptr"], 0, a["id_ptr"], a["dist_ptr"], a["steps_ptr"])
    relit = gpu.Relit(*(colours.args()[f + "_ptr"] for f in RELIT))
    rays, xy = d_rays.data_ptr(), d_xy.data_ptr()
    c_rays = gpu.C.cast(gpu.C.c_void_p(rays), gpu.C.POINTER(gpu.C.c_float))
    c_xy = gpu.C.cast(gpu.C.c_void_p(xy), gpu.C.POINTER(gpu.C.c_uint32))
    refusal = TS.refusal
    who = "scene light passes"

    empty = gpu.Renderer(0)
    try:    # without a program: a bad argument first, then the program, and only then the records
        assert lib.lol_gpu_light_scene_rays(empty._ctx, arr, 3, c_rays, N, 0, -1, out, None) == ERR_ARG
        assert lib.lol_gpu_light_scene_rays(empty._ctx, None, 0, c_rays, N, 1, 256, out, None) == ERR_NO_PROGRAM
        assert lib.lol_gpu_light_scene_pixels(empty._ctx, None, None, 0, 0, 8, 256, c_xy, N, 1, out, None) == ERR_NO_PROGRAM
        assert lib.lol_gpu_relight_scenes(empty._ctx, None, None, 0, out, N, relit, None) == ERR_NO_PROGRAM
    finally:
        empty.close()

    r = open_fresh(scs[0])
    try:
        ctx = r._ctx
        error = lambda: r._lib.lol_gpu_error(ctx).decode()                       # noqa: E731
        into, pixels_into, ptrs = r.light_scene_rays_into, r.light_scene_pixels_into, planes.args()
        no_stride = {k: v for k, v in ptrs.items() if k != "light_stride"}
        # 1. the capture's own, in its order — each beats everything behind it
        assert lib.lol_gpu_light_scene_rays(None, arr, 3, c_rays, N, 0, 256, out, None) == ERR_ARG
        assert refusal(lambda: into(scs, 0, N, 1, -1, **ptrs)) == (ERR_ARG, who + ": no list")
        assert lib.lol_gpu_light_scene_rays(ctx, None, 0, c_rays, N, 1, -1, None, None) == ERR_ARG and error() == who + ": no output"
        assert refusal(lambda: into(scs, rays, N, 1, -1, **ptrs)) == (ERR_ARG, who + ": max_steps < 0 or more than 2^32 - 1 rays")
        assert refusal(lambda: into(scs, rays, 1 << 32, 1, **ptrs)) == (ERR_ARG, who + ": max_steps < 0 or more than 2^32 - 1 rays")
        assert refusal(lambda: into([], rays, N, 1, factors_ptr=ptrs["factors_ptr"])) == (ERR_ARG, "light passes: no hit_id plane")
        assert refusal(lambda: into([], rays, N, 1, id_ptr=ptrs["id_ptr"])) == (ERR_ARG, "light passes: no factors, and the program has lights")
        assert refusal(lambda: into([], rays, N, 1, **dict(ptrs, factors_ptr=ptrs["factors_ptr"] + 4)))[1] == "light passes: factors must be 16-byte aligned"
        assert refusal(lambda: into([], rays, N, 1, light_stride=N - 1, **no_stride))[1] == "light passes: light_stride is neither 0 nor at least n"
        assert lib.lol_gpu_light_scene_pixels(ctx, None, None, 0, 0, 8, 256, c_xy, N, 1, out, None) == ERR_ARG
        assert error() == who + ": no camera or bad frame geometry"
        assert lib.lol_gpu_light_scene_pixels(ctx, cams, arr, 3, 8, 0, 256, c_xy, 0, 0, out, None) == ERR_ARG                 # ... with n = 0 too
        assert lib.lol_gpu_light_scene_pixels(ctx, None, None, 0, 8, 8, 256, None, 63, 1, out, None) == ERR_ARG
        assert error() == who + ": no list of pixels, and n is not w * h"
        # 2. the records, their lists and the planes of all of them, in the header's order
        assert lib.lol_gpu_light_scene_rays(ctx, None, 0, c_rays, N, 1, 256, out, None) == ERR_ARG and error() == who + ": no scenes"
        for n_scenes in (0, -1, gpu.MAX_VIEWS + 1):
            assert lib.lol_gpu_light_scene_rays(ctx, arr, n_scenes, c_rays, N, 1, 256, out, None) == ERR_ARG
            assert error() == who + ": the number of scenes is not in 1 ... LOL_GPU_MAX_VIEWS"
        assert lib.lol_gpu_light_scene_pixels(ctx, None, arr, 3, 8, 8, 256, c_xy, N, 1, out, None) == ERR_ARG and error() == who + ": no cameras"
        for stride in (1, N - 1):
            assert refusal(lambda: into(scs, rays, N, stride, light_stride=N, **no_stride)) == (ERR_ARG, who + ": list_stride is neither 0 nor at least n")
        big = (1 << 32) // 3 + 1
        assert refusal(lambda: into(scs, rays, big, 0, light_stride=big, **no_stride)) == (ERR_ARG, who + ": more than 2^32 - 1 rays over all scenes")
        for light_stride in (N, 3 * N - 1):
            assert refusal(lambda: into(scs + [scenes["scene"]], rays, N, 0, light_stride=light_stride, **no_stride)) == (
                ERR_ARG, who + ": light_stride is neither 0 nor at least n_scenes * n")
        # 3. the scenes, in lol_gpu_render_scene_views' words
        assert refusal(lambda: into(scs + [scenes["scene"]], rays, N, 0, **ptrs)) == (
            ERR_ARG, "a view's scene has not the uploaded program's structure (counts, opcodes, ids)")
        broken = (S.Program * 2)(progs[0], progs[1])
        broken[1].materials = None
        assert lib.lol_gpu_light_scene_rays(ctx, broken, 2, c_rays, N, 0, 256, out, None) == ERR_ARG
        assert error() == "malformed scene of a view: a table is missing"
        roots = (type(progs[1].root_material.contents) * progs[1].n_roots)(*[progs[1].root_material[i] for i in range(progs[1].n_roots)])
        roots[0] = progs[1].n_materials
        bad_root = (S.Program * 2)(progs[0], progs[1])
        bad_root[1].root_material = roots
        assert lib.lol_gpu_light_scene_rays(ctx, bad_root, 2, c_rays, N, 0, 256, out, None) == ERR_ARG
        assert error() == "material index out of range in a view's scene"
        # n = 0: fine behind every refusal, with no list at all, and nothing launched
        into(scs, 0, 0, 0, **ptrs)
        pixels_into(scs, 0, 8, 8, 0, xy_ptr=xy, **ptrs)
        assert refusal(lambda: into(scs + [scenes["scene"]], 0, 0, 0, **ptrs))[0] == ERR_ARG

        # the relight: 1. lol_gpu_relight's own ...
        rel, rp, cp = r.relight_scenes_into, planes.relight_args(), colours.args()
        rp_no_stride = {k: v for k, v in rp.items() if k != "light_stride"}
        assert lib.lol_gpu_relight_scenes(ctx, None, None, 0, None, N, relit, None) == ERR_ARG and error() == "relight: no planes or no output"
        assert refusal(lambda: rel([], None, N, **rp)) == (ERR_ARG, "relight: no output")
        assert refusal(lambda: rel([], None, 1 << 32, **rp, **cp)) == (ERR_ARG, "relight: more than 2^32 - 1 elements")
        assert refusal(lambda: rel([], None, N, factors_ptr=rp["factors_ptr"], **cp)) == (ERR_ARG, "light passes: no hit_id plane")
        assert refusal(lambda: rel([], None, N, light_stride=N - 1, **rp_no_stride, **cp))[1] == "light passes: light_stride is neither 0 nor at least n"
        # ... 2. the records ...
        assert lib.lol_gpu_relight_scenes(ctx, None, None, 0, out, N, relit, None) == ERR_ARG and error() == "relight scenes: no scenes"
        for n_scenes in (0, gpu.MAX_VIEWS + 1):
            assert lib.lol_gpu_relight_scenes(ctx, arr, arr, n_scenes, out, N, relit, None) == ERR_ARG
            assert error() == "relight scenes: the number of scenes is not in 1 ... LOL_GPU_MAX_VIEWS"
        assert refusal(lambda: rel(scs, None, big, light_stride=big, **rp_no_stride, **cp)) == (ERR_ARG, "relight scenes: more than 2^32 - 1 elements over all scenes")
        assert refusal(lambda: rel(scs + [scenes["scene"]], None, N, light_stride=3 * N - 1, **rp_no_stride, **cp)) == (
            ERR_ARG, "relight scenes: light_stride is neither 0 nor at least n_scenes * n")
        # ... 3. the scenes ...
        moved = scs[1].with_lighting(points=[None] * (nl - 1) + [(1., 2., 3.)])
        assert refusal(lambda: rel(scs[:2] + [scenes["scene"]], [scs[0], moved, scenes["scene"]], N, **rp, **cp)) == (
            ERR_ARG, "a view's scene has not the uploaded program's structure (counts, opcodes, ids)")
        # ... 4. the first look that is no look of its scene, by its record: a light moved in record 1 alone; an op in record 2
        assert refusal(lambda: rel(scs, [scs[0], moved, scs[2]], N, **rp, **cp)) == (
            ERR_ARG, "relight scenes: record 1: the look moves a light: capture again")
        assert refusal(lambda: rel(scs, [scs[0], scs[1], scs[1]], N, **rp, **cp)) == (
            ERR_ARG, "relight scenes: record 2: the look differs from the uploaded program in an op (opcode, id or a number): capture again")
        assert refusal(lambda: rel(scs, [scs[0], moved, scs[1]], N, **rp, **cp))[1].startswith("relight scenes: record 1: ")
        rel(scs, None, 0, **rp, **cp)                                             # n = 0
        r.sync()
        torch_cuda.cuda.synchronize()
        assert planes.untouched() and colours.untouched()
        assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), shared.view(np.uint32))
        # the context stays usable
        _, got = scene_capture(torch_cuda, r, scs, N, rays=shared)
        assert_same(got[1], single(torch_cuda, scs[1], ("shared", 1), 7, rays=shared), fields(False), "after the refusals")
    finally:
        r.close()


def test_the_context_is_what_it_was(torch_cuda, scenes):
    """frame, capture and relight over records, frame — on a DEFAULT context, its scene kernel loaded: the frames are equal, kernel_key
    and the tile order are what they were, and the interpreter answered (same bits)"""
    scs = records(scenes)
    shared, _ = ray_lists(scenes)
    r = gpu.Renderer(0)
    try:
        r.prepare(scs[0])
        assert r.kernel_name() == "lol_render_spec", r.specialize_log()
        a = TS.frame(torch_cuda, r, 37, 11)
        key, order = r.kernel_key(), r.tile_order()
        p, got = scene_capture(torch_cuda, r, scs, N, rays=shared)
        assert_same(got[2], single(torch_cuda, scs[2], ("shared", 2), 7, rays=shared), fields(False), "rays on a default context")
        _, px = scene_capture(torch_cuda, r, scs, 13 * 5, size=(13, 5))
        assert_same(px[1], single(torch_cuda, scs[1], ("state", 1), 7, size=(13, 5), all_pixels=True), fields(True), "pixels on a default context")
        lit = scene_relight(torch_cuda, r, scs, record_looks(scs), p, N)
        assert_same(lit[1], SQ.scene_query(torch_cuda, r, "shade", record_looks(scs), N, rays=shared)[1], RELIT, "relit on a default context")
        assert r.kernel_name() == "lol_render_spec"
        assert r.kernel_key() == key and r.tile_order() == order and order["mode"] == "lpt"
        b = TS.frame(torch_cuda, r, 37, 11)
        for f in a:
            assert R.same_bits(a[f], b[f]).all(), f
        assert r.kernel_key() == key
    finally:
        r.close()


def test_two_streams_and_the_special_handles(torch_cuda, scenes):
    """LOL_GPU_STREAM_DEFAULT, the context's own stream, and two torch streams with a capture and its relight in flight on each and no
    wait between them — ten captures and ten relights in all through their rings of 8 sets"""
    scs = records(scenes)
    looks = record_looks(scs)
    shared, _ = ray_lists(scenes)
    nl = len(scs[0].lights())
    r = open_fresh(scs[0])
    try:
        want = [single(torch_cuda, sc, ("shared", rec), 7, rays=shared) for rec, sc in enumerate(scs)]
        want_lit = SQ.scene_query(torch_cuda, r, "shade", looks, N, rays=shared)
        for stream in (0, None):
            p, got = scene_capture(torch_cuda, r, scs, N, rays=shared, stream=stream)
            lit = scene_relight(torch_cuda, r, scs, looks, p, N, stream=stream)
            for rec in range(3):
                assert_same(got[rec], want[rec], fields(False), f"stream {stream}, record {rec}")
                assert_same(lit[rec], want_lit[rec], RELIT, f"stream {stream}, record {rec}: relit")
        s1, s2 = torch_cuda.cuda.Stream(), torch_cuda.cuda.Stream()
        d_rays = torch_cuda.from_numpy(shared.view(np.int32).copy()).to("cuda:0")
        outs = [(Planes(torch_cuda, 3 * N, nl), Colours(torch_cuda, 3 * N)) for _ in range(8)]
        torch_cuda.cuda.synchronize()
        for i, (p, c) in enumerate(outs):                                        # (nothing waits between the calls)
            s = (s1, s2)[i % 2].cuda_stream
            r.light_scene_rays_into(scs, d_rays.data_ptr(), N, 0, stream=s, **p.args())
            r.relight_scenes_into(scs, looks, N, stream=s, **p.relight_args(), **c.args())
        s1.synchronize()
        s2.synchronize()
        for i, (p, c) in enumerate(outs):
            got, lit = split(p.collect(), 3, N), split(c.collect(), 3, N)
            for rec in range(3):
                assert_same(got[rec], want[rec], fields(False), f"call {i} of two streams, record {rec}")
                assert_same(lit[rec], want_lit[rec], RELIT, f"call {i} of two streams, record {rec}: relit")
    finally:
        r.close()


# --------------------------------------------------------------------------------------------------------------------------- the CLI
def test_the_tween_host_relights_an_animation(torch_cuda, scenes, tmp_path):
    """A.lol --tween B.lol --frames 3 --relight L0.lol L1.lol -o DIR writes DIR/look_LLLL_frame_FFFF.ppm: the frames the tweened scenes
    render under each look's intensities and colours, byte for byte; what does not go with it is refused with a sentence each"""
    from test_gpu_scene_view_samples import read_ppm
    a_file, b_file = SQ.tween_files(tmp_path)
    text = open(a_file).read()
    a, other = scenes["scene4"], S.Scene.parse_file(b_file)
    look_files = []
    edits = ([("color = (0.03, 0.03, 0.03)", "color = (0.25, 0.125, 0.5)")],
             [("diffuse_intensity\t= (4, 4, 4),", "diffuse_intensity\t= (0.75, 3, 0.5),"), ("diffuse\t\t= (0, 0, 0),", "diffuse\t\t= (0.375, 0.25, 0.125),")])
    for i, pairs in enumerate(edits):
        look_text = text
        for old, new in pairs:
            assert look_text.count(old) == 1, old
            look_text = look_text.replace(old, new)
        look_files.append(str(tmp_path / f"look{i}.lol"))
        with open(look_files[-1], "w") as f:
            f.write(look_text)
    file_looks = [S.Scene.parse_file(path) for path in look_files]
    assert all(S.same_geometry(a, look) and look.tables() != a.tables() for look in file_looks)
    w, h, n = 32, 16, 3
    scs = [S.tween(a, other, t) for f in range(n) for t in S.shutter_times(f, n, 1)]
    out_dir = tmp_path / "relit"
    base = [a_file, "--tween", b_file, "--frames", str(n), "--size", f"{w}x{h}"]
    p = SQ.run_cli(base + ["--relight"] + look_files + ["-o", str(out_dir)])
    assert p.returncode == 0, p.stdout
    assert sorted(os.listdir(out_dir)) == [f"look_{i:04d}_frame_{f:04d}.ppm" for i in range(2) for f in range(n)]
    r = open_fresh(a)
    try:
        for i, look in enumerate(file_looks):
            out = V.alloc_batch(torch_cuda, n, w, h, None, None, False)
            torch_cuda.cuda.synchronize()
            r.render_scene_views_into(out["frame"].data_ptr(), [a.camera] * n, [look_of(sc, look) for sc in scs], w, h)
            r.sync()
            frames = V.collect(out, *out["geom"])["xrgb"]
            for f in range(n):
                assert np.array_equal(read_ppm(out_dir / f"look_{i:04d}_frame_{f:04d}.ppm", w, h), frames[f] & 0xFFFFFF), (i, f)
            assert not np.array_equal(frames[0], frames[n - 1])
    finally:
        r.close()
    for flags, word in ((["--tween-shutter", "2"], "--tween-shutter"), (["--samples", "2"], "--samples"),
                        (["--lens", "0.0625", "--focus", "4"], "--lens"), (["--move-lights"], "--move-lights")):
        p = SQ.run_cli(base + ["--relight", look_files[0], "-o", str(tmp_path / "no")] + flags)
        assert p.returncode == 1 and f"does not go with {word}:" in p.stdout, p.stdout
    assert not os.path.exists(tmp_path / "no")
