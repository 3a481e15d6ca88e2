"""Relit scene views on the device (lol_gpu_relight_scene_views, relight_views_scenes): pixel (x, y) of view v IS the float32 tree
mean — over the s x s leaves of each record, then over the K records of the view — of lol_gpu_relight_scenes' rgb_linear under each
record's own look, then gamma and the pixel format; and so the pixel and rgb of render_scene_views_into(cameras, looks, ...,
cameras_per_view=K, samples=s).

Every comparison is ray_reference.same_bits: equality of bit patterns, two NaNs counting as the same; no tolerance.

Records are those of tests/test_gpu_scene_queries.py (scene4, scene4 with a sphere moved, scene4 with a colour on material #0),
record r holding scene r % 3, so that the K > 1 records of every view hold different scenes; look r is recipe r % 4 of LOOKS on
record r's scene — a NaN and an infinite intensity, other material colours, a tinted ambient, the scene's own — so that the K looks
of every view differ.  Shapes: 33 x 16 (a tail wave, rows that are no multiple of a round, more than one wave per view) and 5 x 3
(a view smaller than a wave), three views.  What the inputs must show is asserted on the CPU reference before the device is looked
at (`preconditions`): for 5 x 3 at every s and for 33 x 16 at s = 1; the two 33 x 16 cases with s = 2 would cost the CPU reference
6336 more rays (seven seconds), so there the same two properties are asserted on relight_scenes_into's leaves — the reference arm
of the test, not the call under test.
"""
import os

import numpy as np
import pytest

import light_reference as LR
import light_views_reference as LV
import ray_reference as R
import scene_shapes as SH
import test_gpu_scene_light as SL
import test_gpu_scene_queries as SQ
import test_gpu_shades as TS
import test_gpu_views as V
from loltracer_amd import gpu
from loltracer_amd import scene as S
from loltracer_amd.__main__ import look_of
from test_gpu_light import FACTORS, RELIT, Colours, Planes, assert_same, scene_with_lights
from test_gpu_scene_queries import open_fresh, records

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NO_PROGRAM = -3, -4
N_VIEWS = 3
SMALL, BIG = (5, 3), (33, 16)
SMALL_SHAPES = [(s, k) for s in (1, 2, 4) for k in (1, 2, 4, 8, 16)]          # (s, K)
BIG_SHAPES = [(2, 2), (4, 1), (1, 4), (2, 16)]
NAN, INF = float("nan"), float("inf")
_kept = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def recipe(sc, which):
    """look `which` % 4 on the scene `sc`"""
    nl, nm = len(sc.lights()), len(sc.materials())
    which %= 4
    if which == 0:
        return sc.with_look(lights=([((NAN, .5, .25), (INF, 1., 2.))] + [None] * (nl - 1))[:nl], ambient=(.0625, .25, .125))
    if which == 1:
        return sc.with_look(materials=[((.3, .5, .7), (.6, .4, .2), (.2, .1, .3))] * nm)
    if which == 2:
        return sc.with_look(lights=([None] * (nl - 1) + [((.9, .2, .1), (.1, .8, .3))])[:nl], ambient=(.35, .15, .6))
    return sc


def moved_record(sc):
    """a scene of `sc`'s structure with its first solid moved"""
    b = sc.clone()
    solid = next(i for i in range(sc.c.n_nodes) if sc.c.nodes[i].type in (S.NODE_SPHERE, S.NODE_BOX))
    b.c.nodes[solid].point.x += 0.375
    return b


def case(scenes, k, base=None):
    """(the N_VIEWS K records, their looks, every record under its view's FIRST look)"""
    three = records(scenes) if base is None else base
    scs = [three[r % len(three)] for r in range(N_VIEWS * k)]
    looks = [recipe(sc, r) for r, sc in enumerate(scs)]
    first = [recipe(sc, r // k * k) for r, sc in enumerate(scs)]
    return scs, looks, first


def tree(leaves, k, w, h, s, fmt=None):
    """the contract's steps 2 to 4 on the host: tests/test_gpu_light_views.py's numpy tree"""
    return LV.finish(LV.resolve(leaves, N_VIEWS, k, w, h, s), fmt)


def must_show(leaves, under_first, k, w, h, s, what):
    """what the inputs must show, on per-record leaf colours [record][s^2 w h, 3]: in every view with K > 1 two records differ in a
    leaf, and resolving every record under the view's first look would change an output pixel"""
    if k == 1:
        return
    for v in range(N_VIEWS):
        mine = leaves[v * k:(v + 1) * k]
        assert any((~R.same_bits(mine[0], other)).any() for other in mine[1:]), f"{what}: the records of view {v} are alike"
    want, wrong = tree(np.concatenate(leaves), k, w, h, s), tree(np.concatenate(under_first), k, w, h, s)
    per = w * h
    for v in range(N_VIEWS):
        assert (want["pixel"][v * per:(v + 1) * per] != wrong["pixel"][v * per:(v + 1) * per]).any(), f"{what}: view {v} is the same under its first look"


@pytest.fixture(scope="module")
def preconditions(scenes):
    """asserted on the CPU reference, before any test looks at the device"""
    if "pre" in _kept:
        return True
    three = records(scenes)
    memo = {}

    def relit(w, h, s, i, which):
        """the leaf colours of scene i under its recipe `which` % 4 (case()'s looks), each computed once"""
        key = (w, h, s, i, which % 4)
        if key not in memo:
            if key[:4] not in memo:
                memo[key[:4]] = LR.reference(three[i], R.camera_rays(three[i], s * w, s * h))
            memo[key] = LR.relit_reference(memo[key[:4]], recipe(three[i], which))["rgb_linear"]
        return memo[key]

    for (w, h), shapes in ((SMALL, SMALL_SHAPES), (BIG, [(1, 4)])):
        for s, k in shapes:
            scs = case(scenes, k)[0]
            must_show([relit(w, h, s, r % 3, r) for r in range(len(scs))], [relit(w, h, s, r % 3, r // k * k) for r in range(len(scs))],
                      k, w, h, s, f"{w}x{h} s={s} K={k}")
    looks = case(scenes, 4)[1]
    assert np.isnan(looks[0].lights()[0].diffuse_intensity.x) and np.isinf(looks[0].lights()[0].specular_intensity.x)
    assert looks[2].c.ambient_color.tuple() != records(scenes)[2].c.ambient_color.tuple()
    _kept["pre"] = True
    return True


def capture(torch, r, scs, w, h, s, cameras=None, light_stride=0):
    """the planes of ONE lol_gpu_light_scene_pixels over the s w x s h grid of every record"""
    return SL.scene_capture(torch, r, scs, s * s * w * h, size=(s * w, s * h), cameras=cameras, light_stride=light_stride)[0]


def resolve(torch, r, scs, looks, p, k, w, h, s, want=RELIT, stream="torch", ids=None):
    c = Colours(torch, N_VIEWS * w * h, want)
    torch.cuda.synchronize()
    args = p.relight_args()
    if ids is not None:
        args["id_ptr"] = ids.data_ptr()
    r.relight_scene_views_into(scs, looks, N_VIEWS, k, w, h, s, stream=TS.stream_of(torch, stream), **args, **c.args())
    r.sync()
    torch.cuda.synchronize()
    return c.collect()


def leaves_of(torch, r, scs, looks, p, w, h, s):
    """per record, relight_scenes_into's rgb_linear over the same planes"""
    return [d["rgb_linear"] for d in SL.scene_relight(torch, r, scs, looks, p, s * s * w * h, want=("rgb_linear",))]


def held_to_the_tree(torch, r, scs, looks, w, h, s, k, what, first=None, fmt=None, light_stride=0):
    """test 1's comparison for one shape: canaries behind every output (Colours.collect), the planes unchanged"""
    p = capture(torch, r, scs, w, h, s, light_stride=light_stride)
    before = p.collect()
    leaves = leaves_of(torch, r, scs, looks, p, w, h, s)
    if first is not None:
        must_show(leaves, leaves_of(torch, r, scs, first, p, w, h, s), k, w, h, s, what)
    got = resolve(torch, r, scs, looks, p, k, w, h, s)
    assert_same(got, tree(np.concatenate(leaves), k, w, h, s, fmt), RELIT, what)
    assert_same(p.collect(), before, ("id",) + (FACTORS + ("shadow_steps",) if p.nl else ()), what + ": the planes after the resolve")
    return p, got


# -------------------------------------------------------------------------------------------------- 1. the tree mean of relit leaves
@pytest.mark.parametrize("s", [1, 2, 4])
def test_small_views_are_the_tree_mean_of_relit_leaves(torch_cuda, scenes, preconditions, s):
    """5 x 3, a view smaller than a wave, for every K"""
    r = open_fresh(records(scenes)[0])
    try:
        for k in (1, 2, 4, 8, 16):
            scs, looks, _ = case(scenes, k)
            held_to_the_tree(torch_cuda, r, scs, looks, *SMALL, s, k, f"5x3 s={s} K={k}")
    finally:
        r.close()


@pytest.mark.parametrize("s,k", BIG_SHAPES)
def test_views_are_the_tree_mean_of_relit_leaves(torch_cuda, scenes, preconditions, s, k):
    """33 x 16: a tail wave, rows that are no multiple of a round, more than one wave per view; each output alone is its column"""
    scs, looks, first = case(scenes, k)
    r = open_fresh(records(scenes)[0])
    try:
        p, got = held_to_the_tree(torch_cuda, r, scs, looks, *BIG, s, k, f"33x16 s={s} K={k}", first=first if s == 2 else None)
        for f in RELIT:
            alone = resolve(torch_cuda, r, scs, looks, p, k, *BIG, s, want=(f,))
            assert set(alone) == {f}
            assert_same(alone, got, (f,), f"{f} alone")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------- 2. the frames of the looks
@pytest.mark.parametrize("skips", [7, 0], ids=["default-skips", "skips-off"])
def test_relit_views_are_the_frames_of_the_looks(torch_cuda, scenes, preconditions, skips):
    """pixel and rgb are render_scene_views_into(cameras, looks, ..., cameras_per_view=K, samples=s) on the same renderer, under four
    different cameras — the scene's own, one of the orbit, one with x = -0, one beyond the sane range"""
    w, h = BIG
    four = [c for _, c in TS.frame_cameras(records(scenes)[0])]
    r = open_fresh(records(scenes)[0])
    try:
        r.set_exact_skips(skips)
        for s, k in ((2, 1), (1, 2), (2, 2), (4, 4)):
            scs, looks, _ = case(scenes, k)
            cams = [four[i % 4] for i in range(len(scs))]
            p = capture(torch_cuda, r, scs, w, h, s, cameras=cams)
            got = resolve(torch_cuda, r, scs, looks, p, k, w, h, s)
            out = V.alloc_batch(torch_cuda, N_VIEWS, w, h, debug=("rgb",))
            torch_cuda.cuda.synchronize()
            r.render_scene_views_into(out["frame"].data_ptr(), cams, looks, w, h, k, debug=out["dbg"], samples=s)
            r.sync()
            frames = V.collect(out, *out["geom"])
            want = dict(pixel=np.ascontiguousarray(frames["xrgb"].ravel()), rgb=np.ascontiguousarray(frames["rgb"].reshape(-1, 3)))
            assert_same(got, want, ("pixel", "rgb"), f"s={s} K={k} skips={skips}: the frames of the looks")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------- 3. equal scenes, 4. one leaf per pixel
def test_equal_scenes_are_relit_views(torch_cuda, scenes):
    """every scene the uploaded one and every look one look: relight_views_into(look), byte for byte; looks=None: relight_views_into(None)"""
    sc = records(scenes)[0]
    w, h, s, k = 33, 16, 2, 2
    look = recipe(sc, 2)
    r = open_fresh(sc)
    try:
        scs = [sc] * (N_VIEWS * k)
        p = capture(torch_cuda, r, scs, w, h, s)
        for what, lk in (("a look", look), ("no look", None)):
            c = Colours(torch_cuda, N_VIEWS * w * h)
            torch_cuda.cuda.synchronize()
            r.relight_views_into(lk, N_VIEWS, k, w, h, s, stream=TS.stream_of(torch_cuda, "torch"), **p.relight_args(), **c.args())
            r.sync()
            torch_cuda.cuda.synchronize()
            got = resolve(torch_cuda, r, scs, None if lk is None else [lk] * len(scs), p, k, w, h, s)
            assert_same(got, c.collect(), RELIT, f"equal scenes, {what}")
    finally:
        r.close()


def test_one_sample_and_one_record_is_relight_scenes(torch_cuda, scenes):
    w, h = BIG
    scs, looks, _ = case(scenes, 1)
    r = open_fresh(scs[0])
    try:
        p = capture(torch_cuda, r, scs, w, h, 1)
        want = SL.scene_relight(torch_cuda, r, scs, looks, p, w * h)
        got = resolve(torch_cuda, r, scs, looks, p, 1, w, h, 1)
        assert_same(got, {f: np.concatenate([d[f] for d in want]) for f in RELIT}, RELIT, "K = 1, s = 1")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------ 5. both instantiations
def look_dwords(sc):
    """dwords from one look's tables to the next one's: lights | materials | root_material on a multiple of four dwords"""
    p = sc.flatten()
    return (p.n_lights * 9 + p.n_materials * 10 + p.n_roots + 3) & ~3


@pytest.mark.parametrize("which", ["tree2-tables-K2", "scene4-K8", "scene4-K16", "three-lights-K8", "three-lights-K16", "no-lights-K2"])
def test_both_instantiations(torch_cuda, scenes, which):
    """the K looks of a view staged as one run where K look_dwords <= 1024, read where they lie beyond: scene4 (52 dwords a look) is
    staged at K = 8 (416) and at K = 16 (832) alike; a scene with three lights (68 dwords) is staged at K = 8 (544) and NOT at K = 16
    (1088): the threshold between the two kernels; tree2-tables (110 materials, 1120 dwords) is never staged; a scene without lights,
    factors_ptr = 0"""
    w, h = SMALL
    name, k, s = which[:which.rindex("-K")], int(which[which.rindex("-K") + 2:]), 2
    if name == "scene4":
        base = records(scenes)
    else:
        one = SH.scene_of(SH.RUNG["tree2-tables"]) if name == "tree2-tables" else scene_with_lights(3 if name == "three-lights" else 0)
        base = [one, moved_record(one)]
    staged = k * look_dwords(base[0]) <= 1024
    assert look_dwords(base[0]) == {"tree2-tables": 1120, "scene4": 52, "three-lights": 68}.get(name, look_dwords(base[0]))
    assert staged == (which not in ("tree2-tables-K2", "three-lights-K16"))
    scs, looks, first = case(scenes, k, base)
    r = open_fresh(base[0])
    try:
        assert r.interp_variant()[1] == (name == "tree2-tables")
        p, _ = held_to_the_tree(torch_cuda, r, scs, looks, w, h, s, k, which, first=first)
        assert (p.factors is None) == (name == "no-lights")
    finally:
        r.close()


# ----------------------------------------------------------------- 6. a light stride, 7. an id beyond n_roots, 8. a lossy pixel format
def test_a_light_stride_and_an_id_beyond_the_roots(torch_cuda, scenes):
    w, h, s, k = 33, 16, 2, 2
    scs, looks, _ = case(scenes, k)
    n = len(scs) * s * s * w * h
    r = open_fresh(scs[0])
    try:
        p, got = held_to_the_tree(torch_cuda, r, scs, looks, w, h, s, k, "light_stride > N", light_stride=n + 77)      # (Planes.collect: the gaps)
        dense = capture(torch_cuda, r, scs, w, h, s)
        assert_same(resolve(torch_cuda, r, scs, looks, dense, k, w, h, s), got, RELIT, "dense planes")
        # ids beyond n_roots, written into a copy of the id plane, resolve as id 0
        ids = dense.t["id"].clone()
        host = ids.cpu().numpy().view(np.uint32).copy()
        n_roots = scs[0].flatten().n_roots
        hit = np.flatnonzero(host[:n] != 0)[::3]
        assert len(hit) > 64
        beyond, zeroed = host.copy(), host.copy()
        beyond[hit] = np.where(np.arange(len(hit)) % 2, n_roots + 1, 0xFFFFFFFF).astype(np.uint32)
        zeroed[hit] = 0
        ids.copy_(torch_cuda.from_numpy(beyond.view(np.int32)))
        a = resolve(torch_cuda, r, scs, looks, dense, k, w, h, s, ids=ids)
        ids.copy_(torch_cuda.from_numpy(zeroed.view(np.int32)))
        b = resolve(torch_cuda, r, scs, looks, dense, k, w, h, s, ids=ids)
        assert_same(a, b, RELIT, "ids beyond n_roots")
        assert not R.same_bits(a["rgb_linear"], got["rgb_linear"]).all()
    finally:
        r.close()


def test_a_lossy_pixel_format(torch_cuda, scenes):
    w, h, s, k = 33, 16, 2, 2
    scs, looks, _ = case(scenes, k)
    r = open_fresh(scs[0])
    try:
        r.set_pixel_format(TS.LOSSY)
        _, got = held_to_the_tree(torch_cuda, r, scs, looks, w, h, s, k, "lossy", fmt=TS.LOSSY)
        assert (got["pixel"] & 0xFF000000 == 0xFF000000).all()
    finally:
        r.close()


# ----------------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals(torch_cuda, scenes):
    """every refusal in the header's order, each with the later ones present too; nothing written; the context stays usable"""
    w, h, s, k = 5, 3, 2, 2
    scs, looks, _ = case(scenes, k)
    nr, n = len(scs), len(scs) * s * s * w * h
    nl = len(scs[0].lights())
    planes, colours = Planes(torch_cuda, n, nl), Colours(torch_cuda, N_VIEWS * w * h)
    torch_cuda.cuda.synchronize()
    lib = gpu.gpu_lib()
    progs = [sc.flatten() for sc in scs]
    arr = (S.Program * nr)(*progs)
    moved = scs[1].with_lighting(points=[None] * (nl - 1) + [(1., 2., 3.)])
    moved_prog, other_prog = moved.flatten(), scenes["scene"].flatten()                 # (kept: the arrays below point into them)
    bad_looks = (S.Program * nr)(*([progs[0], moved_prog, progs[1]] + progs[3:]))        # record 1 moves a light, record 2 differs in an op
    other = (S.Program * nr)(*([progs[0], progs[1], other_prog] + progs[3:]))            # record 2 has another structure
    a, ca = planes.args(), colours.args()
    relit = gpu.Relit(*(ca[f + "_ptr"] for f in RELIT))
    refusal = TS.refusal

    def passes(**kw):
        v = dict(a, **kw)
        return gpu.LightPasses(v["factors_ptr"] or None, v["light_stride"], v["id_ptr"] or None, None, None)

    def call(ctx, scenes_=other, looks_=bad_looks, n_views=N_VIEWS, k=k, w=w, h=h, s=s, planes=True, out=relit, **kw):
        return lib.lol_gpu_relight_scene_views(ctx, scenes_, looks_, passes(**kw) if planes else None, n_views, k, w, h, s, out, None)

    empty = gpu.Renderer(0)
    try:        # without a program: a bad argument first, then the program, and only then the records
        assert call(empty._ctx, k=3) == ERR_ARG and call(empty._ctx, scenes_=None) == ERR_NO_PROGRAM
        assert call(empty._ctx, k=1, s=1) == ERR_NO_PROGRAM
    finally:
        empty.close()

    r = open_fresh(scs[0])
    try:
        ctx = r._ctx
        error = lambda: r._lib.lol_gpu_error(ctx).decode()                      # noqa: E731
        # 1. everything relight_views_into refuses before its look — with NULL scenes, another structure and bad looks behind it
        assert call(None) == ERR_ARG
        assert call(ctx, scenes_=None, planes=False) == ERR_ARG and error() == "relight: no planes or no output"
        assert call(ctx, scenes_=None, out=None) == ERR_ARG and error() == "relight: no planes or no output"
        assert call(ctx, scenes_=None, out=gpu.Relit(None, None, None)) == ERR_ARG and error() == "relight: no output"
        for bad in dict(n_views=0), dict(w=0), dict(h=-1):
            assert call(ctx, scenes_=None, **bad) == ERR_ARG and error() == "relit views: n_views < 1 or bad frame geometry", bad
        for bad in (0, 3, 32):
            assert call(ctx, scenes_=None, k=bad) == ERR_ARG and error() == "relit views: cams_per_view must be 1, 2, 4, 8 or 16"
        for bad in (0, 3, 8):
            assert call(ctx, scenes_=None, s=bad) == ERR_ARG and error() == "relit views: samples must be 1, 2 or 4"
        assert call(ctx, scenes_=None, n_views=4096, k=16, s=4, w=1024, h=1024) == ERR_ARG and error() == "relit views: more than 2^32 - 1 elements"
        assert call(ctx, scenes_=None, id_ptr=0) == ERR_ARG and error() == "light passes: no hit_id plane"
        assert call(ctx, scenes_=None, factors_ptr=0) == ERR_ARG and error() == "light passes: no factors, and the program has lights"
        assert call(ctx, scenes_=None, factors_ptr=a["factors_ptr"] + 4) == ERR_ARG and error() == "light passes: factors must be 16-byte aligned"
        for stride in (n - 1, s * s * w * h):
            assert call(ctx, scenes_=None, light_stride=stride) == ERR_ARG and error() == "light passes: light_stride is neither 0 nor at least n"
        # 2. the records — with another structure and bad looks behind them
        assert call(ctx, scenes_=None) == ERR_ARG and error() == "relight scene views: no scenes"
        assert call(ctx, n_views=4097, k=1, w=1, h=1, s=2) == ERR_ARG and error().startswith("relight scene views: more than LOL_GPU_MAX_VIEWS records")
        assert call(ctx, n_views=513, k=8, w=1, h=1, s=1) == ERR_ARG and error().startswith("relight scene views: more than LOL_GPU_MAX_VIEWS records")
        # 3. the scenes — with bad looks behind them
        assert call(ctx) == ERR_ARG and error() == "a view's scene has not the uploaded program's structure (counts, opcodes, ids)"
        assert refusal(lambda: r.relight_scene_views_into(scs[:2] + [scenes["scene"]] + scs[3:], [scs[0], moved] + scs[2:], N_VIEWS, k, w, h, s,
                                                          **planes.relight_args(), **ca))[0] == ERR_ARG
        # 4. the first look that is no look of its scene, by its record
        assert call(ctx, scenes_=arr) == ERR_ARG and error() == "relight scene views: record 1: the look moves a light: capture again"
        assert refusal(lambda: r.relight_scene_views_into(scs, scs[:2] + [scs[1]] + looks[3:], N_VIEWS, k, w, h, s, **planes.relight_args(), **ca)) == (
            ERR_ARG, "relight scene views: record 2: the look differs from the uploaded program in an op (opcode, id or a number): capture again")
        # one leaf per pixel: the statuses are the same (the words are relight_scenes_into's)
        one = Planes(torch_cuda, N_VIEWS * w * h, nl)
        torch_cuda.cuda.synchronize()
        o = one.args()
        assert call(ctx, scenes_=None, k=1, s=1, factors_ptr=o["factors_ptr"], id_ptr=o["id_ptr"]) == ERR_ARG and error() == "relight scene views: no scenes"
        assert call(ctx, k=1, s=1, factors_ptr=o["factors_ptr"], id_ptr=o["id_ptr"]) == ERR_ARG
        assert call(ctx, scenes_=arr, k=1, s=1, factors_ptr=o["factors_ptr"], id_ptr=o["id_ptr"]) == ERR_ARG and error().startswith("relight scenes: record 1: ")
        with pytest.raises(ValueError):
            r.relight_scene_views_into(scs[:-1], None, N_VIEWS, k, w, h, s, **planes.relight_args(), **ca)
        r.sync()
        torch_cuda.cuda.synchronize()
        assert planes.untouched() and colours.untouched() and one.untouched()
        # the context stays usable
        held_to_the_tree(torch_cuda, r, scs, looks, w, h, s, k, "after the refusals")
    finally:
        r.close()


# --------------------------------------------------------------------------------------------------------------- 10. state, 11. streams
def test_the_context_is_what_it_was(torch_cuda, scenes):
    """frame, capture and relit scene views, frame — on a DEFAULT context, its scene kernel loaded: the frames are equal, kernel_key
    and the tile order are what they were"""
    w, h, s, k = 5, 3, 2, 2
    scs, looks, _ = case(scenes, k)
    r = gpu.Renderer(0)
    try:
        r.prepare(scs[0])
        assert r.kernel_name() == "lol_render_spec", r.specialize_log()
        a = TS.frame(torch_cuda, r, 37, 11)
        key, order = r.kernel_key(), r.tile_order()
        held_to_the_tree(torch_cuda, r, scs, looks, w, h, s, k, "on a default context")
        assert r.kernel_name() == "lol_render_spec"
        assert r.kernel_key() == key and r.tile_order() == order and order["mode"] == "lpt"
        b = TS.frame(torch_cuda, r, 37, 11)
        for f in a:
            assert R.same_bits(a[f], b[f]).all(), f
        assert r.kernel_key() == key
    finally:
        r.close()


def test_two_streams_and_the_special_handles(torch_cuda, scenes):
    """LOL_GPU_STREAM_DEFAULT, the context's own stream, and ten resolves alternating between two torch streams with no wait between
    them, under two sets of looks: more than the ring of looks has sets.  Every result is checked."""
    w, h, s, k = 33, 16, 2, 2
    scs, looks, first = case(scenes, k)
    r = open_fresh(scs[0])
    try:
        p = capture(torch_cuda, r, scs, w, h, s)
        wants = [resolve(torch_cuda, r, scs, lk, p, k, w, h, s) for lk in (looks, first)]
        assert not R.same_bits(wants[0]["rgb_linear"], wants[1]["rgb_linear"]).all()
        assert_same(wants[0], tree(np.concatenate(leaves_of(torch_cuda, r, scs, looks, p, w, h, s)), k, w, h, s), RELIT, "torch's stream")
        for stream in (0, None):
            assert_same(resolve(torch_cuda, r, scs, looks, p, k, w, h, s, stream=stream), wants[0], RELIT, f"stream {stream}")
        streams = [torch_cuda.cuda.Stream(), torch_cuda.cuda.Stream()]
        outs = [Colours(torch_cuda, N_VIEWS * w * h) for _ in range(10)]
        torch_cuda.cuda.synchronize()
        for i, c in enumerate(outs):                                               # (nothing waits between the calls)
            r.relight_scene_views_into(scs, (looks, first)[i % 3 == 0], N_VIEWS, k, w, h, s, stream=streams[i % 2].cuda_stream,
                                       **p.relight_args(), **c.args())
        for st in streams:
            st.synchronize()
        for i, c in enumerate(outs):
            assert_same(c.collect(), wants[i % 3 == 0], RELIT, f"call {i} of two streams")
    finally:
        r.close()


# -------------------------------------------------------------------------------------------------------------------------- 12. the CLI
def test_the_tween_host_relights_a_supersampled_animation(torch_cuda, scenes, tmp_path):
    """A.lol --tween B.lol --frames 3 --relight L0.lol L1.lol --tween-samples 2 -o DIR writes DIR/look_LLLL_frame_FFFF.ppm: the frames
    render_scene_views_into(looks, samples=2) renders of the tweened scenes under each look, byte for byte; --tween-shutter stays
    refused, and no directory is made"""
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
    w, h, n = 32, 16, 3
    scs = [S.tween(a, other, t) for f in range(n) for t in S.shutter_times(f, n, 1)]
    out_dir = tmp_path / "relit"
    base = [a_file, "--tween", b_file, "--frames", str(n), "--size", f"{w}x{h}"]
    p = SQ.run_cli(base + ["--relight"] + look_files + ["--tween-samples", "2", "-o", str(out_dir)])
    assert p.returncode == 0 and "relight_views_scenes" in p.stdout, p.stdout
    assert sorted(os.listdir(out_dir)) == [f"look_{i:04d}_frame_{f:04d}.ppm" for i in range(2) for f in range(n)]
    r = open_fresh(a)
    try:
        for i, look in enumerate(file_looks):
            frames = []
            for samples in (2, 1):
                out = V.alloc_batch(torch_cuda, n, w, h, None, None, False)
                torch_cuda.cuda.synchronize()
                r.render_scene_views_into(out["frame"].data_ptr(), [a.camera] * n, [look_of(sc, look) for sc in scs], w, h, samples=samples)
                r.sync()
                frames.append(V.collect(out, *out["geom"])["xrgb"])
            for f in range(n):
                assert np.array_equal(read_ppm(out_dir / f"look_{i:04d}_frame_{f:04d}.ppm", w, h), frames[0][f] & 0xFFFFFF), (i, f)
            assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[0][0], frames[0][n - 1])      # averaged; animated
    finally:
        r.close()
    p = SQ.run_cli(base + ["--relight", look_files[0], "--tween-samples", "2", "--tween-shutter", "2", "-o", str(tmp_path / "no")])
    assert p.returncode == 1 and "does not go with --tween-shutter:" in p.stdout and "cameras_per_view=K" in p.stdout, p.stdout
    assert not os.path.exists(tmp_path / "no")
