"""The list kernels on the hostile scenes of tests/scene_shapes.py, with rays of their own (tests/hostile_rays.py), under the library's
default switches (no LOL_GPU_TUNING): ray queries (trace_interp, lol_trace_spec), shading queries (shade_interp, lol_shade_spec), light
passes (light_interp), the two resolves (relight_rays, relight_views) and light updates (light_update_interp).

tests/test_gpu_hostile.py holds the kernels that render FRAMES to the oracle on these scenes: a frame's wave is 64 neighbouring pixels of
one camera.  A list's wave is 64 unrelated origins and directions, which is where the culling plan's skips (every lane must agree), the
interpreter's wave-uniform cool-down and the bound the scene kernels carry along each ray are least protected by coherence — and on
scenes of two or three objects a wrong constant in a cull record, a cool-down that survives a loop it should not or a bound taken over
from a wave-mate's ray cannot show.  Each list goes through every family in two orders, object-major (whole waves may skip the same runs)
and a seeded permutation (the lanes of a wave disagree): a ray's answer must not depend on the order.

Every comparison is the family's own (test_gpu_rays.assert_is_reference, test_gpu_shades.assert_is_reference and both_ways,
test_gpu_light.assert_factors and assert_same, test_gpu_light_update.run_case): ray_reference.same_bits, equality of bit patterns, two
NaNs counting as the same; no tolerance of its own.  tests/test_hostile_rays.py holds, on the CPU, that the lists hold the populations
and reach the objects that make these comparisons mean something.
"""
import contextlib
import os

import numpy as np
import pytest

import hostile_rays as HR
import light_reference as LR
import ray_reference as R
import scene_shapes as C
import shade_reference as SR
import test_gpu_light as TL
import test_gpu_light_update as TU
import test_gpu_light_views as TV
import test_gpu_rays as TR
import test_gpu_shades as TS
from loltracer_amd import gpu
from loltracer_amd import scene as S
from test_gpu_parity import gpu_render

pytestmark = pytest.mark.gpu

names = lambda e: e.name                 # noqa: E731
LIT = [e for e in C.HOSTILE if "point_light" in e.text]
DARK = [e for e in C.HOSTILE if e not in LIT]
AVERAGED = [C.HOSTILE_BY_NAME[n] for n in ("tie-crowd", "stress06", "stress12")]
UPDATE_SIZE = (16, 8)                    # two waves


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@contextlib.contextmanager
def telling(e, what):
    """every failure says which scene it was, what that scene is for and what it holds"""
    try:
        yield
    except AssertionError as err:
        raise AssertionError(f"{e.name} {what}: {err}\n{e.purpose}\n{e.text}") from err


def open_queries(e, specialize):
    """ONE context for the ray and the shading queries of a (scene, mode): both switches on, so that the scene compiler makes one
    module for both — and every context of that (scene, mode) after it finds that module made"""
    assert e.own_kernel
    r = gpu.Renderer(0, specialize=specialize)
    try:
        r.set_ray_queries(True)
        r.set_shade_queries(True)
        r.prepare(C.hostile_scene(e))
        assert r.kernel_name() == TR.FRAME[specialize], r.specialize_log()
        assert r.trace_kernel_name() == TR.TRACE[specialize], r.specialize_log()
        assert r.shade_kernel_name() == TS.SHADE[specialize], r.specialize_log()
    except BaseException:
        r.close()
        raise
    return r


def take(ref, idx):
    return {f: ref[f][idx] for f in ref}


def test_the_library_runs_under_its_default_switches():
    assert "LOL_GPU_TUNING" not in os.environ


def test_the_catalogue_is_the_whole_of_it():
    assert len(C.HOSTILE) == C.N_HOSTILE_GENERATED + len(C.HOSTILE_TIES) and len(DARK) == 5
    assert all(len(C.hostile_scene(e).lights()) == 2 for e in AVERAGED[1:])


# ----------------------------------------------------------------------------------------------------------------- a. ray queries
@pytest.mark.parametrize("mode", ["spec", "interp", "interp-plain", "spec-plain"])
@pytest.mark.parametrize("e", C.HOSTILE, ids=names)
def test_ray_queries(torch_cuda, e, mode):
    """trace_rays of the list in both orders, prefixes of 1 and 65 rays and the whole list, with 256 steps and with ONE: dist, id,
    steps and normal are ray_reference's.  Then trace_pixels of every pixel of e.size under the scene's own camera: the dist, id and
    steps planes of a frame of a second context, which test_gpu_hostile holds to the oracle."""
    sc, (w, h) = C.hostile_scene(e), e.size
    r, r2 = open_queries(e, TR.MODES[mode]), gpu.Renderer(0, specialize=TR.MODES[mode])
    try:
        with telling(e, mode):
            for max_steps in (256, 1):
                ref = R.reference(sc, HR.hostile_ray_list(e), max_steps)
                for order, rays, idx in HR.hostile_ray_orders(e):
                    want = take(ref, idx)
                    for n in (1, 65, len(rays)):
                        got = TR.trace_rays(torch_cuda, r, rays, n=n, max_steps=max_steps)
                        TR.assert_is_reference(got, take(want, slice(0, n)), f"{order} n={n} max_steps={max_steps}", rays)
            assert r.trace_kernel_name() == TR.TRACE[TR.MODES[mode]]
            g = gpu_render(torch_cuda, r2, sc, w, h)
            assert r2.kernel_name() == TR.FRAME[TR.MODES[mode]], r2.specialize_log()
            planes = dict(dist=g["dist"].ravel(), id=g["id"].ravel(), steps=(g["steps"] & 0xFFFF).ravel())
            got = TR.trace_pixels(torch_cuda, r, TR.all_pixels(w, h), w, h)
            TR.assert_is_reference({f: got[f] for f in planes}, planes, f"every pixel of {w}x{h} against the frame's planes")
    finally:
        r2.close()
        r.close()


# ------------------------------------------------------------------------------------------------------------- b. shading queries
@pytest.mark.parametrize("mode", ["spec", "interp"])
@pytest.mark.parametrize("e", C.HOSTILE, ids=names)
def test_shading_queries(torch_cuda, e, mode):
    """both_ways on the list in both orders (skips off: all six outputs; default skips: everything but the shadow steps) against
    shade_reference; then shade_pixels of every pixel of e.size: the pixels, colours and planes of a frame of a second context (the
    shadow steps aside: which waves of escaped rays skip their lights depends on which pixels share a wave)"""
    sc, (w, h) = C.hostile_scene(e), e.size
    r, r2 = open_queries(e, TS.MODES[mode]), gpu.Renderer(0, specialize=TS.MODES[mode])
    try:
        with telling(e, mode):
            ref = SR.reference(sc, HR.hostile_ray_list(e))
            for order, rays, idx in HR.hostile_ray_orders(e):
                TS.both_ways(torch_cuda, r, rays, TS.take(ref, idx), order)
            assert r.shade_kernel_name() == TS.SHADE[TS.MODES[mode]]
            r2.prepare(sc)
            assert r2.kernel_name() == TS.FRAME[TS.MODES[mode]], r2.specialize_log()
            want = TS.frame(torch_cuda, r2, w, h)
            got = TS.shade_pixels(torch_cuda, r, TS.all_pixels(w, h), w, h)
            TS.assert_is_reference(TS.take(got, slice(None), tuple(want)), want, f"every pixel of {w}x{h} against the frame", march_steps_only=True)
    finally:
        r2.close()
        r.close()


# -------------------------------------------------------------------------------------------------- c. light passes and the resolve
@pytest.mark.parametrize("mode", ["default", "interp"])
@pytest.mark.parametrize("e", C.HOSTILE, ids=names)
def test_light_passes_and_the_resolve(torch_cuda, e, mode):
    """capture of the list in both orders, with the exact skips on and off, dense and with a stride between the lights' planes:
    light_reference's factors (shadow_steps when exact).  relight(None) is the shading query of the same context and
    light_reference.relit under the scene itself — in a scene without a light there are no factors, the capture still writes id,
    dist and steps, and the colour is the ambient term.  relight(look) is the shading query of a context that uploaded the look, and
    light_reference.relit_reference.  capture_pixels is the frame's planes, and its relights are the frames."""
    sc, (w, h) = C.hostile_scene(e), e.size
    look = HR.hostile_look(sc)
    nl = len(sc.lights())
    r, r2 = TL.open_renderer(sc, TL.MODES[mode]), TL.open_renderer(look, TL.MODES[mode])
    try:
        with telling(e, mode):
            ref = LR.reference(sc, HR.hostile_ray_list(e))
            for order, rays, idx in HR.hostile_ray_orders(e):
                want, n = take(ref, idx), len(rays)
                for skips in (7, 0):
                    r.set_exact_skips(skips)
                    for stride in (0, n + 7):
                        p, got = TL.capture(torch_cuda, r, rays, stride=stride)
                        assert (p.factors is None) == (nl == 0)
                        TL.assert_factors(got, want, n, f"{order} skips={skips} stride={stride}", skips == 0)
                r.set_exact_skips(7)
                own = TL.relight(torch_cuda, r, None, p)
                TL.assert_same(own, TS.shade_rays(torch_cuda, r, rays, want=TL.RELIT), TL.RELIT, f"{order}: relight(None) against the shading query")
                TL.assert_same(own, LR.relit_reference(want, sc), TL.RELIT, f"{order}: relight(None) against light_reference.relit")
                got = TL.relight(torch_cuda, r, look, p)
                TL.assert_same(got, TS.shade_rays(torch_cuda, r2, rays, want=TL.RELIT), TL.RELIT, f"{order}: relight(look) against a context that uploaded it")
                TL.assert_same(got, LR.relit_reference(want, look), TL.RELIT, f"{order}: relight(look) against light_reference.relit")
            p, got = TL.capture_pixels(torch_cuda, r, w, h)
            own = TS.frame(torch_cuda, r, w, h)
            TL.assert_same(dict(id=got["id"], dist=got["dist"], steps=got["steps"]), dict(own, steps=own["steps"] & 0xFFFF), ("id", "dist", "steps"),
                           f"{w}x{h}: the planes against the frame's")
            TL.assert_same(TL.relight(torch_cuda, r, None, p, want=("rgb", "pixel")), own, ("rgb", "pixel"), f"{w}x{h}: the own frame")
            TL.assert_same(TL.relight(torch_cuda, r, look, p, want=("rgb", "pixel")), TS.frame(torch_cuda, r2, w, h), ("rgb", "pixel"),
                           f"{w}x{h}: the frame of the look")
    finally:
        r2.close()
        r.close()


# ------------------------------------------------------------------------------------------------------------------ d. light updates
@pytest.mark.parametrize("source", ["rays", "pixels"])
@pytest.mark.parametrize("e", LIT, ids=names)
def test_light_updates(torch_cuda, e, source):
    """test_gpu_light_update.run_case on the interpreter under lighting_look — every light moved, every shininess changed: the list in
    both orders, and every pixel of a 16 x 8 frame; every pair of masks; shadow_steps for lists after set_exact_skips(0), for pixels
    always.  The update rebuilds what the march left from the planes alone and reads nothing else of it: on scenes of up to 41
    objects that the culling plan re-orders, with ties, that is not what three-object scenes show."""
    sc = C.hostile_scene(e)
    look = TU.lighting_look(sc)
    with telling(e, source):
        if source == "rays":
            for order, rays, _ in HR.hostile_ray_orders(e):
                TU.run_case(torch_cuda, sc, look, "interp", "rays", rays, order, stride_pad=7 if order == "permuted" else 0)
        else:
            w, h = UPDATE_SIZE
            TU.run_case(torch_cuda, sc, look, "interp", "pixels", R.camera_rays(sc, w, h), f"{w}x{h}", size=UPDATE_SIZE)


@pytest.mark.parametrize("e", DARK, ids=names)
def test_light_updates_without_a_light(torch_cuda, e):
    """a scene without a light has no light to update: any mask but (0, 0) is refused, by a list and by pixels, and (0, 0) launches
    nothing — either way every plane holds what the capture wrote"""
    sc = C.hostile_scene(e)
    look = TU.lighting_look(sc)
    rays = HR.hostile_ray_list(e)
    w, h = UPDATE_SIZE
    r = TL.open_renderer(sc, TL.MODES["interp"])
    try:
        with telling(e, "no light"):
            d_rays = torch_cuda.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
            p, _ = TL.capture(torch_cuda, r, rays)
            pp, _ = TL.capture_pixels(torch_cuda, r, w, h)
            assert p.factors is None and pp.factors is None
            before = [{f: t.cpu().numpy().copy() for f, t in q.t.items()} for q in (p, pp)]
            u, up = TU.update_args(p), TU.update_args(pp)
            for march, spec in ((1, 0), (0, 1), (1, 1), (1 << 63, 0), (0, 2)):
                assert TS.refusal(lambda: r.light_update_rays_into(look, d_rays.data_ptr(), len(rays), march, spec, **u)) == (-3, TU.T["mask"]), (march, spec)
                assert TS.refusal(lambda: r.light_update_pixels_into(look, w * h, w, h, march, spec, **up)) == (-3, TU.T["mask"]), (march, spec)
            r.light_update_rays_into(look, d_rays.data_ptr(), len(rays), 0, 0, **u)
            r.light_update_pixels_into(look, w * h, w, h, 0, 0, **up)
            r.sync()
            torch_cuda.cuda.synchronize()
            for q, was in zip((p, pp), before):
                for f, t in q.t.items():
                    assert np.array_equal(t.cpu().numpy(), was[f]), f"{f} was written"
            assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), rays.view(np.uint32)), "the ray buffer was written"
    finally:
        r.close()


# --------------------------------------------------------------------------------------------------------------- e. an averaged picture
@pytest.mark.parametrize("e", AVERAGED, ids=names)
def test_an_averaged_picture(torch_cuda, e):
    """8 x 4, 2 x 2 samples under each of 2 lens cameras: light_views_into and relight_views_into give the supersampled blend of a
    context on the scene's own kernel; after light_update_pixels_into per camera record under lighting_look, relight_views_held_into
    gives the blend of a context that uploaded the look"""
    sc = C.hostile_scene(e)
    look = TU.lighting_look(sc)
    w, h, s, k = 8, 4, 2, 2
    cams = S.lens_cameras(sc.camera, TV.LENS_FOCUS, TV.LENS_RADIUS, k)
    per, n_all = s * s * w * h, k * s * s * w * h
    a, b0, b = TL.open_renderer(sc, 1), TL.open_renderer(sc, 1), TL.open_renderer(look, 1)
    try:
        with telling(e, "averaged"):
            for q in (b0, b):
                assert q.kernel_name() == "lol_render_spec", q.specialize_log()
            p = TV.capture_views(torch_cuda, a, cams, k, w, h, s)
            got = TV.relight_views(torch_cuda, a, None, p, 1, k, w, h, s, want=("rgb", "pixel"))
            TL.assert_same(got, TV.rendered(torch_cuda, b0, cams, k, w, h, s), ("rgb", "pixel"), "the supersampled blend")
            march, spec = S.light_changes(sc, look)
            assert march == (1 << len(sc.lights())) - 1
            u = TU.update_args(p)
            for rec in range(k):
                a.light_update_pixels_into(look, per, s * w, s * h, march, spec, camera=cams[rec], factors_ptr=u["factors_ptr"] + 16 * rec * per,
                                           id_ptr=u["id_ptr"] + 4 * rec * per, dist_ptr=u["dist_ptr"] + 4 * rec * per, light_stride=n_all,
                                           stream=torch_cuda.cuda.current_stream().cuda_stream)
            c = TL.Colours(torch_cuda, w * h, ("rgb", "pixel"))
            a.relight_views_held_into(look, look, 1, k, w, h, s, stream=torch_cuda.cuda.current_stream().cuda_stream, **p.relight_args(), **c.args())
            a.sync()
            torch_cuda.cuda.synchronize()
            p.collect()
            TL.assert_same(c.collect(), TV.rendered(torch_cuda, b, cams, k, w, h, s), ("rgb", "pixel"), "the supersampled blend of the look")
    finally:
        b.close()
        b0.close()
        a.close()
