"""Light updates on the device: lol_gpu_light_update_rays / lol_gpu_light_update_pixels (light_update_interp) and the resolves of
updated planes (lol_gpu_relight_held, lol_gpu_relight_views_held).

Context A uploads the scene and captures; context B uploads the look — lights moved, shininesses changed — and captures the same
source; A updates.  The updated planes of the masked lights are B's, every other byte is what it was, B's factors are
light_update_reference's from B's own hit_dist / hit_id, and A's relight under the look is B's picture.  Every comparison is
ray_reference.same_bits: no tolerance.  For ray lists with the settled-shadow exit on, shadow_steps is left out (include/lol_gpu.h,
"Light updates": the one difference from a capture); after set_exact_skips(0), and for pixels always, all 16 bytes are compared.
"""
import os
import re

import numpy as np
import pytest

import light_update_reference as UR
import ray_reference as R
import scene_shapes as C
import test_gpu_views as V
from loltracer_amd import gpu
from loltracer_amd import scene as S
from loltracer_amd.__main__ import main as cli_main
from test_gpu_light import (FACTORS, MODES, RELIT, Colours, Planes, assert_same, capture, capture_pixels, forbidden_looks,
                            open_renderer, ray_list, restore)
from test_gpu_shades import frame, refusal, shade_rays, stream_of

pytestmark = pytest.mark.gpu

SEED = 20261020
W, H = 40, 12                            # 480 elements: seven waves and a half
N_RAYS = 1003


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_scenes = {}


def scene_named(scenes, name):
    if name in scenes:
        return scenes[name]
    if name == "three_lights":
        if name not in _scenes:
            _scenes[name] = S.Scene.parse_file(os.path.join(C.SCENES_DIR, "three_lights.lol"))
        return _scenes[name]
    return C.scene_of(C.RUNG[name])


_looks = {}


def lighting_look(sc):
    """the scene with EVERY light moved and every shininess but material 0's changed (kept per scene: the references are keyed by it)"""
    if id(sc) not in _looks:
        pts = [(l.point.x + 1.5, l.point.y - 0.75, l.point.z + 2.25) for l in sc.lights()]
        _looks[id(sc)] = (sc, sc.with_lighting(points=pts, shininess=[None] + [m.shininess * 0.5 + 3 for m in sc.materials()[1:]]))
    return _looks[id(sc)][1]


_long = {}


def long_list(sc, base):
    """about a thousand rays: seeded permutations of `base` one behind the other, so that every ray meets other wave-mates each time
    and the references cost what the distinct rays cost"""
    if id(sc) not in _long:
        rng = np.random.default_rng(SEED)
        reps = -(-N_RAYS // len(base))
        rays = np.ascontiguousarray(np.concatenate([base[rng.permutation(len(base))] for _ in range(reps)])[:N_RAYS], dtype=np.float32)
        rays.setflags(write=False)
        _long[id(sc)] = (sc, rays)
    return _long[id(sc)][1]


def raw(p):
    """every dword of the planes, padding included"""
    out = {f: t.cpu().numpy().view(np.uint32).copy() for f, t in p.t.items()}
    out["factors"] = p.factors.cpu().numpy().view(np.uint32).reshape(-1, 4).copy()
    return out


def update_args(p):
    a = p.args()
    return dict(factors_ptr=a["factors_ptr"], id_ptr=a["id_ptr"], dist_ptr=a["dist_ptr"], light_stride=a["light_stride"])


def masks_of(nl):
    """(march, specular): light 0 alone, the last alone, all, none, specular alone on all, a march and a specular update in one call"""
    full = (1 << nl) - 1
    cases = [(1, 0), (1 << (nl - 1), 0), (full, 0), (0, 0), (0, full), (1, full & ~1), (full, full)]
    return list(dict.fromkeys(cases))


def same_u32_as_f32(a, b):
    return R.same_bits(np.ascontiguousarray(a).view(np.float32), np.ascontiguousarray(b).view(np.float32))


def assert_updated(before, after, want, n, nl, stride, march, spec, all16, what):
    """asserts 1 and 2 of the issue: the masked lights' elements are `want`'s, every other dword is `before`'s"""
    s = stride or n
    allowed = np.zeros(before["factors"].shape, dtype=bool)
    for l in range(nl):
        rows = slice(l * s, l * s + n)
        if march >> l & 1:
            allowed[rows, :] = True
            ok = same_u32_as_f32(after["factors"][rows, :3], want["factors"][rows, :3]).all(axis=1)
            if all16:
                ok &= after["factors"][rows, 3] == want["factors"][rows, 3]
            assert ok.all(), f"{what}: light {l} (marched) differs for {int((~ok).sum())} elements; first {int(np.flatnonzero(~ok)[0])}: " \
                             f"{after['factors'][rows][np.flatnonzero(~ok)[0]]} expected {want['factors'][rows][np.flatnonzero(~ok)[0]]}"
        elif spec >> l & 1:
            allowed[rows, 2] = True
            ok = same_u32_as_f32(after["factors"][rows, 2], want["factors"][rows, 2])
            assert ok.all(), f"{what}: light {l} (specular alone) differs for {int((~ok).sum())} elements; first {int(np.flatnonzero(~ok)[0])}"
    assert np.array_equal(after["factors"][~allowed], before["factors"][~allowed]), f"{what}: a byte outside the masks was written"
    for f in ("id", "dist", "steps"):
        assert np.array_equal(after[f], before[f]), f"{what}: {f} was written"


def relight_held(torch, r, look, p, held, want=RELIT, stream="torch"):
    c = Colours(torch, p.n, want)
    torch.cuda.synchronize()
    r.relight_into(look, p.n, stream=stream_of(torch, stream), held=held, **p.relight_args(), **c.args())
    r.sync()
    torch.cuda.synchronize()
    return c.collect()


def run_case(torch, sc, look, mode, source, rays, what, exacts=(False, True), stride_pad=0, size=(W, H)):
    """the whole of one (scene, mode, source): both settings of the exact skips, every pair of masks one after the other on the same
    planes (each against the planes as they were before it), then the relight.  size: the frame of source "pixels", whose camera
    rays `rays` are"""
    nl = len(sc.lights())
    w, h = size
    a, b = open_renderer(sc, MODES[mode]), open_renderer(look, MODES[mode])
    try:
        for exact in exacts:
            for r in (a, b):
                r.set_exact_skips(0 if exact else 7)
            n = len(rays)
            stride = n + stride_pad if stride_pad and source == "rays" else 0       # (capture_pixels takes no stride)
            if source == "rays":
                d_rays = torch.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
                pa, _ = capture(torch, a, rays, stride=stride)
                pb, got_b = capture(torch, b, rays, stride=stride)
            else:
                pa, _ = capture_pixels(torch, a, w, h)
                pb, got_b = capture_pixels(torch, b, w, h)
            all16 = exact or source == "pixels"
            # 3. B's planes are the oracle's, from B's own hit_dist and hit_id
            ref = UR.reference(look, rays, got_b["dist"], got_b["id"])
            assert_same(got_b, ref, FACTORS + (("shadow_steps",) if exact else ()), f"{what} exact={exact}: B against light_update_reference")
            want = raw(pb)
            for march, spec in masks_of(nl):
                before = raw(pa)
                if source == "rays":
                    a.light_update_rays_into(look, d_rays.data_ptr(), n, march, spec, stream=torch.cuda.current_stream().cuda_stream, **update_args(pa))
                else:
                    a.light_update_pixels_into(look, n, w, h, march, spec, stream=torch.cuda.current_stream().cuda_stream, **update_args(pa))
                a.sync()
                torch.cuda.synchronize()
                assert_updated(before, raw(pa), want, n, nl, stride, march, spec, all16, f"{what} exact={exact} masks=({march}, {spec})")
            pa.collect()                                             # (nothing behind the planes or between them)
            # 4. every light has been marched by now: the relight is B's picture
            got = relight_held(torch, a, look, pa, look)
            if source == "rays":
                assert_same(got, shade_rays(torch, b, rays, want=RELIT), RELIT, f"{what} exact={exact}: relight against B's shading query")
            else:
                assert_same(got, frame(torch, b, w, h), ("rgb", "pixel"), f"{what} exact={exact}: relight against B's frame")
    finally:
        b.close()
        a.close()


# ------------------------------------------------------------------------------------------------ 1 - 5. the planes, scene by scene
@pytest.mark.parametrize("source", ["pixels", "rays"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_example_scenes(torch_cuda, scenes, name, mode, source):
    sc = scenes[name]
    rays = R.camera_rays(sc, W, H) if source == "pixels" else long_list(sc, ray_list(sc))
    if source == "rays":
        assert not np.isfinite(rays).all(), "the list lacks the hostile rays"
    run_case(torch_cuda, sc, lighting_look(sc), mode, source, rays, f"{name} {mode} {source}", stride_pad=7 if mode == "interp" else 0)


@pytest.mark.parametrize("source", ["pixels", "rays"])
@pytest.mark.parametrize("name", ["three_lights", "tree5", "tree9", "tree12", "tree2-tables"])
def test_stack_classes_tables_and_three_lights(torch_cuda, scenes, name, source):
    """one shape per interpreter stack class beyond the two example scenes' (7, 11, 63), the tables read from global memory, and three
    lights with two shininesses"""
    sc = scene_named(scenes, name)
    rays = R.camera_rays(sc, W, H) if source == "pixels" else long_list(sc, R.ray_set(sc, SEED, "ae"))
    a = open_renderer(sc, MODES["interp"])
    try:
        if name != "three_lights":
            assert a.interp_variant() == C.RUNG[name].rung
    finally:
        a.close()
    # (on the interpreter throughout: the scene compiler takes seconds for the 1024 ops of tree9, twice — the scene and its look)
    run_case(torch_cuda, sc, lighting_look(sc), "default" if name == "three_lights" else "interp", source, rays, f"{name} {source}",
             exacts=(True,) if source == "rays" else (False,))


def test_a_look_with_an_infinite_intensity_and_one_light_moved(torch_cuda, scenes):
    """light 0 alone moves: light 1's plane is B's without an update; and the look's colours are hostile"""
    sc = scenes["scene4"]
    inf = float("inf")
    moved = sc.with_lighting(points=[(0.5, 8.0, -2.0), None])
    look = moved.with_look(lights=[((inf, 1.0, 2.0), (1.0, inf, 0.5)), None], materials=[((.2, .1, .3), (.1, .1, .1), (.2, .2, .2))] + [None] * 2)
    assert S.light_changes(sc, look) == (1, 0)
    a, b = open_renderer(sc, 1), open_renderer(look, 1)
    try:
        pa, _ = capture_pixels(torch_cuda, a, W, H)
        pb, _ = capture_pixels(torch_cuda, b, W, H)
        before = raw(pa)
        a.light_update_pixels_into(look, W * H, W, H, *S.light_changes(sc, look), **update_args(pa))
        a.sync()
        after, want = raw(pa), raw(pb)
        assert_updated(before, after, want, W * H, 2, 0, 1, 0, True, "light 0 moved")
        assert np.array_equal(after["factors"], want["factors"])          # light 1 stood still: the whole of B's planes
        got = relight_held(torch_cuda, a, look, pa, moved)                # (held: anything that stands where the planes stand)
        assert_same(got, frame(torch_cuda, b, W, H), ("rgb", "pixel"), "an infinite intensity")
        assert np.isnan(got["rgb_linear"]).any() or (got["rgb_linear"] == 1).any()
    finally:
        b.close()
        a.close()


# ------------------------------------------------------------------------------------------------------------- 6. an averaged picture
def test_an_averaged_picture(torch_cuda, scenes):
    """16 x 8, 2 x 2 samples under each of 2 lens cameras: the host updates record r with light_update_pixels_into on the 32 x 16
    grid, r * 512 elements further on, and resolves with relight_views_held_into"""
    sc = scenes["scene4"]
    look = lighting_look(sc)
    w, h, s, k = 16, 8, 2, 2
    cams = S.lens_cameras(sc.camera, 6.0, 0.25, k)
    per, n_all = s * s * w * h, k * s * s * w * h
    a, b = open_renderer(sc, 1), open_renderer(look, 1)
    try:
        p = Planes(torch_cuda, n_all, 2)
        a.light_views_into(cams, k, w, h, s, stream=torch_cuda.cuda.current_stream().cuda_stream, **p.args())
        march, spec = S.light_changes(sc, look)
        assert (march, spec) == (3, 0)
        u = update_args(p)
        for r in range(k):
            a.light_update_pixels_into(look, per, s * w, s * h, march, spec, camera=cams[r], factors_ptr=u["factors_ptr"] + 16 * r * per,
                                       id_ptr=u["id_ptr"] + 4 * r * per, dist_ptr=u["dist_ptr"] + 4 * r * per, light_stride=n_all,
                                       stream=torch_cuda.cuda.current_stream().cuda_stream)
        c = Colours(torch_cuda, w * h, ("rgb", "pixel"))
        a.relight_views_held_into(look, look, 1, k, w, h, s, stream=torch_cuda.cuda.current_stream().cuda_stream, **p.relight_args(), **c.args())
        a.sync()
        torch_cuda.cuda.synchronize()
        p.collect()
        out = V.alloc_batch(torch_cuda, 1, w, h, debug=("rgb",))
        torch_cuda.cuda.synchronize()
        b.render_blended_views_into(out["frame"].data_ptr(), cams, k, w, h, debug=out["dbg"], samples=s)
        b.sync()
        got_b = V.collect(out, *out["geom"])
        want = dict(rgb=np.ascontiguousarray(got_b["rgb"].reshape(-1, 3)), pixel=np.ascontiguousarray(got_b["xrgb"].ravel()))
        assert_same(c.collect(), want, ("rgb", "pixel"), "the supersampled blend of the look")
        # without `held` the resolve refuses the look, as it always did
        assert refusal(lambda: a.relight_views_into(look, 1, k, w, h, s, **p.relight_args(), **c.args())) == (-3, "relight: the look moves a light: capture again")
    finally:
        b.close()
        a.close()


# ------------------------------------------------------------------------------------------------------------------- 7. refusals
T = {
    "no program": "no scene program uploaded",
    "no look": "light update: no look",
    "no list": "light update: no list",
    "n": "light update: max_steps < 0 or more than 2^32 - 1 rays",
    "geometry": "light update: no camera or bad frame geometry",
    "not all pixels": "light update: no list of pixels, and n is not w * h",
    "no hit_id": "light passes: no hit_id plane",
    "no factors": "light passes: no factors, and the program has lights",
    "misaligned": "light passes: factors must be 16-byte aligned",
    "stride": "light passes: light_stride is neither 0 nor at least n",
    "no hit_dist": "light update: no hit_dist plane",
    "mask": "light update: a mask names a light the program has not (lights from the 64th on: capture again)",
}
LOOK_TEXT = {
    "f[]": "light update: the look differs from the uploaded program in an op (opcode, id or a number): capture again",
    "root_material": "light update: the look gives an object another material: capture again",
    "a count": "light update: the look differs from the uploaded program in a count (ops, lights, materials, roots, max_stack)",
    "NULL materials": "light update: malformed look: a table is missing",
    "root_material out of range": "light update: material index out of range in the look",
}
HELD_TEXT = {
    "f[]": "relight: the held program differs from the uploaded program in an op (opcode, id or a number): capture again",
    "root_material": "relight: the held program gives an object another material: capture again",
    "a count": "relight: the held program differs from the uploaded program in a count (ops, lights, materials, roots, max_stack)",
    "NULL materials": "relight: malformed held program: a table is missing",
    "root_material out of range": "relight: material index out of range in the held program",
}


def test_refusals(torch_cuda, scenes):
    """every line of the header's list: the status, the text, the order, and nothing written — the planes are a pattern throughout"""
    sc = scenes["scene4"]
    look = lighting_look(sc)
    rays = ray_list(sc)[:64]
    d_rays = torch_cuda.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
    d_xy = torch_cuda.zeros(128, dtype=torch_cuda.int32, device="cuda:0")
    p, c = Planes(torch_cuda, 64, 2), Colours(torch_cuda, 64)
    u, ca = update_args(p), c.args()
    lib = gpu.gpu_lib()
    fc = sc.frame_camera(8, 8)
    prog = look.flatten()
    torch_cuda.cuda.synchronize()

    def passes(**kw):
        v = dict(u, **kw)
        return gpu.LightPasses(v["factors_ptr"] or None, v["light_stride"], v["id_ptr"] or None, v["dist_ptr"] or None, None)

    empty = gpu.Renderer(0)
    try:
        assert refusal(lambda: empty.light_update_rays_into(look, d_rays.data_ptr(), 64, 1, 0, **u)) == (-4, T["no program"])
        assert refusal(lambda: empty.light_update_rays_into(look, d_rays.data_ptr(), 1 << 32, 1, 0, **u)) == (-3, T["n"])       # a bad argument first
        assert refusal(lambda: empty.light_update_rays_into(None, d_rays.data_ptr(), 64, 1, 0, **u)) == (-3, T["no look"])
        assert lib.lol_gpu_light_update_pixels(empty._ctx, prog, fc, 8, 8, None, 64, 1, 0, passes(), None) == -4
        assert lib.lol_gpu_light_update_pixels(empty._ctx, prog, None, 8, 8, d_xy.data_ptr(), 64, 1, 0, passes(), None) == -4      # the program before the camera
        assert lib.lol_gpu_relight_held(empty._ctx, prog, prog, passes(), 64, gpu.Relit(*(ca[f + "_ptr"] for f in RELIT)), None) == -4
    finally:
        empty.close()
    r = open_renderer(sc, 1)
    try:
        upd = lambda **kw: r.light_update_rays_into(look, d_rays.data_ptr(), 64, 1, 2, **dict(u, **kw))       # noqa: E731
        assert refusal(lambda: r.light_update_rays_into(None, d_rays.data_ptr(), 64, 1, 0, **u)) == (-3, T["no look"])
        assert refusal(lambda: r.light_update_rays_into(look, 0, 64, 1, 0, **u)) == (-3, T["no list"])
        assert lib.lol_gpu_light_update_rays(r._ctx, prog, d_rays.data_ptr(), 64, 1, 0, None, None) == -3             # no lol_gpu_light_passes
        assert lib.lol_gpu_error(r._ctx).decode() == "light update: no output"
        assert refusal(lambda: r.light_update_rays_into(look, d_rays.data_ptr(), 1 << 32, 1, 0, **u)) == (-3, T["n"])
        assert refusal(lambda: upd(id_ptr=0)) == (-3, T["no hit_id"])
        assert refusal(lambda: upd(factors_ptr=0)) == (-3, T["no factors"])
        assert refusal(lambda: upd(factors_ptr=u["factors_ptr"] + 4)) == (-3, T["misaligned"])
        assert refusal(lambda: upd(light_stride=63)) == (-3, T["stride"])
        assert refusal(lambda: upd(dist_ptr=0)) == (-3, T["no hit_dist"])
        for march, spec in ((4, 0), (0, 4), (1 << 63, 1), (3, 1 << 2)):
            assert refusal(lambda: r.light_update_rays_into(look, d_rays.data_ptr(), 64, march, spec, **u)) == (-3, T["mask"]), (march, spec)
        pix = lambda n=64, w=8, h=8, xy=d_xy.data_ptr(), **kw: r.light_update_pixels_into(look, n, w, h, 3, 0, xy_ptr=xy, frame_camera=fc, **dict(u, **kw))       # noqa: E731
        assert refusal(lambda: pix(w=0)) == (-3, T["geometry"])
        assert refusal(lambda: pix(h=0)) == (-3, T["geometry"])
        assert lib.lol_gpu_light_update_pixels(r._ctx, prog, None, 8, 8, d_xy.data_ptr(), 64, 1, 0, passes(), None) == -3      # no camera
        assert lib.lol_gpu_light_update_pixels(r._ctx, prog, None, 8, 8, d_xy.data_ptr(), 0, 1, 0, passes(), None) == -3       # ... with n = 0 too
        assert refusal(lambda: pix(n=63, xy=0)) == (-3, T["not all pixels"])
        assert refusal(lambda: pix(dist_ptr=0)) == (-3, T["no hit_dist"])
        # the looks an update refuses — and the two a relight refuses, which it takes
        for what, bad in forbidden_looks(sc):
            try:
                if what in LOOK_TEXT:
                    assert refusal(lambda: r.light_update_rays_into(bad, d_rays.data_ptr(), 64, 3, 0, **u)) == (-3, LOOK_TEXT[what]), what
                    assert refusal(lambda: r.relight_into(None, 64, held=bad, **p.relight_args(), **ca)) == (-3, HELD_TEXT[what]), what
                else:
                    assert what in ("light point", "shininess")
                    assert refusal(lambda: r.relight_into(bad, 64, held=sc, **p.relight_args(), **ca))[0] == -3, what
                    assert refusal(lambda: r.relight_into(None, 64, held=bad, **p.relight_args(), **ca))[0] == -3, what
            finally:
                restore(what, bad)
        # a look must stand where `held` stands; the plain resolve keeps its own text
        assert refusal(lambda: r.relight_into(look, 64, **p.relight_args(), **ca)) == (-3, "relight: the look moves a light: capture again")
        assert refusal(lambda: r.relight_into(look, 64, held=sc, **p.relight_args(), **ca)) == (-3, "relight: the look moves a light: capture again")
        assert refusal(lambda: r.relight_into(sc.with_lighting(shininess=[None, 3.0, None]), 64, held=sc, **p.relight_args(), **ca)) == \
            (-3, "relight: the look changes a shininess: capture again")
        assert refusal(lambda: r.relight_into(look, 64, held=look, **dict(p.relight_args(), id_ptr=0), **ca)) == (-3, T["no hit_id"])
        assert refusal(lambda: r.relight_into(look, 1 << 32, held=look, **p.relight_args(), **ca)) == (-3, "relight: more than 2^32 - 1 elements")
        assert refusal(lambda: r.relight_into(look, 64, held=look, **p.relight_args())) == (-3, "relight: no output")
        # n = 0, or both masks 0: fine, and nothing launched
        r.light_update_rays_into(look, 0, 0, 3, 0, **u)
        r.light_update_rays_into(look, d_rays.data_ptr(), 64, 0, 0, **u)
        r.light_update_pixels_into(look, 0, 8, 8, 3, 0, xy_ptr=d_xy.data_ptr(), **u)
        r.relight_into(look, 0, held=look, **p.relight_args(), **ca)
        r.sync()
        torch_cuda.cuda.synchronize()
        assert p.untouched() and c.untouched(), "a refused or empty call wrote something"
        assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), rays.view(np.uint32))
    finally:
        r.close()


# --------------------------------------------------------------------------------------------------------------------- 8. streams
def test_streams_and_the_ring_of_looks(torch_cuda, scenes):
    """the default stream, the context's own, and two torch streams with ten updates in flight between them — more than the ring of
    looks has sets — each to a look and planes of its own, held to light_update_reference"""
    sc = scenes["scene4"]
    rays = ray_list(sc)[:130]
    n = len(rays)
    looks = [sc.with_lighting(points=[(-2.0 + 0.5 * k, 10.0 - 0.25 * k, -1.0 + 0.3 * k), None]) for k in range(10)]
    r = open_renderer(sc, 1)
    try:
        d_rays = torch_cuda.from_numpy(np.ascontiguousarray(rays).copy()).to("cuda:0")
        p0, held = capture(torch_cuda, r, rays)
        wants = [UR.reference(l, rays, held["dist"], held["id"], lights=(0,)) for l in looks]
        for stream in (0, None):
            p, _ = capture(torch_cuda, r, rays, stream=stream)
            r.light_update_rays_into(looks[0], d_rays.data_ptr(), n, 1, 0, stream=stream, **update_args(p))
            r.sync()
            torch_cuda.cuda.synchronize()
            got = p.collect()
            assert_same({f: got[f][:, 0] for f in FACTORS}, {f: wants[0][f][:, 0] for f in FACTORS}, FACTORS, f"stream {stream}")
        streams = [torch_cuda.cuda.Stream(), torch_cuda.cuda.Stream()]
        planes = [Planes(torch_cuda, n, 2) for _ in looks]
        torch_cuda.cuda.synchronize()
        for k, p in enumerate(planes):
            r.light_rays_into(d_rays.data_ptr(), n, stream=streams[k % 2].cuda_stream, **p.args())
        for k, (p, l) in enumerate(zip(planes, looks)):
            r.light_update_rays_into(l, d_rays.data_ptr(), n, 1, 0, stream=streams[k % 2].cuda_stream, **update_args(p))
        for s in streams:
            s.synchronize()
        own = p0.collect()
        for k, p in enumerate(planes):
            got = p.collect()
            assert_same({f: got[f][:, 0] for f in FACTORS}, {f: wants[k][f][:, 0] for f in FACTORS}, FACTORS, f"update {k} of ten in flight")
            assert_same({f: got[f][:, 1] for f in FACTORS}, {f: own[f][:, 1] for f in FACTORS}, FACTORS, f"update {k}: light 1 stood still")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------------- 9. CLI
def test_moved_lights_through_the_cli(torch_cuda, scenes, tmp_path, capsys):
    """python -m loltracer_amd scene4.lol --relight A.lol B.lol C.lol --move-lights -o DIR: the bytes of rendering each look's scene,
    each look reached from the one before; without the flag such looks are refused as they were"""
    w, h = 37, 11
    path = os.path.join(C.SCENES_DIR, "scene4.lol")
    text = open(path).read()
    a = text.replace("point\t\t\t= (-2, 10, -1)", "point\t\t\t= (1, 8, 2)")
    b = re.sub(r"shininess\s*=\s*16", "shininess = 5", a)                                       # the light stays, a shininess changes
    c = re.sub(r"diffuse_intensity\s*=\s*\(4, 4, 4\)", "diffuse_intensity = (0.9, 3, 2)", text)       # back home, another colour
    assert len({text, a, b, c}) == 4
    files = []
    for name, t in (("a.lol", a), ("b.lol", b), ("c.lol", c)):
        files.append(str(tmp_path / name))
        with open(files[-1], "w") as f:
            f.write(t)
    out = str(tmp_path / "looks")
    assert cli_main([path, "--relight", *files, "--move-lights", "--size", f"{w}x{h}", "-o", out]) == 0
    assert "light_update_interp" in capsys.readouterr().out
    for i, f in enumerate(files):
        single = str(tmp_path / f"single{i}.ppm")
        assert cli_main([f, "--size", f"{w}x{h}", "-o", single]) == 0
        assert open(os.path.join(out, f"look_{i:04d}.ppm"), "rb").read() == open(single, "rb").read(), f
    capsys.readouterr()
    assert cli_main([path, "--relight", files[0], "--size", f"{w}x{h}", "-o", str(tmp_path / "refused")]) == 1
    assert "stands at" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "refused"))
