"""tests/light_reference.py held to the oracle and to shade_reference, and scene.same_geometry / Scene.with_look held to what
include/lol_gpu.h says a look may differ in.  No GPU.

factors() fed the oracle's own rays (probe.rd from the camera's position) gives lol_oracle_probe_pixel's shadow[] and shadow_steps[],
bit for bit; relit() of those factors under the scene itself is shade()'s rgb_linear, and under a look it is shade() on the look's
scene: the captured scalars and the linear rest of get_light are the whole of it."""
import ctypes as C

import numpy as np
import pytest

import light_reference as LR
import oracle_lib as O
import ray_reference as R
import shade_reference as SR
from loltracer_amd import scene as S

W, H = 13, 5
NAMES = ["scene4", "scene"]


def looks_of(sc):
    """(name, look) pairs: the looks the GPU tests use (tests/test_gpu_light.py), built with Scene.with_look"""
    nl, nm = len(sc.lights()), len(sc.materials())
    mats = [(m.diffuse.tuple(), m.specular.tuple(), m.ambient.tuple()) for m in sc.materials()]
    inf, nan = float("inf"), float("nan")
    tint = [((.9, .2, .1), (.1, .8, .3))] + [((0, 0, 0), (0, 0, 0))] * (nl - 1)
    hot0 = [((.3, .5, .7), (.6, .4, .2), (.2, .1, .3))] + [None] * (nm - 1)
    return [
        ("a-one-light-off-the-other-tinted", sc.with_look(lights=tint)),
        ("b-materials-permuted-ambient-changed", sc.with_look(materials=mats[1:] + mats[:1], ambient=(.35, .15, .6))),
        ("c-material-0-lit", sc.with_look(materials=hot0)),
        ("d-infinite-diffuse-intensity", sc.with_look(lights=[((inf, 1, inf), None)] * nl)),
        ("e-nan-and-negative-intensities", sc.with_look(lights=[((nan, -2, .5), (-1, nan, 3))] + [((-.5, .25, -3), None)] * (nl - 1),
                                                        materials=hot0)),
    ]


@pytest.mark.parametrize("max_steps", [256, 7])
@pytest.mark.parametrize("name", NAMES)
def test_factors_are_the_probe(scenes, name, max_steps):
    sc = scenes[name]
    rays = R.camera_rays(sc, W, H)
    nl = len(sc.lights())
    for y in range(H):
        for x in range(W):
            p, i = O.probe(sc, W, H, x, y, max_steps), y * W + x
            f = LR.factors(sc, rays[i, :3], rays[i, 3:], max_steps)
            assert R.same_bits(np.float32(f["dist"]), np.float32(p.hit_dist)).all() and f["id"] == p.hit_id and f["steps"] == p.march_steps
            got = np.array([l[0] for l in f["lights"]], np.float32), np.array([l[3] for l in f["lights"]], np.uint32)
            assert R.same_bits(got[0], np.array(p.shadow[:nl], np.float32)).all(), (x, y, got[0], p.shadow[:nl])
            assert np.array_equal(got[1], np.array(p.shadow_steps[:nl], np.uint32)), (x, y)


@pytest.mark.parametrize("name", NAMES)
def test_relit_is_shade(scenes, name):
    """under the scene itself, and under each look: shade() on the look's scene, bit for bit — and the incidences are what shade()
    multiplies, so di lies in [0, 1] and is 0 where the surface faces away"""
    sc = scenes[name]
    rays = R.camera_rays(sc, W, H)
    ref = LR.reference(sc, rays)
    assert ((ref["di"] >= 0) & (ref["di"] <= 1)).all() and (ref["di"] == 0).any() and (ref["id"] == 0).any()
    for what, look in [("itself", sc)] + looks_of(sc):
        assert S.same_geometry(sc, look), what
        got = LR.relit_reference(ref, look)
        for i, r in enumerate(rays):
            want = SR.shade(look, r[:3], r[3:], 256)
            assert R.same_bits(got["rgb_linear"][i], np.array(want["rgb_linear"], np.float32)).all(), (what, i, got["rgb_linear"][i], want["rgb_linear"])
        want = SR.reference(look, rays)
        assert R.same_bits(got["rgb"], want["rgb"]).all() and np.array_equal(got["pixel"], want["pixel"]), what


def test_the_hostile_looks_change_what_the_skips_leave_out(scenes):
    """looks (c) - (e) make escaped rays and back-facing hits differ from the scene's own colours: the values the exact skips leave
    uncomputed matter under them"""
    sc = scenes["scene4"]
    rays = SR.shade_ray_set(sc, 20261018)
    ref = LR.reference(sc, rays)
    own = LR.relit_reference(ref, sc)["rgb_linear"]
    looks = dict(looks_of(sc))
    escaped = ref["id"] == 0
    lit0 = LR.relit_reference(ref, looks["c-material-0-lit"])["rgb_linear"]
    assert (~R.same_bits(lit0[escaped], own[escaped]).all(axis=1)).any()
    hot = LR.relit_reference(ref, looks["d-infinite-diffuse-intensity"])["rgb_linear"]
    back = ~escaped & (ref["di"] == 0).any(axis=1)
    assert back.any() and (hot[back][:, 0] == 1).all() and (hot[back][:, 2] == 1).all()      # inf * 0 = NaN, which v3clamp maps to 1


def test_same_geometry_accepts_and_refuses_what_the_header_says(scenes):
    sc = scenes["scene4"]
    assert S.same_geometry(sc, sc) and S.same_geometry(sc, sc.clone()) and S.same_geometry(sc.flatten(), sc)
    for what, look in looks_of(sc):
        assert S.geometry_difference(sc, look) is None, what
    assert not S.same_geometry(sc, scenes["scene"]) and "differs" in S.geometry_difference(sc, scenes["scene"])

    def changed(edit):
        c = sc.clone()
        edit(c.c)
        return c

    def first_sphere(c):
        return next(c.nodes[i] for i in range(c.n_nodes) if c.nodes[i].type == S.NODE_SPHERE)

    moved = changed(lambda c: setattr(first_sphere(c).point, "x", first_sphere(c).point.x + 0.5))
    assert "number" in S.geometry_difference(sc, moved)
    radius = changed(lambda c: setattr(first_sphere(c), "radius", first_sphere(c).radius * 2))
    assert not S.same_geometry(sc, radius)
    light = changed(lambda c: setattr(c.lights[0].point, "y", c.lights[0].point.y + 1))
    assert "light 0" in S.geometry_difference(sc, light)
    shiny = changed(lambda c: setattr(c.materials[1], "shininess", c.materials[1].shininess + 1))
    assert "shininess" in S.geometry_difference(sc, shiny)
    root = sc.roots()[0]
    worn = changed(lambda c: setattr(c.nodes[root], "material", (c.nodes[root].material + 1) % c.n_materials))
    assert "wears" in S.geometry_difference(sc, worn)
    # a NaN shininess equals itself: bits are compared
    nan = changed(lambda c: setattr(c.materials[1], "shininess", float("nan")))
    assert S.same_geometry(nan, nan.clone()) and not S.same_geometry(sc, nan)
    # the camera is no part of it (a relit frame is under the capture's camera)
    cam = changed(lambda c: setattr(c.camera.point, "z", c.camera.point.z + 1))
    assert S.same_geometry(sc, cam)


def test_with_look_replaces_the_free_numbers_alone(scenes):
    sc = scenes["scene4"]
    nl, nm = len(sc.lights()), len(sc.materials())
    look = sc.with_look(lights=[((1, 2, 3), None)] + [None] * (nl - 1), materials=[None] * (nm - 1) + [(None, (.1, .2, .3), None)],
                        ambient=(.5, .25, .125))
    assert look.lights()[0].diffuse_intensity.tuple() == (1, 2, 3)
    assert look.lights()[0].specular_intensity.tuple() == sc.lights()[0].specular_intensity.tuple()
    assert look.materials()[nm - 1].specular.tuple() == tuple(np.float32(v) for v in (.1, .2, .3))
    assert look.materials()[nm - 1].diffuse.tuple() == sc.materials()[nm - 1].diffuse.tuple()
    assert look.c.ambient_color.tuple() == (.5, .25, .125) and S.same_geometry(sc, look)
    assert C.string_at(C.addressof(look.c.camera), C.sizeof(S.Camera)) == C.string_at(C.addressof(sc.c.camera), C.sizeof(S.Camera))
    assert sc.with_look().tables() == sc.tables()
    with pytest.raises(ValueError):
        sc.with_look(lights=[None] * (nl + 1))
    with pytest.raises(ValueError):
        sc.with_look(materials=[None] * (nm + 1))
