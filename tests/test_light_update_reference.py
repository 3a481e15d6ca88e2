"""tests/light_update_reference.py held to tests/light_reference.py: the factor computed from a capture's hit_dist and hit_id under a
look that moves lights or changes a shininess IS the factor a capture of the look's own scene gives, bit for bit — the claim "the
planes hold enough" that lol_gpu_light_update_* rests on.  No device."""
import numpy as np
import pytest

import light_reference as LR
import light_update_reference as UR
import ray_reference as R

SEED = 20261020
FIELDS = ("shadow", "di", "si", "shadow_steps")


def rays_of(sc):
    """camera rays of a 13 x 5 frame with the eight special rays (NaN, infinite, zero, huge, denormal) inside them"""
    return R.ray_set(sc, SEED, "ae")


def hit_point(sc, rays):
    """p = ro + rd * dist of the first ray that hit something, on the capture's bits"""
    ref = LR.reference(sc, rays)
    i = int(np.flatnonzero((ref["id"] != 0) & np.isfinite(ref["dist"]))[0])
    return tuple(float(v) for v in R.along(tuple(rays[i, :3]), tuple(rays[i, 3:]), ref["dist"][i]))


def lighting_looks(sc, rays):
    """(what, look) pairs: each light moved alone, all moved, a shininess changed (every material's in turn is too slow: the two that
    objects wear), both at once, a light ON a captured hit point, and a light point that is not finite"""
    nl, nm = len(sc.lights()), len(sc.materials())
    out = []
    for l in range(nl):
        pts = [None] * nl
        x, y, z = sc.lights()[l].point.tuple()
        pts[l] = (x + 1.5, y - 0.75, z + 2.25)
        out.append((f"light {l} moved", sc.with_lighting(points=pts)))
    out.append(("every light moved", sc.with_lighting(points=[(3.0 - l, 6.5, 1.0 + l) for l in range(nl)])))
    out.append(("shininess", sc.with_lighting(shininess=[None] + [s.shininess * 0.5 + 3 for s in sc.materials()[1:]])))
    out.append(("shininess of material 0", sc.with_lighting(shininess=[7.0] + [None] * (nm - 1))))
    out.append(("both", sc.with_lighting(points=[(0.5, 8.0, -2.0)] + [None] * (nl - 1), shininess=[2.0] * nm)))
    out.append(("a light on a hit point", sc.with_lighting(points=[hit_point(sc, rays)] + [None] * (nl - 1))))
    out.append(("a light at infinity", sc.with_lighting(points=[(float("inf"), 1.0, 2.0)] + [None] * (nl - 1))))
    return out


@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_the_planes_hold_enough(scenes, name):
    sc = scenes[name]
    rays = rays_of(sc)
    held = LR.reference(sc, rays)
    assert (held["id"] != 0).any() and (held["dist"] >= 100).any(), "the list lacks a hit or an escaped ray"
    assert not np.isfinite(rays).all(), "the list lacks the special rays"
    for what, look in lighting_looks(sc, rays):
        want = LR.reference(look, rays)
        # the march is the held scene's: a look of an update has its geometry
        for f in ("dist", "id", "steps"):
            assert R.same_bits(want[f], held[f]).all(), (what, f)
        got = UR.reference(look, rays, held["dist"], held["id"])
        for f in FIELDS:
            ok = R.same_bits(got[f], want[f])
            assert ok.all(), f"{name}, {what}: {f} differs for {int((~ok).sum())} (ray, light) pairs; first ray {int(np.flatnonzero(~ok.all(axis=1))[0])}"
        if what == "light 0 moved":
            assert not R.same_bits(want["shadow"][:, 0], held["shadow"][:, 0]).all() or not R.same_bits(want["di"][:, 0], held["di"][:, 0]).all()
            for l in range(1, len(sc.lights())):                       # a light that stands where it stood keeps its plane
                for f in FIELDS:
                    assert R.same_bits(want[f][:, l], held[f][:, l]).all(), (what, f, l)
        if what == "shininess":
            assert not R.same_bits(want["si"], held["si"]).all()
            for f in ("shadow", "di", "shadow_steps"):                 # ... and a shininess changes the specular incidence alone
                assert R.same_bits(want[f], held[f]).all(), (what, f)


def test_a_foreign_id_is_taken_for_zero(scenes):
    sc = scenes["scene4"]
    rays = rays_of(sc)[:3]
    held = LR.reference(sc, rays)
    wild = np.full(len(rays), len(sc.roots()) + 5, np.uint32)
    zero = np.zeros(len(rays), np.uint32)
    a, b = UR.reference(sc, rays, held["dist"], wild), UR.reference(sc, rays, held["dist"], zero)
    for f in FIELDS:
        assert R.same_bits(a[f], b[f]).all(), f
