"""tests/hostile_rays.py held to what it claims, and the references of the list families held to the oracle on the hostile scenes.
No GPU.

These are conditions on the INPUTS of tests/test_gpu_hostile_queries.py: the reference alone must satisfy them, so that the GPU tests
cannot pass vacuously — the lists hold every population a skip is decided on, rays of kinds (f) and (g) reach objects the camera's
rays never see, and exact ties go to the first object in file order.  Then the references the GPU tests compare with
(light_reference, light_update_reference; ray_reference and shade_reference have tests/golden/hostile in their own tests) are held to
lol_oracle_probe_pixel and to one another on the hostile scenes' own camera rays, bit for bit.
"""
import hashlib
import time

import numpy as np
import pytest

import hostile_rays as HR
import light_reference as LR
import light_update_reference as UR
import oracle_lib as O
import ray_reference as R
import scene_shapes as SH
import shade_reference as SR
from test_gpu_light_update import lighting_look

names = lambda e: e.name                 # noqa: E731
LIT = [e for e in SH.HOSTILE if "point_light" in e.text]
# the objects the whole list must name at the least (the chosen seed reaches 9, 11 and 14: the margin is for another seed's draws)
DISTINCT_AT_LEAST = {"stress03": 8, "stress04": 9, "tie-crowd": 12}
UPDATE_SIZE = (16, 8)                    # the frame whose pixels the GPU tests of light updates capture


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_lists_are_what_they_have_always_been():
    """Every ray, kind, object and permutation of all 22 lists, as the builder made them before bound_rays was factored out of it
    for tests/test_gpu_scene_records.py: one digest over them in the catalogue's order — and bound_rays is that part of the list.
    The digest was taken with the builder of commit 8126f6e, before the refactoring, and is the refactored builder's too.  It rests on
    numpy's Generator stream and on the bounds lol_gpu_cull_bounds / _clusters return: a change that legitimately moves a culling
    bound moves the lists with it, and the digest is then taken anew — it pins the builder, not the bounds."""
    h, n = hashlib.sha256(), 0
    for e in SH.HOSTILE:
        p = HR.hostile_ray_parts(e)
        for k in ("rays", "permuted"):
            h.update(p[k].tobytes())
        h.update("".join(p["kind"].tolist()).encode())
        h.update(p["obj"].tobytes())
        h.update(p["perm"].astype("int64").tobytes())
        n += len(p["rays"])
    assert n == 6300
    assert h.hexdigest() == "448a5652fa175656248046da3e0b57bf3875439ab08c4572f1e72774c250d3ee"
    e = SH.HOSTILE_BY_NAME["tie-crowd"]
    parts, kind, obj = HR.bound_rays(SH.hostile_scene(e), [HR.SEED, SH.HOSTILE.index(e)])
    p = HR.hostile_ray_parts(e)
    own = p["kind"] != "a"
    assert np.array_equal(bits(np.concatenate(parts)[:own.sum()]), bits(p["rays"][own])) and kind[:own.sum()] == p["kind"][own].tolist()
    assert obj[:own.sum()] == p["obj"][own].tolist() and len(kind) - own.sum() in (0, 1)


@pytest.mark.parametrize("e", SH.HOSTILE, ids=names)
def test_the_list_builds_and_is_what_it_says(e):
    sc = SH.hostile_scene(e)
    p = HR.hostile_ray_parts(e)
    rays = HR.hostile_ray_list(e)
    assert rays is p["rays"] and HR.hostile_ray_list(e) is rays                     # memoised per entry
    assert rays.dtype == np.float32 and rays.ndim == 2 and rays.shape[1] == 6 and not rays.flags.writeable
    assert len(rays) % 64 != 0 and len(rays) > 64
    again = HR._build(e)                                                            # ... and built again it is the same, bit for bit
    assert np.array_equal(bits(again["rays"]), bits(rays)) and np.array_equal(again["perm"], p["perm"])
    # (a) - (e) are ray_set's, as they are, at the front (of the two THINNED scenes, every second one and every special)
    base = R.ray_set(sc, HR.SEED, "abcde")
    if e.name in HR.THINNED:
        base = base[HR.specials_among(sc, base) | (np.arange(len(base)) % HR.THINNED[e.name] == 0)]
    n_base = int((p["kind"] == "a").sum())
    assert n_base in (len(base), len(base) - 1) and np.array_equal(bits(rays[:n_base]), bits(base[:n_base]))
    # the specials: each once, none a duplicate of another ray, none the first or the last ray of the list
    special = HR.specials_among(sc, rays)
    assert not special[0] and not special[-1]
    assert special.sum() == len(R.SPECIALS) and not special[n_base:].any()
    assert len({r.tobytes() for r in rays[special]}) == len(R.SPECIALS)
    assert (~np.isfinite(rays[~special])).sum() == 0                                # nothing else in the list is hostile by its numbers
    # the two orders hold the same rays, and the permutation moves them
    orders = HR.hostile_ray_orders(e)
    assert [o[0] for o in orders] == ["object-major", "permuted"] and orders[0][1] is rays
    _, permuted, perm = orders[1]
    assert sorted(perm.tolist()) == list(range(len(rays))) and np.array_equal(bits(permuted), bits(rays[perm]))
    assert (perm != np.arange(len(rays))).mean() > 0.9 and not permuted.flags.writeable
    # kinds (f) - (h): per object three aimed rays and three grazing per sphere of its test, or two from above; grouped by object
    bounded = HR.bounded_objects(sc)
    prog = sc.flatten()
    after = p["obj"][n_base:]
    assert (after >= 0).all() and (np.diff(after) >= 0).all() and (p["obj"][:n_base] == -1).all()
    for i in range(len(sc.roots())):
        kinds = "".join(p["kind"][p["obj"] == i])
        want = "fff" + "ggg" * (1 + len(HR.cull_clusters(prog, i))) if i in bounded else "hh"
        # (the list's last ray is dropped where its length would be a multiple of 64)
        assert kinds == want or (i == len(sc.roots()) - 1 and kinds == want[:-1]), (i, kinds, want)
    # every direction of (f) - (h) is a unit vector, every origin finite
    tail = rays[n_base:]
    assert np.isfinite(tail).all() and np.allclose(np.linalg.norm(tail[:, 3:].astype(np.float64), axis=1), 1, atol=1e-6)


@pytest.mark.parametrize("e", SH.HOSTILE, ids=names)
def test_aimed_and_grazing_rays_stand_where_they_should(e):
    """(f) starts outside the bound and points at its centre; (g) passes the centre at R' (1 + eps): the miss distance of the ray as
    it is in binary32 lies within a few ulp of R' (1 + eps) — and the three eps are told apart"""
    sc = SH.hostile_scene(e)
    p = HR.hostile_ray_parts(e)
    prog = sc.flatten()
    for i, (c, r) in HR.bounded_objects(sc).items():
        mine = p["obj"] == i
        for q in p["rays"][mine & (p["kind"] == "f")].astype(np.float64):
            to_c = c - q[:3]
            d = float(np.linalg.norm(to_c))
            assert d > r and abs(d - (r + HR.gap_of(r))) <= 1e-5 * max(1.0, d, float(np.abs(c).max()))
            assert float(np.dot(to_c / d, q[3:])) > 1 - 1e-5
        spheres = [(c, r)] + HR.cull_clusters(prog, i)
        graze = p["rays"][mine & (p["kind"] == "g")].astype(np.float64)
        assert len(graze) in (3 * len(spheres), 3 * len(spheres) - 1)               # (the list's last ray may have been dropped)
        for j, (cj, rj) in enumerate(spheres):
            for eps, q in zip(HR.EPS, graze[3 * j:3 * j + 3]):
                to_c = cj - q[:3]
                along = float(np.dot(to_c, q[3:]))
                miss = float(np.linalg.norm(to_c - along * q[3:]))
                assert 0 < along <= HR.BACK_MAX * (1 + 1e-5)
                # binary32 origins of size |C| + R' + back place the ray to about 2^-23 of that
                assert abs(miss - rj * (1 + eps)) <= 4e-7 * (float(np.abs(cj).max()) + rj + HR.BACK_MAX) + 1e-6 * rj, (i, j, eps, miss, rj)


_refs = {}


def list_reference(e):
    if e.name not in _refs:
        _refs[e.name] = LR.reference(SH.hostile_scene(e), HR.hostile_ray_list(e))
    return _refs[e.name]


def populations(sc, ref):
    hit = ref["id"] != 0
    out = dict(escaped=int((~hit).sum()), hit=int(hit.sum()), non_finite=int((~np.isfinite(ref["dist"])).sum()))
    if len(sc.lights()):
        out.update(back_facing=int((ref["di"][hit] == 0).any(axis=1).sum()), dark=int((ref["shadow"][hit] == 0).any(axis=1).sum()),
                   partial=int(((ref["shadow"][hit] > 0) & (ref["shadow"][hit] < 1)).any(axis=1).sum()))
    return out


def test_the_populations_the_gpu_tests_rely_on():
    """every list has an escaped ray, a hit and a ray whose distance is not finite; every scene with a light a hit with di == 0 and a
    hit in full shadow; at least five scenes a hit with 0 < shadow < 1 — the two two-light scenes of the averaged picture among them"""
    partial = []
    for e in SH.HOSTILE:
        sc = SH.hostile_scene(e)
        pop = populations(sc, list_reference(e))
        assert pop["escaped"] and pop["hit"] and pop["non_finite"], (e.name, pop)
        assert (e in LIT) == bool(len(sc.lights()))
        if e in LIT:
            assert pop["back_facing"] and pop["dark"], (e.name, pop)
            if pop["partial"]:
                partial.append(e.name)
    assert len(SH.HOSTILE) - len(LIT) == 5                                          # the five scenes without a light
    assert len(partial) >= 5 and {"stress06", "stress12", "tie-crowd"} <= set(partial), partial
    for name in ("stress06", "stress12"):
        assert len(SH.hostile_scene(SH.HOSTILE_BY_NAME[name]).lights()) == 2


def test_aimed_and_grazing_rays_reach_objects_the_camera_never_sees():
    for e in SH.HOSTILE:
        sc = SH.hostile_scene(e)
        p, ref = HR.hostile_ray_parts(e), list_reference(e)
        base = p["kind"] == "a"
        every = set(ref["id"][ref["id"] != 0].tolist())
        seen = set(ref["id"][base & (ref["id"] != 0)].tolist())
        assert seen <= every and max(every) <= len(sc.roots())
        if e.name in DISTINCT_AT_LEAST:
            assert len(every) >= DISTINCT_AT_LEAST[e.name], (e.name, sorted(every))
        if len(HR.bounded_objects(sc)) >= 4:
            assert len(every) > len(seen), (e.name, sorted(every), sorted(seen))


def test_ties_go_to_the_first_object_in_file_order():
    """an aimed ray at any of tie-crowd's three coincident spheres hits id 3, never 9 or 14; at either twin of a -01 / -10 scene, id 1"""
    checked = 0
    for e in SH.HOSTILE_TIES:
        if not (e.name == "tie-crowd" or e.name.endswith(("-01", "-10"))):
            continue
        p, ref = HR.hostile_ray_parts(e), list_reference(e)
        first = min(e.tie.tied)
        assert first == (3 if e.name == "tie-crowd" else 1)
        for o in e.tie.tied:
            ids = ref["id"][(p["kind"] == "f") & (p["obj"] == o - 1)]
            assert len(ids) == 3 and (ids == first).all(), (e.name, o, ids)
            checked += 1
        assert not (set(e.tie.tied) - {first}) & set(ref["id"].tolist()), e.name
    assert checked == 3 + 6 * 2


def relight_look(sc):
    return HR.hostile_look(sc)


@pytest.mark.parametrize("e", SH.HOSTILE, ids=names)
def test_the_light_references_are_the_oracle_on_the_hostile_scenes(e):
    """on the camera rays of e.size: light_reference.factors is lol_oracle_probe_pixel (shadow, shadow_steps, hit_dist, hit_id,
    march_steps); light_reference.relit under the scene itself and under the GPU tests' look is shade_reference.shade of that scene;
    light_update_reference.reference from the look's own hit_dist / hit_id is light_reference.reference of the look"""
    sc, (w, h) = SH.hostile_scene(e), e.size
    rays = R.camera_rays(sc, w, h)
    nl = len(sc.lights())
    assert nl <= O.PROBE_LIGHTS
    ref = LR.reference(sc, rays)
    for y in range(h):
        for x in range(w):
            p, i = O.probe(sc, w, h, x, y, 256), y * w + x
            assert R.same_bits(ref["dist"][i], np.float32(p.hit_dist)).all() and ref["id"][i] == p.hit_id and ref["steps"][i] == p.march_steps, (x, y)
            assert R.same_bits(ref["shadow"][i], np.array(p.shadow[:nl], np.float32)).all(), (x, y, ref["shadow"][i], p.shadow[:nl])
            assert np.array_equal(ref["shadow_steps"][i], np.array(p.shadow_steps[:nl], np.uint32)), (x, y)
    for what, look in (("itself", sc), ("the look", relight_look(sc))):
        got, want = LR.relit_reference(ref, look), SR.reference(look, rays)
        for f in ("rgb_linear", "rgb", "pixel"):
            assert R.same_bits(got[f], want[f]).all(), (e.name, what, f)
    moved = lighting_look(sc)
    want = LR.reference(moved, rays)
    for f in ("dist", "id", "steps"):                                               # the march is the held scene's
        assert R.same_bits(want[f], ref[f]).all(), f
    got = UR.reference(moved, rays, want["dist"], want["id"])
    for f in ("shadow", "di", "si", "shadow_steps"):
        assert R.same_bits(got[f], want[f]).all(), (e.name, f)


@pytest.mark.parametrize("e", SH.HOSTILE, ids=names)
def test_the_references_of_one_scene_cost_less_than_two_seconds(e):
    """every reference the GPU tests of one scene ask for, on a scene of its own so that nothing is remembered: CPU time below 2 s
    (a scene that exceeds it gets a shorter list, the catalogue stays: hostile_rays.THINNED, whose two scenes took 1.4 and 2.3 s
    with whole lists; the slowest now takes about 1.2 s)"""
    from loltracer_amd import scene as S
    sc = S.Scene.parse_string(e.text)
    rays = HR.hostile_ray_list(e)
    t0 = time.process_time()
    R.reference(sc, rays, 256)
    R.reference(sc, rays, 1)
    SR.reference(sc, rays)
    ref = LR.reference(sc, rays)
    LR.relit_reference(ref, relight_look(sc))
    if len(sc.lights()):
        moved = lighting_look(sc)
        UR.reference(moved, rays, ref["dist"], ref["id"])
        px = R.camera_rays(sc, *UPDATE_SIZE)
        held = LR.reference(sc, px)
        UR.reference(moved, px, held["dist"], held["id"])
    spent = time.process_time() - t0
    assert spent < 2.0, f"{e.name}: {spent:.2f} s for {len(rays)} rays"
