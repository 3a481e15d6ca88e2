"""tests/scene_shapes.py is what it claims: every shape flattens to the declared counts, sits on the declared side of
TABLES_LDS_MAX_DWORDS and on the declared interpreter rung, the rungs are all eight, and every adaptive frame the GPU tests of
tests/test_gpu_families.py render refines SOME pixels and leaves some — says the oracle's mask, on the CPU.  Likewise the hostile
scenes of tests/test_gpu_hostile.py: the features they are there for are in their flattened programs, their ties are exact and go
to the first object in file order in the REFERENCE's own recorded frame and on the oracle, and every program of the catalogue has its LOL_OP_TOP ids strictly ascending."""
import ctypes
import re
import os

import numpy as np
import pytest

import adaptive_reference as R
import oracle_lib as O
import reference_frames as RF
import scene_shapes as C
from loltracer_amd import gpu, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_SHAPES = C.RUNG_SHAPES + [C.MID, C.BIG]


def oracle_mask(sc, w, h, T, camera=None, max_steps=256):
    """adaptive_reference.render's mask.  (It depends on the plain frame alone: the s x s frame is handed in, blank, not computed.)"""
    blank = (np.zeros((h, w), np.uint32), np.zeros((h, w, 3), np.float32))
    return R.render(sc, w, h, 2, T, max_steps=max_steps, camera=camera, full=blank)[2]


def test_the_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "loltracer_amd", "csrc", "lol_kernel.h")).read()
    assert int(re.search(r"TABLES_LDS_MAX_DWORDS\s*=\s*(\d+)", text).group(1)) == C.TABLES_LDS_MAX_DWORDS
    m = re.search(r"MOP_DEEP_FROM\s*=\s*(\d+),\s*MOP_DEEP_SLOTS\s*=\s*(\d+)", text)
    assert (int(m.group(1)) - 1, int(m.group(2))) == (11, 63)
    assert re.search(r"return n_lights \* 9u? \+ n_materials \* 10u? \+ n_roots", text) or "table_dwords" in text


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: s.name)
def test_shape_is_what_it_declares(shape):
    p = C.scene_of(shape).flatten()
    assert (p.n_ops, p.max_stack, p.n_lights) == (shape.n_ops, shape.max_stack, shape.n_lights)
    assert (C.table_dwords(p) > C.TABLES_LDS_MAX_DWORDS) == shape.tables_global, C.table_dwords(p)
    assert C.rung_of(p) == shape.rung


def test_the_rungs_are_all_eight():
    assert {s.rung for s in C.RUNG_SHAPES} == C.ALL_RUNGS and len(C.RUNG_SHAPES) == 8


def test_the_forms_are_the_scene_compilers():
    by = {f.name: f for f in C.FORMS}
    assert by["inline-small"].shape.n_ops <= 256 and by["inline-small"].two_kernels
    assert 257 <= by["mid-out-of-line"].shape.n_ops <= 1024 and by["mid-out-of-line"].specialize == 5
    assert by["mid-inlined"].shape is by["mid-out-of-line"].shape and by["mid-inlined"].specialize == 1 and by["mid-inlined"].second_tier
    assert by["big-out-of-line"].shape.n_ops > 1024 and by["big-out-of-line"].form == "out of line"
    assert by["tables-global"].shape.tables_global
    assert all(f.shape.n_ops <= 1104 for f in C.FORMS)             # (the 8192-op trees are never compiled with the families on)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: s.name)
def test_adaptive_frames_refine_some_pixels_and_leave_some(shape):
    """the single frame under the scene's own camera, and every view of the batch"""
    sc = C.scene_of(shape)
    w, h = shape.size
    n = int(oracle_mask(sc, w, h, shape.contrast).sum())
    assert 0 < n < w * h, n
    views = [int(oracle_mask(sc, w, h, shape.contrast, cam).sum()) for cam in C.cameras(sc)]
    assert 0 < sum(views) < C.N_VIEWS * w * h and sum(1 for v in views if 0 < v < w * h) >= 3, views


def test_fuzz_scenes_show_every_op_and_light_count_and_refine_some():
    kinds, lights = set(), set()
    w, h = C.FUZZ_SIZE
    for i, sc in enumerate(C.fuzz_scenes()):
        p = sc.flatten()
        kinds |= {p.ops[k].op for k in range(p.n_ops)}
        lights.add(p.n_lights)
        assert 0 < int(oracle_mask(sc, w, h, C.FUZZ_CONTRAST).sum()) < w * h, i
    assert kinds == {S.OP_SPHERE, S.OP_RBOX, S.OP_PLANE, S.OP_SMIN, S.OP_SMIN_R, S.OP_TOP}
    assert {0, 1, 3} <= lights
    assert len(C.fuzz_scenes()) == C.N_FUZZ == 8


def test_degenerate_inputs_are_the_six_and_three_have_an_edge():
    w, h = C.DEGENERATE_SIZE
    scs = C.degenerate_scenes()
    assert len(scs) == len(C.DEGENERATE_NAMES) == len(C.DEGENERATE_REFINES_SOME) == 6
    got = tuple(0 < int(oracle_mask(sc, w, h, C.DEGENERATE_CONTRAST).sum()) < w * h for sc in scs)
    assert got == C.DEGENERATE_REFINES_SOME
    assert scs[0].flatten().n_ops == 0 and scs[0].flatten().n_lights == 0


def test_max_steps_frames_refine_some_pixels_unless_nothing_is_marched():
    sc = C.scene_of(C.MAX_STEPS_SHAPE)
    w, h = C.MAX_STEPS_SIZE
    for ms in C.MAX_STEPS:
        n = int(oracle_mask(sc, w, h, 16, max_steps=ms).sum())
        views = sum(int(oracle_mask(sc, w, h, 16, cam, max_steps=ms).sum()) for cam in C.cameras(sc))
        if ms == 0:
            assert n == 0 and views == 0
        else:
            assert 0 < n < w * h and 0 < views < C.N_VIEWS * w * h, (ms, n, views)


# ------------------------------------------------------------------------------------------------------------- hostile scenes
def f32(v):
    return float(np.float32(v))


def test_stress_scene_is_the_generator_it_has_always_been():
    """scene 0 of `soak.py 12 7707 stress`, as the generator wrote it while it still lived in tests/tools/soak.py"""
    want = open(os.path.join(ROOT, "tests", "golden", "hostile", "stress_7707_scene0.lol")).read()
    assert C.stress_scene(np.random.default_rng(7707)) == want
    assert "def stress_scene" not in open(os.path.join(ROOT, "tests", "tools", "soak.py")).read()


def test_the_hostile_catalogue_is_fixed():
    assert [e.name for e in C.HOSTILE[:C.N_HOSTILE_GENERATED]] == ["stress%02d" % i for i in range(14)]
    assert [e.name for e in C.HOSTILE_TIES] == ["tie-spheres-01", "tie-spheres-10", "tie-boxes-01", "tie-boxes-10",
                                                "tie-sphere-union-01", "tie-sphere-union-10", "tie-crowd", "tie-camera"]
    assert len(C.HOSTILE) == len(C.HOSTILE_REFINES_SOME) == 22 and len(C.HOSTILE_BY_NAME) == 22
    assert all(e.size == C.HOSTILE_SIZE for e in C.HOSTILE)


def bounded_objects(prog):
    c, r = (ctypes.c_float * 3)(), ctypes.c_float()
    return sum(gpu.gpu_lib().lol_gpu_cull_bounds(ctypes.byref(prog), i, c, ctypes.byref(r)) == 1 for i in range(prog.n_roots))


def culling_tests(prog, base):
    """the plan's own report: the tests of the generated SDF (each ends in `(vote(...) | vote(...)) != 0`), no device needed"""
    gpu.compile_offline(prog, base)
    return open(base + ".hip").read().count(")) != 0")


def test_generated_hostile_scenes_hold_what_they_are_there_for(tmp_path, monkeypatch):
    """read from the flattened programs (ops[].f), not from the text.  The scale of a scene shows in its largest smoothness: 60
    times 1, 30 or 1000, which no other product of the generator's factors gives; 0.01 times 1000 is 10 likewise."""
    ks, radii, lights, crowds = set(), set(), set(), []
    for e in C.HOSTILE[:C.N_HOSTILE_GENERATED]:
        p = C.hostile_scene(e).flatten()                          # parses and flattens
        lights.add(p.n_lights)
        for i in range(p.n_ops):
            o = p.ops[i]
            if o.op in (S.OP_SMIN, S.OP_SMIN_R):
                ks.add(o.f[0])
            elif o.op == S.OP_SPHERE:
                radii.add(o.f[3])
            elif o.op == S.OP_RBOX:
                radii.add(o.f[6])
        if bounded_objects(p) >= 8:                               # (the k-d split goes down to runs of three)
            crowds.append(e)
    assert 0.0 in ks and any(k < 0 for k in ks)
    assert {f32(0.01), f32(60)} <= ks                             # scale 1
    assert {f32(0.3), f32(1800)} <= ks                            # scale 30
    assert {f32(10), f32(60000)} <= ks                            # scale 1000
    assert any(r < 0 for r in radii) and 0.0 in radii
    assert 0 in lights
    assert len(crowds) >= 2
    # ... and the culling plan really forms clusters for two of the crowds: more tests than the one run of all bounded objects has
    clustered = 0
    for n, e in enumerate(crowds[:3]):
        p = C.hostile_scene(e).flatten()
        monkeypatch.delenv("LOL_GPU_TUNING", raising=False)
        monkeypatch.delenv("LOL_GPU_CULL_CLUSTERS", raising=False)
        kd = culling_tests(p, str(tmp_path / ("kd%d" % n)))
        monkeypatch.setenv("LOL_GPU_TUNING", "1")                 # (the library honours A/B switches only beside this)
        monkeypatch.setenv("LOL_GPU_CULL_CLUSTERS", "0")
        flat = culling_tests(p, str(tmp_path / ("flat%d" % n)))
        clustered += kd > flat >= 1
    assert clustered >= 2


def test_tie_scenes_parse_and_flatten():
    for e in C.HOSTILE_TIES:
        p = C.hostile_scene(e).flatten()
        assert p.n_roots == len(e.tie.objects) and p.n_lights == 1, e.name
    assert bounded_objects(C.hostile_scene(C.HOSTILE_BY_NAME["tie-crowd"]).flatten()) == 15


def oracle_sdf(sc, p):
    oid = ctypes.c_uint32()
    d = O.lib().lol_oracle_sdf(sc.ptr, float(p[0]), float(p[1]), float(p[2]), ctypes.byref(oid))
    return np.float32(d).view(np.uint32), oid.value


@pytest.mark.parametrize("e", C.HOSTILE_TIES, ids=lambda e: e.name)
def test_ties_are_exact_and_go_to_the_first_object(e):
    sc = C.hostile_scene(e)
    w, h = e.size
    first = min(e.tie.tied)
    # the reference itself gives the tie to the first object: the frame its own render_thread stored, and the composition beside it
    # (tests/golden/ref_renderer_frames.npz) ...
    RF.assert_recorded_tie_goes_to_the_first(e)
    # ... and so does the oracle.  The points of the tie: the camera position and, along_ray, the central ray's own points up to the hit (the camera looks down
    # -z from the origin, so that they are (0, 0, -t) exactly, t the distance marched: the central pixel's probe gives the hit)
    assert sc.camera.point.tuple() == (0.0, 0.0, 0.0) and sc.camera.direction.tuple() == (0.0, 0.0, -1.0)
    centre = O.probe(sc, w, h, w // 2, h // 2)
    assert tuple(centre.rd) == (0.0, 0.0, -1.0)
    pts = [(0.0, 0.0, 0.0)]
    if e.tie.along_ray:
        pts += [(0.0, 0.0, -f32(t)) for t in (0.5, 1.0, 1.7, 2.25, 3.1, float(centre.hit_dist) - 0.5, float(centre.hit_dist))]
    alone = [S.Scene.parse_string(C.tie_text((e.tie.objects[i - 1],))) for i in e.tie.tied]
    for p in pts:
        values = {oracle_sdf(one, p)[0] for one in alone}
        assert len(values) == 1, (e.name, p, values)                               # bit-equal: the tie is real
        d, oid = oracle_sdf(sc, p)
        assert (d, oid) == (values.pop(), first), (e.name, p, oid)                 # ... it is the scene's minimum, and the first wins
    # the tied rays: the central pixel; every pixel that shows a tied object at all; every pixel when one step is all there is
    _, _, steps = O.render_rows(sc, w, h, 0, h, 256, want_steps=True)
    ids = steps[..., 2]
    if e.tie.along_ray:
        assert ids[h // 2, w // 2] == first == centre.hit_id
        assert first in ids and not (set(e.tie.tied) - {first}) & set(ids.ravel().tolist())
    _, _, steps = O.render_rows(sc, w, h, 0, h, 1, want_steps=True)
    assert (steps[..., 2] == first).all()
    # ... in another colour than the twin's / than the other tied objects would have
    mats = [sc.nodes()[sc.roots()[i - 1]].material for i in e.tie.tied]
    assert len(set(mats)) == len(mats)


def test_most_generated_hostile_scenes_show_something():
    """at least eight of them show two different hit ids (a miss counts as one)"""
    w, h = C.HOSTILE_SIZE
    shown = 0
    for e in C.HOSTILE[:C.N_HOSTILE_GENERATED]:
        _, _, steps = O.render_rows(C.hostile_scene(e), w, h, 0, h, 256, want_steps=True)
        shown += len(np.unique(steps[..., 2])) >= 2
    assert shown >= 8, shown


def test_which_hostile_scenes_refine_some_pixels():
    got = tuple(0 < int(oracle_mask(C.hostile_scene(e), *e.size, C.HOSTILE_CONTRAST).sum()) < e.size[0] * e.size[1] for e in C.HOSTILE)
    assert got == C.HOSTILE_REFINES_SOME


def every_scene_of_the_catalogue():
    for sh in ALL_SHAPES:
        yield sh.name, C.scene_of(sh)
    for i, sc in enumerate(C.fuzz_scenes()):
        yield "fuzz%d" % i, sc
    for name, sc in zip(C.DEGENERATE_NAMES, C.degenerate_scenes()):
        yield name, sc
    for e in C.HOSTILE:
        yield e.name, C.hostile_scene(e)


def test_top_ids_ascend_in_every_program():
    """lol_scene_flatten emits one LOL_OP_TOP per object, ids 1, 2, ... in program order: what `d < best` in lol_gpu.hip's host_sdf
    (and every other evaluator's strict comparison) needs to be the reference's tie rule.  The flattener refuses to hand out a
    program that breaks it; here it is read back from every program the catalogue has."""
    n = 0
    for name, sc in every_scene_of_the_catalogue():
        p = sc.flatten()
        tops = [p.ops[i].id for i in range(p.n_ops) if p.ops[i].op == S.OP_TOP]
        assert tops == list(range(1, p.n_roots + 1)), name
        n += 1
    assert n == len(ALL_SHAPES) + C.N_FUZZ + 6 + len(C.HOSTILE)
