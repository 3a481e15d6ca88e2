"""tests/scene_shapes.py is what it claims: every shape flattens to the declared counts, sits on the declared side of
TABLES_LDS_MAX_DWORDS and on the declared interpreter rung, the rungs are all eight, and every adaptive frame the GPU tests of
tests/test_gpu_families.py render refines SOME pixels and leaves some — says the oracle's mask, on the CPU."""
import re
import os

import numpy as np
import pytest

import adaptive_reference as R
import scene_shapes as C
from loltracer_amd import scene as S

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
