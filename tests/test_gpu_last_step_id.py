"""The hit id decided once per ray, from the values of the march's last step (Sdf::ID_FROM_LAST: lol_kernel.h, march; lol_codegen.hip,
last_id) — the scene's own kernel for scenes of exactly two top-level objects, under the library's default switches.

What the rule rests on is held where it could give way: the first step given by the host and taken by the lane, a loop that takes no
turn (MAX_STEPS 0 and 1), last steps whose second object the culling skipped (scene4), values that are NaN or infinite (the hostile
and degenerate scenes: the wave is shaded again by the plain pipeline), and exact ties, which go to the lower id in either file order.

Every comparison is test_gpu_parity.check_against_oracle plus the hit distances (test_gpu_hostile.assert_frame_is_oracle): array
equality on bit patterns, no tolerance of its own.  Kernel configurations 1 and 3, as in tests/test_gpu_hostile.py.
"""
import os

import pytest

import scene_shapes as C
from loltracer_amd import gpu, scene as S
from test_gpu_hostile import assert_frame_is_oracle, open_plain, oracle_frames_once, tie_cameras  # noqa: F401  (the fixture)
from test_gpu_parity import gpu_render

SPEC = pytest.mark.parametrize("specialize", [1, 3], ids=["spec", "spec-plain"])
names = lambda e: e.name                 # noqa: E731


def two_objects(sc) -> bool:
    return sc.flatten().n_roots == 2


ALSO = ("inside-a-sphere",)             # one object, seen from inside: no record, and every first step a negative distance


def _two_object_catalogue():
    """every HOSTILE and degenerate scene of tests/scene_shapes.py with exactly two top-level objects, and ALSO"""
    out = [e for e in C.HOSTILE if two_objects(C.hostile_scene(e))]
    for name, text, sc in zip(C.DEGENERATE_NAMES, C.DEGENERATE_CASES, C.degenerate_scenes()):
        if two_objects(sc) or name in ALSO:
            out.append(C.Hostile("degenerate-" + name, "degenerate input of tests/test_gpu_fuzz.py", text, C.DEGENERATE_SIZE))
    return out


CATALOGUE = _two_object_catalogue()

# two identical spheres and nothing else, in both file orders: the material follows the object, the winner is id 1 in both
SPHERE = "sphere { point = (0, 0, -5), radius = 1 }"
TWINS = [C.Hostile("twins-01", "two identical spheres, nothing else", C.tie_text((C._wear(SPHERE, 0), C._wear(SPHERE, 1)))),
         C.Hostile("twins-10", "two identical spheres, nothing else (opposite file order)", C.tie_text((C._wear(SPHERE, 1), C._wear(SPHERE, 0))))]
# |p - (0, 0, -5)| - 1 and p.y + 1 are both 0 at (0, -1, -5) and equal on the cone through it; rays graze both near the contact
TANGENT = C.Hostile("tangent", "a sphere tangent to a plane",
                    C.tie_text(("sphere { material = #1, point = (0, 0, -5), radius = 1 }", "plane { material = #2, y = -1 }")))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def test_the_catalogue_has_the_scenes_it_must(tmp_path):
    """... and scene4's fast SDF is generated with the record, scene.lol's (four objects) is what it was"""
    got = {e.name for e in CATALOGUE}
    assert {"degenerate-inf-squared-length", "degenerate-inside-a-sphere"} <= got, sorted(got)
    assert all(two_objects(S.Scene.parse_string(e.text)) for e in TWINS + [TANGENT])
    assert "LOL_GPU_TUNING" not in os.environ
    src = {}
    for name in ("scene4", "scene"):
        prog = S.Scene.parse_file(os.path.join(C.SCENES_DIR, name + ".lol")).flatten()
        gpu.compile_offline(prog, str(tmp_path / name), assume_fast=True)
        src[name] = (tmp_path / (name + ".hip")).read_text()
    fast = src["scene4"].split("struct SpecSdfFast")[1]
    assert "ID_FROM_LAST = true" in fast and "void eval_rec(" in fast and "ID_FROM_LAST" not in src["scene4"].split("struct SpecSdfFast")[0]
    assert "ID_FROM_LAST" not in src["scene"] and "eval_rec" not in src["scene"]


@pytest.mark.gpu
@SPEC
@pytest.mark.parametrize("max_steps", C.MAX_STEPS)
def test_scene4_max_steps(torch_cuda, max_steps, specialize):
    """the first step given (and, with MAX_STEPS 0 and 1, a loop that takes no turn: first_id stays), culled last steps"""
    e = C.Hostile("scene4", "scene4 at MAX_STEPS %d" % max_steps, "")
    sc, (w, h) = C.scene_of(C.MAX_STEPS_SHAPE), C.MAX_STEPS_SIZE
    r = open_plain(e, specialize)
    try:
        g = gpu_render(torch_cuda, r, sc, w, h, max_steps=max_steps)
        assert_frame_is_oracle(g, e, sc, w, h, "max_steps=%d" % max_steps, max_steps)
        if max_steps >= 7:
            assert {1, 2} <= set(g["id"].ravel().tolist())          # (both objects are seen: the plane and the blob)
    finally:
        r.close()


@pytest.mark.gpu
@SPEC
@pytest.mark.parametrize("e", CATALOGUE, ids=names)
def test_two_object_scenes(torch_cuda, e, specialize):
    """(which kernel a degenerate input gets is not this test's: tests/test_gpu_fuzz.py leaves it open too)"""
    sc, (w, h) = S.Scene.parse_string(e.text), C.HOSTILE_SIZE
    r = gpu.Renderer(0, specialize=specialize) if e.name.startswith("degenerate-") else open_plain(e, specialize)
    try:
        assert_frame_is_oracle(gpu_render(torch_cuda, r, sc, w, h), e, sc, w, h, "fresh")
        assert_frame_is_oracle(gpu_render(torch_cuda, r, sc, w, h, max_steps=1), e, sc, w, h, "max_steps=1", 1)
    finally:
        r.close()


@pytest.mark.gpu
@SPEC
@pytest.mark.parametrize("e", TWINS + [TANGENT], ids=names)
def test_ties(torch_cuda, e, specialize):
    """the first step given (the camera at the origin), taken (x = -0.0) and a camera beyond the sane range (the plain pipeline)"""
    sc, (w, h) = S.Scene.parse_string(e.text), C.HOSTILE_SIZE
    r = open_plain(e, specialize)
    try:
        for view, cam in tie_cameras(sc):
            for max_steps in (256, 1):
                g = gpu_render(torch_cuda, r, sc, w, h, max_steps=max_steps, camera=cam)
                assert_frame_is_oracle(g, e, sc, w, h, "%s, max_steps=%d" % (view, max_steps), max_steps, cam, view)
                ids = set(g["id"].ravel().tolist())
                if e is TANGENT:
                    assert view == "insane" or max_steps == 1 or ids == {0, 1, 2}
                else:
                    assert 2 not in ids and (view == "insane" or 1 in ids)          # the lower id wins everywhere
    finally:
        r.close()
