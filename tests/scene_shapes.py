"""A catalogue of scene shapes for tests/test_gpu_families.py: which scene, what it is for, and what flattening it must give.

Not a test file.  tests/test_scene_shapes.py holds every entry to what it declares here, on the CPU; the GPU tests then ask the
library which kernel and which interpreter rung really ran (Renderer.interp_variant, kernel_name, view_samples_kernel_name,
specialize_state) and compare with the same declarations.

The interpreter's ladder (loltracer_amd/csrc/lol_gpu.hip, interp_rung): operand-stack classes 1, 3, 7, 11, 63 with the tables in LDS,
and 3, 11, 63 with the tables read from global memory, which is where table_dwords = 9 lights + 10 materials + roots exceeds
TABLES_LDS_MAX_DWORDS (lol_kernel.h).
"""
import os
from dataclasses import dataclass, field
from typing import Callable, Optional, Tuple

import numpy as np

from loltracer_amd import scene as S
from test_gpu_fuzz import DEGENERATE_CASES, balanced_tree_text, chain_scene, deep_tree_text, fmt, num, rand_scene

SCENES_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes")
TABLES_LDS_MAX_DWORDS = 1024            # lol_kernel.h
ALL_RUNGS = {(1, False), (3, False), (7, False), (11, False), (63, False), (3, True), (11, True), (63, True)}
N_VIEWS = 4                             # cameras round the scene in every batch (S.orbit_cameras)
SAMPLES = (2, 4)


def table_dwords(prog) -> int:
    return 9 * prog.n_lights + 10 * prog.n_materials + prog.n_roots


def rung_of(prog) -> Tuple[int, bool]:
    """the ladder restated (ONLY for the CPU test of this catalogue: the GPU tests ask the library)"""
    need = max(1, prog.max_stack - 1)
    cls = 1 if need <= 1 else 3 if need <= 3 else 7 if need <= 7 else 11 if need <= 11 else 63
    if table_dwords(prog) <= TABLES_LDS_MAX_DWORDS:
        return cls, False
    return (3 if cls <= 3 else 11 if cls <= 11 else 63), True


@dataclass(frozen=True)
class Shape:
    name: str
    purpose: str
    build: Callable[[], "S.Scene"] = field(repr=False, compare=False)
    n_ops: int
    max_stack: int
    n_lights: int
    rung: Tuple[int, bool]              # (ssize, tables_global) of the interpreter instantiation it must run on
    size: Tuple[int, int]               # the ragged frame size its GPU cases render (sized by the oracle's cost)
    contrast: Optional[int] = 16        # the adaptive contrast its GPU cases use: 0 < refined < w h at `size` (None: not held to that)

    @property
    def tables_global(self) -> bool:
        return self.rung[1]


_scenes = {}


def scene_of(shape: Shape) -> "S.Scene":
    if shape.name not in _scenes:
        _scenes[shape.name] = shape.build()
    return _scenes[shape.name]


def _file(name):
    return lambda: S.Scene.parse_file(os.path.join(SCENES_DIR, name + ".lol"))


def many_materials(n=110, seed=17) -> str:
    """a `materials { ... }` block of n materials: 10 n dwords of table, beyond TABLES_LDS_MAX_DWORDS from n = 103 on.  #0 as in the
    trees (escaped rays), #1 the trees' own, the rest random — the last one is what the plane of `big_table_extra` wears"""
    rng = np.random.default_rng(seed)
    mats = ["{ shininess = 2, diffuse = (0,0,0), specular = (0,0,0), ambient = (.02,.02,.02) }",
            "{ shininess = 8, diffuse = (.5,.5,.5), specular = (.2,.2,.2), ambient = (.1,.1,.1) }"]
    for _ in range(n - 2):
        mats.append("{ shininess = %s, diffuse = %s, specular = %s, ambient = %s }" % (
            num(rng.choice([1, 2, 8, 30.5])), fmt(rng.uniform(0.1, 0.6, 3)), fmt(rng.uniform(0, 0.4, 3)), fmt(rng.uniform(0.05, 0.3, 3))))
    return "materials { %s }\n" % ",\n".join(mats)


def big_table_extra(n=110, plane_y=-3) -> str:
    """a second light and a plane under the tree wearing the LAST material of the table: both ends of both tables are read"""
    return (", point_light { point = (-6,7,2), diffuse_intensity = (1,.8,.6), specular_intensity = (.5,.5,.5) }"
            ", plane { material = #%d, y = %s }" % (n - 1, num(plane_y)))


def compact_tree_text(depth, **kw):
    """test_gpu_fuzz's tree of 4096 small spheres is a sparse cloud: at 12 x 6 every pixel but one is an edge at any contrast.  The
    same tree drawn together into one blob has an inside and a sky, so that an adaptive frame refines some pixels and leaves some"""
    return balanced_tree_text(depth, 3, (1.2, 0.8, 1.0), (0, 0, -6), (0.2, 0.5), 0.25, **kw)


def _tree(text_fn, depth, big_table=False):
    def build():
        kw = dict(materials=many_materials(), extra=big_table_extra()) if big_table else {}
        return S.Scene.parse_string(text_fn(depth, **kw))
    return build


# ---- one shape per interpreter rung, all eight.  (Costs of one aa_reference frame at `size`, s = 2 / s = 4, on one CPU core:
# depth 9 at 20 x 11 about 0.3 s / 1.1 s, depth 12 at 12 x 6 about 0.5 s / 1.9 s; twice that with the second light and the plane.)
RUNG_SHAPES = [
    Shape("scene", "example scene: flat objects, rung 1", _file("scene"), n_ops=8, max_stack=1, n_lights=1, rung=(1, False), size=(37, 19)),
    Shape("scene4", "example scene: the blob, rung 3; the scene compiler's inlined two-kernel module", _file("scene4"),
          n_ops=12, max_stack=3, n_lights=2, rung=(3, False), size=(37, 19)),
    Shape("tree5", "balanced tree of 32 spheres: rung 7, run by no other test of the new families", _tree(deep_tree_text, 5),
          n_ops=64, max_stack=6, n_lights=1, rung=(7, False), size=(29, 15)),
    Shape("tree9", "balanced tree of 512 spheres: rung 11 (the last with 4-bit slot fields)", _tree(deep_tree_text, 9),
          n_ops=1024, max_stack=10, n_lights=1, rung=(11, False), size=(20, 11)),
    Shape("tree12", "balanced tree of 4096 spheres: rung 63 (slots in words of their own)", _tree(compact_tree_text, 12),
          n_ops=8192, max_stack=13, n_lights=1, rung=(63, False), size=(12, 6)),
    Shape("tree2-tables", "4 spheres, 110 materials: rung 3 with the tables in global memory; the scene compiler's TABLES_GLOBAL module",
          _tree(deep_tree_text, 2, big_table=True), n_ops=10, max_stack=3, n_lights=2, rung=(3, True), size=(29, 15)),
    Shape("tree9-tables", "512 spheres, 110 materials: rung 11 with the tables in global memory (run by no test before)",
          _tree(deep_tree_text, 9, big_table=True), n_ops=1026, max_stack=10, n_lights=2, rung=(11, True), size=(20, 11)),
    Shape("tree12-tables", "4096 spheres, 110 materials: rung 63 with the tables in global memory (run by no test before)",
          _tree(compact_tree_text, 12, big_table=True), n_ops=8194, max_stack=13, n_lights=2, rung=(63, True), size=(12, 6)),
]
RUNG = {s.name: s for s in RUNG_SHAPES}

# ---- the scene compiler's forms.  (Stack depth means nothing to straight-line code: the 8192-op trees stay on the interpreter.)
MID = Shape("chain140", "284 ops: the mid-size scene, out of line on the first tier and inlined on the second",
            lambda: chain_scene(140), n_ops=284, max_stack=2, n_lights=1, rung=(1, False), size=(32, 18))
BIG = Shape("chain550", "1104 ops: above the inlining limit, the SDF is one out-of-line function and nothing else",
            lambda: chain_scene(550), n_ops=1104, max_stack=2, n_lights=1, rung=(1, False), size=(24, 13))


@dataclass(frozen=True)
class Form:
    name: str
    shape: Shape
    specialize: int                     # lol_gpu_set_specialize
    form: str                           # what the scene compiler's log must say of the kernel in use: "out of line" or "inlined"
    second_tier: bool                   # the kernel in use is a mid-size scene's second one
    two_kernels: bool                   # <= 256 ops: the module holds the pipeline with and without step counters


FORMS = [
    Form("inline-small", RUNG["scene4"], 1, "inlined", False, True),
    Form("mid-out-of-line", MID, 5, "out of line", False, False),
    Form("mid-inlined", MID, 1, "inlined", True, False),
    Form("big-out-of-line", BIG, 1, "out of line", False, False),
    Form("tables-global", RUNG["tree2-tables"], 1, "inlined", False, True),
]

# ---- eight random scenes (test_gpu_fuzz.rand_scene): 0, 1, 2 and 3 lights and every op kind between them, and each with an adaptive
# frame that refines some pixels and leaves some (the seed was chosen for that, on the CPU: tests/test_scene_shapes.py)
FUZZ_SEED = 20261020
FUZZ_SIZE = (23, 13)
FUZZ_CONTRAST = 16
N_FUZZ = 8


def fuzz_texts():
    rng = np.random.default_rng(FUZZ_SEED)
    return [rand_scene(rng) for _ in range(N_FUZZ)]


def fuzz_scenes():
    if "fuzz" not in _scenes:
        _scenes["fuzz"] = [S.Scene.parse_string(t) for t in fuzz_texts()]
    return _scenes["fuzz"]


# ---- the six degenerate inputs of test_gpu_fuzz.test_degenerate_inputs: no objects at all (nothing to refine, by construction),
# the camera inside a sphere, NaN from a negative shininess, a plane through the camera, |p - c|^2 = inf, |p - c|^2 = 0
DEGENERATE_SIZE = (23, 13)
DEGENERATE_CONTRAST = 16
# which of them have an edge AND a smooth area under their own camera at DEGENERATE_SIZE (what the input is decides, not the renderer)
DEGENERATE_REFINES_SOME = (False, True, True, False, True, False)
DEGENERATE_NAMES = ["no-objects", "inside-a-sphere", "nan-shininess", "camera-on-a-plane", "inf-squared-length", "zero-squared-length"]


def degenerate_scenes():
    if "degenerate" not in _scenes:
        _scenes["degenerate"] = [S.Scene.parse_string(t) for t in DEGENERATE_CASES]
    return _scenes["degenerate"]


# ---- max_steps: scene4 at one small size, contrast 16.  (With 0 steps every ray escapes: one id, one colour, nothing to refine —
# by construction; 1, 7 and 128 refine some pixels and leave some.)
MAX_STEPS = (0, 1, 7, 128)
MAX_STEPS_SHAPE = RUNG["scene4"]
MAX_STEPS_SIZE = (37, 19)


def cameras(sc):
    """the cameras of every batch of the family tests"""
    return S.orbit_cameras(sc, N_VIEWS)
