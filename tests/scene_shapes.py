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
from test_gpu_fuzz import DEGENERATE_CASES, balanced_tree_text, chain_text, deep_tree_text, fmt, num, rand_scene

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
    text: Callable[[], str] = field(repr=False, compare=False)      # the scene as `.lol` text
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
        _scenes[shape.name] = S.Scene.parse_string(shape.text())
    return _scenes[shape.name]


def _file(name):
    return lambda: open(os.path.join(SCENES_DIR, name + ".lol")).read()


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
        return text_fn(depth, **kw)
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
            lambda: chain_text(140), n_ops=284, max_stack=2, n_lights=1, rung=(1, False), size=(32, 18))
BIG = Shape("chain550", "1104 ops: above the inlining limit, the SDF is one out-of-line function and nothing else",
            lambda: chain_text(550), n_ops=1104, max_stack=2, n_lights=1, rung=(1, False), size=(24, 13))


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


# ---- hostile scenes (tests/test_gpu_hostile.py): the inputs that strain what the exact shortcuts are decided from — the culling bounds
# and the k-d plan, the carried bound, the division skip, the fast roots' range fall-back, the host's own first step — and exact ties.
# Its users: tests/test_gpu_hostile.py (every kernel that renders frames), tests/reference_frames.py (the recorded frames of the
# reference's own renderer), the pixel lists of the ties in tests/test_gpu_rays.py and test_gpu_shades.py, and — with lists of rays
# made from each scene's culling bounds, tests/hostile_rays.py — tests/test_gpu_hostile_queries.py (ray and shading queries, light
# passes, the resolves, light updates), whose inputs tests/test_hostile_rays.py holds on the CPU
def stress_scene(rng):
    """Scenes that lean on the culling bounds: many top-level objects of very different sizes and distances, smoothness
    from 0.01 to 60 (and 0 / negative: no bound), coordinates up to 10^4, negative radii, cameras inside objects.
    (The generator of tests/tools/soak.py's `stress` mode, which imports it from here: for a given rng the text is what it has
    always been, byte for byte — tests/test_scene_shapes.py holds scene 0 of seed 7707 to the recorded text.)"""
    scale = float(rng.choice([1, 1, 1, 30, 1000]))

    def leaf():
        c = rng.normal(size=3) * [6, 3, 6] * scale + [0, 1, -8 * scale]
        if rng.random() < 0.6:
            return "sphere { point = %s, radius = %s }" % (fmt(c), num(rng.choice([-1, 0, 0.01, 0.5, 2, 9]) * scale))
        return "box { point = %s, point2 = %s, radius = %s }" % (fmt(c), fmt(rng.uniform(0, 4, 3) * scale), num(rng.choice([0, 0.3, 2]) * scale))

    def tree(d):
        if d == 0 or rng.random() < 0.35:
            return leaf() if rng.random() < 0.93 else "plane { y = %s }" % num(rng.uniform(-5, 0) * scale)
        k = rng.choice([0, -1, 0.01, 0.3, 1, 4, 15, 60]) * scale
        return "smooth_union { smoothness = %s, a = %s, b = %s }" % (num(k), tree(d - 1), tree(int(rng.integers(0, d))))

    mats = "materials { { shininess = 2, diffuse = (0,0,0), specular = (0,0,0), ambient = (.1,.1,.1) }, { shininess = 9, diffuse = (.5,.4,.3), specular = (.3,.3,.3), ambient = (.1,.1,.1) } }"
    comps = ["camera { point = %s, direction = %s, fov = %s }" % (fmt(rng.normal(size=3) * [3, 2, 3] * scale), fmt(rng.normal(size=3) * 0.3 + [0, -0.2, -1]), num(rng.uniform(50, 150)))]
    for _ in range(int(rng.integers(0, 3))):
        comps.append("point_light { point = %s, diffuse_intensity = (2,2,2), specular_intensity = (1,1,1) }" % fmt(rng.normal(size=3) * 8 * scale + [0, 9 * scale, 0]))
    order = [0, 1] if rng.random() < 0.5 else [1, 0]
    objs = []
    crowd = rng.random() < 0.25                      # many shallow objects: the k-d clusters of the culling plan
    for _ in range(int(rng.integers(10, 60)) if crowd else int(rng.integers(1, 9))):
        o = tree(int(rng.integers(0, 2 if crowd else 4)))
        head, rest = o.split("{", 1)
        objs.append("%s{ material = #1,%s" % (head, rest))
    if rng.random() < 0.7:
        objs.insert(int(rng.integers(0, len(objs) + 1)), "plane { material = #1, y = %s }" % num(rng.uniform(-6, -1) * scale))
    return mats + "\nscene { " + ",\n".join(comps + objs) + " }\n"


@dataclass(frozen=True)
class Tie:
    """the objects of a tie scene, in file order, as `.lol` text; `tied`: the 1-based ids of those whose distances are EQUAL binary32
    values at the camera position — and, where `along_ray`, at every point of the central ray up to the hit"""
    objects: Tuple[str, ...]
    tied: Tuple[int, ...]
    along_ray: bool


@dataclass(frozen=True)
class Hostile:
    name: str
    purpose: str
    text: str = field(repr=False)
    size: Tuple[int, int] = (23, 13)
    families: bool = True               # rendered through the supersampled, adaptive, batch and blend kernels too
    own_kernel: bool = True             # the scene compiler takes it on (False: it legitimately stays on the interpreter)
    tie: Optional[Tie] = field(default=None, repr=False)


HOSTILE_SEED = 20264742           # chosen on the CPU for what tests/test_scene_shapes.py holds the generated scenes to
N_HOSTILE_GENERATED = 14
HOSTILE_SIZE = (23, 13)                 # the family tests' own fuzz size
HOSTILE_CONTRAST = 16

# four materials of four colours, so that a wrong winner of a tie is another colour and not only another id; #0 is what a ray that
# escapes wears too
TIE_MATERIALS = ("materials { { shininess = 4, diffuse = (.6,.1,.1), specular = (.2,.2,.2), ambient = (.25,.05,.05) },"
                 " { shininess = 4, diffuse = (.1,.1,.6), specular = (.2,.2,.2), ambient = (.05,.05,.25) },"
                 " { shininess = 8, diffuse = (.1,.6,.1), specular = (.3,.3,.3), ambient = (.05,.25,.05) },"
                 " { shininess = 2, diffuse = (.4,.4,.4), specular = (.1,.1,.1), ambient = (.1,.1,.1) } }\n")
TIE_HEAD = ("camera { point = (0, 0, 0), direction = (0, 0, -1), fov = 60 }",
            "point_light { point = (3, 5, 0), diffuse_intensity = (2,2,2), specular_intensity = (1,1,1) }")


def tie_text(objects, head=TIE_HEAD):
    return TIE_MATERIALS + "scene { " + ",\n".join(tuple(head) + tuple(objects)) + " }\n"


def _wear(obj, material):
    head, rest = obj.split("{", 1)
    return "%s{ material = #%d,%s" % (head, material, rest)


def _tie(name, purpose, objects, tied, along_ray=True):
    return Hostile(name, purpose, tie_text(objects), tie=Tie(tuple(objects), tuple(tied), along_ray))


def _twins(name, purpose, obj_a, obj_b, rest):
    """obj_a wearing #0 then obj_b wearing #1, and the twin scene in the opposite file order: the winner is id 1 in both, its colour
    is not"""
    return [_tie(name + "-01", purpose, (_wear(obj_a, 0), _wear(obj_b, 1)) + rest, (1, 2)),
            _tie(name + "-10", purpose + " (the twin: opposite file order)", (_wear(obj_b, 1), _wear(obj_a, 0)) + rest, (1, 2))]


def _tie_crowd():
    """twelve small spheres on a grid of small integers round three coincident ones (ids 3, 9 and 14 of 16): fifteen bounded objects,
    which the culling plan splits into k-d clusters and evaluates in another order than the file's; the plane, which has no bound,
    is evaluated before all of them"""
    grid = ["sphere { material = #3, point = (%d, %d, %d), radius = 0.5 }" % (x, y, z)
            for z in (-6, -9, -12) for x, y in ((-6, 1), (-3, -1), (3, 1), (6, -1))]
    same = "sphere { point = (0, 0, -6), radius = 1 }"
    objs = grid[:2] + [_wear(same, 0)] + grid[2:6] + ["plane { material = #3, y = -7 }"] + [_wear(same, 1)] + grid[6:10] + [_wear(same, 2)] + grid[10:]
    return objs


_FLOOR = ("plane { material = #3, y = -7 }",)           # (farther from the camera than the tied objects: they are the first step)
TIE_SCENES = (
    _twins("tie-spheres", "two identical spheres", "sphere { point = (0, 0, -5), radius = 1 }", "sphere { point = (0, 0, -5), radius = 1 }", _FLOOR)
    + _twins("tie-boxes", "two identical rounded boxes", "box { point = (0, 0, -5), point2 = (1, 0.5, 0.75), radius = 0.25 }",
             "box { point = (0, 0, -5), point2 = (1, 0.5, 0.75), radius = 0.25 }", _FLOOR)
    # sminf(a, a, k) = a - k / 4: the union of two spheres of radius 1 with k = 4 is |p - c| - 1 - 1, the sphere of radius 2 is
    # |p - c| - 2, and both are exact wherever |p - c| >= 2 (a small integer taken from a larger float): equal everywhere outside
    + _twins("tie-sphere-union", "a sphere and a smooth union of two spheres of the same value", "sphere { point = (0, 0, -8), radius = 2 }",
             "smooth_union { smoothness = 4, a = sphere { point = (0, 0, -8), radius = 1 }, b = sphere { point = (0, 0, -8), radius = 1 } }", _FLOOR)
    + [_tie("tie-crowd", "three coincident spheres in a crowd that the culling plan clusters and re-orders", _tie_crowd(), (3, 9, 14)),
       # |(-3, 0, -4)| - 1 = 5 - 1 and |(0, 0, -6)| - 2 = 6 - 2: both 4 at the camera and nowhere else on the central ray
       _tie("tie-camera", "the camera exactly equidistant from two different spheres: a tie on the first step only",
            ("sphere { material = #0, point = (-3, 0, -4), radius = 1 }", "sphere { material = #1, point = (0, 0, -6), radius = 2 }") + _FLOOR,
            (1, 2), along_ray=False)]
)


def hostile_texts():
    rng = np.random.default_rng(HOSTILE_SEED)
    return [stress_scene(rng) for _ in range(N_HOSTILE_GENERATED)]


def _generated():
    return [Hostile("stress%02d" % i, "scene %d of stress_scene under HOSTILE_SEED" % i, t) for i, t in enumerate(hostile_texts())]


HOSTILE = _generated() + TIE_SCENES
HOSTILE_BY_NAME = {e.name: e for e in HOSTILE}
HOSTILE_TIES = [e for e in HOSTILE if e.tie is not None]


def hostile_scene(e: Hostile) -> "S.Scene":
    if ("hostile", e.name) not in _scenes:
        _scenes[("hostile", e.name)] = S.Scene.parse_string(e.text)
    return _scenes[("hostile", e.name)]


# which of HOSTILE, in its order, have an edge AND a smooth area under their own camera at their size and HOSTILE_CONTRAST (what the
# input is decides: tests/test_scene_shapes.py holds the tuple to adaptive_reference).  Six of the generated scenes are one object
# seen from inside, or from so near that it fills the frame: they are kept, as what they are.
# (Cost of one aa_reference frame at s = 4 on one CPU core: 0.10 s for the slowest, stress04 with its 41 objects; no size is reduced.)
HOSTILE_REFINES_SOME = (True, False, False, True, True, False, True, False, False, True, True, True, True, False,
                        True, True, True, True, True, True, True, True)
