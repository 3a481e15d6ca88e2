"""A catalogue of record sets for tests/test_gpu_scene_records.py: scenes of ONE structure whose numbers differ so much that the host's
per-record decisions differ — which objects have a culling bound, the order of evaluation, which objects carry the tie rule, how many
test records the interpreter list has and how long it is, the three exact skips, the first step, what an insane camera switches off.

Not a test file.  The three call families that take a scene per record (scene views, supersampled scene views, scene queries) build
all of that on the host per record (loltracer_amd/csrc/lol_gpu.hip, build_scene_records) and then run every record's list with the
fast paths the UPLOADED scene proved.  tests/test_scene_records.py holds every set to what it declares here, on the CPU, through
lol_gpu_interp_list_info and the oracle; the GPU tests then hold every record to the oracle's frame of that record's own scene.

A set: the text of the scene to upload and builders of 5 to 8 records of its structure — Scene.clone() with numbers edited, nothing
else.  A record's camera is its own scene's (edited like any other number).  Frames are HOSTILE_SIZE, 23 x 13: five ragged waves.
"""
import ctypes
from dataclasses import dataclass, field
from typing import Callable, Dict, Tuple

import numpy as np

import reference_frames as RF
import scene_shapes as SH
from loltracer_amd import scene as S
from scene_shapes import fmt, num

SIZE = SH.HOSTILE_SIZE
SEED = 20261021


@dataclass(frozen=True)
class Record:
    label: str
    scene: "S.Scene" = field(repr=False, compare=False)
    tied: Tuple[int, ...] = ()          # 1-based ids whose values are EQUAL binary32 along the central ray (the lowest wins)
    coincide: bool = True               # ... and everywhere else: the tied objects are one shape (False: equal on the plane y = 0 only)

    @property
    def camera(self):
        return RF.copy_camera(self.scene.camera)


@dataclass(frozen=True)
class RecordSet:
    name: str
    purpose: str
    text: Callable[[], str] = field(repr=False, compare=False)               # the scene to upload, as `.lol` text
    build: Callable[["S.Scene"], list] = field(repr=False, compare=False)    # the uploaded Scene -> [Record]
    uploads: Tuple[str, ...] = ()       # labels of the records that the "which scene is uploaded" test uploads in turn
    blends: bool = False                # K = 2 and K = 4 over its records
    samples: Tuple[int, ...] = (2,)
    size: Tuple[int, int] = SIZE


_kept: Dict = {}


def uploaded(rs: RecordSet) -> "S.Scene":
    if ("scene", rs.name) not in _kept:
        _kept[("scene", rs.name)] = S.Scene.parse_string(rs.text())
    return _kept[("scene", rs.name)]


def records(rs: RecordSet) -> list:
    """the records of a set: built once, never changed afterwards (references are cached by the Scene objects' ids)"""
    if ("records", rs.name) not in _kept:
        _kept[("records", rs.name)] = rs.build(uploaded(rs))
    return _kept[("records", rs.name)]


def record(rs: RecordSet, label: str) -> Record:
    return next(r for r in records(rs) if r.label == label)


def root_node(sc, obj_id):
    """the node of top-level object `obj_id` (1-based, file order)"""
    return sc.c.nodes[sc.c.roots[obj_id - 1]]


def leaves(sc, node_index):
    """indices of the primitives under a node, left to right"""
    n = sc.c.nodes[node_index]
    if n.type != S.NODE_SMOOTH_UNION:
        return [node_index]
    return leaves(sc, n.a) + leaves(sc, n.b)


def unions(sc, node_index):
    n = sc.c.nodes[node_index]
    if n.type != S.NODE_SMOOTH_UNION:
        return []
    return [node_index] + unions(sc, n.a) + unions(sc, n.b)


def put(v3, xyz):
    v3.x, v3.y, v3.z = (float(t) for t in xyz)


def insane_camera():
    """test_gpu_views.insane_camera's numbers — 10^16 away, not camera_sane — restated so that this catalogue loads no test module
    (tests/test_gpu_scene_records.py holds the two to each other)"""
    cam = S.Camera()
    cam.point = S.V3(1.0e16, 3.0, 2.5)
    cam.direction = S.V3(-1.0, 0.0, 0.0)
    cam.fov = float(np.float32(np.float32(60.0) / np.float32(180) * np.pi))
    return cam


def set_camera(sc, cam):
    ctypes.memmove(ctypes.byref(sc.c.camera), ctypes.byref(cam), ctypes.sizeof(S.Camera))


# ------------------------------------------------------------------------------------------------------------- crowd-regrouped
GRID_IDS = (1, 2, 4, 5, 6, 7, 10, 11, 12, 13, 15, 16)           # tie-crowd's twelve grid spheres; 3, 9 and 14 coincide, 8 is the plane
COINCIDENT = (3, 9, 14)
APART = ((-1.5, 2.0, -7.0), (0.0, -2.0, -7.5), (1.5, 2.0, -8.0))           # where the three coincident spheres go when pulled apart
RADII = (0.375, 0.5, 0.75, 1.0)


def _permuted(base, seed):
    """the grid spheres' centres dealt out anew among the same twelve ids, with seeded radii (another picture, other k-d clusters)"""
    sc = base.clone()
    rng = np.random.default_rng([SEED, seed])
    perm = rng.permutation(len(GRID_IDS))
    radii = rng.choice(RADII, size=len(GRID_IDS))
    for k, obj in enumerate(GRID_IDS):
        src = root_node(base, GRID_IDS[perm[k]])
        put(root_node(sc, obj).point, src.point.tuple())
        root_node(sc, obj).radius = float(radii[k])
    return sc


def _crowd(base):
    apart = base.clone()
    for obj, c in zip(COINCIDENT, APART):
        put(root_node(apart, obj).point, c)
    # ids 5 and 12, wearing #1 and #2, take the place in the middle of the view; the three that were there go apart
    pair = _permuted(apart, 3)
    for obj, mat in ((5, 1), (12, 2)):
        n = root_node(pair, obj)
        put(n.point, (0.0, 0.0, -6.0))
        n.radius, n.material = 1.0, mat
    # ids 4 and 13 mirror each other in the plane y = 0, which holds the central ray: equal values there, and the HIGHER id, on the
    # lower side of the k-d split, is evaluated first — the tie is decided by MOP_TIE and by nothing else
    mirror = _permuted(apart, 4)
    for obj, mat, y in ((4, 1, 0.75), (13, 2, -0.75)):
        n = root_node(mirror, obj)
        put(n.point, (0.0, y, -6.0))
        n.radius, n.material = 1.0, mat
    # every sphere in one place: a 15-way tie.  Object 1 wears a material no other object has
    heap = base.clone()
    for obj in range(1, 17):
        n = root_node(heap, obj)
        if n.type == S.NODE_SPHERE:
            put(n.point, (0.0, 0.0, -6.0))
            n.radius = 1.0
            n.material = 1 if obj == 1 else 3 if obj == 9 else n.material
    return [Record("file", base, COINCIDENT), Record("permuted-1", _permuted(base, 1), COINCIDENT), Record("apart", apart),
            Record("permuted-2", _permuted(base, 2), COINCIDENT), Record("pair-5-12", pair, (5, 12)),
            Record("heap", heap, tuple(i for i in range(1, 17) if i != 8)), Record("mirror-4-13", mirror, (4, 13), coincide=False)]


CROWD = RecordSet("crowd-regrouped", "tie-crowd's fifteen spheres regrouped: other k-d clusters, other orders of evaluation, the tie elsewhere",
                  lambda: SH.HOSTILE_BY_NAME["tie-crowd"].text, _crowd, uploads=("file", "permuted-2", "heap"), blends=True, samples=(2, 4))


# ----------------------------------------------------------------------------------------------------------------- bound-flips
# nine objects in file order (ids 1 ... 9): sphere, box, union of two spheres, PLANE, union of three spheres, nested union of
# (sphere + box) and (sphere + sphere), box, sphere, sphere.  The camera at (0, 1, 1.5) looks down -z; nothing contains the origin.
FLIPS_MATERIALS = ("materials { { shininess = 2, diffuse = (0,0,0), specular = (0,0,0), ambient = (.3,.35,.5) },"
                   " { shininess = 8, diffuse = (.7,.2,.2), specular = (.3,.3,.3), ambient = (.2,.05,.05) },"
                   " { shininess = 16, diffuse = (.2,.6,.2), specular = (.4,.4,.4), ambient = (.05,.2,.05) },"
                   " { shininess = 4, diffuse = (.3,.3,.7), specular = (.1,.1,.1), ambient = (.05,.05,.2) } }\n")
FLIPS_OBJECTS = (
    "sphere { material = #1, point = (-3, 1, -5), radius = 1 }",
    "box { material = #2, point = (3, 0.5, -6), point2 = (1, 0.75, 0.5), radius = 0.25 }",
    "smooth_union { material = #1, smoothness = 1, a = sphere { point = (-1, 2.5, -7), radius = 0.75 }, b = sphere { point = (0, 3, -7), radius = 0.5 } }",
    "plane { material = #3, y = -1 }",
    "smooth_union { material = #2, smoothness = 0.5, a = sphere { point = (0, 0, -4), radius = 0.5 }, b = smooth_union { smoothness = 0.75,"
    " a = sphere { point = (0.75, 0.25, -4.5), radius = 0.5 }, b = sphere { point = (1.5, 0, -4), radius = 0.375 } } }",
    "smooth_union { material = #3, smoothness = 1.5, a = smooth_union { smoothness = 0.25, a = sphere { point = (-2, 0, -8), radius = 1 },"
    " b = box { point = (-3.5, 0, -8), point2 = (0.5, 1, 0.5), radius = 0.125 } }, b = smooth_union { smoothness = 2,"
    " a = sphere { point = (-1, 1.5, -9), radius = 0.75 }, b = sphere { point = (-2.5, 2, -9), radius = 0.5 } } }",
    "box { material = #1, point = (2, 3, -8), point2 = (0.75, 0.5, 0.5), radius = 0.125 }",
    "sphere { material = #3, point = (4, 2.5, -9), radius = 1.25 }",
    "sphere { material = #2, point = (-0.5, -0.5, -3), radius = 0.375 }",
)
FLIPS_HEAD = ("ambient { color = (1, 1, 1) }", "camera { point = (0, 1, 1.5), direction = (0, -0.125, -1), fov = 80 }",
              "point_light { point = (4, 8, 2), diffuse_intensity = (1.5,1.5,1.5), specular_intensity = (1,1,1) }",
              "point_light { point = (-6, 5, -2), diffuse_intensity = (.5,.5,.75), specular_intensity = (.25,.25,.5) }")
FLIPS_N = len(FLIPS_OBJECTS)
FLIPS_PLANE = 4
FAR = 1e19                               # a centre there: no bound (test_culling.test_what_has_no_bound), and no finite scene


def flips_text():
    return FLIPS_MATERIALS + "scene { " + ",\n".join(FLIPS_HEAD + FLIPS_OBJECTS) + " }\n"


def unbound(sc, obj_id, how=0):
    """takes top-level object `obj_id`'s culling bound away, by the edit that fits its kind: a sphere's centre goes to 1e19, a box gets
    a negative point2 component, a union the smoothness 0 (how = 0) or -2"""
    n = root_node(sc, obj_id)
    if n.type == S.NODE_SPHERE:
        n.point.x = FAR
    elif n.type == S.NODE_BOX:
        n.half_extent.x = -n.half_extent.x
    elif n.type == S.NODE_SMOOTH_UNION:
        n.smoothness = 0.0 if how == 0 else -2.0
    else:
        raise ValueError("a plane never has a bound")
    return sc


def _flips(base):
    def without(ids, hows=()):
        sc = base.clone()
        for i, obj in enumerate(ids):
            unbound(sc, obj, hows[i] if i < len(hows) else 0)
        return sc
    shrunk = base.clone()                # a negative radius keeps its bound, a tiny one: |q| - r with r < 0 is >= |q|
    root_node(shrunk, 8).radius = -1.25
    return [Record("all-bounded", base), Record("minus-1", without((3,))), Record("minus-3", without((3, 5, 2), (0, 1))),
            Record("minus-5", without((3, 5, 2, 1, 6), (0, 1))), Record("none-bounded", without((1, 2, 3, 5, 6, 7, 8, 9), (0, 0, 1, 0, 1))),
            Record("minus-2", without((9, 7))), Record("negative-radius", shrunk)]


FLIPS = RecordSet("bound-flips", "from every object bounded to none and back: lists of different lengths, orders and numbers of tests",
                  flips_text, _flips, uploads=("all-bounded", "none-bounded", "minus-3"), blends=True)


# ----------------------------------------------------------------------------------------------------------------- other-scale
# stress_scene's manner — objects of very different sizes and distances, smoothness from 0.01 to 60, a negative and a zero radius —
# with the camera 0.04 above the floor and 0.03 in front of a sphere, so that a record 1000 times as large still has surfaces
# within MAX_DIST = 100 of its camera
SCALE_OBJECTS = (
    "sphere { material = #1, point = (-0.03, -0.94, -0.075), radius = 0.05 }",
    "plane { material = #2, y = -1 }",
    "smooth_union { material = #1, smoothness = 0.01, a = sphere { point = (-0.05, -0.98, -0.04), radius = 0.01 }, b = sphere { point = (-0.04, -0.98, -0.05), radius = 0.01 } }",
    "box { material = #2, point = (0.07, -0.97, -0.05), point2 = (0.01, 0.02, 0.01), radius = 0.005 }",
    "smooth_union { material = #2, smoothness = 60, a = sphere { point = (40, 10, -70), radius = 9 }, b = smooth_union { smoothness = 4,"
    " a = sphere { point = (-12, 2, -25), radius = 2 }, b = box { point = (-5, 0, -20), point2 = (2, 3, 1), radius = 0.3 } } }",
    "sphere { material = #1, point = (0.03, -0.96, -0.09), radius = -1 }",
    "smooth_union { material = #1, smoothness = 0.3, a = sphere { point = (-0.3, -0.8, -0.5), radius = 0.25 }, b = sphere { point = (0.1, -0.9, -0.6), radius = 0 } }",
    "sphere { material = #2, point = (0.5, -0.5, -1.5), radius = 0.5 }",
)
SCALE_HEAD = ("ambient { color = (1, 1, 1) }", "camera { point = (0, -0.96, 0), direction = (0, -0.25, -1), fov = 110 }",
              "point_light { point = (3, 9, 4), diffuse_intensity = (2,2,2), specular_intensity = (1,1,1) }")
SCALE_MATERIALS = ("materials { { shininess = 2, diffuse = (0,0,0), specular = (0,0,0), ambient = (.1,.1,.1) },"
                   " { shininess = 9, diffuse = (.5,.4,.3), specular = (.3,.3,.3), ambient = (.1,.1,.1) },"
                   " { shininess = 3, diffuse = (.2,.4,.6), specular = (.2,.2,.2), ambient = (.05,.1,.15) } }\n")


def scale_text():
    return SCALE_MATERIALS + "scene { " + ",\n".join(SCALE_HEAD + SCALE_OBJECTS) + " }\n"


def scaled(base, factor):
    """every coordinate, radius, box size and smoothness, the lights' positions and the camera's, times `factor` (a power of two
    would be exact; 30 and 1000 are not, and need not be: the record is held to the oracle on its own numbers)"""
    sc = base.clone()
    f = np.float32(factor)
    mul = lambda v: float(np.float32(v) * f)                                     # noqa: E731
    for i in range(sc.c.n_nodes):
        n = sc.c.nodes[i]
        put(n.point, [mul(v) for v in n.point.tuple()])
        put(n.half_extent, [mul(v) for v in n.half_extent.tuple()])
        n.radius, n.smoothness = mul(n.radius), mul(n.smoothness)
    for i in range(sc.c.n_lights):
        put(sc.c.lights[i].point, [mul(v) for v in sc.c.lights[i].point.tuple()])
    put(sc.c.camera.point, [mul(v) for v in sc.c.camera.point.tuple()])
    return sc


def all_unions(sc):
    return [i for i in range(sc.c.n_nodes) if sc.c.nodes[i].type == S.NODE_SMOOTH_UNION]


MIXED_UNPROVEN = (float(np.float32(0.01)), 4.0)                             # the constants `mixed` replaces; 0.3 and 60 stay proven


def _scales(base):
    tiny = base.clone()
    root_node(tiny, 8).radius = 2.0 ** -21
    unproven, mixed = base.clone(), base.clone()
    for j, i in enumerate(all_unions(base)):                                     # k * 1.125 + 1/16: a constant of no upload of the set
        k = float(np.float32(base.c.nodes[i].smoothness) * np.float32(1.125) + np.float32(0.0625))
        unproven.c.nodes[i].smoothness = k
        if base.c.nodes[i].smoothness in MIXED_UNPROVEN:
            mixed.c.nodes[i].smoothness = k
    return [Record("scale-1", base), Record("scale-30", scaled(base, 30)), Record("tiny-radius", tiny), Record("scale-1000", scaled(base, 1000)),
            Record("unproven", unproven), Record("mixed", mixed)]


SCALES = RecordSet("other-scale", "records 30 and 1000 times the uploaded scene's size, a radius below 2^-20, smoothness constants no upload proved",
                   scale_text, _scales, uploads=("scale-1", "scale-1000", "unproven"))


# ------------------------------------------------------------------------------------------------------------------ skip-flips
def _skips(base):
    def tinted(step):
        """(every record its own shade of material #3, so that no two records show the same picture under one camera)"""
        sc = base.clone()
        sc.c.materials[3].diffuse.y = 0.25 + 0.0625 * step
        return sc
    lit = tinted(0)
    put(lit.c.materials[0].diffuse, (0.375, 0.25, 0.125))
    dull = tinted(1)
    dull.c.materials[2].shininess = -3.0
    glare = tinted(2)
    glare.c.lights[1].specular_intensity.y = float("inf")
    sane = tinted(3)
    far_light = tinted(4)
    far_light.c.lights[1].point.x = 1e16
    minus_zero = tinted(5)
    set_camera(minus_zero, RF.cam_at(-0.0, 1.0, 1.5, 0.0, -0.125, -1.0, 80.0))
    origin = tinted(6)
    set_camera(origin, RF.cam_at(0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 80.0))
    insane = tinted(7)
    set_camera(insane, insane_camera())
    return [Record("diffuse-0", lit), Record("negative-shininess", dull), Record("infinite-intensity", glare), Record("sane", sane),
            Record("light-1e16", far_light), Record("camera-minus-zero", minus_zero), Record("camera-origin", origin),
            Record("camera-insane", insane)]


# what the host decides for each record of skip-flips: (miss skip, dark skip, settled shadows = FINITE, the camera is sane, the first
# step is given)
SKIPS_DECLARED = {
    "diffuse-0": (False, True, True, True, True), "negative-shininess": (True, False, True, True, True),
    "infinite-intensity": (False, False, True, True, True), "sane": (True, True, True, True, True),
    "light-1e16": (True, True, False, True, True), "camera-minus-zero": (True, True, True, True, False),
    "camera-origin": (True, True, True, True, True), "camera-insane": (True, True, True, False, False),
}

SKIPS = RecordSet("skip-flips", "each host decision switched off alone: the three exact skips, FINITE, SANE, the first step",
                  flips_text, _skips, uploads=("sane", "infinite-intensity", "light-1e16"))


# ------------------------------------------------------------------------------------------------------------------------ deep
DEEP_K = (0.5, 0.375)


def _deep_tree(rng, depth, centre, k):
    if depth == 0:
        return "sphere { point = %s, radius = %s }" % (fmt(rng.normal(size=3) * [1.2, 0.8, 0.6] + centre), num(rng.uniform(0.3, 0.6)))
    return "smooth_union { smoothness = %s, a = %s, b = %s }" % (num(k), _deep_tree(rng, depth - 1, centre, k), _deep_tree(rng, depth - 1, centre, k))


def deep_text():
    """two balanced depth-4 trees of 16 spheres each (operand stack 5: rung 7) beside three loose spheres and a plane"""
    rng = np.random.default_rng([SEED, 4])
    trees = [_deep_tree(rng, 4, c, k).replace("{", "{ material = #%d," % m, 1) for c, k, m in (((-2.5, 1, -7), DEEP_K[0], 1), ((2.5, 1, -7), DEEP_K[1], 2))]
    objs = ("sphere { material = #3, point = (0, 3.5, -8), radius = 0.75 }", trees[0], "plane { material = #3, y = -1.5 }",
            "sphere { material = #2, point = (0, -0.5, -4), radius = 0.5 }", trees[1], "sphere { material = #1, point = (-4.5, 2.5, -10), radius = 1 }")
    head = ("ambient { color = (1, 1, 1) }", "camera { point = (0, 1, 2), direction = (0, -0.1, -1), fov = 80 }",
            "point_light { point = (2, 9, 3), diffuse_intensity = (2,2,2), specular_intensity = (1,1,1) }")
    return FLIPS_MATERIALS + "scene { " + ",\n".join(head + objs) + " }\n"


DEEP_TREES = (2, 5)                     # the ids of the two trees


def _deep(base):
    def moved(sc, obj, d):
        for i in leaves(sc, sc.c.roots[obj - 1]):
            p = sc.c.nodes[i].point
            put(p, (p.x + d[0], p.y + d[1], p.z + d[2]))
        return sc
    behind = moved(base.clone(), 2, (5.0, 0.5, -4.0))                            # the first tree behind the second
    negative = base.clone()
    for i in leaves(negative, negative.c.roots[5 - 1]):
        negative.c.nodes[i].radius = -negative.c.nodes[i].radius
    sharp = base.clone()
    for i in unions(sharp, sharp.c.roots[2 - 1]):
        sharp.c.nodes[i].smoothness = 0.0
    both = moved(sharp.clone(), 5, (-5.0, 0.0, -3.0))
    put(root_node(both, 4).point, (1.5, 0.0, -3.5))
    return [Record("file", base), Record("behind", behind), Record("negative-radii", negative), Record("smoothness-0", sharp),
            Record("smoothness-0-behind", both)]


DEEP = RecordSet("deep", "rung 7: cull test records between objects that use the operand stack, one tree moved, shrunk, un-smoothed",
                 deep_text, _deep, uploads=("file", "smoothness-0", "negative-radii"))


SETS = (CROWD, FLIPS, SCALES, SKIPS, DEEP)
BY_NAME = {s.name: s for s in SETS}


# -------------------------------------------------------------------------------- the host's three conditions, restated
def _finite(v):
    return v - v == 0.0


def _six(a, b):
    return a.tuple() + b.tuple()


def miss_skip_ok(sc) -> bool:
    """lol_gpu.hip, miss_skip_ok — restated ONLY for tests/test_scene_records.py (the GPU test asks the library)"""
    m = sc.materials()[0]
    return (all(v == 0.0 for v in _six(m.diffuse, m.specular)) and m.shininess >= 0.0
            and all(_finite(v) for l in sc.lights() for v in _six(l.diffuse_intensity, l.specular_intensity)))


def dark_skip_ok(sc) -> bool:
    return (all(_finite(v) for l in sc.lights() for v in _six(l.diffuse_intensity, l.specular_intensity))
            and all(m.shininess >= 0.0 and all(_finite(v) for v in _six(m.diffuse, m.specular)) for m in sc.materials()))


def _sane(v):
    return _finite(v) and abs(v) < float(np.float32(1e15))


def shadow_settle_ok(sc) -> bool:
    p = sc.flatten()
    for i in range(p.n_ops):
        o = p.ops[i]
        nf = {S.OP_SPHERE: 4, S.OP_RBOX: 7, S.OP_PLANE: 1, S.OP_SMIN: 1, S.OP_SMIN_R: 1}.get(o.op, 0)
        if not all(_sane(o.f[j]) for j in range(nf)):
            return False
    return all(_sane(v) for l in sc.lights() for v in l.point.tuple())


def camera_sane(sc, w, h) -> bool:
    fc = sc.frame_camera(w, h)
    return all(_sane(v) for v in np.frombuffer(bytes(memoryview(fc).cast("B")), np.float32).tolist())


def first_step_given(sc, w, h, oracle_sdf) -> bool:
    """program_first_step: a sane camera, no negative zero in its origin, and the scene's value there within [EPSILON, MAX_DIST]"""
    o = sc.camera.point.tuple()
    if not camera_sane(sc, w, h) or any(np.float32(v).view(np.uint32) == 0x80000000 for v in o):
        return False
    d = float(oracle_sdf(sc, o))
    return float(np.float32(0.001)) <= d <= 100.0
