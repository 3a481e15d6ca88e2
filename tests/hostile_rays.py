"""The list of rays of a hostile scene (tests/scene_shapes.py, HOSTILE): what tests/test_gpu_hostile_queries.py gives the list kernels —
ray queries, shading queries, light passes, the resolves and light updates — on the scenes that strain the exact shortcuts.  Not a
test file.  tests/test_hostile_rays.py holds, on the CPU, that the lists are what they claim.

A frame's wave holds 64 neighbouring pixels of one camera; a list's wave holds 64 unrelated rays, and that is where the culling plan's
skips (a run of objects is jumped over only if EVERY lane may skip it), the interpreter's wave-uniform cool-down and the scene
kernels' bound carried along each ray are least protected by coherence.  The parts of a list:

  (a) - (e)  ray_reference.ray_set(sc, SEED, "abcde") as it is: camera rays, rays from their hits towards light 0, those directions
             times 0.5 and 2, origins inside objects, the eight specials inside waves (THINNED: two scenes keep half of them);
  (f) aimed  for every top-level object with a finite culling bound (C, R') (lol_gpu_cull_bounds: no device needed), three rays from
             C + (R' + gap) u towards C, u a seeded unit vector, gap = clamp(0.25 |R'|, 0.5, 20): small against MAX_DIST = 100, so
             that an object far from the scene's camera, or hidden from it, is still reached;
  (g) grazing  for the same objects, three rays tangent to the bounding sphere — where the culling test flips: they pass C at the
             distance R' (1 + eps), eps = -2^-10, 0, +2^-10, from C + R' (1 + eps) u - back v along v, v a unit vector normal to u,
             back = min(60, R' + gap); where lol_gpu_cull_bounds_clusters gives two spheres, each of those is grazed too;
  (h) unbounded  for an object WITHOUT a bound (a plane, a union with k <= 0): two rays straight down (-y) from seeded points 1 and
             30 above the scene's camera.

bound_rays(sc, seed) makes (f) - (h) for ANY scene — tests/test_gpu_scene_records.py builds the list of every record from that
record's own bounds with it; for the entries of HOSTILE the lists are byte for byte what they were before it was factored out
(tests/test_hostile_rays.py holds their digests).

The list comes in two orders.  Object-major: the kinds one behind the other, (f) - (h) grouped by object, so that whole waves may skip
the same runs.  A seeded permutation of it: the lanes of a wave disagree, and the cool-down is exercised.  A ray's answer must not
depend on the order.  The length is no multiple of 64 (a trailing ray is dropped if it is): the last wave is ragged.
"""
import ctypes as C

import numpy as np

import ray_reference as R
import scene_shapes as SH
from loltracer_amd import gpu

# chosen on the CPU for what tests/test_hostile_rays.py holds the lists to (the populations and the distinct objects reached)
SEED = 20261020
EPS = (-2.0 ** -10, 0.0, 2.0 ** -10)
BACK_MAX = 60.0
ABOVE = (1.0, 30.0)
KINDS = "afgh"                           # (a) - (e) are ray_set's own and all go as "a"
# The two scenes whose references cost most (two lights, shadow marches of 30 steps on average: over 2 s of CPU time for the whole
# list) keep every second ray of (a) - (e), and every special: a shorter list of their own, the catalogue stays as it is.
THINNED = {"stress06": 2, "stress12": 2}


def specials_among(sc, rays):
    """which rays of a list are ray_reference's SPECIALS, which ray_set makes from the central ray of its 13 x 5 frame"""
    a = R.camera_rays(sc, 13, 5)
    specials = {s.tobytes() for s in R.special_rays(a[len(a) // 2, :3], a[len(a) // 2, 3:])}
    return np.array([r.tobytes() in specials for r in rays], dtype=bool)


def cull_bounds(prog, root):
    """(C, R') of top-level object `root` (0-based), or None where it has no finite bound"""
    c, r = (C.c_float * 3)(), C.c_float()
    if gpu.gpu_lib().lol_gpu_cull_bounds(C.byref(prog), root, c, C.byref(r)) != 1:
        return None
    c, r = np.array(list(c), np.float64), float(r.value)
    return (c, r) if np.isfinite(c).all() and np.isfinite(r) else None


def cull_clusters(prog, root):
    """the two spheres (C_j, R'_j) the culling plan tests a spread-out union with, or []"""
    out = ((C.c_float * 4) * 3)()
    n = gpu.gpu_lib().lol_gpu_cull_bounds_clusters(C.byref(prog), root, out)
    cl = [(np.array(list(out[j])[:3], np.float64), float(out[j][3])) for j in range(n)]
    return [(c, r) for c, r in cl if np.isfinite(c).all() and np.isfinite(r)]


def bounded_objects(sc):
    """{0-based index of a top-level object: (C, R')} of the objects with a finite bound"""
    prog = sc.flatten()
    return {i: b for i in range(prog.n_roots) for b in [cull_bounds(prog, i)] if b is not None}


def gap_of(r):
    return float(np.clip(0.25 * abs(r), 0.5, 20.0))


def _unit(rng):
    while True:
        u = rng.normal(size=3)
        n = float(np.linalg.norm(u))
        if n > 1e-3:
            return u / n


def _normal_to(rng, u):
    while True:
        v = np.cross(u, rng.normal(size=3))
        n = float(np.linalg.norm(v))
        if n > 1e-3:
            return v / n


def _ray(origin, direction):
    d = np.asarray(direction, np.float32)
    return np.concatenate([np.asarray(origin, np.float64).astype(np.float32), R.v3normalize(d)]).astype(np.float32)


def aimed(rng, c, r):
    out = []
    for _ in range(3):
        u = _unit(rng)
        out.append(_ray(c + (r + gap_of(r)) * u, -u))
    return out


def grazing(rng, c, r):
    out = []
    back = min(BACK_MAX, r + gap_of(r))
    for eps in EPS:
        u = _unit(rng)
        v = _normal_to(rng, u)
        out.append(_ray(c + r * (1.0 + eps) * u - back * v, v))
    return out


_looks = {}


def hostile_look(sc):
    """the scene under another look — every light's intensities, every material's colours and the ambient colour replaced, as in
    test_gpu_light.test_light_counts_and_large_tables — kept per scene: the references are keyed by it"""
    if id(sc) not in _looks:
        nl, nm = len(sc.lights()), len(sc.materials())
        _looks[id(sc)] = (sc, sc.with_look(lights=[((.2, .9, .4), (.7, .1, .5))] * nl, materials=[((.1, .2, .3), (.3, .2, .1), (.4, .4, .1))] * nm,
                                           ambient=(.6, .5, .4)))
    return _looks[id(sc)][1]


_lists = {}


def bound_rays(sc, seed):
    """parts (f) - (h) for `sc` under `seed` (anything numpy's default_rng takes), object-major: (rays [n, 6] f32, kind [n], obj [n]) —
    aimed and grazing rays made from the scene's OWN culling bounds, and the rays straight down for its objects without one"""
    rng = np.random.default_rng(seed)
    rays, kind, obj = [], [], []
    prog = sc.flatten()
    cam = np.array(sc.camera.point.tuple(), np.float64)
    for i in range(prog.n_roots):
        b = cull_bounds(prog, i)
        if b is None:
            new = [("h", np.concatenate([(cam + [rng.uniform(-1, 1), up, rng.uniform(-1, 1)]).astype(np.float32),
                                         np.array([0, -1, 0], np.float32)]).astype(np.float32)) for up in ABOVE]
        else:
            new = [("f", q) for q in aimed(rng, *b)] + [("g", q) for q in grazing(rng, *b)]
            for cl in cull_clusters(prog, i):
                new += [("g", q) for q in grazing(rng, *cl)]
        rays.append(np.array([q for _, q in new], np.float32).reshape(-1, 6))
        kind += [k for k, _ in new]
        obj += [i] * len(new)
    return rays, kind, obj


def _build(e):
    sc = SH.hostile_scene(e)
    base = R.ray_set(sc, SEED, "abcde")
    if e.name in THINNED:
        keep = specials_among(sc, base) | (np.arange(len(base)) % THINNED[e.name] == 0)
        base = base[keep]
    more, more_kind, more_obj = bound_rays(sc, [SEED, SH.HOSTILE.index(e)])
    rays, kind, obj = [base] + more, ["a"] * len(base) + more_kind, [-1] * len(base) + more_obj
    rays = np.ascontiguousarray(np.concatenate(rays), dtype=np.float32)
    if len(rays) % 64 == 0:
        rays, kind, obj = rays[:-1], kind[:-1], obj[:-1]
    perm = np.random.default_rng([SEED, SH.HOSTILE.index(e), 1]).permutation(len(rays))
    out = dict(rays=rays, kind=np.array(kind), obj=np.array(obj, np.int64), perm=perm, permuted=np.ascontiguousarray(rays[perm]))
    for a in out.values():
        a.setflags(write=False)
    return out


def hostile_ray_parts(e):
    """dict(rays [n, 6] f32 object-major, kind [n] of KINDS, obj [n]: the 0-based object a ray of (f) - (h) was made for or -1,
    perm [n], permuted = rays[perm]) of entry `e` of scene_shapes.HOSTILE; once per entry, read-only"""
    if e.name not in _lists:
        _lists[e.name] = _build(e)
    return _lists[e.name]


def hostile_ray_list(e):
    """the list of entry `e` of scene_shapes.HOSTILE in object-major order: n x 6 float32, read-only, the same array every time"""
    return hostile_ray_parts(e)["rays"]


def hostile_ray_orders(e):
    """[(name of the order, rays, index into hostile_ray_list(e) of each ray)]: object-major and the seeded permutation"""
    p = hostile_ray_parts(e)
    return [("object-major", p["rays"], np.arange(len(p["rays"]))), ("permuted", p["permuted"], p["perm"])]
