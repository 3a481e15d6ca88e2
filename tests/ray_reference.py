"""The reference for ray queries (lol_gpu_trace_rays), restated for ARBITRARY rays.  Not a test file.

trace() is get_intersection (naive_renderer.c:48-69) and get_normal (:114-125) statement by statement in numpy binary32 scalars: every
+, * and / is one correctly rounded binary32 operation, as in the reference, which has no FMA.  The scene's distances come from the
oracle's own sdf() (lol_oracle_sdf) and the final normalisation from its v3normalize (lol_oracle_v3normalize), so nothing new is
needed under oracle/.  tests/test_ray_reference.py holds it to lol_oracle_probe_pixel, field by field, on the oracle's own rays.

same_bits() is how every comparison of the ray tests is made: equality of bit patterns.  Two NaNs count as the same: IEEE 754 leaves the
sign and payload of a NaN that an invalid operation produces to the implementation (x86 gives 0xFFC00000, gfx950 0x7FC00000), and
nothing in the reference looks at either.

ray_set() builds the list of rays the GPU tests share.
"""
import ctypes as C

import numpy as np

import oracle_lib as O

F = np.float32
EPSILON, MAX_DIST = F(0.001), F(100.0)
K = ((F(1), F(-1), F(-1)), (F(-1), F(-1), F(1)), (F(-1), F(1), F(-1)), (F(1), F(1), F(1)))      # k0 .. k3, naive_renderer.c:115-118


def sdf(sc, p):
    """sdf(scene, p) of naive_renderer.c:31-44: (distance, 1-based id of the nearest top-level object)"""
    did = C.c_uint32(0)
    d = O.lib().lol_oracle_sdf(sc.ptr, float(p[0]), float(p[1]), float(p[2]), C.byref(did))
    return F(d), int(did.value)


def v3normalize(v):
    a, out = (C.c_float * 3)(float(v[0]), float(v[1]), float(v[2])), (C.c_float * 3)()
    O.lib().lol_oracle_v3normalize(a, out)
    return (F(out[0]), F(out[1]), F(out[2]))


def along(ro, rd, t):
    """v3add(ro, v3scale(rd, t))"""
    return tuple(F(ro[k] + F(rd[k] * t)) for k in range(3))


def trace(sc, ro, rd, max_steps):
    """(dist, id, steps, normal) of one ray: binary32 scalars, an int, an int and three binary32 scalars"""
    ro, rd = tuple(F(v) for v in ro), tuple(F(v) for v in rd)
    with np.errstate(all="ignore"):
        dist, hit, steps = F(0.0), 0, 0
        for _ in range(max_steps):                               # :56
            d, hit = sdf(sc, along(ro, rd, dist))                # :57-58, :60
            dist = F(dist + d)                                   # :59
            steps += 1
            if d < EPSILON or dist > MAX_DIST:                   # :61
                break
        if dist >= MAX_DIST:                                     # :65
            hit = 0
        p = along(ro, rd, dist)                                  # :227
        h = F(dist / F(100.0))                                   # :119 — a division
        terms = []
        for k in K:                                              # :120-123
            s, _ = sdf(sc, tuple(F(p[j] + F(k[j] * h)) for j in range(3)))
            terms.append(tuple(F(k[j] * s) for j in range(3)))
        acc = terms[3]
        for t in (terms[2], terms[1], terms[0]):                 # :124 — v3add(p0, v3add(p1, v3add(p2, p3)))
            acc = tuple(F(t[j] + acc[j]) for j in range(3))
        return dist, hit, steps, v3normalize(acc)


_memo = {}


def reference(sc, rays, max_steps=256):
    """trace() of every ray of `rays` (n x 6 float32): dict(dist [n] f32, id [n] u32, steps [n] u32, normal [n, 3] f32).  Each ray is
    computed once per (scene, max_steps) whatever list it comes in: prefixes and permutations of a list cost nothing."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = len(rays)
    out = dict(dist=np.zeros(n, np.float32), id=np.zeros(n, np.uint32), steps=np.zeros(n, np.uint32), normal=np.zeros((n, 3), np.float32))
    for i, r in enumerate(rays):
        key = (id(sc), max_steps, r.tobytes())
        if key not in _memo:
            _memo[key] = (sc, trace(sc, r[:3], r[3:], max_steps))          # (the scene is kept: its id stays its own)
        d, hit, steps, nrm = _memo[key][1]
        out["dist"][i], out["id"][i], out["steps"][i], out["normal"][i] = d, hit, steps, nrm
    for a in out.values():
        a.setflags(write=False)
    return out


def same_bits(a, b):
    """elementwise: the same bit pattern, or both NaN"""
    a, b = np.ascontiguousarray(a, dtype=None), np.ascontiguousarray(b, dtype=None)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype == np.float32:
        return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return a == b


def differing(got, want, fields=("dist", "id", "steps", "normal")):
    """indices of the rays of which a field of `got` is not the reference's; (field, index) pairs"""
    bad = []
    for f in fields:
        ok = same_bits(got[f], want[f])
        if ok.ndim == 2:
            ok = ok.all(axis=1)
        bad += [(f, int(i)) for i in np.flatnonzero(~ok)]
    return bad


def camera_rays(sc, w, h, camera=None):
    """the primary rays of a w x h frame, row-major: the oracle's own probe.rd from the camera's position"""
    cam = camera if camera is not None else sc.camera
    ro = cam.point.tuple()
    rays = np.zeros((h * w, 6), np.float32)
    for y in range(h):
        for x in range(w):
            rays[y * w + x] = ro + tuple(O.probe(sc, w, h, x, y, 1, camera=cam).rd)
    return rays


SPECIALS = ("zero-direction", "nan-direction", "inf-origin", "origin-1e20", "origin-1e15", "origin-below-1e15", "minus-zero-origin",
            "denormal-direction")


def special_rays(ro, rd):
    """the eight special rays, made from an ordinary one"""
    ro, rd = np.asarray(ro, np.float32), np.asarray(rd, np.float32)
    below = np.nextafter(F(1e15), F(0))
    out = {
        "zero-direction": np.concatenate([ro, [0, 0, 0]]),
        "nan-direction": np.concatenate([ro, [rd[0], np.nan, rd[2]]]),
        "inf-origin": np.concatenate([[ro[0], np.inf, ro[2]], rd]),
        "origin-1e20": np.concatenate([[1e20, ro[1], ro[2]], rd]),
        "origin-1e15": np.concatenate([[ro[0], ro[1], 1e15], rd]),
        "origin-below-1e15": np.concatenate([[ro[0], ro[1], below], rd]),
        "minus-zero-origin": np.concatenate([[-0.0, -0.0, ro[2]], rd]),
        "denormal-direction": np.concatenate([ro, [1e-40, 0, 0]]),
    }
    return [out[k].astype(np.float32) for k in SPECIALS]


_sets = {}


def ray_set(sc, seed, kinds="abcde"):
    """The rays the GPU tests share, n x 6 float32, read-only:
      (a) the camera rays of a 13 x 5 frame;
      (b) from each of their hits, p + 0.01 n towards light 0 (towards (0, 10, 0) in a scene without one), with a unit direction:
          per-lane origins, a direction the fast SDF's carried bound accepts;
      (c) the directions of (b) times 0.5 and times 2: the second is refused by the carried bound's vote;
      (d) origins inside objects: the points 0.1 beyond those hits along their rays where the scene's distance is negative, in a
          seeded direction;
      (e) the SPECIALS, inserted at seeded positions INSIDE the waves of ordinary rays, not grouped at the end."""
    key = (id(sc), seed, kinds)
    if key in _sets:
        return _sets[key][1]
    rng = np.random.default_rng(seed)
    a = camera_rays(sc, 13, 5)
    ref = reference(sc, a)
    lights = sc.lights()
    light = np.array(lights[0].point.tuple() if lights else (0.0, 10.0, 0.0), np.float32)
    b, d = [], []
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(ref["id"] != 0):
            ro, rd, dist, n = a[i, :3], a[i, 3:], ref["dist"][i], ref["normal"][i]
            p = np.array(along(ro, rd, dist), np.float32)
            o = (p + F(0.01) * n).astype(np.float32)
            b.append(np.concatenate([o, v3normalize(light - o)]).astype(np.float32))
            q = np.array(along(ro, rd, F(dist + F(0.1))), np.float32)
            if sdf(sc, q)[0] < 0:
                d.append(np.concatenate([q, v3normalize(rng.normal(size=3).astype(np.float32))]).astype(np.float32))
    b = np.array(b, np.float32).reshape(-1, 6)
    c = np.concatenate([b * np.array([1, 1, 1, 0.5, 0.5, 0.5], np.float32), b * np.array([1, 1, 1, 2, 2, 2], np.float32)])
    parts = dict(a=a, b=b, c=c, d=np.array(d, np.float32).reshape(-1, 6))
    rays = np.concatenate([parts[k] for k in "abcd" if k in kinds]).astype(np.float32)
    if "e" in kinds:
        specials = special_rays(a[len(a) // 2, :3], a[len(a) // 2, 3:])
        # one position per special, each strictly inside a wave of 64 (never its first or last lane), no two in the same place
        at = sorted(int(w * 64 + rng.integers(1, 63)) for w in rng.choice(max(1, len(rays) // 64), size=len(specials), replace=True))
        for k, (pos, s) in enumerate(zip(at, specials)):
            rays = np.insert(rays, min(pos + k, len(rays) - 1), s, axis=0)
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    rays.setflags(write=False)
    _sets[key] = (sc, rays)
    return rays
