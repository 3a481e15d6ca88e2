"""The reference for shading queries (lol_gpu_shade_rays), restated for ARBITRARY rays.  Not a test file.

shade() is naive_renderer.c:225-232 for one ray (ro, rd): ray_reference.trace() (get_intersection, get_normal) followed by get_light
(:129-175) with in_shadow / softshadow (:73-100) and get_material (:103-112), statement by statement in numpy binary32 scalars: every
+, * and / is one correctly rounded binary32 operation, as in the reference, which has no FMA; the shadow quotient is (w * s) / dist.
The eye get_light reads from the scene (:132) is the ray's own origin.  The scene's distances come from the oracle's own sdf()
(lol_oracle_sdf), and v3len, v3dot, v3normalize, clamp, minf, maxf, v3clamp and powf are the oracle's exports too, so nothing new is
needed under oracle/.  tests/test_shade_reference.py holds it to lol_oracle_probe_pixel, field by field, on the oracle's own rays.

Gamma goes through oracle_lib.powf (the host libm's powf, as the reference's v3pow) and pack() is colorf_to_pixfmt (renderer.h:17-22)
for a given pixel format.

shade_ray_set() builds the list of rays the GPU tests share.
"""
import ctypes as C

import numpy as np

import oracle_lib as O
import ray_reference as R

F = np.float32
FIELDS = ("rgb_linear", "rgb", "pixel", "dist", "id", "steps")


def _f3(v):
    return (C.c_float * 3)(float(v[0]), float(v[1]), float(v[2]))


def v3len(v):
    return F(O.lib().lol_oracle_v3len(_f3(v)))


def v3dot(a, b):
    return F(O.lib().lol_oracle_v3dot(_f3(a), _f3(b)))


def clamp(v, lo, hi):
    return F(O.lib().lol_oracle_clamp(float(v), float(lo), float(hi)))


def minf(a, b):
    return F(O.lib().lol_oracle_minf(float(a), float(b)))


def maxf(a, b):
    return F(O.lib().lol_oracle_maxf(float(a), float(b)))


def v3clamp(v, lo, hi):
    out = (C.c_float * 3)()
    O.lib().lol_oracle_v3clamp(_f3(v), float(lo), float(hi), out)
    return (F(out[0]), F(out[1]), F(out[2]))


def powf(x, y):
    return F(O.powf(np.array([x], np.float32), np.array([y], np.float32))[0])


def sub(a, b):
    return tuple(F(a[k] - b[k]) for k in range(3))


def add(a, b):
    return tuple(F(a[k] + b[k]) for k in range(3))


def mul(a, b):
    return tuple(F(a[k] * b[k]) for k in range(3))


def scale(a, f):
    return tuple(F(a[k] * f) for k in range(3))


def t3(v):
    return tuple(F(c) for c in v.tuple())


def softshadow(sc, ro, rd, max_steps, max_dist, w):
    """naive_renderer.c:73-90: (factor, iterations of the loop that ran)"""
    res, dist, steps = F(1.0), F(0.0), 0
    for _ in range(max_steps):                                   # :80
        s, _id = R.sdf(sc, R.along(ro, rd, dist))                # :81-82
        res = minf(res, F(F(w * s) / dist))                      # :83 — (w * scene_dist) / dist
        dist = F(dist + s)                                       # :84
        steps += 1
        if res < F(-1) or dist > max_dist:                       # :85
            break
    return maxf(res, F(0.0)), steps                              # :88


def in_shadow(sc, light_point, p):
    """naive_renderer.c:93-100"""
    to_light = sub(light_point, p)
    light_dist = v3len(to_light)
    d = R.v3normalize(to_light)
    return softshadow(sc, add(p, d), d, 128, light_dist, F(50.0))


def get_material(sc, obj_id):
    """naive_renderer.c:103-112: the material of the object's root node, #0 for an escaped ray"""
    mid = sc.nodes()[sc.roots()[obj_id - 1]].material if obj_id else 0
    return sc.materials()[mid]


def shade(sc, ro, rd, max_steps):
    """dict(dist, id, steps (march), shadow [per light], shadow_steps [per light], rgb_linear) of one ray: binary32 scalars and ints"""
    ro, rd = tuple(F(v) for v in ro), tuple(F(v) for v in rd)
    dist, hit, steps, n = R.trace(sc, ro, rd, max_steps)
    with np.errstate(all="ignore"):
        p = R.along(ro, rd, dist)                                # :227
        mat = get_material(sc, hit)                              # :130
        m_diff, m_spec, m_amb, shininess = t3(mat.diffuse), t3(mat.specular), t3(mat.ambient), F(mat.shininess)
        total = (F(0.0), F(0.0), F(0.0))                         # :131
        shadows, shadow_steps = [], []
        for light in sc.lights():                                # :135
            lp = t3(light.point)
            shadow, ss = in_shadow(sc, lp, p)                    # :136
            shadows.append(shadow)
            shadow_steps.append(ss)
            light_dir = R.v3normalize(sub(lp, p))                # :142
            refl = sub(scale(n, F(F(2.0) * v3dot(light_dir, n))), light_dir)       # :143-144
            camera_dir = R.v3normalize(sub(ro, p))               # :145 — the eye is the ray's origin
            di = clamp(v3dot(n, light_dir), 0.0, 1.0)            # :148
            total = add(total, mul(scale(t3(light.diffuse_intensity), F(shadow * di)), m_diff))       # :150-155
            si = F(di * powf(clamp(v3dot(refl, camera_dir), 0.0, 1.0), shininess))                    # :158-161
            total = add(total, mul(scale(t3(light.specular_intensity), F(shadow * si)), m_spec))      # :163-168
        total = add(total, mul(t3(sc.c.ambient_color), m_amb))   # :171-172
        rgb_linear = v3clamp(total, 0.0, 1.0)                    # :174
    return dict(dist=dist, id=hit, steps=steps, shadow=shadows, shadow_steps=shadow_steps, rgb_linear=rgb_linear)


def gamma(rgb_linear):
    """v3pow(colorf, 1.f / 2.2f), naive_renderer.c:231, on [n, 3] float32"""
    a = np.ascontiguousarray(rgb_linear, dtype=np.float32)
    return O.powf(a.ravel(), np.full(a.size, F(1.0) / F(2.2), np.float32)).reshape(a.shape)


def pack(rgb, fmt=None):
    """colorf_to_pixfmt (renderer.h:17-22) of [n, 3] float32 colours after gamma: Uint8 c = colorf * 255, then SDL_MapRGB for a format
    given as shifts, losses and an alpha mask (loltracer_amd.gpu.PixelFormat; None = XRGB8888)"""
    c8 = (np.ascontiguousarray(rgb, dtype=np.float32) * F(255.0)).astype(np.int32).astype(np.uint32) & 0xFF
    shift = (16, 8, 0) if fmt is None else (fmt.r_shift, fmt.g_shift, fmt.b_shift)
    loss = (0, 0, 0) if fmt is None else (fmt.r_loss, fmt.g_loss, fmt.b_loss)
    px = np.full(len(c8), 0 if fmt is None else fmt.a_mask, np.uint32)
    for k in range(3):
        px |= ((c8[:, k] >> np.uint32(loss[k])) << np.uint32(shift[k])).astype(np.uint32)
    return px


_memo = {}


def reference(sc, rays, max_steps=256, fmt=None):
    """shade() of every ray of `rays` (n x 6 float32), in the layout of the query's outputs: dict(rgb_linear [n, 3] f32, rgb [n, 3] f32,
    pixel [n] u32, dist [n] f32, id [n] u32, steps [n] u32: march steps | shadow steps summed over the lights << 16), and
    `shadow` [n, lights] f32.  Each ray is computed once per (scene, max_steps) whatever list it comes in."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n, nl = len(rays), len(sc.lights())
    out = dict(rgb_linear=np.zeros((n, 3), np.float32), dist=np.zeros(n, np.float32), id=np.zeros(n, np.uint32), steps=np.zeros(n, np.uint32),
               shadow=np.zeros((n, nl), np.float32))
    for i, r in enumerate(rays):
        key = (id(sc), max_steps, r.tobytes())
        if key not in _memo:
            _memo[key] = (sc, shade(sc, r[:3], r[3:], max_steps))          # (the scene is kept: its id stays its own)
        s = _memo[key][1]
        out["rgb_linear"][i], out["dist"][i], out["id"][i] = s["rgb_linear"], s["dist"], s["id"]
        out["steps"][i] = (s["steps"] & 0xFFFF) | (sum(s["shadow_steps"]) << 16)
        out["shadow"][i] = s["shadow"]
    out["rgb"] = gamma(out["rgb_linear"])
    out["pixel"] = pack(out["rgb"], fmt)
    for a in out.values():
        a.setflags(write=False)
    return out


def differing(got, want, fields=FIELDS, march_steps_only=False):
    """(field, index) pairs of the rays of which a field of `got` is not the reference's.  march_steps_only: the low 16 bits of
    `steps` alone (with the exact skips on, the shadow steps really marched are fewer than the reference's)"""
    bad = []
    for f in fields:
        g, w = got[f], want[f]
        if f == "steps" and march_steps_only:
            g, w = g & 0xFFFF, w & 0xFFFF
        ok = R.same_bits(g, w)
        if ok.ndim == 2:
            ok = ok.all(axis=1)
        bad += [(f, int(i)) for i in np.flatnonzero(~ok)]
    return bad


_sets = {}


def shade_ray_set(sc, seed):
    """ray_reference.ray_set(sc, seed) — kinds (a) - (e), the SPECIALS inside waves — filled up to a whole number of waves of 64 with
    its own first rays, plus
      (f) 64 escaped camera rays, a wave of their own, followed by 64 rays that alternate escaped and hit: a wave that mixes both.
    n x 6 float32, read-only."""
    key = (id(sc), seed)
    if key in _sets:
        return _sets[key][1]
    base = R.ray_set(sc, seed)
    a = R.camera_rays(sc, 13, 5)
    ids = reference(sc, a)["id"]
    escaped, hit = a[ids == 0], a[ids != 0]
    assert len(escaped) and len(hit), "the 13 x 5 frame has no escaped ray or no hit to build (f) from"
    fill = (-len(base)) % 64
    mixed = np.empty((64, 6), np.float32)
    mixed[0::2] = np.resize(escaped, (32, 6))
    mixed[1::2] = np.resize(hit, (32, 6))
    rays = np.ascontiguousarray(np.concatenate([base, base[:fill], np.resize(escaped, (64, 6)), mixed]), dtype=np.float32)
    rays.setflags(write=False)
    _sets[key] = (sc, rays)
    return rays


def waves(ids):
    """per wave of 64 rays of a list: (every ray escaped, some did and some did not)"""
    out = []
    for at in range(0, len(ids), 64):
        w = ids[at:at + 64]
        out.append((bool((w == 0).all()), bool((w == 0).any() and (w != 0).any())))
    return out
