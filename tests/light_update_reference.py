"""The reference for light updates (lol_gpu_light_update_rays, lol_gpu_light_update_pixels).  Not a test file.

factor() is light_reference.factors() with the march replaced by a read: from a ray, the distance and the object id a capture wrote for
it (hit_dist, hit_id) and the look, the factor of ONE light — p = ro + rd * dist on those bits, get_normal's four taps at p
(naive_renderer.c:114-125), and the statements of get_light (:136-161) for that light on the look's tables.  Nothing marches from the
eye.  tests/test_light_update_reference.py holds it to light_reference.reference of the look's own scene, bit for bit: that the planes
of a capture hold enough to bring them to a look that moves lights or changes a shininess.
"""
import numpy as np

import ray_reference as R
import shade_reference as SR

F = np.float32


def normal_at(sc, p, dist):
    """get_normal(scene, p, dist), :114-125, as ray_reference.trace writes it"""
    h = F(F(dist) / F(100.0))                                    # :119
    terms = []
    for k in R.K:                                                # :120-123
        s, _ = R.sdf(sc, tuple(F(p[j] + F(k[j] * h)) for j in range(3)))
        terms.append(tuple(F(k[j] * s) for j in range(3)))
    acc = terms[3]
    for t in (terms[2], terms[1], terms[0]):                     # :124
        acc = tuple(F(t[j] + acc[j]) for j in range(3))
    return R.v3normalize(acc)


def factor(look, ro, rd, hit_dist, hit_id, light):
    """(shadow, di, si, shadow_steps) of light number `light` of the scene `look` for the ray (ro, rd) whose capture wrote hit_dist
    and hit_id; an id beyond the look's objects is taken for 0"""
    ro, rd = tuple(F(v) for v in ro), tuple(F(v) for v in rd)
    dist, hit = F(hit_dist), int(hit_id)
    if hit > len(look.roots()):
        hit = 0
    with np.errstate(all="ignore"):
        p = R.along(ro, rd, dist)                                # :227
        n = normal_at(look, p, dist)
        shininess = F(SR.get_material(look, hit).shininess)      # :130
        lp = SR.t3(look.lights()[light].point)
        shadow, ss = SR.in_shadow(look, lp, p)                   # :136
        light_dir = R.v3normalize(SR.sub(lp, p))                 # :142
        refl = SR.sub(SR.scale(n, F(F(2.0) * SR.v3dot(light_dir, n))), light_dir)      # :143-144
        camera_dir = R.v3normalize(SR.sub(ro, p))                # :145 — the eye is the ray's origin
        di = SR.clamp(SR.v3dot(n, light_dir), 0.0, 1.0)          # :148
        si = F(di * SR.powf(SR.clamp(SR.v3dot(refl, camera_dir), 0.0, 1.0), shininess))       # :158-161
    return shadow, di, si, ss


_memo = {}


def reference(look, rays, hit_dist, hit_id, lights=None):
    """factor() of every ray of `rays` (n x 6 float32) and every light of `lights` (default: all), from the planes hit_dist / hit_id
    of a capture, in the layout of light_reference.reference: dict(shadow, di, si [n, lights of the scene] f32, shadow_steps u32);
    columns of lights that were not asked for stay 0.  Each (ray, dist, id, light) is computed once per look; read-only arrays."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n, nl = len(rays), len(look.lights())
    lights = range(nl) if lights is None else lights
    out = dict(shadow=np.zeros((n, nl), np.float32), di=np.zeros((n, nl), np.float32), si=np.zeros((n, nl), np.float32),
               shadow_steps=np.zeros((n, nl), np.uint32))
    dist = np.ascontiguousarray(hit_dist, dtype=np.float32)
    for i, r in enumerate(rays):
        for l in lights:
            key = (id(look), r.tobytes(), dist[i].tobytes(), int(hit_id[i]), l)
            if key not in _memo:
                _memo[key] = (look, factor(look, r[:3], r[3:], dist[i], hit_id[i], l))       # (the scene is kept: its id stays its own)
            out["shadow"][i, l], out["di"][i, l], out["si"][i, l], out["shadow_steps"][i, l] = _memo[key][1]
    for a in out.values():
        a.setflags(write=False)
    return out
