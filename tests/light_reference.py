"""The reference for light passes and relighting (lol_gpu_light_rays, lol_gpu_relight).  Not a test file.

factors() is shade_reference.shade() — naive_renderer.c:225-232 for one ray, statement by statement in binary32 scalars — up to the
three scalars get_light needs per light, which shade() computes on its way and does not return: the shadow factor (:136), the diffuse
incidence (:148) and the specular incidence (:158-161), with the iterations of the shadow loop (:80).  relit() is the rest of get_light
(:150-174) on those scalars under ANOTHER scene's lights, materials and ambient colour.  Both are written with shade_reference's helpers
and the oracle's exported primitives: nothing new is needed under oracle/.  tests/test_light_reference.py holds factors() to
lol_oracle_probe_pixel and relit() to shade(), bit for bit.

Gamma and pack come from shade_reference.
"""
import numpy as np

import ray_reference as R
import shade_reference as SR

F = np.float32


def factors(sc, ro, rd, max_steps):
    """dict(dist, id, steps (march), lights = [(shadow, di, si, shadow_steps) per light, in file order]) of one ray"""
    ro, rd = tuple(F(v) for v in ro), tuple(F(v) for v in rd)
    dist, hit, steps, n = R.trace(sc, ro, rd, max_steps)
    with np.errstate(all="ignore"):
        p = R.along(ro, rd, dist)                                # :227
        shininess = F(SR.get_material(sc, hit).shininess)        # :130
        out = []
        for light in sc.lights():                                # :135
            lp = SR.t3(light.point)
            shadow, ss = SR.in_shadow(sc, lp, p)                 # :136
            light_dir = R.v3normalize(SR.sub(lp, p))             # :142
            refl = SR.sub(SR.scale(n, F(F(2.0) * SR.v3dot(light_dir, n))), light_dir)      # :143-144
            camera_dir = R.v3normalize(SR.sub(ro, p))            # :145 — the eye is the ray's origin
            di = SR.clamp(SR.v3dot(n, light_dir), 0.0, 1.0)      # :148
            si = F(di * SR.powf(SR.clamp(SR.v3dot(refl, camera_dir), 0.0, 1.0), shininess))       # :158-161
            out.append((shadow, di, si, ss))
    return dict(dist=dist, id=hit, steps=steps, lights=out)


def relit(lights, obj_id, look):
    """rgb_linear of get_light (:131-174) from the captured scalars of one ray (factors()["lights"]) and its object id, under the
    lights' intensities, the materials' colours and the ambient colour of the scene `look`"""
    mat = SR.get_material(look, int(obj_id))
    m_diff, m_spec, m_amb = SR.t3(mat.diffuse), SR.t3(mat.specular), SR.t3(mat.ambient)
    with np.errstate(all="ignore"):
        total = (F(0.0), F(0.0), F(0.0))                         # :131
        for light, (shadow, di, si, _steps) in zip(look.lights(), lights):
            shadow, di, si = F(shadow), F(di), F(si)
            total = SR.add(total, SR.mul(SR.scale(SR.t3(light.diffuse_intensity), F(shadow * di)), m_diff))       # :150-155
            total = SR.add(total, SR.mul(SR.scale(SR.t3(light.specular_intensity), F(shadow * si)), m_spec))      # :163-168
        total = SR.add(total, SR.mul(SR.t3(look.c.ambient_color), m_amb))                                          # :171-172
        return SR.v3clamp(total, 0.0, 1.0)                       # :174


_memo = {}


def reference(sc, rays, max_steps=256):
    """factors() of every ray of `rays` (n x 6 float32) in the layout of the capture's planes: dict(shadow, di, si [n, lights] f32,
    shadow_steps [n, lights] u32, dist [n] f32, id [n] u32, steps [n] u32: the march's).  Each ray is computed once per
    (scene, max_steps) whatever list it comes in; the arrays are read-only."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n, nl = len(rays), len(sc.lights())
    out = dict(shadow=np.zeros((n, nl), np.float32), di=np.zeros((n, nl), np.float32), si=np.zeros((n, nl), np.float32),
               shadow_steps=np.zeros((n, nl), np.uint32), dist=np.zeros(n, np.float32), id=np.zeros(n, np.uint32), steps=np.zeros(n, np.uint32))
    for i, r in enumerate(rays):
        key = (id(sc), max_steps, r.tobytes())
        if key not in _memo:
            _memo[key] = (sc, factors(sc, r[:3], r[3:], max_steps))          # (the scene is kept: its id stays its own)
        f = _memo[key][1]
        out["dist"][i], out["id"][i], out["steps"][i] = f["dist"], f["id"], f["steps"] & 0xFFFF
        for l, (shadow, di, si, ss) in enumerate(f["lights"]):
            out["shadow"][i, l], out["di"][i, l], out["si"][i, l], out["shadow_steps"][i, l] = shadow, di, si, ss
    for a in out.values():
        a.setflags(write=False)
    return out


def relit_reference(ref, look, fmt=None):
    """relit() of every ray of reference()'s planes under `look`: dict(rgb_linear, rgb [n, 3] f32, pixel [n] u32) as a shading query
    lays them out"""
    n = len(ref["id"])
    lin = np.zeros((n, 3), np.float32)
    for i in range(n):
        lights = list(zip(ref["shadow"][i], ref["di"][i], ref["si"][i], ref["shadow_steps"][i]))
        lin[i] = relit(lights, ref["id"][i], look)
    rgb = SR.gamma(lin)
    return dict(rgb_linear=lin, rgb=rgb, pixel=SR.pack(rgb, fmt))
