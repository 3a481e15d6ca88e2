"""A replay of the reference's shadow march (softshadow / in_shadow, naive_renderer.c:73-100) in binary32 numpy arithmetic, every
product, quotient and sum rounded on its own, the scene's distance taken from the oracle (lol_oracle_sdf).  Test infrastructure only.

What it is for: the kernels end a shadow march once fl(t + s) == t (lol_kernel.h, soft_shadow: "the stationary exit").  The oracle
runs those turns like the reference does, and cannot be changed; the replay says, for one ray, at which turn it stopped moving, what
(t, res) were at every turn, and how many turns a kernel therefore RUNS — beside the counts the oracle reports, which the replay
must reproduce first (replay_matches_oracle).
"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

import oracle_lib as O

F32 = np.float32
TURNS = 128                      # in_shadow's max_steps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stationary_shadow_rays.json")


def _sdf_many(sc, q, alive, out):
    fn, ptr, idp = O.lib().lol_oracle_sdf, sc.ptr, C.byref(C.c_uint32())
    pts = q.tolist()
    for j in np.flatnonzero(alive).tolist():
        x, y, z = pts[j]
        out[j] = fn(ptr, x, y, z, idp)


def shadow_rays(sc, w, h, pixels, max_steps=256):
    """The shadow rays of the given (x, y, light) triples of a w x h frame under the scene's own camera, as get_light / in_shadow
    build them: (ro [n, 3] = p + dir, dir [n, 3], max_dist [n]) in float32, p = ro + rd * hit_dist from the oracle's own probe."""
    lib = O.lib()
    cam = sc.c.camera
    ro_cam = np.array([cam.point.x, cam.point.y, cam.point.z], dtype=F32)
    ros, dirs, dists = [], [], []
    probes = {}
    f3 = C.c_float * 3
    for x, y, li in pixels:
        if (x, y) not in probes:
            pr = O.probe(sc, w, h, x, y, max_steps)
            rd = np.array(list(pr.rd), dtype=F32)
            probes[(x, y)] = ro_cam + rd * F32(pr.hit_dist)               # v3add(ro, v3scale(rd, hit.dist))
        p = probes[(x, y)]
        lp = sc.c.lights[li].point
        v = np.array([lp.x, lp.y, lp.z], dtype=F32) - p                   # v3sub(lp, p)
        out = f3()
        lib.lol_oracle_v3normalize(f3(*v.tolist()), out)
        d = np.array(list(out), dtype=F32)
        ros.append(p + d)
        dirs.append(d)
        dists.append(F32(lib.lol_oracle_v3len(f3(*v.tolist()))))
    return np.array(ros, dtype=F32).reshape(-1, 3), np.array(dirs, dtype=F32).reshape(-1, 3), np.array(dists, dtype=F32)


def replay(sc, ro, rd, max_dist, turns=TURNS):
    """softshadow(sc, ro, rd, 128, max_dist, 50) for n rays at once.  Returns a dict of
         t, res          [n, turns + 1] float32: the state BEFORE turn i (column i) — column `turns` is the state the reference ends in;
                         a ray the reference has left keeps its last state
         count           [n] the turns the reference runs (res < -1 or t > max_dist ends it)
         settled         [n] the turns up to and including the first that left res <= 0 (= count where none did): the oracle's
                         "settled" count, what a kernel runs under FLAG_SHADOW_SETTLED without the stationary exit
         still           [n] the first turn k (1-based) after which fl(t + s) == t, 0 where there is none while the reference runs
         factor          [n] maxf(res, 0) at the end"""
    ro, rd = np.ascontiguousarray(ro, dtype=F32), np.ascontiguousarray(rd, dtype=F32)
    max_dist = np.ascontiguousarray(max_dist, dtype=F32)
    n = len(ro)
    T, RES = np.zeros((n, turns + 1), dtype=F32), np.ones((n, turns + 1), dtype=F32)
    t, res = np.zeros(n, dtype=F32), np.ones(n, dtype=F32)
    alive = np.ones(n, dtype=bool)
    count, settled, still = np.full(n, turns), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    s = np.zeros(n, dtype=F32)
    with np.errstate(all="ignore"):
        for i in range(turns):
            q = ro + rd * t[:, None]                                      # v3add(ro, v3scale(rd, dist))
            _sdf_many(sc, q, alive, s)
            v = (F32(50.0) * s) / t                                       # w * scene_dist / dist
            res_n = np.where(res < v, res, v)                             # minf: the second operand on NaN or equal
            t_n = t + s
            assert q.dtype == v.dtype == res_n.dtype == t_n.dtype == F32
            still = np.where(alive & (still == 0) & (t_n == t), i + 1, still)
            settled = np.where(alive & (settled == 0) & (res_n <= 0), i + 1, settled)
            t, res = np.where(alive, t_n, t), np.where(alive, res_n, res)
            out = alive & ((res < F32(-1.0)) | (t > max_dist))
            count = np.where(out, i + 1, count)
            alive &= ~out
            T[:, i + 1], RES[:, i + 1] = t, res
    settled = np.where(settled == 0, count, settled)
    still = np.where((still > 0) & (still <= count), still, 0)
    return dict(t=T, res=RES, count=count, settled=settled, still=still, factor=np.where(res > 0, res, F32(0.0)))


def executed(rep, settled_exit=True):
    """The turns a kernel runs for each replayed ray: up to the reference's exit (or, under FLAG_SHADOW_SETTLED, the first turn that
    left res <= 0), or the turn after which the ray stands still — whichever comes first."""
    end = rep["settled"] if settled_exit else rep["count"]
    return np.where(rep["still"] > 0, np.minimum(end, rep["still"]), end)


def rays_run_to_the_end(osteps, n_lights):
    """(x, y, light) of every shadow ray of a frame that a kernel marches for all 128 turns under its default skips: the pixel is a
    hit, the light's diffuse incidence is not exactly 0, and the oracle's settled count of that light is 128.  osteps:
    oracle_lib.render_rows(..., want_steps=True)[2]."""
    out = []
    for li in range(min(n_lights, 4)):
        m = (osteps[..., 8 + li] == TURNS) & (osteps[..., 2] != 0) & (((osteps[..., 3] >> li) & 1) == 0)
        ys, xs = np.nonzero(m)
        out += [(int(x), int(y), li) for x, y in zip(xs, ys)]
    return sorted(out, key=lambda e: (e[1], e[0], e[2]))


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def record_golden(scenes, w=160, h=90, per_scene=64, path=GOLDEN):
    """tests/golden/stationary_shadow_rays.json: per scene `per_scene` rays the oracle runs to 128 turns, evenly spaced over the
    frame's list of them (nothing is chosen by what the rays do): pixel, light, and origin / direction / light distance as the bit
    patterns of their float32 values."""
    doc = dict(w=w, h=h, note="shadow rays (ro = p + dir, dir, max_dist as float32 bit patterns) that the oracle marches for all 128 turns; "
                              "written by tests/tools/stationary_shadow_model.py --record-rays", scenes={})
    for name, sc in scenes.items():
        _, _, osteps = O.render_rows(sc, w, h, 0, h, 256, want_steps=True)
        all_rays = rays_run_to_the_end(osteps, sc.c.n_lights)
        pick = [all_rays[i] for i in np.linspace(0, len(all_rays) - 1, per_scene).astype(int)]
        ro, rd, md = shadow_rays(sc, w, h, pick)
        doc["scenes"][name] = [dict(x=x, y=y, light=li, ro=bits(ro[i]).tolist(), dir=bits(rd[i]).tolist(), max_dist=int(bits(md[i:i + 1])[0]))
                               for i, (x, y, li) in enumerate(pick)]
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    return doc


def load_golden(path=GOLDEN):
    with open(path) as f:
        doc = json.load(f)
    out = {}
    for name, rays in doc["scenes"].items():
        u = lambda k: np.array([r[k] for r in rays], dtype=np.uint32)
        out[name] = dict(pixels=[(r["x"], r["y"], r["light"]) for r in rays], ro=u("ro").view(F32), dir=u("dir").view(F32),
                         max_dist=u("max_dist").view(F32))
    return doc["w"], doc["h"], out
