"""The culling bound kept past the march (lol_codegen.hip, keep_constants; lol_kernel.h, bound_keep / taps_begin / taps_done).  When the
march's loop ends, the fast SDF's register lb bounds the object along the march's ray from some T <= rt (rt: the t of the lane's last
evaluation).  The struct's head then keeps, per lane,
    kb = fl(K1 - Ek),  K1 = fma(|K|, -2^-20, K),  K = fma(ts, -ctc, lb),  ts = fl(rt + |fl(dist - rt)|)
(dist = rt + the last step, which may be NEGATIVE), and the one carried check of the bodies, fl(fma(rt, ctc, |best|)) < lb, is armed
for the four normal taps q_j = fl(p_j +- h), p = p(dist):  lb = fma(|h|, -c_tap, kb), rt = 0.
Wherever that check passes, the plain SDF's value of the object at q must be > |best|.
(A second hook that started the shadow marches from fl(kb - (1 + 2^-20)) was built, held to the same three checks and measured; it
did not separate from the taps alone and went out again with its constant and its cases — LABNOTES 8.)

Four things are held here, none of them with the code under test as the checker:
  * the constants the generator writes for scene4 lie on the safe side of what follows from the scene's TREE and the cluster spheres'
    own constants, re-derived in exact rational arithmetic;
  * the implication, in rational arithmetic with every rounding of the hooks' expressions and of the points themselves, at the WORST
    admissible best (the largest the check lets through), for a bound that came from the object's value (premises: D 1-Lipschitz,
    |plain value - D| <= et (D + 2 Rm)) and for one that came from the cluster spheres (conclusion: make_test's premise for every
    sphere), last steps that are negative, zero and far included, near the object and 10^6 away from it;
  * a replay against the ORACLE's SDF: rays of scene4 (and of a chain of smooth unions with a round box, the carry forced on) are
    marched with the oracle, kb is formed from the oracle's object values with the generated constants, and wherever the tap check
    fires, the oracle's object value at that point must be > best — and above the worst best the check would let through there.  At
    least 1000 firing tap points per scene, or the test fails: a condition, not a measurement;
  * generation: the hooks are there for scene4, gone — with the switch recorded — under LOL_GPU_CULL_KEEP=0 (and 2: bit 1 is the only
    one), absent from scene3 and from the exact SDF, and the bodies are the text they were."""
import os
import re
import tempfile
from fractions import Fraction as F

import numpy as np
import pytest

import test_cull_carry_bound as CB
import test_cull_value_carry_bound as VB
from loltracer_amd import gpu, scene as S
from test_cull_carry_bound import bits, f32, rnd
from test_cull_value_carry_bound import E, H, RHO

ROOT = VB.ROOT
MIN_POINTS = 1000
EPSILON = np.float32(0.001)


# ------------------------------------------------------------------ what the generator writes

def source_of(sc):
    with tempfile.TemporaryDirectory() as d:
        gpu.compile_offline(sc.flatten(), os.path.join(d, "s"), assume_fast=True)
        return open(os.path.join(d, "s.hip")).read()


def fast_of(src):
    fast = src[src.index("struct SpecSdfFast"):]
    return fast[:fast.index("\n};")]


def head_of(fast):
    """the part SdfEmitter::head_inlined writes: up to the first body"""
    return fast[:min(fast.index(n) for n in ("void eval(", "void eval_rec(") if n in fast)]


def hooks(fast):
    """the constants of the hooks (None where the hook is absent)"""
    head = head_of(fast)
    out = dict(keep=None, c_tap=None)
    m = re.search(r"float bound_keep\(float dist\) const \{\n\s*const float ts = rt \+ __builtin_fabsf\(dist - rt\);\n"
                  r"\s*const float kg = __builtin_fmaf\(ts, -" + H + r", lb\);\n"
                  r"\s*return __builtin_fmaf\(__builtin_fabsf\(kg\), -0x1p-20f, kg\) - " + H + r";\n\s*\}", head)
    if m:
        out["keep"] = dict(ctc=bits(int(m.group(1), 16)), ek=bits(int(m.group(2), 16)))
    m = re.search(r"void taps_begin\(float h, float kb\) \{ lb = __builtin_fmaf\(__builtin_fabsf\(h\), -" + H + r", kb\); rt = 0\.f; carry = false; \}\n"
                  r"\s*__device__ __forceinline__ void taps_done\(\) \{ lb = -__builtin_inff\(\); \}", head)
    if m:
        out["c_tap"] = bits(int(m.group(1), 16))
    return out


def spheres_of(fast):
    """the cluster spheres of the carried test as the body writes them (test_cull_carry_bound.carry_source, for any scene)"""
    body = fast[fast.index("void eval("):fast.index("void eval_dist(")]
    ab = {int(m.group(1)): (int(m.group(2), 16), int(m.group(3), 16))
          for m in re.finditer(r"__builtin_amdgcn_sqrtf\(cl(\d+)\), " + H + ", " + H + r"\)", body)}
    out = []
    for j in sorted(ab):
        c = re.search(r"cx%d = p\.x - %s, cy%d = p\.y - %s, cz%d = p\.z - %s" % (j, H, j, H, j, H), body)
        u = re.search(r"cu%d = \(best \+ %s\) \* %s" % (j, H, H), body)
        out.append(dict(c=[bits(int(c.group(i), 16)) for i in (1, 2, 3)], rm=bits(int(u.group(1), 16)), k=bits(int(u.group(2), 16)),
                        a=bits(ab[j][0]), b=bits(ab[j][1])))
    ctt = bits(int(re.search(r"__builtin_fmaf\(rt, " + H + r", lm\)", body).group(1), 16))
    return out, ctt


def everything(sc):
    """the scene's generated constants: the value bound's (k), the cluster spheres, the hooks', and the tree's premises"""
    src = source_of(sc)
    fast = fast_of(src)
    exact = src[src.index("struct SpecSdfExact"):src.index("struct SpecSdfFast")]
    _, _, k = VB.generated(sc)
    assert k is not None
    sph, ctt_c = spheres_of(fast)
    obj = VB.objects_of(sc.flatten())[k["id"] - 1]
    return dict(sc=sc, src=src, exact=exact, fast=fast, k=k, spheres=sph, ctt_c=ctt_c, hooks=hooks(fast), obj=obj, prem=VB.derive(obj))


@pytest.fixture(scope="module")
def s4():
    return everything(VB.scene4())


def consts_of(g):
    h = g["hooks"]
    return dict(g["k"], ek=h["keep"]["ek"], c_tap=h["c_tap"])


# ------------------------------------------------------------------ 1. the constants

def test_the_constants_lie_on_the_safe_side(s4):
    h, k, prem = s4["hooks"], s4["k"], s4["prem"]
    assert h["keep"] is not None and h["c_tap"] is not None
    assert h["keep"]["ctc"] == k["ctc"]                                  # ONE left-hand side: the check's own
    et = prem["et"]
    B = (prem["R"] + prem["cn"]) * (1 + 2 * et)
    gam = 1 - et
    for s in s4["spheres"]:
        B = max(B, s["rm"] + VB.norm_up(s["c"]))
        gam = max(gam, 1 / s["k"])
    assert gam <= 1
    ek, c_tap = h["keep"]["ek"], h["c_tap"]
    assert ek >= 3 * E * B + F(1, 2 ** 100)
    assert c_tap * c_tap >= 3
    # ctc ts >= ct t* under ts >= t* (1 - 2 e)
    assert k["ctc"] >= RHO * gam * (1 + F(1, 2 ** 21)) and k["ctc"] * (1 - 2 * E) >= RHO * gam
    # ... and not absurdly so: the bound is worth something
    assert ek <= 4 * 3 * E * B and c_tap * c_tap <= 3 * (1 + F(1, 2 ** 21))


# ------------------------------------------------------------------ 2. the implication, in rational arithmetic

def keep(c, lb, rt, dist):
    """the kernel's kb from lb, every rounding included (bound_keep)"""
    ts = rnd(rt + abs(rnd(dist - rt)))
    kg = rnd(lb - ts * c["ctc"])
    return rnd(rnd(kg - abs(kg) * F(1, 2 ** 20)) - c["ek"])


def tap_lb(c, kb, h):
    return rnd(kb - abs(h) * c["c_tap"])


def below(x):
    """the largest binary32 < x (x a positive binary32)"""
    return F(float(np.nextafter(np.float32(float(x)), np.float32(0))))


def tap_points(p, h):
    """normal_and_id's four taps, k3 down to k0"""
    out = []
    for px, py, pz in ((1, 1, 1), (-1, 1, -1), (-1, -1, 1), (1, -1, -1)):
        out.append([rnd(p[0] + px * h), rnd(p[1] + py * h), rnd(p[2] + pz * h)])
    return out


def dist_up(a, b):
    return VB.norm_up([x - y for x, y in zip(a, b)])


def least_plain_value_at(prem, V, sep):
    """the least value the plain SDF can have at a point within `sep` (real distance) of the point where it had the value V: D is
    1-Lipschitz and |plain - D| <= et (D + 2 Rm) at both points"""
    et, R = prem["et"], prem["R"]
    y = (V - 2 * et * R) / (1 + et)
    return (y - sep) * (1 - et) - 2 * et * R


def cluster_lb(spheres, ctt, pT, T):
    """the register after a full test passed at p(T) (test_cull_carry_bound.check)"""
    lm = None
    for s in spheres:
        cl = CB.len2([rnd(p - x) for p, x in zip(pT, s["c"])])
        h = rnd(CB.sqrt_hw(cl) * s["a"] + s["b"])
        lm = h if lm is None else min(lm, h)
    lg = rnd(T * ctt + lm)
    return rnd(abs(lg) * F(-1, 2 ** 20) + lg)


def holds_at(g, source, V, pT, q, worst):
    """the conclusion at q for the worst best, both signs: the value source through the premises, the cluster source exactly"""
    if source == "value":
        assert least_plain_value_at(g["prem"], V, dist_up(q, pT)) > worst, (source, V, pT, q, worst)
    else:
        for s in g["spheres"]:
            d2 = sum((a - b) ** 2 for a, b in zip(q, s["c"]))
            u = (worst + s["rm"]) * s["k"]
            assert u > 0 and d2 > u * u, (source, pT, q, worst)


CASES = ["random", "negative_last_step", "zero_last_step", "long_last_step", "far_away", "tiny_h", "first_turn"]


@pytest.mark.parametrize("source", ["value", "cluster"])
@pytest.mark.parametrize("case", CASES)
def test_the_kept_bound_implies_that_the_object_loses(s4, case, source):
    g, c = s4, consts_of(s4)
    Cc = [F(x) for x in g["obj"]["c"]]
    rng = np.random.default_rng(CASES.index(case) * 2 + (source == "value") + 20261021)
    lim = F(float(np.float32(1 + 2 ** -20)))
    taps = 0
    for i in range(120):
        # a ray that passes the object at some distance, marched from T to rt, then a last step d to dist
        aim = np.array([float(x) for x in Cc]) + rng.normal(size=3) * rng.uniform(0, 25)
        ro = aim - rng.normal(size=3) * rng.uniform(5, 40)
        if case == "far_away":
            ro = aim + rng.normal(size=3) * 1e6
        rd = CB.normalize(aim - ro)
        if not CB.len2(rd) <= lim:
            continue
        ro = [f32(x) for x in ro]
        T = f32(rng.uniform(0, 60)) if case != "first_turn" else F(0)
        if case == "far_away":
            T = f32(rng.uniform(0, 2e6))
        rt = rnd(T + f32(abs(rng.normal()) * 3 * (i % 3)))                # (every third: T == rt)
        if case == "first_turn":
            rt = F(0)
        d = f32(rng.uniform(-0.5, 0.001) if case == "negative_last_step" else 0.0 if case == "zero_last_step" else
                rng.uniform(5, 60) if case == "long_last_step" else rng.uniform(-0.01, 1.0))
        if case == "negative_last_step" and i % 4 == 0:
            d = -f32(abs(rng.normal()) * 5) - (rt - T)                     # dist behind T itself
        dist = rnd(rt + d)
        pT, p = CB.point(ro, rd, T), CB.point(ro, rd, dist)
        V = None
        if source == "value":
            # any value the object may have at p(T): at most |p(T) - C| + Rm in real arithmetic, and the rounding lemma above it
            top = (dist_up(pT, Cc) + g["prem"]["R"]) * (1 + g["prem"]["et"])
            V = f32(float(top) * rng.uniform(0.05, 1.0))
            lb = VB.kernel_lb(c, V, T)
        else:
            lb = cluster_lb(g["spheres"], g["ctt_c"], pT, T)
        kb = keep(c, lb, rt, dist)
        h = rnd(dist / 100)
        if case == "tiny_h":
            h = F(float(np.float32(10.0 ** rng.uniform(-44, -30))))
        lbt = tap_lb(c, kb, h)
        if lbt > 0:
            for q in tap_points(p, h):
                taps += 1
                holds_at(g, source, V, pT, q, below(lbt))
    assert taps >= 40, taps


def test_no_bound_in_is_no_bound_out(s4):
    """-inf stays -inf and NaN stays NaN through bound_keep and taps_begin, in binary32 (the fmas stand as a multiply and an add: only
    the classes matter here); a bound that is not positive passes no check"""
    c = {n: np.float32(float(v)) for n, v in consts_of(s4).items() if n in ("ctc", "ek", "c_tap")}
    with np.errstate(invalid="ignore", over="ignore"):
        for lb in (np.float32(-np.inf), np.float32(np.nan)):
            for rt, dist in ((np.float32(3), np.float32(2.5)), (np.float32(0), np.float32(np.inf)), (np.float32(7), np.float32(-1))):
                ts = rt + np.abs(dist - rt)
                kg = ts * -c["ctc"] + lb
                kb = (np.abs(kg) * np.float32(-2.0 ** -20) + kg) - c["ek"]
                for armed in (np.abs(np.float32(0.07)) * -c["c_tap"] + kb, np.abs(np.float32(-0.0)) * -c["c_tap"] + kb):
                    assert (np.isnan(armed) if np.isnan(lb) else armed == -np.inf) and not np.float32(0) < armed
        # a NaN dist (a NaN step) gives NaN whatever lb holds
        ts = np.float32(4) + np.abs(np.float32(np.nan) - np.float32(4))
        assert np.isnan((ts * -c["ctc"] + np.float32(9)))
    with open(os.path.join(ROOT, "loltracer_amd", "csrc", "lol_kernel.h")) as f:
        text = f.read()
    assert "bool ask; float kb = -__builtin_inff(); };" in text           # a Marched no march made carries no bound


# ------------------------------------------------------------------ 3. the replay against the oracle

def as_f(x):
    return F(float(x))


def march(full, ro, rd, n=256):
    """the oracle's march: the points it evaluates [(t, p)], and the dist it ends with (get_intersection: dist += d, then the test)"""
    ro, rd = np.asarray(ro, dtype=np.float32), np.asarray(rd, dtype=np.float32)
    dist, pts = np.float32(0), []
    for _ in range(n):
        p = (ro + (rd * dist).astype(np.float32)).astype(np.float32)
        d = full.sdf(p)
        pts.append((dist, p))
        dist = np.float32(dist + d)
        if not np.isfinite(d) or d < EPSILON or dist > np.float32(100):
            break
    return pts, dist


def replay_kept(g, obj_scene, rest_scene, full, rays):
    """-> (firing tap points, points that fired although the object's value is not above best — or not above the worst best the check
    lets through there)"""
    c = consts_of(g)
    taps = bad = 0
    for ro, rd in rays:
        if not VB.may_carry(rd):
            continue
        pts, dist = march(full, ro, rd)
        if not np.isfinite(dist):
            continue
        # the register at the end of the loop: at most the largest fold of the object's value over the points of the ray
        lb = None
        for t, p in pts:
            V = obj_scene.sdf(p)
            if np.isfinite(V):
                v = VB.kernel_lb(c, as_f(V), as_f(t))
                lb = v if lb is None or v > lb else lb
        if lb is None:
            continue
        kb = keep(c, lb, as_f(pts[-1][0]), as_f(dist))
        p = (np.asarray(ro, dtype=np.float32) + (np.asarray(rd, dtype=np.float32) * dist).astype(np.float32)).astype(np.float32)
        h = np.float32(dist / np.float32(100))
        lbt = tap_lb(c, kb, as_f(h))
        if lbt > 0:
            for sx, sy, sz in ((1, 1, 1), (-1, 1, -1), (-1, -1, 1), (1, -1, -1)):
                q = np.array([p[0] + np.float32(sx) * h, p[1] + np.float32(sy) * h, p[2] + np.float32(sz) * h], dtype=np.float32)
                best, V = rest_scene.sdf(q), obj_scene.sdf(q)
                if abs(as_f(best)) < lbt:
                    taps += 1
                    bad += not (V > best and as_f(V) >= lbt)               # (>= lbt: above every binary32 below it)
    return taps, bad


def floor_rays(sc, blob, lo, hi, n, box, seed):
    """camera rays to points of the floor y = -1 where the object's value lies in (lo, hi): next to the object and its shadow"""
    cam = np.array(sc.camera.point.tuple(), dtype=np.float32)
    rng = np.random.default_rng(seed)
    rays = []
    for _ in range(200 * n):
        if len(rays) >= n:
            break
        p = np.array([rng.uniform(box[0], box[1]), -1 + 0.001, rng.uniform(box[2], box[3])], dtype=np.float32)
        if lo < blob.sdf(p) < hi:
            rays.append((cam, VB.normalize32(p - cam)))
    return rays


def test_scene4_replayed_against_the_oracle(s4):
    sc = s4["sc"]
    full, blob, plane = VB.Sub(sc, [0, 1]), VB.Sub(sc, [0]), VB.Sub(sc, [1])
    rays = floor_rays(sc, blob, 0.05, 6.0, 1200, (-14, 16, -22, 4), 29)
    # ... and rays that end ON the blob (the taps there need the blob: the check must not fire) and rays that escape
    cam = np.array(sc.camera.point.tuple(), dtype=np.float32)
    rng = np.random.default_rng(30)
    for _ in range(40):
        rays.append((cam, VB.normalize32(np.array([rng.uniform(-4, 8), rng.uniform(0, 5), rng.uniform(-12, -3)], dtype=np.float32) - cam)))
    taps, bad = replay_kept(s4, blob, plane, full, rays)
    assert bad == 0 and taps >= MIN_POINTS, (taps, bad)


def chain_scene():
    from test_gpu_cull_value_carry import CAMERA, CHAIN, FLOOR, text
    return S.Scene.parse_string(text(CAMERA, CHAIN, FLOOR))


def test_the_chain_with_a_round_box_replayed_against_the_oracle(monkeypatch):
    """the chain of tests/test_gpu_cull_value_carry.py, the cluster carry forced on: the hooks are generated, their constants are on the
    safe side of THIS tree, and the oracle's rays reach the floor beside the object (the same floor of firing points)"""
    monkeypatch.setenv("LOL_GPU_TUNING", "1")
    monkeypatch.setenv("LOL_GPU_CULL_CARRY", "1")
    g = everything(chain_scene())
    test_the_constants_lie_on_the_safe_side(g)
    sc = g["sc"]
    root = g["k"]["id"] - 1
    n = sc.c.n_roots
    assert n == 2
    full, one, rest = VB.Sub(sc, list(range(n))), VB.Sub(sc, [root]), VB.Sub(sc, [i for i in range(n) if i != root])
    rays = floor_rays(sc, one, 0.05, 6.0, 1200, (-10, 14, -18, 2), 31)
    assert len(rays) == 1200
    taps, bad = replay_kept(g, one, rest, full, rays)
    assert bad == 0 and taps >= MIN_POINTS, (taps, bad)


# ------------------------------------------------------------------ 4. generation

def scene_named(name):
    return S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol"))


def bodies_of(fast):
    return fast[min(fast.index(n) for n in ("void eval(", "void eval_rec(") if n in fast):]


def test_generation_and_the_switch(s4, monkeypatch):
    names = ("bound_keep", "taps_begin", "taps_done")
    fast = s4["fast"]
    assert all(n + "(" in head_of(fast) for n in names)
    assert not any(n in s4["exact"] for n in names)
    assert not any(n in bodies_of(fast) for n in names)                  # the bodies know nothing of the hooks
    assert "lb = -__builtin_inff(); carry = false;" in fast               # loop_done() still forgets the ray
    s3 = source_of(scene_named("scene3"))
    assert not any(n in s3 for n in names)
    monkeypatch.setenv("LOL_GPU_TUNING", "1")
    got = {}
    for mask in (0, 1, 2, 3):
        monkeypatch.setenv("LOL_GPU_CULL_KEEP", str(mask))
        src = source_of(s4["sc"])
        assert "LOL_GPU_CULL_KEEP=%d" % mask in gpu.tuning_switches()
        f = fast_of(src)
        h = hooks(f)
        assert (h["keep"] is not None, h["c_tap"] is not None, "taps_done" in f) == (bool(mask & 1),) * 3
        got[mask] = (src, f)
    assert got[1][0] == s4["src"] == got[3][0]                            # the default is the taps
    assert not any(n in got[0][0] for n in names) and got[2][0] == got[0][0]
    # whatever the mask, the bodies are one text, and the source without the hooks is the source with them minus their lines
    assert len({bodies_of(f) for _, f in got.values()}) == 1
    lines = [l for l in got[3][0].split("\n")]
    start = next(i for i, l in enumerate(lines) if "float bound_keep(float dist) const {" in l)
    end = next(i for i, l in enumerate(lines) if "void taps_done()" in l)
    assert "\n".join(lines[:start] + lines[end + 1:]) == got[0][0]
    monkeypatch.setenv("LOL_GPU_CULL_KEEP", "3")
    monkeypatch.setenv("LOL_GPU_CULL_VALUE_CARRY", "0")                   # only beside the value carry
    assert not any(n in source_of(s4["sc"]) for n in names)
