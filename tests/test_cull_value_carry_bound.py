"""The object's own last value carried along a ray as a culling bound (lol_codegen.hip, value_carry_constants; the specialised kernel's
fast SDF, outermost run of one object).  After an evaluation of the object at p(T) with binary32 value V the kernel folds, per lane,
    lb = max(lb, fl(G - |G| 2^-20)),  G = fma(T, ctt, fl(fma(|V|, -dl, V) - Ef))
into the register of the cluster bound, and at every later point p(t), t >= T, of the same ray the object is skipped where
    fl(fma(t, ctc, |best|)) < lb.
That must imply that the plain SDF's value of the object at p(t) is > |best|: it then loses eval_dist's minimum and eval's strict '<'
with its tie rule alike.

Three things are held here, none of them with the code under test as the checker:
  * the constants the generator writes for scene4 lie on the safe side of what follows from the scene's TREE — its depth, centres,
    radii and smoothness — re-derived in exact rational arithmetic, the enclosing sphere (C, R) included (checked leaf by leaf);
  * the implication, in rational arithmetic with every rounding of the kernel's expressions, at the WORST admissible best (the
    largest the check lets through), V and T: from the premises  |plain value - D| <= et (|p - C| + R)  (make_test's rounding lemma),
    D >= |p - C| - R  and  D 1-Lipschitz  to  plain value at t > |best|;
  * the bound replayed against the oracle: rays of scene4 (floor points just outside the blob's shadow and their shadow rays to both
    lights, rays past the blob) and of the hostile scenes of tests/scene_shapes.py (constants derived here from their trees, as the
    generator derives them) are marched with the oracle's own SDF; for every pair T < t of points visited on one ray where the
    inequality fires — with the ORACLE's object value at T and the oracle's best at t — the oracle's object value at t must be
    > best.  At least 1000 pairs must fire per scene, or the test fails: it is a condition, not a measurement."""
import ctypes as C
import math
import os
import re
import tempfile
from fractions import Fraction as F

import numpy as np
import pytest

import oracle_lib as O
import scene_shapes as SH
from loltracer_amd import gpu, scene as S
from test_cull_carry_bound import bits, f32, next_up, rnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = F(1, 2 ** 24)
RHO = 1 + F(1, 2 ** 20)
ETA4 = F(4, 2 ** 150)                       # >= 2 sqrt(3) eta
H = r"__builtin_bit_cast\(float, (0x[0-9a-f]+)u\)"
MIN_PAIRS = 1000


# ------------------------------------------------------------------ the tree, and what follows from it

def f_up(x):
    """the smallest binary32 >= x (a positive Fraction)"""
    v = np.float32(float(x))
    while F(float(v)) < x:
        v = np.nextafter(v, np.float32(np.inf))
    return F(float(v))


def f_down(x):
    v = np.float32(float(x))
    while F(float(v)) > x:
        v = np.nextafter(v, np.float32(-np.inf))
    return F(float(v))


def enclose(a, b):
    """the sphere round two spheres (c, r), in doubles, with the slack lol_codegen.hip's own takes"""
    (ca, ra), (cb, rb) = a, b
    d = math.sqrt(sum((y - x) ** 2 for x, y in zip(ca, cb)))
    if d + rb <= ra:
        return a
    if d + ra <= rb:
        return b
    r = 0.5 * (d + ra + rb)
    t = (r - ra) / d if d > 0 else 0.0
    return [x + (y - x) * t for x, y in zip(ca, cb)], r * (1.0 + 1e-12)


def objects_of(prog):
    """per top-level object, in file order: None where the bound does not apply (a plane, a smoothness that is not positive and
    finite, a negative box field, absurd values), else dict(leaves=[(centre, radius + slack above it, magnitude)], levels, c, r):
    the radius is what the BOUND takes (0 for a sphere of negative radius), the magnitude m what the leaf's VALUE can add to
    |p - centre|: |radius| for a sphere, |b| + r for a round box"""
    out, st = [], []
    sane = lambda v: math.isfinite(v) and abs(v) < 1e15               # noqa: E731
    for i in range(prog.n_ops):
        o = prog.ops[i]
        f = [float(x) for x in o.f]
        if o.op == S.OP_SPHERE:
            ok = all(sane(v) for v in f[:4])
            st.append(dict(ok=ok, leaves=[[f[:3], max(f[3], 0.0), abs(f[3])]], levels=1, s=(f[:3], max(f[3], 0.0))))
        elif o.op == S.OP_RBOX:
            ok = all(sane(v) for v in f[:7]) and all(v >= 0 for v in f[3:7])
            r = math.sqrt(f[3] ** 2 + f[4] ** 2 + f[5] ** 2) * (1.0 + 1e-12) + f[6]
            st.append(dict(ok=ok, leaves=[[f[:3], r, r]], levels=1, s=(f[:3], r)))
        elif o.op == S.OP_PLANE:
            st.append(dict(ok=False, leaves=[], levels=1, s=([0.0, 0.0, 0.0], 0.0)))
        elif o.op in (S.OP_SMIN, S.OP_SMIN_R):
            b, a = st.pop(), st.pop()
            k = f[0]
            c, r = enclose(a["s"], b["s"])
            leaves = [[c_, r_ + 0.25 * k, m_] for c_, r_, m_ in a["leaves"] + b["leaves"]]
            st.append(dict(ok=a["ok"] and b["ok"] and sane(k) and k > 0, leaves=leaves, levels=max(a["levels"], b["levels"]) + 1,
                           s=(c, r + 0.25 * k)))
        elif o.op == S.OP_TOP:
            v = st.pop()
            out.append(dict(leaves=v["leaves"], levels=v["levels"], c=v["s"][0], r=v["s"][1]) if v["ok"] and sane(v["s"][1]) else None)
    return out


def sphere_encloses_every_leaf(obj):
    """|c_i - C| + r_i + slack_i <= R for every leaf, exactly"""
    Cc, R = [F(x) for x in obj["c"]], F(obj["r"])
    for c, r, _ in obj["leaves"]:
        m = R - F(r)
        if not (m >= 0 and sum((F(x) - y) ** 2 for x, y in zip(c, Cc)) <= m * m):
            return False
    return True


def norm_up(c):
    """a rational >= |c|"""
    c2 = sum(F(x) ** 2 for x in c)
    n = F(math.sqrt(float(c2))) * (1 + F(1, 2 ** 30)) + F(1, 2 ** 100)
    assert n * n >= c2
    return n


def derive(obj):
    """the four constants from the tree, each rounded to binary32 towards the safe side, and what the proof's premises need.
    R here is Rm: the bound's radius, or more where the magnitude of a leaf's value asks for it (a sphere of negative radius r has
    the value |p - c| + |r| but the bound radius 0): every intermediate value of the evaluation is within |p - C| + Rm."""
    et = 40 * E * obj["levels"]
    R, cn = F(obj["r"]), norm_up(obj["c"])
    for c, _, m in obj["leaves"]:
        R = max(R, norm_up([F(x) - F(y) for x, y in zip(c, obj["c"])]) + F(m))
    kap = (1 - et) / (1 + E)
    a = kap * (1 - E) / (1 + et)
    err = kap * (2 * et * R * (1 - E) / (1 + et) + 2 * E * (R + cn) + ETA4) + 2 * et * R
    return dict(dl=f_up(1 - a + 4 * E), ef=f_up(err * (1 + 4 * E) + F(1, 2 ** 100)), ctt=f_down(RHO * (1 - E) * kap * (1 - F(1, 2 ** 20))),
                ctc=f_up(RHO * (1 - et) * (1 + F(1, 2 ** 20))), et=et, R=R, cn=cn)


# ------------------------------------------------------------------ what the generator writes for scene4

def scene4():
    return S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", "scene4.lol"))


def generated(sc):
    """the fast SDF of the scene's own kernel and the constants of its value bound (None where it has none)"""
    with tempfile.TemporaryDirectory() as d:
        gpu.compile_offline(sc.flatten(), os.path.join(d, "s"), assume_fast=True)
        src = open(os.path.join(d, "s.hip")).read()
    exact = src[src.index("struct SpecSdfExact"):src.index("struct SpecSdfFast")]
    fast = src[src.index("struct SpecSdfFast"):]
    fast = fast[:fast.index("\n};")]
    found = []
    for body in (fast[fast.index("void eval("):fast.index("void eval_dist(")], fast[fast.index("void eval_dist("):]):
        m = re.search(r"const float vg = __builtin_fmaf\(rt, " + H + r", __builtin_fmaf\(__builtin_fabsf\(t(\d+)\), -" + H + r", t(\d+)\) - " + H + r"\);\n"
                      r"\s*lb = maxf_\(__builtin_fmaf\(__builtin_fabsf\(vg\), -0x1p-20f, vg\), lb\);", body)
        if m is None:
            return exact, fast, None
        assert m.group(2) == m.group(4)
        c = re.search(r"__builtin_fmaf\(rt, " + H + r", __builtin_fabsf\(best\)\) < lb", body)
        found.append(dict(ctt=bits(int(m.group(1), 16)), dl=bits(int(m.group(3), 16)), ef=bits(int(m.group(5), 16)), ctc=bits(int(c.group(1), 16)),
                          value="t" + m.group(2)))
    assert found[0] == found[1]
    body = fast[fast.index("void eval("):fast.index("void eval_dist(")]
    ident = int(re.search(r"if \(%s < best[^\n]*best_id = (\d+)u; \}" % found[0]["value"], body).group(1))
    return exact, fast, dict(found[0], id=ident)                          # id: the object's, 1-based in file order


@pytest.fixture(scope="module")
def s4():
    sc = scene4()
    objs = objects_of(sc.flatten())
    assert [o is not None for o in objs] == [True, False]               # the blob, then the plane
    exact, fast, got = generated(sc)
    return dict(sc=sc, obj=objs[0], exact=exact, fast=fast, got=got)


def test_scene4_folds_the_value_into_the_carried_bound(s4):
    fast, got = s4["fast"], s4["got"]
    assert got is not None and "vg" not in s4["exact"]
    for body in (fast[fast.index("void eval("):fast.index("void eval_dist(")], fast[fast.index("void eval_dist("):]):
        # the value the bound is made of is the object's own, the one that joins the minimum, on a ray that may carry
        assert re.search(r"(best = vmin_\(%s, best\);|if \(%s < best[^\n]*\n)\s*if \(carry\) \{\n\s*const float vg" % (got["value"], got["value"]), body)
        # the carried check comes before the cool-down counter, against ONE register, and nothing else reads lb
        assert re.search(r"\) < lb\)\) == 0\) need0 = false; else if \(cool\[0\] == 0u\) \{", body)
        assert body.count("< lb") == 1 and len(re.findall(r"\blb\b", body)) == 5
    assert "lb = -__builtin_inff(); carry = false;" in fast           # loop_done() forgets the ray


def test_the_constants_lie_on_the_safe_side_of_the_tree(s4):
    obj, got = s4["obj"], s4["got"]
    assert obj["levels"] == 4 and len(obj["leaves"]) == 5
    assert sphere_encloses_every_leaf(obj)
    want = derive(obj)
    assert got["dl"] >= want["dl"] and got["ef"] >= want["ef"] and 0 < got["ctt"] <= want["ctt"] and got["ctc"] >= want["ctc"]
    # ... and not absurdly so: the bound is worth something (Ef about 4 et R, dl about 2 et)
    assert got["ef"] <= 8 * want["et"] * want["R"] and got["dl"] <= 4 * want["et"]


# ------------------------------------------------------------------ the implication, in rational arithmetic

def kernel_lb(k, V, T):
    """the kernel's lb' from a value V at T, every rounding included"""
    w = rnd(V - abs(V) * k["dl"])
    u = rnd(w - k["ef"])
    g = rnd(T * k["ctt"] + u)
    return rnd(g - abs(g) * F(1, 2 ** 20))


def worst_best(k, t, lb):
    """the largest |best| (a binary32) that fl(fma(t, ctc, |best|)) < lb lets through, or None"""
    if not rnd(t * k["ctc"]) < lb:
        return None
    lo, hi = 0, 0x7f800000
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if rnd(t * k["ctc"] + bits(mid)) < lb:
            lo = mid
        else:
            hi = mid
    return bits(lo)


def least_plain_value(p, V, T, t):
    """the least value the plain SDF can have at p(t) when it had V at p(T), t >= T >= 0, from the premises (module docstring)"""
    et, R, cn = p["et"], p["R"], p["cn"]
    y = (V - 2 * et * R) / (1 + et)                                      # D(p(T)) >= this: V <= y + et (y + 2R)
    x = (y * (1 - E) - RHO * ((1 + E) * t - (1 - E) * T) - 2 * E * (R + cn) - ETA4) / (1 + E)
    return x * (1 - et) - 2 * et * R


CASES = ["random", "inside", "tiny", "step0", "ulp_step", "far", "huge"]


@pytest.mark.parametrize("case", CASES)
def test_the_value_bound_implies_that_the_object_loses(s4, case):
    k, prem = s4["got"], derive(s4["obj"])
    rng = np.random.default_rng(CASES.index(case) + 20261019)
    fired = 0
    for i in range(300):
        T = f32(rng.uniform(0, 100))
        V = f32(rng.uniform(0, 60))
        t = rnd(T + f32(abs(rng.normal()) * (0.5 if i % 2 else 5)))
        if case == "inside":
            V = f32(-rng.uniform(0, float(prem["R"])))
        elif case == "tiny":
            V = next_up(f_up(k["ef"] / (1 - k["dl"])), int(rng.integers(0, 1000)))      # G a few ulps of Ef above 0, or just below
            T = f32(rng.uniform(0, 1e-30)) if i % 3 == 0 else F(0)
            t = rnd(T + F(float(np.nextafter(np.float32(0), np.float32(1)))) * int(rng.integers(0, 1000)))
        elif case == "step0":
            t = T
        elif case == "ulp_step":
            t = next_up(T)
        elif case == "far":
            T = f32(rng.uniform(95, 100)); V = f32(rng.uniform(0, 120)); t = f32(rng.uniform(float(T), 100.0))
        elif case == "huge":
            T = f32(rng.uniform(0, 1e6)); V = f32(10 ** rng.uniform(0, 15)); t = rnd(T + f32(10 ** rng.uniform(-3, 6)))
        assert t >= T >= 0
        lb = kernel_lb(k, V, T)
        worst = worst_best(k, t, lb)
        if worst is None:
            continue
        fired += 1
        assert least_plain_value(prem, V, T, t) > worst, (case, V, T, t, worst)
    if case == "inside":
        assert fired == 0                    # (a negative V gives a negative lb, and the check's left-hand side is never negative)
    else:
        assert fired >= (1 if case == "tiny" else 50), fired


def test_a_value_that_is_no_number_leaves_the_bound(s4):
    """maxf_(x, lb) = x > lb ? x : lb keeps lb for a NaN x and for x = -inf; lb' is NaN for V = NaN and V = +inf (inf - inf) and -inf
    for V = -inf"""
    with open(os.path.join(ROOT, "loltracer_amd", "csrc", "lol_kernel.h")) as f:
        assert "float maxf_(float a, float b) { return a > b ? a : b; }" in f.read()
    dl, ef, ctt = (np.float32(float(s4["got"][n])) for n in ("dl", "ef", "ctt"))
    with np.errstate(invalid="ignore"):
        for V in (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)):
            g = np.float32(3) * ctt + ((V - np.abs(V) * dl) - ef)
            lbn = g - np.abs(g) * np.float32(2 ** -20)
            assert not (lbn > np.float32(-np.inf))


# ------------------------------------------------------------------ the bound replayed against the oracle

class Sub:
    """the scene with some of its top-level objects only, for the oracle's sdf()"""
    def __init__(self, sc, roots):
        self.s = S.SceneStruct()
        C.memmove(C.byref(self.s), C.byref(sc.c), C.sizeof(S.SceneStruct))
        self.arr = (C.c_int32 * max(len(roots), 1))(*[sc.c.roots[i] for i in roots])
        self.s.roots = C.cast(self.arr, C.POINTER(C.c_int32))
        self.s.n_roots = len(roots)
        self.keep = sc

    def sdf(self, p):
        i = C.c_uint32()
        return np.float32(O.lib().lol_oracle_sdf(C.byref(self.s), float(p[0]), float(p[1]), float(p[2]), C.byref(i)))


def normalize32(v):
    v = np.asarray(v, dtype=np.float32)
    l2 = np.float32(np.float32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return (v * (np.float32(1) / np.sqrt(l2))).astype(np.float32)


def may_carry(rd):
    l2 = np.float32(np.float32(rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2])
    return bool(l2 <= np.float32(1 + 2 ** -20))


def visit(full, ro, rd, n, t_max, shadow):
    """the points p(t) = fl(ro + fl(rd t)) a march (or shadow march) of the oracle's SDF visits, t never decreasing"""
    ro, rd = np.asarray(ro, dtype=np.float32), np.asarray(rd, dtype=np.float32)
    t, out = np.float32(0), []
    for _ in range(n):
        p = (ro + (rd * t).astype(np.float32)).astype(np.float32)
        d = full.sdf(p)
        out.append((t, p))
        if not np.isfinite(d) or d < (0 if shadow else np.float32(0.001)):
            break
        t = np.float32(t + d)
        if t > t_max:
            break
    return out


WORST_POINTS = 1500


def replay(k, obj_scene, rest_scene, full, rays):
    """-> (pairs that fired, pairs that fired although the object's value at t is not > best).  Beside the best the scene really has at
    t, the first WORST_POINTS points that some earlier point's bound reaches are also held to the WORST best that bound would let
    through there (the largest binary32 b with fl(fma(t, ctc, b)) < lb): the oracle's object value at t must be above that too —
    what the check promises whatever else the scene holds.  Those count as bad pairs, not as fired ones."""
    fired = bad = worst_left = 0
    worst_left = WORST_POINTS
    for ro, rd, n, t_max, shadow in rays:
        if not may_carry(rd):
            continue
        pts = visit(full, ro, rd, n, t_max, shadow)
        if len(pts) < 2:
            continue
        V = np.array([obj_scene.sdf(p) for _, p in pts], dtype=np.float32)
        best = np.array([rest_scene.sdf(p) for _, p in pts], dtype=np.float32)
        lb = np.full(len(pts), -np.inf, dtype=np.float32)
        lhs = np.full(len(pts), np.inf, dtype=np.float32)
        for i, (t, _) in enumerate(pts):
            if np.isfinite(V[i]):
                lb[i] = np.float32(float(kernel_lb(k, F(float(V[i])), F(float(t)))))
            if np.isfinite(best[i]):
                lhs[i] = np.float32(float(rnd(F(float(t)) * k["ctc"] + abs(F(float(best[i]))))))
        fires = np.triu(lhs[None, :] < lb[:, None], 1)                    # [i, j]: set at i (T), checked at j (t), i < j
        loses = (V > best)[None, :]
        fired += int(fires.sum())
        bad += int((fires & ~loses).sum())
        for j in range(1, len(pts)):
            if worst_left <= 0:
                break
            top = F(float(lb[:j].max()))
            tc = F(float(pts[j][0])) * k["ctc"]
            if not rnd(tc) < top:
                continue
            worst_left -= 1
            w = next_up(f32(float(top - tc)), 3)                           # near the largest b with fl(tc + b) < lb: step down to it
            while w > 0 and not rnd(tc + w) < top:
                w = F(float(np.nextafter(np.float32(float(w)), np.float32(0))))
            if rnd(tc + w) < top and not F(float(V[j])) > w:
                bad += 1
    return fired, bad


def shadow_rays(sc, p):
    out = []
    for l in sc.lights():
        to = (np.array(l.point.tuple(), dtype=np.float32) - p).astype(np.float32)
        dist = np.sqrt(np.float32(np.float32(to[0] * to[0] + to[1] * to[1]) + to[2] * to[2]))
        d = normalize32(to)
        out.append(((p + d).astype(np.float32), d, 128, dist, True))
    return out


def test_scene4_replayed_against_the_oracle(s4):
    sc, k = s4["sc"], s4["got"]
    full, blob, plane = Sub(sc, [0, 1]), Sub(sc, [0]), Sub(sc, [1])
    cam = np.array(sc.camera.point.tuple(), dtype=np.float32)
    rays = []
    # floor points just outside the blob's shadow: on the floor, one step of 0.25 ... 1.5 outside where the blob's value is 0.3 ... 2
    rng = np.random.default_rng(4)
    while len(rays) < 3 * 60:
        p = np.array([rng.uniform(-12, 14), -1 + 0.001, rng.uniform(-20, 3)], dtype=np.float32)
        if not 0.3 < blob.sdf(p) < 2.0:
            continue
        rays += shadow_rays(sc, p)                                         # its shadow rays to both lights ...
        rays.append((cam, normalize32(p - cam), 256, np.float32(100), False))      # ... and the ray that finds it
    fired, bad = replay(k, blob, plane, full, rays)
    assert bad == 0 and fired >= MIN_PAIRS, (fired, bad)


MIXED_MATS = "materials { { shininess = 2, diffuse = (0,0,0), specular = (0,0,0), ambient = (.1,.1,.1) }, { shininess = 9, diffuse = (.5,.4,.3), specular = (.3,.3,.3), ambient = (.1,.1,.1) } }\n"


def mixed_scale_text(radius):
    """two small spheres in a smooth union with a sphere of a large NEGATIVE radius, over a plane: the bound takes radius 0 for that
    sphere, its value is |p - c| + |radius|, and where it is the saturated operand of the union the sum b + (a - b) is rounded at
    ulp(|radius|) / 2 — far above what the tree's bound radius alone would allow for"""
    return (MIXED_MATS + "scene { camera { point = (0, 3, 6), direction = (0, -0.2, -1), fov = 90 },\n"
            "point_light { point = (3, 9, 0), diffuse_intensity = (2,2,2), specular_intensity = (1,1,1) },\n"
            "smooth_union { material = #1, smoothness = 1, a = smooth_union { smoothness = 1, a = sphere { point = (-5, 1, -8), radius = 1.5 },"
            " b = sphere { point = (5, 1, -8), radius = 1.5 } }, b = sphere { point = (0, 1, -8), radius = %s } },\n"
            "plane { material = #1, y = -1 } }\n" % radius)


MIXED = [SH.Hostile("mixed-scale-2e4", "a leaf of radius -20000 beside leaves of radius 1.5", mixed_scale_text("-20000")),
         SH.Hostile("mixed-scale-2e6", "a leaf of radius -2000000 beside leaves of radius 1.5", mixed_scale_text("-2000000"))]
# ... and a chain of smooth unions with a round box in it (the scene of tests/test_gpu_cull_value_carry.py): the generator's (C, R, levels)
# for a tree of unequal depth and a box's |b| + r
MIXED.append(SH.Hostile("chain-with-a-round-box", "a chain of three smooth unions over spheres and a round box", MIXED_MATS +
    "scene { camera { point = (-2, 6, 3), direction = (0.3, -0.7, -1), fov = 150 },\n"
    "point_light { point = (-2, 10, -1), diffuse_intensity = (4,4,4), specular_intensity = (4,4,4) },\n"
    "smooth_union { material = #1, smoothness = 1.5, a = smooth_union { smoothness = 1, a = smooth_union { smoothness = 2,"
    " a = sphere { point = (0, 1, -6), radius = 1 }, b = box { point = (5, 1, -10), point2 = (1.5, 0.5, 1), radius = 0.25 } },"
    " b = sphere { point = (-3, 2, -4), radius = 1.2 } }, b = sphere { point = (7, 2.5, -12), radius = 2 } },\n"
    "plane { material = #1, y = -1 } }\n"))
_parsed = {}


def scene_of(e):
    if e.name not in _parsed:
        _parsed[e.name] = S.Scene.parse_string(e.text)
    return _parsed[e.name]


def hostile_cases():
    """the hostile scenes in which the bound has something to say — an object it applies to (the one of the most leaves) beside at
    least one other object — and the scenes of MIXED above, for which the generator must emit the bound"""
    out = []
    for e in list(SH.HOSTILE) + MIXED:
        objs = objects_of(scene_of(e).flatten())
        cand = [i for i, o in enumerate(objs) if o is not None]
        if len(objs) >= 2 and cand:
            out.append((e, max(cand, key=lambda i: (len(objs[i]["leaves"]), -i))))
    return out


def replay_round(e, sc, obj, root, k):
    """rays that leave the object's sphere outwards and radially, towards whatever else the scene holds, and rays from the camera past
    it; more of the same until enough pairs have fired (at most 1000 rays)"""
    n = sc.c.n_roots
    full, one, rest = Sub(sc, list(range(n))), Sub(sc, [root]), Sub(sc, [i for i in range(n) if i != root])
    rng = np.random.default_rng(len(e.text) + root)
    Cc, R = np.array(obj["c"]), max(obj["r"], 1e-3)
    cam = np.array(sc.camera.point.tuple(), dtype=np.float32)
    fired = bad = 0
    for _ in range(25):
        rays = []
        for i in range(10):                                                # straight at a leaf's centre: the value falls as fast as it can
            c, r, _ = obj["leaves"][i % len(obj["leaves"])]
            u = rng.normal(size=3); u /= np.linalg.norm(u)
            ro = (np.array(c) + u * (r + rng.uniform(1, 8))).astype(np.float32)
            rays.append((ro, normalize32(-u), 256, np.float32(100 + 20 * R), False))
        for i in range(30):
            u = rng.normal(size=3); u /= np.linalg.norm(u)
            v = rng.normal(size=3); v /= np.linalg.norm(v)
            ro = (Cc + u * R * rng.uniform(0.2, 1.5)).astype(np.float32)
            rays.append((ro, normalize32(u + (0.7 if i % 3 else 0.0) * v), 256, np.float32(100 + 20 * R), False))
        for _ in range(10):
            u = rng.normal(size=3); u /= np.linalg.norm(u)
            rays.append((cam, normalize32(Cc + u * R * 1.2 - cam), 256, np.float32(100 + 20 * R), False))
        f, b = replay(k, one, rest, full, rays)
        fired, bad = fired + f, bad + b
        if fired >= MIN_PAIRS or bad:
            break
    return fired, bad


@pytest.mark.parametrize("e,root", hostile_cases(), ids=lambda v: v.name if hasattr(v, "name") else str(v))
def test_hostile_scenes_replayed_against_the_oracle(e, root, monkeypatch):
    """with the constants derived here from the tree, for the object of the most leaves; and, wherever the generator emits the bound
    with the carry forced on, with the constants IT writes, for the object it writes them for — which must also lie on the safe side
    of the tree's"""
    sc = scene_of(e)
    objs = objects_of(sc.flatten())
    assert sphere_encloses_every_leaf(objs[root]), e.text
    fired, bad = replay_round(e, sc, objs[root], root, derive(objs[root]))
    assert bad == 0 and fired >= MIN_PAIRS, (e.name, fired, bad, e.text)
    monkeypatch.setenv("LOL_GPU_TUNING", "1")
    monkeypatch.setenv("LOL_GPU_CULL_CARRY", "1")
    try:
        got = generated(sc)[2]
    except (RuntimeError, ValueError):                                     # (no kernel of its own, or no fast SDF: nothing is emitted)
        got = None
    assert got is not None or e not in MIXED
    if got is not None:
        obj = objs[got["id"] - 1]
        assert obj is not None and sphere_encloses_every_leaf(obj), e.text
        want = derive(obj)
        assert got["dl"] >= want["dl"] and got["ef"] >= want["ef"] and 0 < got["ctt"] <= want["ctt"] and got["ctc"] >= want["ctc"], (e.name, got, want)
        fired, bad = replay_round(e, sc, obj, got["id"] - 1, got)
        assert bad == 0 and (fired >= MIN_PAIRS or got["id"] - 1 != root), (e.name, fired, bad, e.text)


def test_the_model_runs_on_the_constants_the_generator_writes(s4):
    """tests/tools/value_carry_model.py holds scene4's constants as bit patterns: they are the generated ones"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("value_carry_model", os.path.join(ROOT, "tests", "tools", "value_carry_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    got, fast = s4["got"], s4["fast"]
    assert (F(float(m.V_DL)), F(float(m.V_EF)), F(float(m.V_CTT)), F(float(m.CTC))) == (got["dl"], got["ef"], got["ctt"], got["ctc"])
    as_bits = lambda x: "0x%08xu" % int(np.float32(x).view(np.uint32))      # noqa: E731
    for c, rm, k, a, b in m.CLUSTERS:
        for x in tuple(c) + (rm, k, a, b):
            assert as_bits(x) in fast
    assert as_bits(m.CTT) in fast


# ------------------------------------------------------------------ the switch and the policy

def test_the_switch_and_the_policy(monkeypatch):
    """Generated where the carried bound's outermost run is ONE object (scene4), never for scene.lol's group of objects, even with the
    cluster carry forced on there; LOL_GPU_CULL_VALUE_CARRY (beside LOL_GPU_TUNING) turns it off, and with it off the code is the
    code of the cluster carry alone; the library records the switch."""
    def fast_of(name):
        sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol"))
        return generated(sc)
    assert fast_of("scene4")[2] is not None and fast_of("scene")[2] is None
    monkeypatch.setenv("LOL_GPU_TUNING", "1")
    monkeypatch.setenv("LOL_GPU_CULL_VALUE_CARRY", "0")
    _, fast, got = fast_of("scene4")
    assert got is None and "ray_begin" in fast and "if (cool[0] == 0u) {\n\t\t  if (vote(" in fast and "maxf_(" not in fast
    assert "LOL_GPU_CULL_VALUE_CARRY=0" in gpu.tuning_switches()
    monkeypatch.setenv("LOL_GPU_CULL_VALUE_CARRY", "1")
    monkeypatch.setenv("LOL_GPU_CULL_CARRY", "1")
    assert fast_of("scene4")[2] is not None
    _, fast, got = fast_of("scene")
    assert got is None and "ray_begin" in fast
    monkeypatch.setenv("LOL_GPU_CULL_CARRY", "0")
    assert fast_of("scene4")[2] is None
