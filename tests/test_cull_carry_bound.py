"""The culling bound carried along a ray (lol_codegen.hip, carry_constants; the specialised kernel's fast SDF).  At a point p(T) of a
march or shadow loop the full test of an object's cluster spheres sets, per lane,
    lb = fl(G - |G| 2^-20),  G = fma(T, ctt, min_j fma(v_sqrt(cl_j), A_j, B_j))
and at every later point p(t), t >= T, of the same ray the object is skipped where
    fl(fma(t, ctc, |best|)) < lb.
That must imply, for every sphere j, |p(t) - C_j| > (|best| + rm_j) k_j in real arithmetic (the premise of make_test's proof, for
either sign of best).  Checked here in exact rational arithmetic with the constants the generator really writes for scene4, at the
WORST best (the largest |best| the check still lets through), over random rays, rays aimed at the centres, steps of 0 and of one
denormal, t near 100, |ro| near the 10^15 sanity cap and negative best; v_sqrt_f32 is taken 4 ulps above the rounded root.
p(t) = fl(ro + fl(rd t)) componentwise, as march() and soft_shadow() compute it; |rd| <= 1 + 2^-20 from the loop's own check
len2(rd) <= 1 + 2^-20 in binary32 (ray_begin), which is checked here too."""
import os
import re
import struct
from fractions import Fraction as F

import numpy as np
import pytest

from loltracer_amd import gpu, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = F(1, 2 ** 24)
RHO = 1 + F(1, 2 ** 20)


def rnd(x):
    """x (a Fraction) rounded to the nearest binary32, ties to even, subnormals included (no overflow in these cases)."""
    if x == 0:
        return F(0)
    sign, a = (-1, -x) if x < 0 else (1, x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if F(2) ** e > a:
        e -= 1
    q = F(2) ** (max(e, -126) - 23)
    n = a / q
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > F(1, 2) or (rem == F(1, 2) and fl % 2 == 1):
        fl += 1
    r = fl * q
    assert r < F(2) ** 128
    return sign * r


def f32(x):
    return F(float(np.float32(x)))


def bits(u):
    return F(struct.unpack("<f", struct.pack("<I", u))[0])


def next_up(x, n=1):
    v = np.float32(float(x))
    for _ in range(n):
        v = np.nextafter(v, np.float32(np.inf))
    return F(float(v))


def sqrt_hw(x):
    """The root of a binary32 square, 4 ulps above the correctly rounded one (the worst a v_sqrt_f32 within 4 ulps may give)."""
    return next_up(F(float(np.float32(np.sqrt(np.float64(float(x)))))), 4)


def point(ro, rd, t):
    return [rnd(o + rnd(d * t)) for o, d in zip(ro, rd)]


def len2(v):
    return rnd(rnd(rnd(v[0] * v[0]) + rnd(v[1] * v[1])) + rnd(v[2] * v[2]))


def carry_source():
    """The generated fast SDF of scene4 and the constants of its carried bound."""
    import tempfile
    sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", "scene4.lol"))
    with tempfile.TemporaryDirectory() as d:
        gpu.compile_offline(sc.flatten(), os.path.join(d, "s4"), assume_fast=True)
        src = open(os.path.join(d, "s4.hip")).read()
    fast = src[src.index("struct SpecSdfFast"):]
    body = fast[fast.index("void eval("):fast.index("void eval_dist(")]
    h = r"__builtin_bit_cast\(float, (0x[0-9a-f]+)u\)"
    ctc = int(re.search(r"__builtin_fmaf\(rt, " + h + r", __builtin_fabsf\(best\)\) < lb", body).group(1), 16)
    ctt = int(re.search(r"__builtin_fmaf\(rt, " + h + r", lm\)", body).group(1), 16)
    ab = {int(m.group(1)): (int(m.group(2), 16), int(m.group(3), 16))
          for m in re.finditer(r"__builtin_amdgcn_sqrtf\(cl(\d+)\), " + h + ", " + h + r"\)", body)}
    spheres = []
    for j in sorted(ab):
        c = re.search(r"cx%d = p\.x - %s, cy%d = p\.y - %s, cz%d = p\.z - %s" % (j, h, j, h, j, h), body)
        u = re.search(r"cu%d = \(best \+ %s\) \* %s" % (j, h, h), body)
        spheres.append(dict(c=[bits(int(c.group(i), 16)) for i in (1, 2, 3)], rm=bits(int(u.group(1), 16)), k=bits(int(u.group(2), 16)),
                            a=bits(ab[j][0]), b=bits(ab[j][1])))
    return fast, spheres, bits(ctt), bits(ctc)


@pytest.fixture(scope="module")
def consts():
    return carry_source()


def test_scene4_carries_the_bound_of_its_two_cluster_spheres(consts):
    fast, spheres, ctt, ctc = consts
    assert len(spheres) == 2
    assert "len2(rd) <= 0x1.00001p+0f" in fast                       # the loop's check behind rho = 1 + 2^-20
    assert "lb = -__builtin_inff(); carry = false;" in fast           # loop_done() forgets the ray


def test_the_constants_lie_on_the_safe_side(consts):
    _, spheres, ctt, ctc = consts
    for s in spheres:
        k, rm = s["k"], s["rm"]
        assert k >= 1 and rm > 0
        assert 0 < s["a"] <= (1 - F(1, 2 ** 20)) * (1 - E) / (k * (1 + E))
        # B <= -rm - (2^-73 + 2e|C|)/k  <=>  (-B - rm) k - 2^-73 >= 2e|C|  (both sides >= 0: compare squares)
        lhs = (-s["b"] - rm) * k - F(1, 2 ** 73)
        assert lhs >= 0 and lhs * lhs >= 4 * E * E * sum(c * c for c in s["c"])
        assert ctt <= RHO * (1 - E) / (k * (1 + E)) * (1 - F(1, 2 ** 20))
        assert ctc >= RHO / k * (1 + F(1, 2 ** 20))


def test_the_loop_check_bounds_the_direction():
    """fl(len2(rd)) <= 1 + 2^-20 in binary32 => |rd| <= 1 + 2^-20 exactly, at the boundary and for denormal components."""
    rng = np.random.default_rng(7)
    lim = F(float(np.float32(1 + 2 ** -20)))
    n_at_edge = 0
    for i in range(3000):
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        v = v * (1 + rng.uniform(-2e-6, 2e-6))
        if i % 10 == 0:
            v[rng.integers(3)] = 1e-42                                    # a denormal component
        rd = [f32(x) for x in v.astype(np.float32)]
        if len2(rd) <= lim:
            n_at_edge += len2(rd) > 1
            assert sum(x * x for x in rd) <= RHO * RHO, rd
    assert n_at_edge > 100


def normalize(v):
    v = [f32(x) for x in v]
    r = rnd(1 / f32(np.sqrt(np.float32(float(len2(v))))))
    return [rnd(x * r) for x in v]


def check(spheres, ctt, ctc, ro, rd, T, t):
    """lb set at p(T); at p(t) every best the check lets through (the worst one, both signs) must give the premise.
    Returns whether the check let anything through."""
    if not len2(rd) <= F(float(np.float32(1 + 2 ** -20))):
        return False                                                      # (the loop does not carry this ray)
    assert t >= T >= 0
    pT = point(ro, rd, T)
    lm = None
    for s in spheres:
        c = [rnd(p - x) for p, x in zip(pT, s["c"])]
        cl = len2(c)
        h = rnd(sqrt_hw(cl) * s["a"] + s["b"])
        lm = h if lm is None else min(lm, h)
    lg = rnd(T * ctt + lm)
    lb = rnd(abs(lg) * F(-1, 2 ** 20) + lg)
    if not rnd(t * ctc) < lb:
        return False
    # the largest |best| (a binary32) with fl(t ctc + |best|) < lb, by bisection on the bit patterns of non-negative floats
    lo, hi = 0, 0x7f800000
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if rnd(t * ctc + bits(mid)) < lb:
            lo = mid
        else:
            hi = mid
    worst = bits(lo)
    assert rnd(t * ctc + worst) < lb
    pt = point(ro, rd, t)
    for best in (worst, -worst):
        for s in spheres:
            d2 = sum((p - x) ** 2 for p, x in zip(pt, s["c"]))
            u = (abs(best) + s["rm"]) * s["k"]
            assert u > 0 and d2 > u * u, (ro, rd, T, t, best)
    return True


def test_the_carried_bound_implies_the_test(consts):
    _, spheres, ctt, ctc = consts
    rng = np.random.default_rng(20261016)
    centre = [float(x) for x in spheres[0]["c"]]
    passed = 0
    for i in range(400):
        ro = rng.uniform(-20, 20, 3) + [0, 5, 0]
        if i % 2:
            aim = np.array(centre) if i % 4 == 1 else np.array([float(x) for x in spheres[1]["c"]])
            v = aim - ro                                                   # straight at a centre: the bound shrinks fastest
        else:
            v = rng.normal(size=3)
        rd = normalize(v)
        T = f32(rng.uniform(0, 60))
        t = T
        for _ in range(int(rng.integers(0, 6))):
            t = rnd(t + f32(abs(rng.normal()) * 0.7))                     # march steps: t only grows
        passed += check(spheres, ctt, ctc, [f32(x) for x in ro], rd, T, t)
    assert passed > 100                                                   # (the check does let waves through)


@pytest.mark.parametrize("case", ["step0", "denormal", "near100", "big_ro", "ulp_step"])
def test_adversarial_steps(consts, case):
    _, spheres, ctt, ctc = consts
    rng = np.random.default_rng(["step0", "denormal", "near100", "big_ro", "ulp_step"].index(case) + 11)
    passed = 0
    for i in range(60):
        ro = rng.uniform(-30, 30, 3) + [0, 8, 0]
        aim = np.array([float(x) for x in spheres[i % 2]["c"]])
        rd = normalize(aim - ro if i % 3 else rng.normal(size=3))
        if case == "step0":
            T = f32(rng.uniform(0, 40)); t = T
        elif case == "denormal":
            T = F(0); t = F(float(np.nextafter(np.float32(0), np.float32(1)))) * int(rng.integers(1, 1000))
        elif case == "near100":
            T = f32(rng.uniform(95, 100)); t = f32(100.0)
        elif case == "big_ro":
            ro = rng.uniform(-1, 1, 3) * 9.9e14
            aim = ro + rng.normal(size=3) * 1e9
            rd = normalize(aim - ro)
            sph = [dict(s, c=[f32(x) for x in aim + rng.normal(size=3) * 1e8]) for s in spheres]
            T = f32(rng.uniform(0, 50)); t = rnd(T + f32(rng.uniform(0, 50)))
            check(sph, ctt, ctc, [f32(x) for x in ro], rd, T, t)
            sph = [dict(s, c=[f32(x) for x in ro + rng.normal(size=3) * 3e7]) for s in spheres]
            passed += check(sph, ctt, ctc, [f32(x) for x in ro], rd, T, t)
            continue
        else:                                                              # one ulp of t
            T = f32(rng.uniform(1, 90)); t = next_up(T)
        passed += check(spheres, ctt, ctc, [f32(x) for x in ro], rd, T, t)
    if case != "big_ro":
        assert passed > 10


def test_the_switch_and_the_policy(tmp_path, monkeypatch):
    """Carried where the outermost run is one object's cluster pair (scene4), not for scene.lol's group of objects; LOL_GPU_CULL_CARRY
    (beside LOL_GPU_TUNING) forces it off or on; the exact SDF never carries."""
    def fast_of(name):
        sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol"))
        base = str(tmp_path / name)
        gpu.compile_offline(sc.flatten(), base, assume_fast=True)
        src = open(base + ".hip").read()
        exact = src[src.index("struct SpecSdfExact"):src.index("struct SpecSdfFast")]
        assert "lb = " not in exact and "ray_begin" not in exact
        return src[src.index("struct SpecSdfFast"):]
    assert "ray_begin" in fast_of("scene4") and "ray_begin" not in fast_of("scene")
    monkeypatch.setenv("LOL_GPU_TUNING", "1")
    monkeypatch.setenv("LOL_GPU_CULL_CARRY", "0")
    assert "ray_begin" not in fast_of("scene4")
    monkeypatch.setenv("LOL_GPU_CULL_CARRY", "1")
    assert "ray_begin" in fast_of("scene")
