"""The fold of the object's own value into the carried culling bound, only where it can matter (lol_codegen.hip, SdfForm::vgate).

After every evaluation of the carried object the kernel folded lb' = f(V, T) into lb.  Where the object's value V is the lane's minimum
the loop steps by V, and no later check of that lane can pass because of lb' (decide_form's comment): the fold is dead there, and the
generated code now leaves it out where EVERY lane in EXEC has V <= the minimum of the other objects — a vote before the join.  Leaving
a fold out is always allowed (lb stays a bound), so nothing here is about exactness; what is held:
  * the generated text: the gate exactly where the value bound is, in all three passes, in front of the join, with the fold's block
    kept a branch; gone with LOL_GPU_CULL_UPDATE_GATED=0 beside LOL_GPU_TUNING; the inequalities between the constants written;
  * a replay of the generated state machine (carried check, cool-down, the two-sphere test, both folds) in binary32 around the
    oracle's own object values, one wave of 64 lanes at a time, on the recorded shadow rays of scene4
    (tests/golden/stationary_shadow_rays.json) and on primary and shadow rays of pixels along the blob's silhouette: with and without
    the gate the wave evaluates the object at the same turns, lane for lane, and no bound that the gate left out would have let a
    later check of its lane pass.
No device."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import shadow_replay as R
import test_cull_carry_bound as CB
import test_cull_value_carry_bound as VB
from loltracer_amd import gpu, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GATE = r"const bool carry = this->carry && vote\(%s > best\) != 0;\n"
JOIN = r"\s*(best = vmin_\(%s, best\);|if \(%s < best[^\n]*)\n\s*if \(carry\) \{\n\s*const float vg[^\n]*\n\s*lb = maxf_[^\n]*\n\s*asm volatile\(\"\"\);\n\s*\}\n"
EPS, FAR, TURNS = F32(0.001), F32(100), 128
COOLDOWN = 3


def fast_of(sc):
    return VB.generated(sc)


def passes_of(fast):
    return (fast[fast.index("void eval_rec("):fast.index("void eval(")] if "void eval_rec(" in fast else None,
            fast[fast.index("void eval("):fast.index("void eval_dist(")], fast[fast.index("void eval_dist("):])


# ------------------------------------------------------------------ the generated text

def test_scene4_gates_the_fold_in_every_pass():
    exact, fast, got = fast_of(VB.scene4())
    assert got is not None and "this->carry" not in exact
    bodies = passes_of(fast)
    assert bodies[0] is not None                                          # scene4 marches through eval_rec()
    for body in bodies:
        v = got["value"]
        assert len(re.findall(GATE % v + JOIN % (v, v), body)) == 1 and body.count("this->carry") == 1 and body.count("asm volatile") == 1
    # nothing above the passes knows of it: the struct's head is the text it was
    assert "this->carry" not in fast[:fast.index("void eval_rec(")]


def test_the_written_constants_make_the_skipped_fold_dead():
    """ctc (1 - 2^-24)^2 >= ctt and >= 1 - dl, exactly, for the constants in the source: with V the lane's minimum at T every later
    t >= (T + V)(1 - 2^-24), lb' <= ctt T + (1 - dl) V, and fl(fma(t, ctc, |best|)) >= ctc t (1 - 2^-24)"""
    got = fast_of(VB.scene4())[2]
    lhs = got["ctc"] * (1 - VB.E) ** 2
    assert lhs >= got["ctt"] and lhs >= 1 - got["dl"]


def test_the_switch(monkeypatch):
    """LOL_GPU_CULL_UPDATE_GATED=0 beside LOL_GPU_TUNING: the fold after every evaluation, as before, and the switch recorded; the gate
    never without the value bound"""
    monkeypatch.setenv("LOL_GPU_TUNING", "1")
    monkeypatch.setenv("LOL_GPU_CULL_UPDATE_GATED", "0")
    _, fast, got = fast_of(VB.scene4())
    assert got is not None and "this->carry" not in fast and "asm volatile" not in fast
    assert "LOL_GPU_CULL_UPDATE_GATED=0" in gpu.tuning_switches()
    monkeypatch.setenv("LOL_GPU_CULL_UPDATE_GATED", "1")
    assert "this->carry" in fast_of(VB.scene4())[1]
    monkeypatch.setenv("LOL_GPU_CULL_VALUE_CARRY", "0")
    assert "this->carry" not in fast_of(VB.scene4())[1]


@pytest.mark.parametrize("name", ["scene", "scene2", "scene3"])
def test_the_other_example_scenes_have_no_gate(name):
    sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol"))
    exact, fast, got = fast_of(sc)
    assert got is None and "this->carry" not in exact + fast


@pytest.mark.parametrize("e", VB.MIXED, ids=lambda e: e.name)
def test_the_gate_goes_where_the_value_bound_goes(e, monkeypatch):
    """one bounded object behind a carried bound, after a plane: the object is the last of the plan, and its fold is gated"""
    monkeypatch.setenv("LOL_GPU_TUNING", "1")
    monkeypatch.setenv("LOL_GPU_CULL_CARRY", "1")
    _, fast, got = fast_of(VB.scene_of(e))
    assert got is not None
    for body in passes_of(fast)[1:]:
        assert len(re.findall(GATE % got["value"] + JOIN % (got["value"], got["value"]), body)) == 1
    lhs = got["ctc"] * (1 - VB.E) ** 2
    assert lhs >= got["ctt"] and lhs >= 1 - got["dl"]


def test_a_carried_object_that_is_not_the_last_of_the_plan_keeps_its_fold_unconditional(monkeypatch):
    """three bounded objects and no floor, the carry forced on: the first object has nothing before it and gets no test, the second is
    the plan's outermost run — ONE object, so it carries a value bound — and the third is evaluated after it.  `best` before the
    second object's join is then NOT the minimum of all the others, and the fold stays as it was: no vote, no kept branch.  (The
    other way out of eligibility, constants that fail the two inequalities, no tree reaches: ctc >= rho (1 - et)(1 + 2^-20) lies
    above ctt = rho (1 - e) kap (1 - 2^-20) and above 1 - dl < 1 - 2 et for every et; the generator checks it all the same.)"""
    from test_gpu_cull_value_carry import BLOB, CAMERA, CHAIN, SECOND, text
    monkeypatch.setenv("LOL_GPU_TUNING", "1")
    monkeypatch.setenv("LOL_GPU_CULL_CARRY", "1")
    for objects in ((BLOB, SECOND, CHAIN), (CHAIN, BLOB, SECOND)):
        _, fast, got = fast_of(S.Scene.parse_string(text(CAMERA, *objects)))
        assert got is not None and "const float vg" in fast                   # the value bound is there ...
        assert "this->carry" not in fast and "asm volatile" not in fast       # ... and its fold is not gated
        body = fast[fast.index("void eval_dist("):]
        assert body.index("const float vg") < body.rindex("best = vmin_(")    # (an object joins the minimum after the carried one)
    # with a floor in front and ONE bounded object behind it the same object is gated
    _, fast, got = fast_of(S.Scene.parse_string(text(CAMERA, CHAIN, "plane { material = #2, y = -1 }")))
    assert got is not None and "this->carry" in fast


# ------------------------------------------------------------------ the state machine of a wave, replayed

def fma(a, b, c):
    """(one rounding too many where the double sum is inexact: the same in both arms of the comparison)"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


class Machine:
    def __init__(self):
        sc = VB.scene4()
        _, spheres, ctt, ctc_carry = CB.carry_source()
        got = fast_of(sc)[2]
        f = lambda x: F32(float(x))      # noqa: E731
        self.spheres = [dict(c=np.array([f(x) for x in s["c"]], dtype=F32), rm=f(s["rm"]), k=f(s["k"]), a=f(s["a"]), b=f(s["b"])) for s in spheres]
        self.ctt, self.ctc = f(ctt), f(got["ctc"])
        assert ctc_carry == got["ctc"]                                    # ONE left-hand side for both bounds
        self.v_ctt, self.dl, self.ef = f(got["ctt"]), f(got["dl"]), f(got["ef"])
        self.sc = sc
        self.blob, self.plane = VB.Sub(sc, [0]), VB.Sub(sc, [1])

    def values(self, sub, p, alive, out):
        for j in np.flatnonzero(alive):
            out[j] = sub.sdf(p[j])
        return out

    def run(self, ro, rd, turns, t_max, shadow, gated):
        """one wave: the lanes' rays (ro [n, 3] or [3], rd [n, 3], t_max [n] or a scalar).  -> (per turn: the lanes in EXEC and whether
        the object was evaluated; the folds taken; the folds the gate left out; per lane the end t)"""
        n = len(rd)
        ro = np.broadcast_to(np.asarray(ro, dtype=F32), (n, 3))
        t_max = np.broadcast_to(np.asarray(t_max, dtype=F32), (n,))
        t, res = np.zeros(n, dtype=F32), np.ones(n, dtype=F32)
        alive = np.ones(n, dtype=bool)
        lb = np.full(n, -np.inf, dtype=F32)
        left_out = np.full(n, -np.inf, dtype=F32)                         # the largest lb' the gate left out, per lane
        l2 = ((rd[:, 0] * rd[:, 0]).astype(F32) + (rd[:, 1] * rd[:, 1]).astype(F32)).astype(F32) + (rd[:, 2] * rd[:, 2]).astype(F32)
        carry = bool((l2.astype(F32) <= F32(1 + 2 ** -20)).all())
        cool, log, folds, skipped_folds = 0, [], 0, 0
        b, V = np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
        with np.errstate(all="ignore"):
            for _ in range(turns):
                if not alive.any():
                    break
                p = (ro + (rd * t[:, None]).astype(F32)).astype(F32)
                self.values(self.plane, p, alive, b)
                lhs = fma(t, self.ctc, np.abs(b))
                # what the gate's argument promises: a bound it left out never decides a later check of its lane
                assert not (alive & (lhs < left_out)).any()
                need = True
                if (lhs[alive] < lb[alive]).all():
                    need = False
                elif cool == 0:
                    ok, lm = np.ones(n, dtype=bool), None
                    for s in self.spheres:
                        c = (p - s["c"]).astype(F32)
                        cl = ((c[:, 0] * c[:, 0]).astype(F32) + (c[:, 1] * c[:, 1]).astype(F32)).astype(F32) + (c[:, 2] * c[:, 2]).astype(F32)
                        cu = ((b + s["rm"]).astype(F32) * s["k"]).astype(F32)
                        ok &= (cl > (cu * cu).astype(F32)) & (cu > 0)
                        m = fma(np.sqrt(cl).astype(F32), s["a"], s["b"])
                        lm = m if lm is None else np.minimum(m, lm)
                    need = not ok[alive].all()
                    if need:
                        cool = COOLDOWN
                    elif carry:
                        lg = fma(t, self.ctt, lm)
                        new = fma(np.abs(lg), F32(-2 ** -20), lg)
                        lb = np.where(alive & (new > lb), new, lb)
                else:
                    cool -= 1
                log.append((alive.copy(), need))
                best = b.copy()
                if need:
                    self.values(self.blob, p, alive, V)
                    vg = fma(t, self.v_ctt, (fma(np.abs(V), -self.dl, V) - self.ef).astype(F32))
                    new = fma(np.abs(vg), F32(-2 ** -20), vg)
                    if carry and (not gated or (V[alive] > b[alive]).any()):
                        lb = np.where(alive & (new > lb), new, lb)
                        folds += 1
                    elif carry:
                        left_out = np.where(alive & (new > left_out), new, left_out)
                        skipped_folds += 1
                    best = np.minimum(V, b)
                if shadow:
                    v = ((F32(50) * best).astype(F32) / t).astype(F32)
                    res = np.where(alive, np.minimum(res, v), res)
                    tn = (t + best).astype(F32)
                    out = (res <= 0) | (tn > t_max) | (tn == t)
                else:
                    tn = (t + best).astype(F32)
                    out = (best < EPS) | (tn > FAR)
                t = np.where(alive, tn, t)
                alive = alive & ~out
        return log, folds, skipped_folds, t


@pytest.fixture(scope="module")
def machine():
    return Machine()


def same_evaluations(machine, ro, rd, turns, t_max, shadow):
    a = machine.run(ro, rd, turns, t_max, shadow, gated=False)
    g = machine.run(ro, rd, turns, t_max, shadow, gated=True)
    assert len(a[0]) == len(g[0])
    for (al, need), (al_g, need_g) in zip(a[0], g[0]):
        assert np.array_equal(al, al_g) and need == need_g
    assert np.array_equal(R.bits(a[3]), R.bits(g[3])) and a[2] == 0 and a[1] == g[1] + g[2]
    evaluated = sum(need for _, need in a[0])
    return len(a[0]), evaluated, g[2]


def test_the_recorded_shadow_rays_of_scene4_skip_the_same_evaluations(machine):
    _, _, rays = R.load_golden()
    r = rays["scene4"]
    assert len(r["ro"]) == 64                                             # one wave
    turns, evaluated, left_out = same_evaluations(machine, r["ro"].reshape(-1, 3), r["dir"].reshape(-1, 3), TURNS, r["max_dist"], True)
    print("recorded shadow rays: %d turns, %d evaluations of the blob, %d folds left out" % (turns, evaluated, left_out))
    # (64 rays from all over the frame in one wave: some lane is always over the floor, away from the blob, so this wave folds at
    # every turn — the gate must then change nothing at all; the coherent waves below are where it leaves folds out)
    assert evaluated >= 20


W, H = 160, 90
# 16x4 patches of a 160x90 frame of scene4: across the blob's silhouette against the floor, on the floor under the blob, on the blob
PATCHES = [(40, 40), (72, 52), (100, 30), (16, 60), (130, 70), (88, 44)]


@pytest.mark.parametrize("x0,y0", PATCHES)
def test_primary_and_shadow_rays_skip_the_same_evaluations(machine, x0, y0):
    sc = machine.sc
    cam = np.array(sc.camera.point.tuple(), dtype=F32)
    pix = [(x, y) for y in range(y0, y0 + 4) for x in range(x0, x0 + 16)]
    probes = [O.probe(sc, W, H, x, y, 256) for x, y in pix]
    rd = np.array([list(pr.rd) for pr in probes], dtype=F32)
    turns, evaluated, left_out = same_evaluations(machine, cam, rd, 256, FAR, False)
    log, _, _, t = machine.run(cam, rd, 256, FAR, False, gated=True)
    assert np.array_equal(R.bits(t), R.bits(np.array([pr.hit_dist for pr in probes], dtype=F32)))      # the replay marches as the oracle does
    print("patch (%d, %d): march %d turns, %d evaluations, %d folds left out" % (x0, y0, turns, evaluated, left_out))
    total = [evaluated, left_out]
    hit = [i for i, pr in enumerate(probes) if pr.hit_dist < 100]
    if hit:
        for li in range(sc.c.n_lights):
            ro, dr, md = R.shadow_rays(sc, W, H, [(pix[i][0], pix[i][1], li) for i in hit])
            turns, evaluated, left_out = same_evaluations(machine, ro, dr, TURNS, md, True)
            print("  light %d: %d lanes, %d turns, %d evaluations, %d folds left out" % (li, len(hit), turns, evaluated, left_out))
            total = [total[0] + evaluated, total[1] + left_out]
    assert total[0] > 0


def test_the_gate_leaves_folds_out_on_these_rays(machine):
    """... so the comparison above compares something: over the marches of the patches both sides of the gate are taken often"""
    sc = machine.sc
    cam = np.array(sc.camera.point.tuple(), dtype=F32)
    taken = out = 0
    for x0, y0 in PATCHES:
        rd = np.array([list(O.probe(sc, W, H, x, y, 256).rd) for y in range(y0, y0 + 4) for x in range(x0, x0 + 16)], dtype=F32)
        _, folds, left, _ = machine.run(cam, rd, 256, FAR, False, gated=True)
        taken += folds
        out += left
    assert taken >= 30 and out >= 30, (taken, out)


def test_the_model_runs_and_its_machines_agree():
    """tests/tools/bound_upkeep_model.py (the constants are value_carry_model.py's, which tests/test_cull_value_carry_bound.py holds to
    the generator's): three regions of C3, and the committed record of 400"""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bound_upkeep_model", os.path.join(ROOT, "tests", "tools", "bound_upkeep_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    tot = m.totals()
    for x0, y0 in ((1920, 1072), (1024, 1600), (2560, 800)):
        m.region(x0, y0, tot)
    for loop in ("march", "shadow"):
        c = tot[loop]
        assert c["wave_steps_where_the_machines_differ"] == 0 and c["always"]["blob"] == c["gated"]["blob"] > 0
        assert c["gated"]["fold"] == c["always"]["fold"] - c["always"]["blob_where_every_lane_is_at_its_minimum"]
    with open(os.path.join(ROOT, "profiles", "r27_bound_upkeep_model.json")) as f:
        rec = json.load(f)
    assert rec["regions"] == 400 and all(rec[l]["wave_steps_where_the_machines_differ"] == 0 for l in ("march", "shadow"))
    # ... and the part that is not built is modelled on the same regions: the kept bound never makes a wave test or evaluate MORE
    kept = rec["kept_bound_not_built"]
    assert kept["taps"]["kept"]["test"] <= kept["taps"]["now"]["test"] and kept["taps"]["kept"]["blob"] <= kept["taps"]["now"]["blob"]
    assert kept["shadow_loops_kept"]["blob"] <= kept["shadow_loops_gated"]["blob"]
