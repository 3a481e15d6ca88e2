#!/usr/bin/env python3
"""Where is the upkeep of the carried culling bound paid for nothing (lol_codegen.hip, SdfForm::vgate)?
CPU model of C3 (scene4 at 3840x2160, 256 march steps), numpy only — no device, no oracle.  It stands on value_carry_model.py: that
model's binary32 tracer of scene4, its camera, cluster tests, cool-down and the constants of the generated kernel (which
tests/test_cull_value_carry_bound.py holds to what the generator writes).  Added here: the stationary exit of the shadow march
(lol_kernel.h, soft_shadow: a lane leaves once fl(t + s) == t), pixels dealt to the sixteen waves of a 64x16 region by the steps
they RUN, and two state machines over the steps of a wave, side by side on the same steps:
    always   the object's value is folded into lb after EVERY evaluation of the blob on a ray that may carry (the parent's code)
    gated    ... only where some lane in EXEC has a blob value greater than the plane's, the minimum of the other objects
What it answers: at how many of a wave's blob evaluations every lane's blob value is the minimum (the fold is then dead in every
lane: decide_form's comment), and whether leaving the fold out there ever costs a skip — the two machines must evaluate the blob
at the same wave-steps.  Cost in VALU instructions: 6 for a fold (fma, add, fmac, fma, v_cmp, v_cndmask), 1 for the gate's compare.
A model, not a measurement.
Beside it, the part of the proposal that is NOT built (LABNOTES 8, "the bound kept past the march"), so that its figure stands on the
same 400 regions: a third machine, `kept`, is the gated one with the lane's bound at the end of the march carried on — in real
arithmetic with a slack of 10^-3, a model and no proof — as kb = lb - ctc t*, t* = rt + |dist - rt| (rt: the t of the march's last
evaluation; the last step may be negative).  At the four normal taps (within sqrt(3) h of p(dist), h = dist / 100) the carried check
|plane| < kb - sqrt(3) h stands in front of the cluster test, which today runs again at every tap because loop_done() forgot the
bound; each shadow march starts from lb = kb - |dir| instead of -inf.  Cost: 26 VALU for the two-sphere test, 10 more where it
passes on a carrying ray and sets lb (two v_sqrt among them), 139 for an evaluation of the blob with its fold.
Usage: python tests/tools/bound_upkeep_model.py [--regions 400] [--seed 1] [--out profiles/rNN_bound_upkeep_model.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import value_carry_model as M      # noqa: E402

f32 = np.float32
FOLD_VALU, GATE_VALU = 6, 1
TEST_VALU, SET_VALU, BLOB_VALU = 26, 10, 139
POLICIES = ("always", "gated")


def trace(ro, rd, alive, n_steps, t_max, shadow):
    """value_carry_model.trace with the stationary exit: per step the lanes that evaluate it, their t, the plane's value, the blob's
    and the squared distances of the cluster tests"""
    t = np.zeros(alive.shape, dtype=f32)
    res = np.ones(alive.shape, dtype=f32)
    rec = []
    alive = alive.copy()
    for _ in range(n_steps):
        if not alive.any():
            break
        p = ro + rd * t[..., None]
        b, v = M.plane(p), M.blob(p)
        cl = [((p[..., 0] - c[0]) ** 2 + (p[..., 1] - c[1]) ** 2) + (p[..., 2] - c[2]) ** 2 for c, *_ in M.CLUSTERS]
        rec.append((alive.copy(), t.copy(), b, v, cl))
        d = np.minimum(b, v)
        if shadow:
            with np.errstate(divide="ignore", invalid="ignore"):
                res = np.where(alive, np.minimum(res, f32(50) * d / t), res)
        tn = np.where(alive, t + d, t)
        still = (tn == t) if shadow else np.zeros(alive.shape, dtype=bool)
        t = tn
        alive = alive & ~(((res <= 0) | (t > t_max) | still) if shadow else (d < f32(0.001)) | (t > f32(100)))
    return rec, t


def run_waves(rec, order, tot, kept_lb=None):
    """the machines over one loop's steps; order: [16, 64] pixel indices of the region's waves.  kept_lb [pixels]: also run `kept`,
    the gated machine started from that bound (counted in tot["kept"]).  -> the gated machine's lb at the end, per pixel"""
    n = order.shape[0]
    names = POLICIES + (("kept",) if kept_lb is not None else ())
    st = {p: dict(cool=np.zeros(n, dtype=np.int64), lb=np.full(order.shape, -np.inf, dtype=f32)) for p in names}
    if kept_lb is not None:
        st["kept"]["lb"] = kept_lb[order].astype(f32)
    for alive, t, b, v, cl in rec:
        al, tt, bb, vv = alive[order], t[order], b[order], v[order]
        runs = al.any(axis=1)
        if not runs.any():
            break
        every = lambda c: (c | ~al).all(axis=1)                        # noqa: E731 — a vote of the lanes still in EXEC
        passes, lm = np.ones(order.shape, dtype=bool), None
        for (c, rm, k, A, B), l2 in zip(M.CLUSTERS, cl):
            cu = (bb + rm) * k
            passes &= (l2[order] > cu * cu) & (cu > 0)
            s = np.sqrt(l2[order]) * A + B
            lm = s if lm is None else np.minimum(lm, s)
        full = every(passes)
        g = tt * M.CTT + lm
        lb_cluster = g - np.abs(g) * f32(2 ** -20)
        g = tt * M.V_CTT + ((vv - np.abs(vv) * M.V_DL) - M.V_EF)
        lb_value = g - np.abs(g) * f32(2 ** -20)
        lhs = tt * M.CTC + np.abs(bb)
        all_minimum = every(~(vv > bb))                                 # the gate's vote: no lane's blob value above the plane's
        tot["wave_steps"] += int(runs.sum())
        evaluated = {}
        for name in names:
            s = st[name]
            carried = every(lhs < s["lb"])
            free = s["cool"] == 0
            test = ~carried & free
            ok = test & full
            ev = runs & ~carried & ~ok
            s["cool"] = np.where(test & ~full, M.COOLDOWN, np.where(~carried & ~free, s["cool"] - 1, s["cool"]))
            s["lb"] = np.where(ok[:, None] & al, np.maximum(lb_cluster, s["lb"]), s["lb"])
            fold = ev if name == "always" else ev & ~all_minimum
            s["lb"] = np.where(fold[:, None] & al, np.maximum(lb_value, s["lb"]), s["lb"])
            c = tot[name]
            c["blob"] += int(ev.sum())
            c["test"] += int((runs & test).sum())
            c["test_passed"] += int((runs & ok).sum())
            c["fold"] += int(fold.sum())
            c["blob_where_every_lane_is_at_its_minimum"] += int((ev & all_minimum).sum())
            evaluated[name] = ev
        tot["wave_steps_where_the_machines_differ"] += int((evaluated["always"] != evaluated["gated"]).sum())
    out = np.full(order.size, -np.inf, dtype=f32)
    out[order.ravel()] = st["gated"]["lb"].ravel()
    return out


SLACK = f32(1e-3)
TAPS = [np.asarray(k, dtype=f32) for k in ((1, 1, 1), (-1, 1, -1), (-1, -1, 1), (1, -1, -1))]      # k3 down to k0, as the kernel runs them


def run_taps(p, dist, hit, kb, order, tot):
    """the four normal taps of every lit wave (a wave in which every ray escaped takes none: FLAG_MISS_SKIP), today and with the
    kept bound in front of the cluster test.  After loop_done() the counter is 0 and lb is -inf: today every tap tests again."""
    h = dist / f32(100)
    for w in range(order.shape[0]):
        lanes = order[w]
        if not hit[lanes].any():
            continue
        tot["lit_waves"] += 1
        cool = dict(now=0, kept=0)
        decided = 0
        for k in TAPS:
            q = p[lanes] + k * h[lanes, None]
            b = M.plane(q)
            passes = np.ones(len(lanes), dtype=bool)
            for (c, rm, kk, A, B) in M.CLUSTERS:
                l2 = ((q[:, 0] - c[0]) ** 2 + (q[:, 1] - c[1]) ** 2) + (q[:, 2] - c[2]) ** 2
                cu = (b + rm) * kk
                passes &= (l2 > cu * cu) & (cu > 0)
            full = bool(passes.all())
            room = kb[lanes] - f32(np.sqrt(3.0)) * h[lanes] * (f32(1) + SLACK)
            carried = bool((np.abs(b) < room - np.abs(room) * SLACK).all())
            decided += carried
            for name in ("now", "kept"):
                if name == "kept" and carried:
                    continue
                if cool[name] == 0:
                    tot[name]["test"] += 1
                    if not full:
                        cool[name] = M.COOLDOWN
                        tot[name]["blob"] += 1
                else:
                    cool[name] -= 1
                    tot[name]["blob"] += 1
        tot["taps_the_kept_bound_decides"] += decided
        tot["lit_waves_with_all_four_taps_decided"] += decided == 4


def region(x0, y0, tot):
    ys, xs = np.mgrid[y0:y0 + 16, x0:x0 + 64]
    xs, ys = xs.ravel(), ys.ravel()
    ro = np.asarray(M.CAM_P, dtype=f32)
    rd = M.camera_rays(xs, ys)
    loops = []
    rec, t = trace(ro, rd, np.ones(xs.shape, dtype=bool), M.STEPS, f32(100), False)
    loops.append(("march", rec))
    steps = sum(a.astype(np.int64) for a, *_ in rec)
    rt = np.zeros(xs.shape, dtype=f32)                                               # the t of each lane's last evaluation
    for alive, tt, *_ in rec:
        rt = np.where(alive, tt, rt)
    hit = t < f32(100)
    p = ro + rd * t[..., None]
    e = f32(0.0001)
    taps = [np.asarray(k, dtype=f32) for k in ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1))]
    nrm = M.normalize(sum(k * np.minimum(M.plane(p + k * e), M.blob(p + k * e))[..., None] for k in taps))
    for light in M.LIGHTS:
        to = np.asarray(light, dtype=f32) - p
        dist = np.sqrt((to[..., 0] ** 2 + to[..., 1] ** 2) + to[..., 2] ** 2)
        ld = to * (f32(1) / dist)[..., None]
        di = np.clip((nrm * ld).sum(axis=-1), 0, 1)
        rec, _ = trace(p + ld, ld, hit & (di > 0), 128, dist, True)
        loops.append(("shadow", rec))
        steps = steps + sum(a.astype(np.int64) for a, *_ in rec)
    dealt = np.argsort(steps, kind="stable").reshape(16, 64)                        # pixels dealt to waves by the steps they run
    lb = run_waves(loops[0][1], dealt, tot["march"])
    with np.errstate(invalid="ignore"):
        star = rt + np.abs(t - rt)
        kb = lb - M.CTC * star
        kb = np.where(np.isfinite(kb), kb - np.abs(kb) * SLACK, f32(-np.inf)).astype(f32)
    run_taps(p, t, hit, kb, dealt, tot["taps"])
    for loop, rec in loops[1:]:
        ray_lb = np.where(np.isfinite(kb), kb - (f32(1) + SLACK), f32(-np.inf)).astype(f32)      # |dir| <= 1 + 2^-20
        run_waves(rec, dealt, tot[loop], kept_lb=ray_lb)
    tot["lane_steps"] += int(steps.sum())
    tot["pixels"] += 1024


def totals():
    new = lambda: dict(wave_steps=0, wave_steps_where_the_machines_differ=0,      # noqa: E731
                       **{p: dict(blob=0, test=0, test_passed=0, fold=0, blob_where_every_lane_is_at_its_minimum=0) for p in POLICIES + ("kept",)})
    tot = dict(march=new(), shadow=new(), lane_steps=0, pixels=0,
               taps=dict(lit_waves=0, taps_the_kept_bound_decides=0, lit_waves_with_all_four_taps_decided=0, now=dict(test=0, blob=0), kept=dict(test=0, blob=0)))
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=400)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    tot = totals()
    for _ in range(a.regions):
        region(int(rng.integers(0, M.W // 64)) * 64, int(rng.integers(0, M.H // 16)) * 16, tot)
    out = dict(workload="c3: scene4 3840x2160, 256 steps, still camera: pixels dealt by executed steps", regions=a.regions, seed=a.seed,
               pixels=tot["pixels"], loop_steps_per_pixel=tot["lane_steps"] / tot["pixels"], valu_per_fold=FOLD_VALU, valu_per_gate=GATE_VALU)
    saved = 0
    for loop in ("march", "shadow"):
        c = tot[loop]
        al, ga = c["always"], c["gated"]
        out[loop] = dict(wave_steps=c["wave_steps"], always=al, gated=ga, **({"kept": c["kept"]} if loop == "shadow" else {}),
                         wave_steps_where_the_machines_differ=c["wave_steps_where_the_machines_differ"],
                         share_of_blob_evaluations_where_every_lane_is_at_its_minimum=al["blob_where_every_lane_is_at_its_minimum"] / max(al["blob"], 1))
        saved += FOLD_VALU * (al["fold"] - ga["fold"]) - GATE_VALU * ga["blob"]
    waves = tot["pixels"] / 64
    out["blob_evaluations_per_pixel"] = (tot["march"]["always"]["blob"] + tot["shadow"]["always"]["blob"]) / waves
    out["valu_instructions_saved_per_pixel"] = saved / waves
    # ---- the part that is not built: the bound kept past the march (against the gated machine)
    tp, sh = tot["taps"], tot["shadow"]
    g, k = sh["gated"], sh["kept"]
    tap_saved = TEST_VALU * (tp["now"]["test"] - tp["kept"]["test"]) + BLOB_VALU * (tp["now"]["blob"] - tp["kept"]["blob"])
    ray_saved = (TEST_VALU * (g["test"] - k["test"]) + SET_VALU * (g["test_passed"] - k["test_passed"]) + BLOB_VALU * (g["blob"] - k["blob"])
                 + FOLD_VALU * (g["fold"] - k["fold"]))
    out["kept_bound_not_built"] = dict(
        what="modelled in real arithmetic with a slack of 1e-3: no proof, no device", valu_per_test=TEST_VALU, valu_per_set=SET_VALU,
        valu_per_blob_evaluation=BLOB_VALU, taps=tp, shadow_loops_gated=g, shadow_loops_kept=k,
        valu_instructions_saved_per_pixel_at_the_taps=tap_saved / waves,
        valu_instructions_saved_per_pixel_in_the_shadow_loops=ray_saved / waves,
        valu_instructions_saved_per_pixel=(tap_saved + ray_saved) / waves)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
