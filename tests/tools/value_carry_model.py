#!/usr/bin/env python3
"""What is the object's own last value worth as a culling bound carried along the ray (lol_codegen.hip, value_carry_constants)?
CPU model of C3 (scene4 at 3840x2160, 256 march steps), numpy only — no device, no oracle: a binary32 sphere tracer of scene4 with
the kernel's camera, its two-cluster culling test, the cool-down of 3, the carried cluster bound and the settled-shadow exit.  It
traces random 64x16 regions of the frame; the pixels of a region are dealt to 16 waves by their step count, as the library deals
them for a camera that stands still.  What a pixel computes does not depend on what its wave skips, so every pixel is
traced once and the POLICIES — state machines over the steps of a wave — are run side by side on the same steps:
    parent        the carried cluster bound, checked where the cool-down counter is 0 (the code before this change)
    check_first   the same bound, checked before the counter: the new order alone, without the value
    value_inside  + the object's value folded into lb after every evaluation, the check still behind the counter
    value         + the check before the counter (the code as generated now)
    perfect_test  the blob is evaluated exactly where the cluster test of the wave fails, and a test is paid only where it passes
                  ("never test in vain, never overshoot"): the headroom of scheduling the tests
    needed        the blob is evaluated only where it wins against the plane in some lane that still marches: the floor
Cost of a wave step in VALU instructions, from the disassembly of scene4's kernel: 20 for a step, 11 for a test, 135 for an
evaluation of the blob, 5 for the value bound's update.  A model, not a measurement: the constants are scene4's as generated.
Usage: python tests/tools/value_carry_model.py [--regions 60] [--seed 1] [--out profiles/rNN_value_carry_model.json]"""
import argparse
import json
import struct

import numpy as np

f32 = np.float32
W, H, STEPS = 3840, 2160, 256
CAM_P, CAM_D, FOV = (-2, 6, 3), (0.3, -0.7, -1), 150
LIGHTS = [(-2, 10, -1), (-7, 2, -5)]
K = f32(3)
SPHERES = [((0, 1, -6), 1), ((-1, 0.5, -3), 3), ((2, 2, -10), 2), ((6, 2, -10), 5), ((-3, 4.5, -3), 0.5)]   # t1 t2 t4 t5 t7
bits = lambda u: f32(struct.unpack("<f", struct.pack("<I", u))[0])      # noqa: E731
# The constants of scene4's generated kernel, as bit patterns.  To regenerate after a change of the generator: gpu.compile_offline(
# Scene.parse_file("tests/golden/scenes/scene4.lol").flatten(), base, assume_fast=True) writes base.hip; in `struct SpecSdfFast` the
# cluster tests are cx / cy / cz (centres), cu (rm, k) and the two fma(v_sqrt(cl), A, B) lines, CTT sits in `fma(rt, CTT, lm)`, CTC in
# `fma(rt, CTC, |best|) < lb`, and V_CTT, V_DL, V_EF in the `vg` line.  tests/test_cull_value_carry_bound.py
# (test_the_model_runs_on_the_constants_the_generator_writes) fails when these drift from what the generator writes.
CLUSTERS = [((bits(0xbfae6d7c), bits(0x3fae3c72), bits(0xc04a6daf)), bits(0x40b58dd0), bits(0x3f800800), bits(0x3f7fefef), bits(0xc0b58dd1)),
            ((bits(0x40b00000), bits(0x40000000), bits(0xc1200000)), bits(0x40f83e17), bits(0x3f800800), bits(0x3f7fefef), bits(0xc0f83e1a))]
CTT, CTC = bits(0x3f7fefff), bits(0x3f7fff80)
V_DL, V_EF, V_CTT = bits(0x37a2ff9b), bits(0x39dff374), bits(0x3f7fff5d)
COST = dict(step=20, test=11, blob=135, update=5)
COOLDOWN = 3


def smin(a, b):
    h = np.clip(f32(.5) + f32(.5) * (b - a) / K, f32(0), f32(1))
    return (b + (a - b) * h) - K * h * (f32(1) - h)


def sphere(p, c, r):
    q = p - np.asarray(c, dtype=f32)
    return np.sqrt((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) - f32(r)


def blob(p):
    t = [sphere(p, c, r) for c, r in SPHERES]
    return smin(smin(t[0], t[1]), smin(t[4], smin(t[2], t[3])))


def plane(p):
    return p[..., 1] - f32(-1)


def normalize(v):
    l2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
    return v * (f32(1) / np.sqrt(l2))[..., None]


def camera_rays(xs, ys):
    d = np.asarray(CAM_D, dtype=f32)
    right = normalize(np.cross(d, np.asarray((0, 1, 0), dtype=f32)).astype(f32))
    up = np.cross(right, d).astype(f32)
    height = f32(np.arctan(f32(FOV / 2)))
    width = f32(W / H) * height
    vx = (xs.astype(f32) + f32(.5)) / f32(W) * f32(2) - f32(1)
    vy = f32(1) - (ys.astype(f32) + f32(.5)) / f32(H) * f32(2)
    return normalize((right * (vx * width)[..., None] + up * (vy * height)[..., None]) + d)


def trace(ro, rd, alive, n_steps, t_max, shadow):
    """one loop for every pixel: per step the lanes that evaluate it, their t, the plane's value and the blob's; and the end state"""
    t = np.zeros(alive.shape, dtype=f32)
    res = np.ones(alive.shape, dtype=f32)
    rec = []
    alive = alive.copy()
    d_last = np.zeros(alive.shape, dtype=f32)
    for _ in range(n_steps):
        if not alive.any():
            break
        p = ro + rd * t[..., None]
        b, v = plane(p), blob(p)
        cl = [((p[..., 0] - c[0]) ** 2 + (p[..., 1] - c[1]) ** 2) + (p[..., 2] - c[2]) ** 2 for c, *_ in CLUSTERS]
        rec.append((alive.copy(), t.copy(), b, v, cl))
        d = np.minimum(b, v)
        if shadow:
            with np.errstate(divide="ignore", invalid="ignore"):
                res = np.where(alive, np.minimum(res, f32(50) * d / t), res)
        t = np.where(alive, t + d, t)
        d_last = np.where(alive, d, d_last)
        alive = alive & ~((res <= 0) | (t > t_max) if shadow else (d < f32(0.001)) | (t > f32(100)))
    return rec, t, res


POLICIES = ["parent", "check_first", "value_inside", "value", "perfect_test", "needed"]
N_REAL = 4                                   # the first four are state machines the kernel could run


def run_policies(rec, order, tot):
    """the wave-level state machines over one loop's steps; order: [16, 64] pixel indices of the region's waves"""
    n = order.shape[0]
    st = {p: dict(cool=np.zeros(n, dtype=np.int64), lb=np.full(order.shape, -np.inf, dtype=f32)) for p in POLICIES[:N_REAL]}
    for alive, t, b, v, cl in rec:
        al, tt, bb, vv = alive[order], t[order], b[order], v[order]
        runs = al.any(axis=1)
        if not runs.any():
            break
        every = lambda c: (c | ~al).all(axis=1)                        # noqa: E731 — a vote of the lanes still in EXEC
        passes, lm = np.ones(order.shape, dtype=bool), None
        for (c, rm, k, A, B), l2 in zip(CLUSTERS, cl):
            cu = (bb + rm) * k
            passes &= (l2[order] > cu * cu) & (cu > 0)
            s = np.sqrt(l2[order]) * A + B
            lm = s if lm is None else np.minimum(lm, s)
        full = every(passes)
        wins = ~every(~(vv < bb))                                       # the blob wins against the plane in some lane
        g = tt * CTT + lm
        lb_cluster = g - np.abs(g) * f32(2 ** -20)
        g = tt * V_CTT + ((vv - np.abs(vv) * V_DL) - V_EF)
        lb_value = g - np.abs(g) * f32(2 ** -20)
        lhs = tt * CTC + np.abs(bb)
        tot["wave_steps"] += int(runs.sum())
        tot["needed"]["blob"] += int((runs & wins).sum())
        tot["perfect_test"]["blob"] += int((runs & ~full).sum())
        tot["perfect_test"]["test"] += int((runs & full).sum())
        for name in POLICIES[:N_REAL]:
            s = st[name]
            carried = every(lhs < s["lb"])
            free = s["cool"] == 0
            if name in ("value", "check_first"):
                skip_c = carried
                test = ~carried & free
            else:
                skip_c = carried & free
                test = ~carried & free
            ok = test & full
            ev = ~skip_c & ~ok
            s["cool"] = np.where(test & ~full, COOLDOWN, np.where(~skip_c & ~free, s["cool"] - 1, s["cool"]))
            if name in ("parent", "check_first"):
                s["lb"] = np.where(ok[:, None] & al, lb_cluster, s["lb"])
            else:
                s["lb"] = np.where(ok[:, None] & al, np.maximum(lb_cluster, s["lb"]), s["lb"])
                s["lb"] = np.where(ev[:, None] & al, np.maximum(lb_value, s["lb"]), s["lb"])
                tot[name]["update"] += int((runs & ev).sum())
            tot[name]["blob"] += int((runs & ev).sum())
            tot[name]["test"] += int((runs & test).sum())
            tot[name]["blob_not_winning"] += int((runs & ev & ~wins).sum())
            tot[name]["skipped_by_lb"] += int((runs & skip_c).sum())


def region(x0, y0, tot):
    ys, xs = np.mgrid[y0:y0 + 16, x0:x0 + 64]
    xs, ys = xs.ravel(), ys.ravel()
    ro = np.asarray(CAM_P, dtype=f32)
    rd = camera_rays(xs, ys)
    loops = []
    rec, t, _ = trace(ro, rd, np.ones(xs.shape, dtype=bool), STEPS, f32(100), False)
    loops.append(rec)
    steps = sum(a.astype(np.int64) for a, *_ in rec)
    hit = t < f32(100)
    p = ro + rd * t[..., None]
    e = f32(0.0001)
    taps = [np.asarray(k, dtype=f32) for k in ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1))]
    nrm = normalize(sum(k * np.minimum(plane(p + k * e), blob(p + k * e))[..., None] for k in taps))
    for light in LIGHTS:
        to = np.asarray(light, dtype=f32) - p
        dist = np.sqrt((to[..., 0] ** 2 + to[..., 1] ** 2) + to[..., 2] ** 2)
        ld = to * (f32(1) / dist)[..., None]
        di = np.clip((nrm * ld).sum(axis=-1), 0, 1)
        rec, _, _ = trace(p + ld, ld, hit & (di > 0), 128, dist, True)
        loops.append(rec)
        steps = steps + sum(a.astype(np.int64) for a, *_ in rec)
    dealt = np.argsort(steps, kind="stable").reshape(16, 64)                        # pixels dealt to waves by step count
    rect = np.arange(1024).reshape(4, 4, 4, 16).swapaxes(1, 2).reshape(16, 64)      # 16x4 rectangles
    for rec in loops:
        run_policies(rec, dealt, tot["dealt"])
        run_policies(rec, rect, tot["rectangles"])
    tot["lane_steps"] += int(steps.sum())
    tot["pixels"] += 1024


def summary(t):
    out = dict(wave_steps=t["wave_steps"])
    for name in POLICIES:
        c = t[name]
        cyc = COST["step"] * t["wave_steps"] + COST["test"] * c["test"] + COST["blob"] * c["blob"] + COST["update"] * c["update"]
        out[name] = dict(blob_evaluations=c["blob"], tests=c["test"], share_of_steps_that_evaluate_the_blob=c["blob"] / t["wave_steps"],
                         loop_valu_instructions=cyc)
        if name in POLICIES[:N_REAL]:
            out[name].update(steps_skipped_by_the_carried_bound=c["skipped_by_lb"],
                             share_of_blob_evaluations_the_blob_does_not_win=c["blob_not_winning"] / max(c["blob"], 1))
    base = out["parent"]
    for name in POLICIES[1:]:
        out[name]["blob_evaluations_vs_parent"] = out[name]["blob_evaluations"] / base["blob_evaluations"] - 1
        out[name]["loop_valu_instructions_vs_parent"] = out[name]["loop_valu_instructions"] / base["loop_valu_instructions"] - 1
    out["lane_efficiency"] = t["lane_steps_total"] / (64 * t["wave_steps"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=60)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    new = lambda: dict(wave_steps=0, **{p: dict(blob=0, test=0, update=0, blob_not_winning=0, skipped_by_lb=0) for p in POLICIES})   # noqa: E731
    tot = dict(dealt=new(), rectangles=new(), lane_steps=0, pixels=0)
    for _ in range(a.regions):
        region(int(rng.integers(0, W // 64)) * 64, int(rng.integers(0, H // 16)) * 16, tot)
    out = dict(workload="c3: scene4 3840x2160, 256 steps", regions=a.regions, seed=a.seed, pixels=tot["pixels"], cost_per_wave_step=COST,
               cooldown=COOLDOWN, loop_steps_per_pixel=tot["lane_steps"] / tot["pixels"])
    for order in ("dealt", "rectangles"):
        tot[order]["lane_steps_total"] = tot["lane_steps"]
        out[order] = summary(tot[order])
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
