#!/usr/bin/env python3
"""What the stationary exit of the shadow march (lol_kernel.h, soft_shadow) can save, modelled on the CPU: no GPU.

The oracle runs the turns of a ray that has stopped moving, like the reference, and cannot be changed; so the shadow marches of
sampled 64 x 16 regions of C3 (scene4, 3840 x 2160) and C2 (scene.lol, 1920 x 1080, march limit 128) are replayed with
lol_oracle_sdf and binary32 numpy arithmetic (tests/shadow_replay.py).  For every sampled ray the replay must first reproduce the
oracle's per-light settled count; then, per workload:

  dead turns per pixel      settled shadow turns a kernel ran before the change and leaves out now
  wave-steps, rectangles    a new view: wave k of a region is its k-th 16 x 4 rectangle
  wave-steps, dealt         a repeated view: the region's pixels sorted by what they cost, wave k gets the k-th 64 of them
                            (lol_sched.hip, deal_by_cost_kernel: by cost, then by position)

A wave's steps are max over its lanes of the march steps plus, per light, max over its lanes of that light's shadow turns (the
loops are per-lane loops one behind the other: a wave stays in each as long as any lane does); normal taps and everything outside
the loops are left out, so the ratios are upper bounds for the frame rate.  `dealt_by_reported` deals the new kernel's lanes by the
reference's count instead of the executed one: what store_pixel's pixel_cost must not do.

    python tests/tools/stationary_shadow_model.py [--out profiles/r26_stationary_shadow_model.json] [--record-rays]

--record-rays rewrites tests/golden/stationary_shadow_rays.json (the rays of tests/test_shadow_fixed_point.py) and exits.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle_lib as O            # noqa: E402
import shadow_replay as SR        # noqa: E402
from loltracer_amd import scene as S      # noqa: E402

REGION_W, REGION_H = 64, 16
WORKLOADS = {"c3": dict(scene="scene4", w=3840, h=2160, max_steps=256, strips=20, per_strip=15),
             "c2": dict(scene="scene", w=1920, h=1080, max_steps=128, strips=20, per_strip=15)}


def wave_steps(march, shadow, groups):
    """sum over the waves (`groups`: [n_waves, 64] pixel indices) of max march + sum over lights of max shadow turns"""
    return int(march[groups].max(axis=1).sum() + shadow[groups].max(axis=1).sum())


def model(name, cfg):
    sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", cfg["scene"] + ".lol"))
    w, h, nl = cfg["w"], cfg["h"], min(sc.c.n_lights, 4)
    # (evenly spaced over the frame, its edges included: whole regions, so that the dealing can be modelled)
    rows = sorted({int(y) // REGION_H * REGION_H for y in np.linspace(0, h - REGION_H, cfg["strips"])})
    cols = sorted({int(x) // REGION_W * REGION_W for x in np.linspace(0, w - REGION_W, cfg["per_strip"])})
    tot = dict(pixels=0, rays=0, rays_128=0, rays_128_stationary=0, settled=0, executed=0, march=0,
               rect_before=0, rect_after=0, dealt_before=0, dealt_after=0, dealt_by_reported=0)
    rect = np.array([[(k // 4 * 4 + l // 16) * REGION_W + k % 4 * 16 + l % 16 for l in range(64)] for k in range(16)])
    for y0 in rows:
        _, _, osteps = O.render_rows(sc, w, h, y0, y0 + REGION_H, cfg["max_steps"], want_steps=True)
        assert O.last_counters.settle_violations == 0
        for x0 in cols:
            o = osteps[y0:y0 + REGION_H, x0:x0 + REGION_W].astype(np.int64)
            hit = o[..., 2] != 0
            # the rays a kernel marches under its default skips: a hit, and a diffuse incidence that is not exactly 0
            rays = [(x0 + x, y0 + y, li) for li in range(nl) for y, x in zip(*np.nonzero(hit & (((o[..., 3] >> li) & 1) == 0)))]
            rep = SR.replay(sc, *SR.shadow_rays(sc, w, h, rays, cfg["max_steps"]))
            before = np.zeros((REGION_H, REGION_W, nl), dtype=np.int64)
            after = np.zeros_like(before)
            ran = SR.executed(rep)
            for i, (x, y, li) in enumerate(rays):
                assert rep["settled"][i] == o[y - y0, x - x0, 8 + li] and rep["count"][i] == o[y - y0, x - x0, 4 + li], \
                    f"{name}: the replay of pixel ({x}, {y}) light {li} gives {rep['settled'][i]} / {rep['count'][i]} turns, the oracle " \
                    f"{o[y - y0, x - x0, 8 + li]} / {o[y - y0, x - x0, 4 + li]}"
                before[y - y0, x - x0, li] = rep["settled"][i]
                after[y - y0, x - x0, li] = ran[i]
            march = o[..., 0].reshape(-1)
            before, after = before.reshape(-1, nl), after.reshape(-1, nl)
            pos = np.arange(REGION_W * REGION_H)
            deal = lambda cost: np.lexsort((pos, cost)).reshape(16, 64)
            full = rep["settled"] == SR.TURNS
            tot["pixels"] += REGION_W * REGION_H
            tot["rays"] += len(rays)
            tot["rays_128"] += int(full.sum())
            tot["rays_128_stationary"] += int((full & (ran < SR.TURNS)).sum())
            tot["settled"] += int(before.sum())
            tot["executed"] += int(after.sum())
            tot["march"] += int(march.sum())
            tot["rect_before"] += wave_steps(march, before, rect)
            tot["rect_after"] += wave_steps(march, after, rect)
            tot["dealt_before"] += wave_steps(march, before, deal(march + before.sum(axis=1)))
            tot["dealt_after"] += wave_steps(march, after, deal(march + after.sum(axis=1)))
            tot["dealt_by_reported"] += wave_steps(march, after, deal(march + before.sum(axis=1)))
    px = tot["pixels"]
    out = dict(workload=name, scene=cfg["scene"], w=w, h=h, region_rows=rows, region_columns=cols, regions=len(rows) * len(cols), **tot)
    out["per_pixel"] = dict(march_steps=tot["march"] / px, settled_shadow_steps=tot["settled"] / px, executed_shadow_steps=tot["executed"] / px,
                            dead_turns=(tot["settled"] - tot["executed"]) / px, dead_share_of_shadow_steps=(tot["settled"] - tot["executed"]) / max(tot["settled"], 1))
    out["rays_128_share_of_needed"] = tot["rays_128"] / max(tot["rays"], 1)
    out["stationary_share_of_rays_128"] = tot["rays_128_stationary"] / max(tot["rays_128"], 1)
    out["creeping_share_of_needed"] = (tot["rays_128"] - tot["rays_128_stationary"]) / max(tot["rays"], 1)
    # the loops alone: steps x lanes a wave holds, before over after (1.10 = ten per cent more frames if nothing else cost time)
    out["predicted_loop_gain"] = dict(value_new_view=tot["rect_before"] / tot["rect_after"], value=tot["dealt_before"] / tot["dealt_after"],
                                      value_if_dealt_by_reported_count=tot["dealt_before"] / tot["dealt_by_reported"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_stationary_shadow_model.json"))
    ap.add_argument("--record-rays", action="store_true")
    ap.add_argument("--workload", action="append", choices=list(WORKLOADS))
    a = ap.parse_args()
    if a.record_rays:
        scenes = {n: S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", n + ".lol")) for n in ("scene4", "scene3")}
        SR.record_golden(scenes)
        print("wrote", SR.GOLDEN)
        return
    doc = dict(tool="tests/tools/stationary_shadow_model.py", source="CPU: oracle/lol_oracle.c step planes + tests/shadow_replay.py; no GPU",
               wave_model="per wave: max march steps + sum over lights of max shadow turns; loops only",
               workloads=[model(n, WORKLOADS[n]) for n in (a.workload or list(WORKLOADS))])
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for m in doc["workloads"]:
        print(m["workload"], json.dumps(m["per_pixel"]), json.dumps(m["predicted_loop_gain"]),
              "rays to 128: %.2f %% of needed, %.0f %% of them stationary" % (100 * m["rays_128_share_of_needed"], 100 * m["stationary_share_of_rays_128"]))


if __name__ == "__main__":
    main()
