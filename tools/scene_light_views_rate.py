"""What the averaged resolve over records costs (lol_gpu_relight_scene_views) beside the resolve of single leaves over the same elements
and beside the march it replaces.  scene4 with one sphere moving (scene.tween from the sphere at (0, 1, -6) to (1.5, 2, -5)), 64
records of a 128 x 128 frame with 2 x 2 samples per pixel, as two workloads: 64 frames of one record each (an antialiased animation)
and 16 frames of K = 4 records each (a motion-blurred one).  A context without the scene compiler (specialize 4: the interpreter with
the upload's proven fast paths — what captures, resolves and scene views run on whatever the context is).  Every record has a look of
its own (two looks alternate over the records).  Arms, ALTERNATING in one process, every arm warmed up first:
    V    one relight_scene_views_into over the captured leaves, a look per record: the new call
    R    one relight_scenes_into over the same N elements under the same looks: the same bytes read, a colour per LEAF written, no
         averaging
    M    one render_scene_views_into(looks, samples=2, cameras_per_view=K): the march that V replaces
    C    one light_scene_pixels_into over the 64 sample grids: the capture V and R read
Before anything is timed V's pixels are held equal, byte for byte, to M's.  A window repeats its arm until it lasts at least
--window-s; HIP events around the window; --windows windows per arm; medians and ranges in milliseconds per call.
`looks_to_beat_the_march` is the smallest number of looks L with C + L V < L M.

    python tools/scene_light_views_rate.py --out profiles/r28_relit_scene_views_rate.json                  (on the GPU box)
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from loltracer_amd import gpu  # noqa: E402
from loltracer_amd.__main__ import look_of  # noqa: E402
from ray_rate import window  # noqa: E402
from scene_queries_rate import RECORDS, moving_scenes  # noqa: E402

SIDE, SAMPLES = 128, 2
MAX_STEPS = 256
LOOKS = (dict(lights=[((.9, .2, .1), (.1, .8, .3)), ((2., 1.5, 1.), (1., 1.5, 2.))], ambient=(.35, .15, .6)),
         dict(lights=[((.3, .7, 1.2), (.6, .6, .1)), ((1., 2.5, .5), (2., .5, 1.))], ambient=(.1, .3, .2)))
WORKLOADS = (("64 frames, 2 x 2 samples", 1), ("16 frames, 2 x 2 samples, 4 records each", 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "scene_light_views_rate needs a GPU"
    base, scenes = moving_scenes()
    nl = len(base.lights())
    grid = SAMPLES * SIDE
    leaves, total = grid * grid, RECORDS * grid * grid
    q = gpu.Renderer(0, specialize=4)
    q.prepare(base)
    handle = q.next_stream()
    stream = torch.cuda.ExternalStream(handle)
    progs = [sc.flatten() for sc in scenes]
    base_looks = [base.with_look(**look) for look in LOOKS]
    look_progs = [look_of(sc, base_looks[rec % 2]).flatten() for rec, sc in enumerate(scenes)]
    fc = base.frame_camera(SIDE, SIDE)          # (the same bits for the 128 x 128 frame and its 256 x 256 sample grid)
    zeros = lambda count: torch.zeros(count, dtype=torch.int32, device="cuda")      # noqa: E731
    factors, ids, px_leaf = zeros(4 * nl * total), zeros(total), zeros(total)
    rows = []
    for name, k in WORKLOADS:
        n_views = RECORDS // k
        px_v, px_m = zeros(n_views * SIDE * SIDE), zeros(n_views * SIDE * SIDE)
        issue = {
            "V": lambda: q.relight_scene_views_into(progs, look_progs, n_views, k, SIDE, SIDE, SAMPLES, factors_ptr=factors.data_ptr(),
                                                    id_ptr=ids.data_ptr(), pixel_ptr=px_v.data_ptr(), stream=handle),
            "R": lambda: q.relight_scenes_into(progs, look_progs, leaves, factors_ptr=factors.data_ptr(), id_ptr=ids.data_ptr(),
                                               pixel_ptr=px_leaf.data_ptr(), stream=handle),
            "M": lambda: q.render_scene_views_into(px_m.data_ptr(), [fc] * RECORDS, look_progs, SIDE, SIDE, k, MAX_STEPS, stream=handle,
                                                   samples=SAMPLES),
            "C": lambda: q.light_scene_pixels_into(progs, leaves, grid, grid, 0, MAX_STEPS, factors_ptr=factors.data_ptr(), id_ptr=ids.data_ptr(),
                                                   stream=handle, cameras=[fc] * RECORDS),
        }
        # the answers first: the resolve of the captured leaves is the march of the looks, byte for byte
        issue["C"]()
        issue["V"]()
        issue["M"]()
        q.sync()
        torch.cuda.synchronize()
        assert torch.equal(px_v, px_m), f"{name}: the relit scene views are not the frames of the looks"
        distinct = len({row.tobytes() for row in px_v.view(n_views, -1).cpu().numpy()})
        assert distinct > n_views // 2, "the views are alike"
        arms = list(issue)
        reps = {}
        for a in arms:                                            # warm-up, and the repeats
            window(torch, stream, issue[a], 2)
            ms = window(torch, stream, issue[a], 2)
            reps[a] = max(1, math.ceil(args.window_s * 1e3 / (ms / 2)))
        dev = {a: [] for a in arms}
        for _ in range(args.windows):
            for a in arms:                                        # alternating
                dev[a].append(window(torch, stream, issue[a], reps[a]) / reps[a])
        row = {"workload": name, "views": n_views, "records_per_view": k, "samples": SAMPLES, "elements": total, "lights": nl,
               "pixels_equal_v_m": True, "distinct_views": distinct, "arms": {}}
        for a in arms:
            med = statistics.median(dev[a])
            row["arms"][a] = {"median_ms": round(med, 4), "min_ms": round(min(dev[a]), 4), "max_ms": round(max(dev[a]), 4),
                              "windows": len(dev[a]), "repeats_per_window": reps[a]}
        m = {a: row["arms"][a]["median_ms"] for a in arms}
        row["v_over_r"], row["m_over_v"] = round(m["V"] / m["R"], 3), round(m["M"] / m["V"], 2)
        row["looks_to_beat_the_march"] = math.floor(m["C"] / (m["M"] - m["V"])) + 1 if m["M"] > m["V"] else None
        # what V must read and write at the least: an id and nl factors per leaf, a packed pixel per pixel
        row["v_bytes"] = total * (4 + 16 * nl) + n_views * SIDE * SIDE * 4
        row["v_gbytes_per_s"] = round(row["v_bytes"] / m["V"] / 1e6, 1)
        rows.append(row)
    doc = {"tool": "scene_light_views_rate", "device": torch.cuda.get_device_name(0), "scene": "scene4", "records": RECORDS, "frame": [SIDE, SIDE],
           "windows": args.windows, "window_s": args.window_s, "unit": "ms per call", "max_steps": MAX_STEPS,
           "arms_are": {"V": "one relight_scene_views_into over the 64 records' leaves, a look per record",
                        "R": "one relight_scenes_into over the same elements and looks: a pixel per leaf, no averaging",
                        "M": "one render_scene_views_into(looks, samples=2, cameras_per_view=K): the march V replaces",
                        "C": "one light_scene_pixels_into over the 64 sample grids"},
           "results": rows, "kernel_key": q.kernel_key()}
    q.close()
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
