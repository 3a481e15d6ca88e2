"""What a ray query costs (lol_gpu_trace_pixels) beside the frame that holds the same rays.  scene4 and scene.lol at 1920x1080 under
the scene's own camera; every arm on the scene's own kernels, all three exact step skips on.  Arms, ALTERNATING in one process,
every arm warmed up first:
    A  the plain frame (render_into, the default tile order: a still view goes through the longest-first tables)
    B  trace_pixels_into over the same pixels listed row-major: a wave's 64 rays are a 64 x 1 strip of the frame
    C  the same pixels listed tile by tile: a wave's 64 rays are the 16 x 4 patch a frame's wave has
B and C take the primary march and the four normal taps of every pixel and none of its shadow marches: a strict subset of A's
SDF evaluations.  They write 24 bytes per ray (dist, id, steps, normal) where A writes 4.
A window repeats its call until it lasts at least --window-s; HIP events around the window; --windows windows per arm, median and
range recorded, in milliseconds per frame's worth of rays.  The step counts that explain the arms' relation come from one frame
with lol_gpu_debug.steps: march steps (what B and C pay, plus 4 taps a ray) and shadow steps (what only A pays).

Also: the wall time of pick() against the alternative it replaces — a whole frame with hit_id and hit_dist planes and the copy of
one element of each.  One JSON document on stdout (or --out FILE).

    python tools/ray_rate.py --out profiles/r13_ray_rate.json                                               (on the GPU box)
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from loltracer_amd import gpu, scene as S  # noqa: E402


def window(torch, stream, issue, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        issue()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def pixel_lists(w, h):
    """(row-major, tile by tile): every pixel of the frame once, as uint32 pairs; the second in 16 x 4 patches, patches row by row
    (the frame's edge patches are cut, so their waves hold parts of two patches: 1080 is a multiple of 4, 1920 of 16)"""
    ys, xs = np.mgrid[0:h, 0:w]
    rows = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)
    order = np.lexsort((xs.ravel() % 16, ys.ravel() % 4, xs.ravel() // 16, ys.ravel() // 4))
    return rows, rows[order]


def measure(torch, sc, name, w, h, args):
    r = gpu.Renderer(0)
    r.set_ray_queries(True)
    r.prepare(sc)
    assert r.kernel_name() == "lol_render_spec" and r.trace_kernel_name() == "lol_trace_spec", r.specialize_log()
    assert r.miss_skip_active() == 7, r.miss_skip_active()
    handle = r.next_stream()
    stream = torch.cuda.ExternalStream(handle)
    n = w * h
    frame = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    lists = [torch.from_numpy(a.view(np.int32).copy()).to("cuda") for a in pixel_lists(w, h)]
    dist = torch.zeros(n, dtype=torch.float32, device="cuda")
    hid, steps = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    normal = torch.zeros(3 * n, dtype=torch.float32, device="cuda")
    out = dict(dist_ptr=dist.data_ptr(), id_ptr=hid.data_ptr(), steps_ptr=steps.data_ptr(), normal_ptr=normal.data_ptr())
    issue = {
        "A": lambda: r.render_into(frame.data_ptr(), w, h, 256, stream=handle),
        "B": lambda: r.trace_pixels_into(lists[0].data_ptr(), n, w, h, 256, stream=handle, **out),
        "C": lambda: r.trace_pixels_into(lists[1].data_ptr(), n, w, h, 256, stream=handle, **out),
    }
    arms = "ABC"
    reps = {}
    for a in arms:                                        # warm-up (A: until the frame goes through its tables), and the repeats
        window(torch, stream, issue[a], 6)
        ms = window(torch, stream, issue[a], 4)
        reps[a] = max(1, math.ceil(args.window_s * 1e3 / (ms / 4)))
    dev = {a: [] for a in arms}
    for _ in range(args.windows):
        for a in arms:                                    # alternating
            dev[a].append(window(torch, stream, issue[a], reps[a]) / reps[a])
    row = {"scene": name, "w": w, "h": h, "rays": n, "arms": {}}
    for a in arms:
        med = statistics.median(dev[a])
        row["arms"][a] = {"median_ms": round(med, 4), "min_ms": round(min(dev[a]), 4), "max_ms": round(max(dev[a]), 4),
                          "windows": len(dev[a]), "repeats_per_window": reps[a], "mrays_per_s": round(n / med / 1e3, 1)}
    a_ms = row["arms"]["A"]["median_ms"]
    row["b_over_a"], row["c_over_a"] = round(row["arms"]["B"]["median_ms"] / a_ms, 4), round(row["arms"]["C"]["median_ms"] / a_ms, 4)
    row["b_over_c"] = round(row["arms"]["B"]["median_ms"] / row["arms"]["C"]["median_ms"], 4)
    # what the arms evaluate: one frame with the step counters
    dsteps = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    r.render_into(frame.data_ptr(), w, h, 256, debug=gpu.Debug(None, None, None, dsteps.data_ptr()), stream=handle)
    r.sync()
    st = dsteps.cpu().numpy().view(np.uint32)
    march, shadow = int((st & 0xFFFF).sum()), int((st >> 16).sum())
    hits = int((hid.cpu().numpy() != 0).sum())
    row["evaluations"] = {"march_steps": march, "shadow_steps": shadow, "normal_taps_of_a_query": 4 * n, "rays_that_hit": hits,
                          "query_over_frame": round((march + 4 * n) / (march + shadow + 4 * hits), 4)}
    row["bytes_written_per_ray"] = {"A": 4, "B": 24, "C": 24}
    # pick() against the frame it replaces
    xy = (w // 2, h // 2)
    ddist, did = torch.zeros((h, w), dtype=torch.float32, device="cuda"), torch.zeros((h, w), dtype=torch.int32, device="cuda")
    dbg = gpu.Debug(None, ddist.data_ptr(), did.data_ptr(), None)

    def by_frame():
        r.render_into(frame.data_ptr(), w, h, 256, debug=dbg, stream=handle)
        r.sync()
        return float(ddist[xy[1], xy[0]].item()), int(did[xy[1], xy[0]].item())

    def by_pick():
        p = r.pick(xy[0], xy[1], w, h)
        return p["dist"], p["id"]

    assert by_frame() == by_pick()
    wall = {"pick": [], "frame": []}
    for _ in range(args.windows * 3):
        for k, f in (("pick", by_pick), ("frame", by_frame)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    row["pick"] = {"pixel": list(xy), "pick_wall_ms": round(statistics.median(wall["pick"]), 4),
                   "frame_with_planes_and_copy_wall_ms": round(statistics.median(wall["frame"]), 4), "calls": len(wall["pick"])}
    print(json.dumps(row), file=sys.stderr, flush=True)
    keys = {"kernel_key": r.kernel_key(), "trace_kernel": r.trace_kernel_name()}
    r.close()
    return row, keys


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--scenes", default="scene4,scene")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "ray_rate needs a GPU"
    w, h = (int(v) for v in args.size.lower().split("x"))
    doc = {"tool": "ray_rate", "device": torch.cuda.get_device_name(0), "windows": args.windows, "window_s": args.window_s,
           "unit": "ms per w h rays",
           "arms": {"A": "render_into, default tile order, skips 7", "B": "trace_pixels_into, pixels row-major (64 x 1 strips per wave)",
                    "C": "trace_pixels_into, pixels tile by tile (16 x 4 patches per wave)"},
           "rows": [], "kernel_keys": {}}
    for name in args.scenes.split(","):
        sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol"))
        row, keys = measure(torch, sc, name, w, h, args)
        doc["rows"].append(row)
        doc["kernel_keys"][name] = keys
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
