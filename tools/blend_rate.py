"""What averaging over cameras costs (lol_gpu_render_views_blend): n views of K cameras each against the same n K rays without the
averaging.  scene4 and scene.lol; 64 views of 128x128 with K = 4 and K = 16, one view of 1920x1080 with K = 8; shutter cameras
between neighbours of an orbit (scene.shutter_cameras).  Arms, ALTERNATING in one process, every shape warmed up first:
    A  one render_views_into of the n K cameras: the same rays, packed per ray, no averaging (code blends do not touch)
    B  one render_blended_views_into: the linear pass over the n K cameras and the resolve pass
    C  the host-side alternative: n K calls of render_into on one stream, fixed row order (the average would still be the host's)
A window repeats its call until it lasts at least --window-s; HIP events around the window; --windows windows per arm, median and
range recorded, in milliseconds per n views.  B may exceed A by A's own spread between windows plus the resolve pass; the resolve
pass's time comes from kernel traces of runs of their own (--kernel-trace SCENE=FILE,...: rocprofv3's CSV of a short run of arms A
and B on that scene alone), which also give the two render kernels' own durations: the linear kernel of B beside the batch kernel
of A.  One JSON document on stdout (or --out FILE).

    rocprofv3 --kernel-trace --stats --output-format csv -d out -o scene4 -- python tools/blend_rate.py --scenes scene4 --arms AB \
        --windows 1 --window-s 0.02                                                        (and the same for scene)
    python tools/blend_rate.py --kernel-trace scene4=out/scene4_kernel_trace.csv,scene=out/scene_kernel_trace.csv \
        --out profiles/r11_blend_rate.json                                                                    (on the GPU box)
"""
import argparse
import csv
import json
import math
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from loltracer_amd import gpu, scene as S  # noqa: E402

SHAPES = "128x128x64x4,128x128x64x16,1920x1080x1x8"


def window(torch, stream, issue, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        issue()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def trace_times(path):
    """{(kernel, z): (median microseconds per dispatch, dispatches)} from a rocprofv3 kernel-trace CSV, z = the grid's third
    dimension, for kernel in 'resolve<K>' (blend_resolve), 'lin' (lol_render_spec_batch_lin) and 'batch' (lol_render_spec_batch)"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            m = re.search(r"blend_resolve<(\d+)>", name)
            base = re.sub(r"\.kd$", "", name.strip())
            kind = "resolve<%s>" % m.group(1) if m else {"lol_render_spec_batch_lin": "lin", "lol_render_spec_batch": "batch"}.get(base)
            if kind:
                out.setdefault((kind, int(row["Grid_Size_Z"])), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: (statistics.median(v), len(v)) for k, v in out.items()}


def measure(torch, sc, name, shapes, arms, args, resolve):
    plain = gpu.Renderer(0)
    plain.set_view_batches(True)
    plain.prepare(sc)
    plain.set_tile_order("rows")
    blend = gpu.Renderer(0)
    blend.set_view_blends(True)
    blend.prepare(sc)
    assert plain.kernel_name() == "lol_render_spec" and blend.view_blend_kernel_name(2) == "lol_render_spec_batch_lin", blend.specialize_log()
    handles = {"A": plain.next_stream(), "B": blend.next_stream()}
    handles["C"] = handles["A"]
    streams = {a: torch.cuda.ExternalStream(h) for a, h in handles.items()}
    rows = []
    for (w, h, n, k) in shapes:
        orbit = S.orbit_cameras(sc, max(8, n))
        cams = []
        for v in range(n):
            cams += S.shutter_cameras(orbit[v % len(orbit)], orbit[(v + 1) % len(orbit)], k)
        fcs = [sc.frame_camera(w, h, c) for c in cams]
        rays = torch.zeros((n * k, h, w), dtype=torch.int32, device="cuda")
        views = torch.zeros((n, h, w), dtype=torch.int32, device="cuda")
        issue = {
            "A": lambda: plain.render_views_into(rays.data_ptr(), fcs, w, h, 256, stream=handles["A"]),
            "B": lambda: blend.render_blended_views_into(views.data_ptr(), fcs, k, w, h, 256, stream=handles["B"]),
            "C": lambda: [plain.render_into(rays[i].data_ptr(), w, h, 256, stream=handles["C"], frame_camera=fc) for i, fc in enumerate(fcs)],
        }
        reps = {}
        for a in arms:                                    # warm-up, and how often a window repeats its call
            window(torch, streams[a], issue[a], 1)
            ms = window(torch, streams[a], issue[a], 2)
            reps[a] = max(1, math.ceil(args.window_s * 1e3 / (ms / 2)))
        dev = {a: [] for a in arms}
        for _ in range(args.windows):
            for a in arms:                                # alternating
                dev[a].append(window(torch, streams[a], issue[a], reps[a]) / reps[a])
        row = {"scene": name, "w": w, "h": h, "views": n, "cameras_per_view": k, "arms": {}}
        for a in arms:
            med = statistics.median(dev[a])
            row["arms"][a] = {"median_ms": round(med, 4), "min_ms": round(min(dev[a]), 4), "max_ms": round(max(dev[a]), 4),
                              "windows": len(dev[a]), "repeats_per_window": reps[a],
                              "mrays_per_s": round(n * k * w * h / med / 1e3, 1)}
        if ("resolve<%d>" % k, n) in resolve:
            row["resolve_us"], row["resolve_dispatches"] = round(resolve[("resolve<%d>" % k, n)][0], 2), resolve[("resolve<%d>" % k, n)][1]
        for kind in ("lin", "batch"):                     # the render kernels of B and A: n K frames in the grid's z
            if (kind, n * k) in resolve:
                row[kind + "_kernel_us"], row[kind + "_kernel_dispatches"] = round(resolve[(kind, n * k)][0], 2), resolve[(kind, n * k)][1]
        if "A" in arms and "B" in arms:
            a, b = row["arms"]["A"], row["arms"]["B"]
            row["b_minus_a_ms"] = round(b["median_ms"] - a["median_ms"], 4)
            row["b_over_a"] = round(b["median_ms"] / a["median_ms"], 4)
            row["a_spread_ms"] = round(a["max_ms"] - a["min_ms"], 4)
            if "resolve_us" in row:
                row["allowed_excess_ms"] = round(row["a_spread_ms"] + row["resolve_us"] / 1e3, 4)
                row["within_allowed_excess"] = bool(row["b_minus_a_ms"] <= row["allowed_excess_ms"])
        if "B" in arms and "C" in arms:
            row["b_over_c"] = round(row["arms"]["B"]["median_ms"] / row["arms"]["C"]["median_ms"], 4)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del rays, views, issue
        torch.cuda.empty_cache()
    keys = {"batch_module_kernel_key": plain.kernel_key(), "blend_module_kernel_key": blend.kernel_key()}
    plain.close()
    blend.close()
    return rows, keys


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--scenes", default="scene4,scene")
    ap.add_argument("--shapes", default=SHAPES, help="WxHxVIEWSxK,...")
    ap.add_argument("--arms", default="ABC")
    ap.add_argument("--kernel-trace", default=None, help="SCENE=FILE,... (or one FILE for all scenes): rocprofv3 kernel-trace CSVs of runs of arms A and B")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "blend_rate needs a GPU"
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    # SCENE=FILE per scene; a bare FILE is a trace of every scene (arm B alone): the resolve pass's time only, since the scenes'
    # render kernels have equal grids and cannot be told apart in it
    traces = dict(item.split("=", 1) if "=" in item else ("*", item) for item in args.kernel_trace.split(",")) if args.kernel_trace else {}
    resolve = {name: trace_times(path) for name, path in traces.items()}
    if "*" in resolve:
        resolve["*"] = {k: v for k, v in resolve["*"].items() if k[0].startswith("resolve")}
    doc = {"tool": "blend_rate", "device": torch.cuda.get_device_name(0), "windows": args.windows, "window_s": args.window_s,
           "unit": "ms per n views of K cameras",
           "arms": {"A": "1 x render_views_into of the n K cameras (no averaging)", "B": "1 x render_blended_views_into",
                    "C": "n K x render_into, one stream, rows (no averaging)"},
           "trace_source": "rocprofv3 --kernel-trace of arms A and B, one run per scene, median per dispatch" if resolve else None,
           "rows": [], "kernel_keys": {}}
    for name in args.scenes.split(","):
        sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol"))
        rows, keys = measure(torch, sc, name, shapes, args.arms, args, resolve.get(name, resolve.get("*", {})))
        doc["rows"] += rows
        doc["kernel_keys"][name] = keys
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
