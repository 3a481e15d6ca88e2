"""What averaging over cameras costs a SUPERSAMPLED batch (lol_gpu_render_views_blend_samples): n views of K cameras with s x s
samples each against the same n K supersampled frames without the camera averaging.  The method of tools/blend_rate.py.  scene4
and scene.lol; 64 views of 128x128 with K = 4, 16 views of 128x128 with K = 16, one view of 1920x1080 with K = 8, all with s = 2;
shutter cameras between neighbours of an orbit (scene.shutter_cameras).  Arms, ALTERNATING in one process, every shape warmed up
first:
    A  one render_views_into(..., samples=s) of the n K cameras: the same rays, reduced and packed per camera, no averaging over
       cameras (code supersampled blends do not touch)
    B  one render_blended_views_into(..., samples=s): the supersampled linear pass over the n K cameras and the resolve pass
    C  the host-side alternative: n K calls of render_into on one stream with set_samples(s), fixed row order
A window repeats its call until it lasts at least --window-s; HIP events around the window; --windows windows per arm, median and
range recorded, in milliseconds per n views.  B may exceed A by A's own spread between windows plus the resolve pass; the resolve
pass is blend_resolve<K>, the kernel of plain blends on the same amount of data, so its time is read from a kernel-stats CSV of a
plain blend (--resolve-stats, default profiles/r11_blend_kernel_stats.csv: the mean per dispatch of blend_resolve<K>, recorded for
64 x 128x128 with K = 4 and K = 16 and 1 x 1920x1080 with K = 8 — for 16 views with K = 16 that figure is an upper bound).  One JSON
document on stdout (or --out FILE).

    python tools/blend_aa_rate.py --out profiles/r12_blend_aa_rate.json                                      (on the GPU box)
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

SHAPES = "128x128x64x4x2,128x128x16x16x2,1920x1080x1x8x2"


def window(torch, stream, issue, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        issue()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def resolve_stats(path):
    """{K: mean microseconds per dispatch of blend_resolve<K>} from a rocprofv3 kernel-stats CSV"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            m = re.search(r"blend_resolve<(\d+)>", row["Name"])
            if m:
                out[int(m.group(1))] = float(row["AverageNs"]) / 1e3
    return out


def measure(torch, sc, name, shapes, arms, args, resolve):
    plain = gpu.Renderer(0)
    plain.set_samples(2)                     # (the module then carries lol_render_spec_aa, arm C's kernel)
    plain.set_view_samples(True)
    plain.prepare(sc)
    plain.set_tile_order("rows")
    blend = gpu.Renderer(0)
    blend.set_view_blend_samples(True)
    blend.prepare(sc)
    assert plain.view_samples_kernel_name(2, -1) == "lol_render_spec_batch_aa", plain.specialize_log()
    assert blend.view_blend_samples_kernel_name(2, 2) == "lol_render_spec_batch_aa_lin", blend.specialize_log()
    handles = {"A": plain.next_stream(), "B": blend.next_stream()}
    handles["C"] = handles["A"]
    streams = {a: torch.cuda.ExternalStream(h) for a, h in handles.items()}
    rows = []
    for (w, h, n, k, s) in shapes:
        plain.set_samples(s)
        orbit = S.orbit_cameras(sc, max(8, n))
        cams = []
        for v in range(n):
            cams += S.shutter_cameras(orbit[v % len(orbit)], orbit[(v + 1) % len(orbit)], k)
        fcs = [sc.frame_camera(w, h, c) for c in cams]
        rays = torch.zeros((n * k, h, w), dtype=torch.int32, device="cuda")
        views = torch.zeros((n, h, w), dtype=torch.int32, device="cuda")
        issue = {
            "A": lambda: plain.render_views_into(rays.data_ptr(), fcs, w, h, 256, stream=handles["A"], samples=s),
            "B": lambda: blend.render_blended_views_into(views.data_ptr(), fcs, k, w, h, 256, stream=handles["B"], samples=s),
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
        row = {"scene": name, "w": w, "h": h, "views": n, "cameras_per_view": k, "samples": s, "arms": {}}
        for a in arms:
            med = statistics.median(dev[a])
            row["arms"][a] = {"median_ms": round(med, 4), "min_ms": round(min(dev[a]), 4), "max_ms": round(max(dev[a]), 4),
                              "windows": len(dev[a]), "repeats_per_window": reps[a],
                              "mrays_per_s": round(n * k * s * s * w * h / med / 1e3, 1)}
        if k in resolve:
            row["resolve_us"] = round(resolve[k], 2)
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
    keys = {"view_samples_module_kernel_key": plain.kernel_key(), "blend_samples_module_kernel_key": blend.kernel_key()}
    plain.close()
    blend.close()
    return rows, keys


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--scenes", default="scene4,scene")
    ap.add_argument("--shapes", default=SHAPES, help="WxHxVIEWSxKxS,...")
    ap.add_argument("--arms", default="ABC")
    ap.add_argument("--resolve-stats", default=os.path.join(ROOT, "profiles", "r11_blend_kernel_stats.csv"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "blend_aa_rate needs a GPU"
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    resolve = resolve_stats(args.resolve_stats) if args.resolve_stats and os.path.exists(args.resolve_stats) else {}
    doc = {"tool": "blend_aa_rate", "device": torch.cuda.get_device_name(0), "windows": args.windows, "window_s": args.window_s,
           "unit": "ms per n views of K cameras with s x s samples",
           "arms": {"A": "1 x render_views_into(samples=s) of the n K cameras (no averaging over cameras)",
                    "B": "1 x render_blended_views_into(samples=s)",
                    "C": "n K x render_into with set_samples(s), one stream, rows (no averaging over cameras)"},
           "resolve_source": os.path.relpath(args.resolve_stats, ROOT) + ": mean per dispatch of blend_resolve<K> in a plain blend" if resolve else None,
           "rows": [], "kernel_keys": {}}
    for name in args.scenes.split(","):
        sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol"))
        rows, keys = measure(torch, sc, name, shapes, args.arms, args, resolve)
        doc["rows"] += rows
        doc["kernel_keys"][name] = keys
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
