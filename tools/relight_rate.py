"""What a new LOOK costs through lol_gpu_relight beside the frame it replaces.  scene4 at 3840x2160 and scene.lol at 1920x1080 under
the scene's own camera, all exact skips on, default tile order.  The light passes of every pixel are captured once (light_pixels_into);
the look changes the lights' intensities and the ambient colour.  Arms, ALTERNATING in one process, every arm warmed up first:
    R1      relight_into(look), pixel output alone
    R3      relight_into(look), rgb_linear, rgb and pixel
    F       render_into on a second context that uploaded the look: the cheapest way to a frame of a look without this feature,
            once the upload is paid
and, once each (a few windows, not alternated with the arms above):
    U       upload_program(look) + render_into + sync on a third context, two looks in turn, WALL clock: what a new look costs
            today (the scene's module comes from the code-object cache after the first upload of each look)
    L       light_pixels_into of every pixel: the capture
    S       shade_pixels_into of the same pixels (row-major list) on the capturing context, pixel output
    P       render_into on the capturing context: the plain frame
A window repeats its call until it lasts at least --window-s; HIP events around the window; --windows windows per arm, median and
range recorded, in milliseconds per call.  Bytes per look are computed from the shapes — per element 4 (hit_id) + 16 n_lights read
and 4 (pixel) or 28 (all three) written — and the achieved GB/s is set against the 6290 GB/s the micro-architecture guide quotes for
a float4 copy.  One JSON document on stdout (or --out FILE).

    python tools/relight_rate.py --out profiles/r20_relight_rate.json                                       (on the GPU box)
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from loltracer_amd import gpu, scene as S  # noqa: E402
from ray_rate import pixel_lists, window  # noqa: E402

COPY_GBPS = 6290.0


def summary(ms, reps, n):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "windows": len(ms),
            "repeats_per_window": reps, "mpixels_per_s": round(n / med / 1e3, 1)}


def measure(torch, sc, name, w, h, args):
    nl, n = len(sc.lights()), w * h
    looks = [sc.with_look(lights=[((2.5, 1.0, 0.5), (0.5, 1.0, 2.5))] * nl, ambient=(0.06, 0.03, 0.02)),
             sc.with_look(lights=[((0.5, 1.5, 3.0), (1.0, 1.0, 1.0))] * nl, ambient=(0.02, 0.04, 0.08))]
    progs = [l.flatten() for l in looks]
    r, r2, r3 = gpu.Renderer(0), gpu.Renderer(0), gpu.Renderer(0)
    r.prepare(sc)
    r2.prepare(looks[0])
    r3.prepare(looks[1])
    for q in (r, r2, r3):
        assert q.kernel_name() == "lol_render_spec" and q.miss_skip_active() == 7, q.specialize_log()
    handle = r.next_stream()
    stream = torch.cuda.ExternalStream(handle)
    h2 = r2.next_stream()
    stream2 = torch.cuda.ExternalStream(h2)
    factors = torch.zeros(max(1, 4 * n * nl), dtype=torch.int32, device="cuda")
    hid = torch.zeros(n, dtype=torch.int32, device="cuda")
    px, frame = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros((h, w), dtype=torch.int32, device="cuda")
    lin, rgb = (torch.zeros(3 * n, dtype=torch.float32, device="cuda") for _ in range(2))
    rows = torch.from_numpy(pixel_lists(w, h)[0].view(np.int32).copy()).to("cuda")
    planes = dict(factors_ptr=factors.data_ptr() if nl else 0, id_ptr=hid.data_ptr())
    capture = lambda: r.light_pixels_into(n, w, h, 256, stream=handle, **planes)      # noqa: E731
    capture()
    r.sync()
    # the relit frame is the frame of the context that uploaded the look: pixel for pixel
    r.relight_into(progs[0], n, pixel_ptr=px.data_ptr(), stream=handle, **planes)
    r2.render_into(frame.data_ptr(), w, h, 256, stream=h2)
    r.sync()
    r2.sync()
    torch.cuda.synchronize()
    assert torch.equal(frame.ravel(), px), "the relit frame is not the frame of the look"
    issue = {
        "R1": (stream, lambda: r.relight_into(progs[0], n, pixel_ptr=px.data_ptr(), stream=handle, **planes)),
        "F": (stream2, lambda: r2.render_into(frame.data_ptr(), w, h, 256, stream=h2)),
        "R3": (stream, lambda: r.relight_into(progs[0], n, rgb_linear_ptr=lin.data_ptr(), rgb_ptr=rgb.data_ptr(), pixel_ptr=px.data_ptr(),
                                              stream=handle, **planes)),
    }
    once = {
        "L": (stream, capture),
        "S": (stream, lambda: r.shade_pixels_into(rows.data_ptr(), n, w, h, 256, pixel_ptr=px.data_ptr(), stream=handle)),
        "P": (stream, lambda: r.render_into(frame.data_ptr(), w, h, 256, stream=handle)),
    }
    reps = {}
    for a, (st, call) in {**issue, **once}.items():       # warm-up, and the repeats
        window(torch, st, call, 6)
        ms = window(torch, st, call, 4)
        reps[a] = max(1, math.ceil(args.window_s * 1e3 / (ms / 4)))
    dev = {a: [] for a in {**issue, **once}}
    for _ in range(args.windows):
        for a, (st, call) in issue.items():               # alternating
            dev[a].append(window(torch, st, call, reps[a]) / reps[a])
    for a, (st, call) in once.items():
        for _ in range(3):
            dev[a].append(window(torch, st, call, reps[a]) / reps[a])
    wall = []
    for k in range(2 + 2 * args.upload_reps):             # (the first two uploads fill the code-object cache: not recorded)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r3.upload_program(progs[k % 2], wait=True)
        r3.render_into(frame.data_ptr(), w, h, 256)
        r3.sync()
        if k >= 2:
            wall.append((time.perf_counter() - t0) * 1e3)
    row = {"scene": name, "w": w, "h": h, "pixels": n, "lights": nl, "arms": {a: summary(dev[a], reps[a], n) for a in dev}}
    row["arms"]["U"] = {"median_ms": round(statistics.median(wall), 3), "min_ms": round(min(wall), 3), "max_ms": round(max(wall), 3),
                        "calls": len(wall), "clock": "wall"}
    read = n * (4 + 16 * nl)
    row["bytes_per_look"] = {"R1": read + 4 * n, "R3": read + 28 * n}
    for a in ("R1", "R3"):
        gbps = row["bytes_per_look"][a] / row["arms"][a]["median_ms"] / 1e6
        row["arms"][a]["gbytes_per_s"] = round(gbps, 1)
        row["arms"][a]["of_float4_copy"] = round(gbps / COPY_GBPS, 4)
        row["arms"][a]["ms_at_float4_copy_rate"] = round(row["bytes_per_look"][a] / COPY_GBPS / 1e6, 4)
    f = row["arms"]["F"]["median_ms"]
    row["r1_over_f"] = round(row["arms"]["R1"]["median_ms"] / f, 4)
    row["r3_over_f"] = round(row["arms"]["R3"]["median_ms"] / f, 4)
    row["u_over_f"] = round(row["arms"]["U"]["median_ms"] / f, 2)
    row["l_over_p"] = round(row["arms"]["L"]["median_ms"] / row["arms"]["P"]["median_ms"], 4)
    row["l_over_s"] = round(row["arms"]["L"]["median_ms"] / row["arms"]["S"]["median_ms"], 4)
    row["capture_bytes_written"] = n * (4 + 16 * nl)
    print(json.dumps(row), file=sys.stderr, flush=True)
    keys = {"kernel_key": r.kernel_key(), "shade_kernel": r.shade_kernel_name(), "interp_variant": list(r.interp_variant())}
    for q in (r, r2, r3):
        q.close()
    return row, keys


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--upload-reps", type=int, default=4)
    ap.add_argument("--cases", default="scene4:3840x2160,scene:1920x1080")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "relight_rate needs a GPU"
    doc = {"tool": "relight_rate", "device": torch.cuda.get_device_name(0), "windows": args.windows, "window_s": args.window_s,
           "unit": "ms per call over w h elements", "float4_copy_gbytes_per_s": COPY_GBPS,
           "arms": {"R1": "relight_into(look), pixel alone", "R3": "relight_into(look), rgb_linear + rgb + pixel",
                    "F": "render_into on a context that uploaded the look (scene's own kernel, default tile order, skips 7)",
                    "U": "upload_program(look) + render_into + sync, two looks in turn, wall clock",
                    "L": "light_pixels_into, every pixel (light_interp): factors + hit_id",
                    "S": "shade_pixels_into, the same pixels row-major, pixel output (the capturing context's shading kernel)",
                    "P": "render_into on the capturing context"},
           "rows": [], "kernel_keys": {}}
    for case in args.cases.split(","):
        name, size = case.split(":")
        w, h = (int(v) for v in size.lower().split("x"))
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
