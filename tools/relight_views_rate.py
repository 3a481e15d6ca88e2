"""What an AVERAGED frame of a new look costs through lol_gpu_relight_views beside the render it replaces, and what the new kernel's
lane mapping (one lane per sample, butterfly over a pixel's samples, cameras looped in the lane) achieves beside the parent's
relight_rays over the same elements.  Each case is one view under the scene's own camera (K = 1) or a lens round it (K > 1), all exact
skips on.  The light passes of every leaf are captured once (light_views_into: K captures of the s w x s h frame); the look changes
the lights' intensities and the ambient colour.  Before anything is timed the relit view is checked pixel for pixel against the
render of a context that uploaded the look.  Arms, ALTERNATING in one process, every arm warmed up first:
    V       relight_views_into(look), pixel output alone: N leaves read, w h pixels written
    R       relight_into(look) over the same N elements, pixel output alone: the parent's kernel reading the same bytes (and writing
            4 N more) — the yardstick for the new kernel's bandwidth
    F       the supersampled frame (K = 1: render_into after set_samples(s)) or blend (K > 1: render_blended_views_into(..., samples=s))
            on a second context that uploaded the look, its scene module carrying that form
and, once each (a few windows, not alternated with the arms above):
    U       upload_program(look) + that render + sync on a third context, two looks in turn, WALL clock
    L       light_views_into of every leaf: the capture, K launches
    P       light_pixels_into of the plain w x h frame: one plain capture (the capture's cost is about s^2 K of these)
A window repeats its call until it lasts at least --window-s; HIP events around the window; --windows windows per arm, median and
range recorded, in milliseconds per call.  Algorithmic traffic per call: N (4 + 16 n_lights) bytes read and 4 per pixel (V) or per
element (R) written; GB/s from it.  One JSON document on stdout (or --out FILE).

    python tools/relight_views_rate.py --out profiles/r22_relight_views_rate.json                           (on the GPU box)
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from loltracer_amd import gpu, scene as S  # noqa: E402
from ray_rate import window  # noqa: E402

COPY_GBPS = 6290.0
LENS_FOCUS, LENS_RADIUS = 6.0, 0.25
CASES = "scene4:1920x1080:2:1,scene4:1920x1080:4:1,scene4:1920x1080:2:4,scene:1920x1080:2:1"


def summary(ms, reps):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "windows": len(ms), "repeats_per_window": reps}


def look_renderer(look, s, k):
    """a context that uploaded the look, its scene module carrying the form the case renders"""
    r = gpu.Renderer(0)
    if k == 1:
        r.set_samples(s)
    elif s > 1:
        r.set_view_blend_samples(True)
    else:
        r.set_view_blends(True)
    r.prepare(look)
    return r


def measure(torch, sc, name, w, h, s, k, args):
    nl, n_px = len(sc.lights()), w * h
    n = k * s * s * n_px
    looks = [sc.with_look(lights=[((2.5, 1.0, 0.5), (0.5, 1.0, 2.5))] * nl, ambient=(0.06, 0.03, 0.02)),
             sc.with_look(lights=[((0.5, 1.5, 3.0), (1.0, 1.0, 1.0))] * nl, ambient=(0.02, 0.04, 0.08))]
    progs = [l.flatten() for l in looks]
    cams = S.lens_cameras(sc.camera, LENS_FOCUS, LENS_RADIUS, k)
    r = gpu.Renderer(0)
    r.prepare(sc)
    r2, r3 = look_renderer(looks[0], s, k), look_renderer(looks[1], s, k)
    for q in (r, r2, r3):
        assert q.miss_skip_active() == 7, q.specialize_log()
    handle, h2 = r.next_stream(), r2.next_stream()
    stream, stream2 = torch.cuda.ExternalStream(handle), torch.cuda.ExternalStream(h2)
    factors = torch.zeros(max(1, 4 * n * nl), dtype=torch.int32, device="cuda")
    hid = torch.zeros(n, dtype=torch.int32, device="cuda")
    px, frame = torch.zeros(n_px, dtype=torch.int32, device="cuda"), torch.zeros((h, w), dtype=torch.int32, device="cuda")
    leaves = torch.zeros(n, dtype=torch.int32, device="cuda")
    one = dict(factors=torch.zeros(max(1, 4 * n_px * nl), dtype=torch.int32, device="cuda"), hid=torch.zeros(n_px, dtype=torch.int32, device="cuda"))
    planes = dict(factors_ptr=factors.data_ptr() if nl else 0, id_ptr=hid.data_ptr())
    capture = lambda: r.light_views_into(cams, k, w, h, s, 256, stream=handle, **planes)      # noqa: E731

    def render(q, st):
        if k == 1:
            q.render_into(frame.data_ptr(), w, h, 256, stream=st)
        else:
            q.render_blended_views_into(frame.data_ptr(), cams, k, w, h, 256, stream=st, samples=s)

    torch.cuda.synchronize()              # torch's fills run on ITS stream; everything below on the renderers' own
    capture()
    r.sync()
    # the relit view is the view of the context that uploaded the look: pixel for pixel
    r.relight_views_into(progs[0], 1, k, w, h, s, pixel_ptr=px.data_ptr(), stream=handle, **planes)
    render(r2, h2)
    r.sync()
    r2.sync()
    torch.cuda.synchronize()
    assert torch.equal(frame.ravel(), px), "the relit view is not the view of the look"
    issue = {
        "V": (stream, lambda: r.relight_views_into(progs[0], 1, k, w, h, s, pixel_ptr=px.data_ptr(), stream=handle, **planes)),
        "R": (stream, lambda: r.relight_into(progs[0], n, pixel_ptr=leaves.data_ptr(), stream=handle, **planes)),
        "F": (stream2, lambda: render(r2, h2)),
    }
    once = {
        "L": (stream, capture),
        "P": (stream, lambda: r.light_pixels_into(n_px, w, h, 256, factors_ptr=one["factors"].data_ptr() if nl else 0,
                                                  id_ptr=one["hid"].data_ptr(), stream=handle)),
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
    for i in range(2 + 2 * args.upload_reps):             # (the first two uploads fill the code-object cache: not recorded)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r3.upload_program(progs[i % 2], wait=True)
        render(r3, None)
        r3.sync()
        if i >= 2:
            wall.append((time.perf_counter() - t0) * 1e3)
    row = {"scene": name, "w": w, "h": h, "samples": s, "cameras_per_view": k, "pixels": n_px, "elements": n, "lights": nl,
           "arms": {a: summary(dev[a], reps[a]) for a in dev}}
    row["arms"]["U"] = {"median_ms": round(statistics.median(wall), 3), "min_ms": round(min(wall), 3), "max_ms": round(max(wall), 3),
                        "calls": len(wall), "clock": "wall"}
    read = n * (4 + 16 * nl)
    row["bytes_per_call"] = {"V": read + 4 * n_px, "R": read + 4 * n}
    for a in ("V", "R"):
        gbps = row["bytes_per_call"][a] / row["arms"][a]["median_ms"] / 1e6
        row["arms"][a]["gbytes_per_s"] = round(gbps, 1)
        row["arms"][a]["of_float4_copy"] = round(gbps / COPY_GBPS, 4)
    A = {a: row["arms"][a]["median_ms"] for a in row["arms"]}
    row["v_over_r"] = round(A["V"] / A["R"], 4)
    row["v_over_f"] = round(A["V"] / A["F"], 4)
    row["u_over_f"] = round(A["U"] / A["F"], 2)
    row["l_over_p"] = round(A["L"] / A["P"], 2)
    row["plain_captures_in_the_capture"] = s * s * k
    # looks after which capture + relights is cheaper than rendering each look (F), and than uploading and rendering each (U)
    row["break_even_looks"] = {"against_F": math.ceil(A["L"] / (A["F"] - A["V"])) if A["F"] > A["V"] else None,
                               "against_U": math.ceil(A["L"] / (A["U"] - A["V"])) if A["U"] > A["V"] else None}
    print(json.dumps(row), file=sys.stderr, flush=True)
    keys = {"kernel_key": r.kernel_key(), "render_kernel": r2.kernel_name() if k == 1 else r2.view_blend_samples_kernel_name(k, s) if s > 1
            else r2.view_blend_kernel_name(k), "interp_variant": list(r.interp_variant())}
    for q in (r, r2, r3):
        q.close()
    return row, keys


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--upload-reps", type=int, default=4)
    ap.add_argument("--cases", default=CASES, help="scene:WxH:samples:cameras, comma-separated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "relight_views_rate needs a GPU"
    doc = {"tool": "relight_views_rate", "device": torch.cuda.get_device_name(0), "windows": args.windows, "window_s": args.window_s,
           "unit": "ms per call", "float4_copy_gbytes_per_s": COPY_GBPS,
           "lane_mapping": "one lane per sample: lane = group * s^2 + (j s + i), xor butterfly over the lane bits of the sample, the K cameras "
                           "looped in the lane with a pairwise accumulator; a wave takes its 64 pixels in s^2 rounds and lane (group, k) keeps the "
                           "pixel of round k, so the divisions, gamma, packing and stores run once per pixel (one lane per pixel was not built)",
           "arms": {"V": "relight_views_into(look), pixel alone (relight_views)",
                    "R": "relight_into(look) over the same N elements, pixel alone (relight_rays, the parent's kernel)",
                    "F": "the supersampled frame or blend on a context that uploaded the look (its module carries the form, skips 7)",
                    "U": "upload_program(look) + that render + sync, two looks in turn, wall clock",
                    "L": "light_views_into, every leaf: K launches of light_interp",
                    "P": "light_pixels_into of the plain w x h frame"},
           "rows": [], "kernel_keys": {}}
    for case in args.cases.split(","):
        name, size, s, k = case.split(":")
        w, h = (int(v) for v in size.lower().split("x"))
        sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol"))
        row, keys = measure(torch, sc, name, w, h, int(s), int(k), args)
        doc["rows"].append(row)
        doc["kernel_keys"][case] = keys
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
