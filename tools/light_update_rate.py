"""What bringing captured light passes to a look that MOVES LIGHTS costs beside the capture it replaces.  scene4 at 3840x2160 and
scene.lol at 1920x1080 under the scene's own camera, all exact skips on.  The look moves every light and changes every shininess but
material 0's.  Before any timing the updated planes are held, bit for bit, to a fresh capture of a context that uploaded the look.
Arms, ALTERNATING in one process, every arm warmed up first:
    C       light_pixels_into of every pixel with hit_dist: the full capture (light_interp) — the yardstick
    U1      light_update_pixels_into, light 0 marched
    Uall    light_update_pixels_into, every light marched
    S       light_update_pixels_into, specular incidence alone on every light (no shadow march)
An update writes what it reads back in the next repeat, so a window of repeats is a window of equal work.  A window repeats its call
until it lasts at least --window-s; HIP events around the window; --windows windows per arm; median and range in milliseconds per call.
One JSON document on stdout (or --out FILE).

    python tools/light_update_rate.py --out profiles/r24_light_update_rate.json                             (on the GPU box)
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

from loltracer_amd import gpu, scene as S  # noqa: E402
from ray_rate import window  # noqa: E402


def summary(ms, reps, n):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "windows": len(ms),
            "repeats_per_window": reps, "mpixels_per_s": round(n / med / 1e3, 1)}


def measure(torch, sc, name, w, h, args):
    nl, n = len(sc.lights()), w * h
    full = (1 << nl) - 1
    look = sc.with_lighting(points=[(l.point.x + 1.5, l.point.y - 0.75, l.point.z + 2.25) for l in sc.lights()],
                            shininess=[None] + [m.shininess * 0.5 + 3 for m in sc.materials()[1:]])
    prog = look.flatten()
    r, r2 = gpu.Renderer(0), gpu.Renderer(0)
    r.prepare(sc)
    r2.prepare(look)
    for q in (r, r2):
        assert q.miss_skip_active() == 7, q.specialize_log()
    handle = r.next_stream()
    stream = torch.cuda.ExternalStream(handle)
    h2 = r2.next_stream()

    def planes():
        return dict(factors=torch.zeros(4 * n * nl, dtype=torch.int32, device="cuda"), id=torch.zeros(n, dtype=torch.int32, device="cuda"),
                    dist=torch.zeros(n, dtype=torch.float32, device="cuda"))

    def ptrs(p):
        return dict(factors_ptr=p["factors"].data_ptr(), id_ptr=p["id"].data_ptr(), dist_ptr=p["dist"].data_ptr())

    pa, pb = planes(), planes()
    capture = lambda: r.light_pixels_into(n, w, h, 256, stream=handle, **ptrs(pa))      # noqa: E731
    update = lambda march, spec: r.light_update_pixels_into(prog, n, w, h, march, spec, stream=handle, **ptrs(pa))      # noqa: E731
    # the check: the updated planes are a fresh capture under the look, all 16 bytes of every element
    capture()
    r2.light_pixels_into(n, w, h, 256, stream=h2, **ptrs(pb))
    r.sync()
    r2.sync()
    for f in ("id", "dist"):
        assert torch.equal(pa[f].view(torch.int32), pb[f].view(torch.int32)), f
    assert not torch.equal(pa["factors"], pb["factors"])
    update(0, full)
    r.sync()
    fa, fb = pa["factors"].view(nl, n, 4), pb["factors"].view(nl, n, 4)
    assert torch.equal(fa[:, :, 2], fb[:, :, 2]), "specular update: the incidence is not the capture's"
    update(full, 0)
    r.sync()
    torch.cuda.synchronize()
    assert torch.equal(pa["factors"], pb["factors"]), "the updated planes are not a fresh capture under the look"
    arms = {"C": capture, "U1": lambda: update(1, 0), "Uall": lambda: update(full, 0), "S": lambda: update(0, full)}
    reps = {}
    for a, call in arms.items():                          # warm-up, and the repeats
        window(torch, stream, call, 6)
        ms = window(torch, stream, call, 4)
        reps[a] = max(1, math.ceil(args.window_s * 1e3 / (ms / 4)))
    dev = {a: [] for a in arms}
    for _ in range(args.windows):
        for a, call in arms.items():                      # alternating
            dev[a].append(window(torch, stream, call, reps[a]) / reps[a])
    row = {"scene": name, "w": w, "h": h, "pixels": n, "lights": nl, "arms": {a: summary(dev[a], reps[a], n) for a in dev}}
    c = row["arms"]["C"]
    for a in ("U1", "Uall", "S"):
        row[a.lower() + "_over_c"] = round(row["arms"][a]["median_ms"] / c["median_ms"], 4)
        row[a.lower() + "_median_below_c_best_window"] = row["arms"][a]["median_ms"] < c["min_ms"]
    row["bytes_per_element"] = {"C": {"written": 8 + 16 * nl}, "U1": {"read": 8, "written": 16}, "Uall": {"read": 8, "written": 16 * nl},
                                "S": {"read": 8, "written": 4 * nl}}
    print(json.dumps(row), file=sys.stderr, flush=True)
    keys = {"kernel_key": r.kernel_key(), "interp_variant": list(r.interp_variant())}
    for q in (r, r2):
        q.close()
    return row, keys


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--cases", default="scene4:3840x2160,scene:1920x1080")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "light_update_rate needs a GPU"
    doc = {"tool": "light_update_rate", "device": torch.cuda.get_device_name(0), "windows": args.windows, "window_s": args.window_s,
           "unit": "ms per call over w h elements", "checked": "updated planes equal a fresh capture under the look, before any timing",
           "arms": {"C": "light_pixels_into, every pixel, factors + hit_id + hit_dist (light_interp): the full capture",
                    "U1": "light_update_pixels_into, march_lights = 1 (light_update_interp)",
                    "Uall": "light_update_pixels_into, every light marched",
                    "S": "light_update_pixels_into, specular_lights = every light: no shadow march"},
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
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
