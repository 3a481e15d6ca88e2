"""What a shading query costs (lol_gpu_shade_pixels, lol_gpu_shade_rays) beside the frame that holds the same rays.  scene4 and
scene.lol at 1920x1080 under the scene's own camera; every arm on the scene's own kernels, all three exact step skips on.  Arms,
ALTERNATING in one process, every arm warmed up first:
    A1, A2  the plain frame (render_into, LOL_GPU_TILES_ROWS), twice: their difference is the spread the others are read against
    B       shade_pixels_into over the same pixels listed tile by tile: a wave's 64 rays are the 16 x 4 patch a frame's wave has
    C       the same pixels listed row-major: a wave's 64 rays are a 64 x 1 strip of the frame
    D       shade_rays_into on those rays as a list, row-major: the camera rays built once with torch in float32 from the frame
            camera — close to the pixels' rays, not bit for bit theirs: the arm measures the list path, the tests hold parity
B does the frame's arithmetic with per-lane stores in the place of the LDS-staged row segments.  The queries write one packed pixel
per ray, as the frame does.
A window repeats its call until it lasts at least --window-s; HIP events around the window; --windows windows per arm, median and
range recorded, in milliseconds per frame's worth of rays.  One JSON document on stdout (or --out FILE).

    python tools/shade_rate.py --out profiles/r15_shade_rate.json                                           (on the GPU box)
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from loltracer_amd import gpu, scene as S  # noqa: E402
from ray_rate import pixel_lists, window  # noqa: E402


def camera_rays(torch, sc, w, h):
    """n x 6 float32 on the device: the pinhole rays of the frame, row-major, in float32 torch arithmetic"""
    fc = sc.frame_camera(w, h)
    t = lambda v: torch.tensor(v.tuple(), dtype=torch.float32, device="cuda")      # noqa: E731
    xs = (torch.arange(w, dtype=torch.float32, device="cuda") + .5) / w * 2. - 1.
    ys = 1. - (torch.arange(h, dtype=torch.float32, device="cuda") + .5) / h * 2.
    rd = (xs[None, :, None] * fc.width) * t(fc.right) + (ys[:, None, None] * fc.height) * t(fc.up) + t(fc.dir)
    rd = rd / rd.norm(dim=-1, keepdim=True)
    rays = torch.empty((h * w, 6), dtype=torch.float32, device="cuda")
    rays[:, :3] = t(fc.origin)
    rays[:, 3:] = rd.reshape(-1, 3)
    return rays.contiguous()


def measure(torch, sc, name, w, h, args):
    r = gpu.Renderer(0)
    r.set_shade_queries(True)
    r.set_tile_order("rows")
    r.prepare(sc)
    assert r.kernel_name() == "lol_render_spec" and r.shade_kernel_name() == "lol_shade_spec", r.specialize_log()
    assert r.miss_skip_active() == 7, r.miss_skip_active()
    handle = r.next_stream()
    stream = torch.cuda.ExternalStream(handle)
    n = w * h
    frame = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    rows, tiles = (torch.from_numpy(a.view(np.int32).copy()).to("cuda") for a in pixel_lists(w, h))
    rays = camera_rays(torch, sc, w, h)
    px = torch.zeros(n, dtype=torch.int32, device="cuda")
    frame_call = lambda: r.render_into(frame.data_ptr(), w, h, 256, stream=handle)      # noqa: E731
    issue = {
        "A1": frame_call,
        "B": lambda: r.shade_pixels_into(tiles.data_ptr(), n, w, h, 256, pixel_ptr=px.data_ptr(), stream=handle),
        "C": lambda: r.shade_pixels_into(rows.data_ptr(), n, w, h, 256, pixel_ptr=px.data_ptr(), stream=handle),
        "A2": frame_call,
        "D": lambda: r.shade_rays_into(rays.data_ptr(), n, 256, pixel_ptr=px.data_ptr(), stream=handle),
    }
    arms = list(issue)
    # the row-major query writes the frame: pixel for pixel
    issue["A1"]()
    issue["C"]()
    r.sync()
    torch.cuda.synchronize()
    assert torch.equal(frame.ravel(), px), "shade_pixels over the frame's pixels is not the frame"
    reps = {}
    for a in arms:                                        # warm-up, and the repeats
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
    a1, a2 = row["arms"]["A1"]["median_ms"], row["arms"]["A2"]["median_ms"]
    a_ms = (a1 + a2) / 2
    row["a_spread"] = round(abs(a1 - a2) / a_ms, 4)
    for k in "BCD":
        row[k.lower() + "_over_a"] = round(row["arms"][k]["median_ms"] / a_ms, 4)
    print(json.dumps(row), file=sys.stderr, flush=True)
    keys = {"kernel_key": r.kernel_key(), "shade_kernel": r.shade_kernel_name()}
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
    assert torch.cuda.is_available(), "shade_rate needs a GPU"
    w, h = (int(v) for v in args.size.lower().split("x"))
    doc = {"tool": "shade_rate", "device": torch.cuda.get_device_name(0), "windows": args.windows, "window_s": args.window_s,
           "unit": "ms per w h rays",
           "arms": {"A1": "render_into, LOL_GPU_TILES_ROWS, skips 7", "A2": "the same again",
                    "B": "shade_pixels_into, pixels tile by tile (16 x 4 patches per wave), pixel output",
                    "C": "shade_pixels_into, pixels row-major (64 x 1 strips per wave), pixel output",
                    "D": "shade_rays_into, the frame's rays as a list (row-major), pixel output"},
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
