"""What a batch of views buys (lol_gpu_render_views): K small frames under K cameras as K calls of render_into against ONE call of
render_views_into.  scene4 and scene.lol; 64x36, 128x128, 256x256 and 512x512 with K = 256, 1920x1080 with K = 32; cameras on a
circle round the scene (scene.orbit_cameras).  Arms, ALTERNATING in one process, every shape warmed up first:
    A  K calls of render_into on one stream, fixed row order
    B  the same with set_frames_in_flight(4) and a ring of four destinations
    C  as B under the default longest-first mode: what a host gets today for a moving camera
    D  one render_views_into per K views (the scene's module compiled with set_view_batches)
A, B and C run on a renderer without the switch: code paths batches do not touch.  A window repeats its K views until it lasts
at least --window-s (a single small batch is milliseconds); HIP events around the window (the first on the stream of the window's
first launch, with every stream idle; the last = the latest of one event per stream); --windows windows per arm, median and range
recorded, in milliseconds per K views.  Also, for A and D: host time of queueing the K views once on idle streams (the launching
loop alone, no sync inside it; median of 5 per window).
One JSON document on stdout (or --out FILE).

    python tools/batch_rate.py [--windows 7] [--window-s 0.25] [--out profiles/r9_batch_rate.json]     (on the GPU box)
    python tools/batch_rate.py --scenes scene4 --shapes 128x128x256 --arms AD --windows 2               (a short run, e.g. under
                                                                                                         rocprofv3 --kernel-trace)
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

from loltracer_amd import gpu, scene as S  # noqa: E402

SHAPES = "64x36x256,128x128x256,256x256x256,512x512x256,1920x1080x32"


class Arm:
    """one way of rendering K views; issue() queues them once and returns nothing, streams = every stream it queues on"""

    def __init__(self, torch, r, fcs, w, h, streams, batch):
        self.torch, self.r, self.fcs, self.w, self.h, self.batch = torch, r, fcs, w, h, batch
        self.streams = [torch.cuda.ExternalStream(s) for s in streams]
        self.handles = streams
        k = len(fcs)
        if batch:
            self.dst = [torch.zeros((k, h, w), dtype=torch.int32, device="cuda")]
        else:
            self.dst = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in streams]

    def issue(self):
        r, w, h = self.r, self.w, self.h
        if self.batch:
            r.render_views_into(self.dst[0].data_ptr(), self.fcs, w, h, 256, stream=self.handles[0])
            return
        n = len(self.handles)
        for i, fc in enumerate(self.fcs):
            r.render_into(self.dst[i % n].data_ptr(), w, h, 256, stream=self.handles[i % n], frame_camera=fc)

    def window(self, reps):
        """(device ms, host ms of the launching loop) for reps x K views"""
        torch = self.torch
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        ends = [torch.cuda.Event(enable_timing=True) for _ in self.streams]
        e0.record(self.streams[0])
        t0 = time.perf_counter()
        for _ in range(reps):
            self.issue()
        host_ms = (time.perf_counter() - t0) * 1e3
        for e, s in zip(ends, self.streams):
            e.record(s)
        torch.cuda.synchronize()
        return max(e0.elapsed_time(e) for e in ends), host_ms

    def host_ms_once(self, n=5):
        """host time of queueing the K views ONCE on idle streams, nothing waited for inside the timed part: a long window's
        launching loop also measures the queues filling up (HIP's, and the ring of view records), i.e. the device"""
        out = []
        for _ in range(n):
            self.torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.issue()
            out.append((time.perf_counter() - t0) * 1e3)
        self.torch.cuda.synchronize()
        return statistics.median(out)


def own_streams(torch, r, n):
    """the first n of the renderer's own frame streams (raw handles): the rotation restarts at stream 0
    (lol_gpu_set_frames_in_flight) and every frame launched with stream=None moves it on by one"""
    r.set_frames_in_flight(n)
    tiny = torch.zeros((4, 16), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        out.append(r.next_stream())
        r.render_into(tiny.data_ptr(), 16, 4, 1)
    r.sync()
    return out


def measure(torch, sc, name, shapes, arms, args):
    plain = gpu.Renderer(0)
    plain.prepare(sc)
    batch = gpu.Renderer(0)
    batch.set_view_batches(True)
    batch.prepare(sc)
    assert plain.kernel_name() == "lol_render_spec" and batch.kernel_name() == "lol_render_spec", plain.specialize_log()
    one = own_streams(torch, plain, 1)
    four = own_streams(torch, plain, 4)
    assert len(set(four)) == 4 and four[0] == one[0], four
    bstream = [batch.next_stream()]
    rows = []
    for (w, h, k) in shapes:
        cams = S.orbit_cameras(sc, k)
        fcs = [sc.frame_camera(w, h, c) for c in cams]
        made = {}
        for a in arms:
            if a == "A":
                made[a] = Arm(torch, plain, fcs, w, h, one, False)
            elif a in "BC":
                made[a] = Arm(torch, plain, fcs, w, h, four, False)
            else:
                made[a] = Arm(torch, batch, fcs, w, h, bstream, True)

        def select(a):
            if a in "AB":
                plain.set_tile_order("rows")
            elif a == "C":
                plain.set_tile_order("lpt")
        reps = {}
        for a in arms:                                    # warm-up, and how often a window repeats its K views
            select(a)
            made[a].window(1)
            ms, _ = made[a].window(2)
            reps[a] = max(1, math.ceil(args.window_s * 1e3 / (ms / 2)))
        dev = {a: [] for a in arms}
        host = {a: [] for a in arms}
        for _ in range(args.windows):
            for a in arms:                                # alternating
                select(a)
                ms, _ = made[a].window(reps[a])
                dev[a].append(ms / reps[a])
                if a in "AD":
                    host[a].append(made[a].host_ms_once())
        row = {"scene": name, "w": w, "h": h, "views": k, "arms": {}}
        for a in arms:
            med = statistics.median(dev[a])
            row["arms"][a] = {"median_ms": round(med, 4), "min_ms": round(min(dev[a]), 4), "max_ms": round(max(dev[a]), 4),
                              "windows": len(dev[a]), "repeats_per_window": reps[a],
                              "mpixels_per_s": round(k * w * h / med / 1e3, 1)}
            if a in "AD":
                row["arms"][a]["host_ms_launching"] = round(statistics.median(host[a]), 4)
        if "D" in arms and len(arms) > 1:
            others = [a for a in arms if a != "D"]
            best = min(others, key=lambda a: row["arms"][a]["median_ms"])
            best_window = min(row["arms"][a]["min_ms"] for a in others)
            d = row["arms"]["D"]
            row["best_other_arm"] = best
            row["d_over_best_other_median"] = round(d["median_ms"] / row["arms"][best]["median_ms"], 4)
            row["d_median_beats_best_other_window"] = bool(d["median_ms"] < best_window)
            if "A" in arms:
                row["d_host_over_a_host"] = round(d["host_ms_launching"] / row["arms"]["A"]["host_ms_launching"], 4)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del made
        torch.cuda.empty_cache()
    keys = {"plain_kernel_key": plain.kernel_key(), "batch_module_kernel_key": batch.kernel_key()}
    plain.close()
    batch.close()
    return rows, keys


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--scenes", default="scene4,scene")
    ap.add_argument("--shapes", default=SHAPES, help="WxHxK,...")
    ap.add_argument("--arms", default="ABCD")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "batch_rate needs a GPU"
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    doc = {"tool": "batch_rate", "device": torch.cuda.get_device_name(0), "windows": args.windows, "window_s": args.window_s,
           "unit": "ms per K views", "arms": {"A": "K x render_into, one stream, rows", "B": "K x render_into, 4 streams, rows",
                                              "C": "K x render_into, 4 streams, lpt (default)", "D": "1 x render_views_into"},
           "rows": [], "kernel_keys": {}}
    for name in args.scenes.split(","):
        sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol"))
        rows, keys = measure(torch, sc, name, shapes, args.arms, args)
        doc["rows"] += rows
        doc["kernel_keys"][name] = keys
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
