"""What a SUPERSAMPLED batch of views buys (lol_gpu_render_views_samples): K small frames under K cameras with s x s samples per
pixel — on every pixel (contrast -1) or edge-adaptively (contrast T) — as K calls of render_into on a renderer with set_samples /
set_adaptive_samples against ONE call of render_views_into(samples=s, adaptive=T).  scene4 and scene.lol; 64x36, 128x128 and
256x256 with K = 256, and 1920x1080 with K = 32 for s = 2; cameras on a circle round the scene (scene.orbit_cameras).  Arms,
ALTERNATING in one process, every shape warmed up first (the method of tools/batch_rate.py):
    A  K calls of render_into on one stream
    B  the same with set_frames_in_flight(4) and a ring of four destinations
    D  one render_views_into per K views (the scene's module compiled with set_view_samples)
A and B run on a renderer whose module was compiled with set_samples: code paths this feature does not touch.  A window repeats its
K views until it lasts at least --window-s; HIP events around the window (the first on the stream of the window's first launch, with
every stream idle; the last = the latest of one event per stream); --windows windows per arm, median and range recorded, in
milliseconds per K views.  For adaptive rows also the fraction of the batch's pixels that were refined, and D against the batch
that supersamples every pixel.
One JSON document on stdout (or --out FILE).

    python tools/batch_aa_rate.py [--windows 7] [--window-s 0.25] [--out profiles/r10_batch_aa_rate.json]     (on the GPU box)
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from loltracer_amd import gpu, scene as S  # noqa: E402

SHAPES = "64x36x256,128x128x256,256x256x256,1920x1080x32"
BIG = 1920 * 1080                    # shapes from this many pixels on are measured at s = 2 alone


class Arm:
    """one way of rendering K views with s x s samples and contrast T; issue() queues them once"""

    def __init__(self, torch, r, fcs, w, h, s, T, streams, batch):
        self.torch, self.r, self.fcs, self.w, self.h, self.s, self.T, self.batch = torch, r, fcs, w, h, s, T, batch
        self.streams = [torch.cuda.ExternalStream(x) for x in streams]
        self.handles = streams
        k = len(fcs)
        if batch:
            self.dst = [torch.zeros((k, h, w), dtype=torch.int32, device="cuda")]
        else:
            self.dst = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in streams]

    def issue(self):
        r, w, h = self.r, self.w, self.h
        if self.batch:
            r.render_views_into(self.dst[0].data_ptr(), self.fcs, w, h, 256, stream=self.handles[0], samples=self.s, adaptive=self.T)
            return
        n = len(self.handles)
        for i, fc in enumerate(self.fcs):
            r.render_into(self.dst[i % n].data_ptr(), w, h, 256, stream=self.handles[i % n], frame_camera=fc)

    def window(self, reps):
        """device ms for reps x K views"""
        torch = self.torch
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        ends = [torch.cuda.Event(enable_timing=True) for _ in self.streams]
        e0.record(self.streams[0])
        for _ in range(reps):
            self.issue()
        for e, st in zip(ends, self.streams):
            e.record(st)
        torch.cuda.synchronize()
        return max(e0.elapsed_time(e) for e in ends)


def own_streams(torch, r, n):
    """the first n of the renderer's own frame streams (raw handles), as tools/batch_rate.py finds them"""
    r.set_frames_in_flight(n)
    tiny = torch.zeros((4, 16), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        out.append(r.next_stream())
        r.render_into(tiny.data_ptr(), 16, 4, 1)
    r.sync()
    return out


def measure(torch, sc, name, shapes, args):
    loop = gpu.Renderer(0)
    loop.set_samples(2)                  # before prepare(): its module carries lol_render_spec_aa / _aa_list (s is read at run time)
    loop.prepare(sc)
    loop.set_samples(1)
    one = own_streams(torch, loop, 1)
    four = own_streams(torch, loop, 4)
    assert len(set(four)) == 4 and four[0] == one[0], four
    loop.set_tile_order("rows")
    batch = gpu.Renderer(0)
    batch.set_view_samples(True)
    batch.prepare(sc)
    for r in (loop, batch):
        assert r.kernel_name() == "lol_render_spec", r.specialize_log()
    assert batch.view_samples_kernel_name(2, -1) == "lol_render_spec_batch_aa", batch.specialize_log()
    assert batch.view_samples_kernel_name(2, 16) == "lol_render_spec_batch_aa_list", batch.specialize_log()
    bstream = [batch.next_stream()]
    rows = []
    for (w, h, k) in shapes:
        fcs = [sc.frame_camera(w, h, c) for c in S.orbit_cameras(sc, k)]
        full_median = {}
        for s in args.samples:
            if w * h >= BIG and s != 2:
                continue
            for T in args.contrasts:
                loop.set_samples(s)
                loop.set_adaptive_samples(T)
                assert loop.kernel_name() == ("lol_render_spec_aa_list" if T >= 0 else "lol_render_spec_aa")
                made = {"A": Arm(torch, loop, fcs, w, h, s, T, one, False), "B": Arm(torch, loop, fcs, w, h, s, T, four, False),
                        "D": Arm(torch, batch, fcs, w, h, s, T, bstream, True)}
                reps = {}
                for a in "ABD":                              # warm-up, and how often a window repeats its K views
                    made[a].window(1)
                    ms = made[a].window(2)
                    reps[a] = max(1, math.ceil(args.window_s * 1e3 / (ms / 2)))
                dev = {a: [] for a in "ABD"}
                for _ in range(args.windows):
                    for a in "ABD":                          # alternating
                        dev[a].append(made[a].window(reps[a]) / reps[a])
                row = {"scene": name, "w": w, "h": h, "views": k, "samples": s, "contrast": T, "arms": {}}
                for a in "ABD":
                    med = statistics.median(dev[a])
                    row["arms"][a] = {"median_ms": round(med, 4), "min_ms": round(min(dev[a]), 4), "max_ms": round(max(dev[a]), 4),
                                      "windows": len(dev[a]), "repeats_per_window": reps[a],
                                      "mpixels_per_s": round(k * w * h / med / 1e3, 1)}
                best = min("AB", key=lambda a: row["arms"][a]["median_ms"])
                d = row["arms"]["D"]
                row["best_other_arm"] = best
                row["d_over_best_other_median"] = round(d["median_ms"] / row["arms"][best]["median_ms"], 4)
                row["d_median_beats_best_other_window"] = bool(d["median_ms"] < min(row["arms"][a]["min_ms"] for a in "AB"))
                if T >= 0:
                    row["refined_fraction"] = round(batch.views_refined() / float(k * w * h), 4)
                    if s in full_median:
                        row["d_over_full_batch"] = round(d["median_ms"] / full_median[s], 4)
                else:
                    full_median[s] = d["median_ms"]
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del made
                torch.cuda.empty_cache()
    keys = {"loop_module_kernel_key": loop.kernel_key(), "batch_module_kernel_key": batch.kernel_key()}
    loop.close()
    batch.close()
    return rows, keys


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--scenes", default="scene4,scene")
    ap.add_argument("--shapes", default=SHAPES, help="WxHxK,...")
    ap.add_argument("--samples", default="2,4")
    ap.add_argument("--contrasts", default="-1,16", help="-1 = every pixel; list -1 first for d_over_full_batch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.samples = [int(v) for v in args.samples.split(",")]
    args.contrasts = [int(v) for v in args.contrasts.split(",")]
    import torch
    assert torch.cuda.is_available(), "batch_aa_rate needs a GPU"
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    doc = {"tool": "batch_aa_rate", "device": torch.cuda.get_device_name(0), "windows": args.windows, "window_s": args.window_s,
           "unit": "ms per K views", "arms": {"A": "K x render_into with set_samples / set_adaptive_samples, one stream, rows",
                                              "B": "the same over 4 streams", "D": "1 x render_views_into(samples, adaptive)"},
           "rows": [], "kernel_keys": {}}
    for name in args.scenes.split(","):
        sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol"))
        rows, keys = measure(torch, sc, name, shapes, args)
        doc["rows"] += rows
        doc["kernel_keys"][name] = keys
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
