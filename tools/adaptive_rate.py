"""What adaptive supersampling costs (lol_gpu_set_adaptive_samples), against the full s x s frame of the same size on the same
code: scene4 at 3840x2160 and scene.lol at 1920x1080, s = 2 and 4, contrasts 0, 8, 16, 32 and 255.  Every frame is timed with HIP
events on its stream; the variants of one configuration alternate frame by frame (full, then each contrast, repeated).  For each
adaptive variant: the refined fraction and the split of its time across the three passes (lol_gpu_adaptive_pass_ms: the plain
frame, the mask and list, the refined pixels).  All on the scene's own kernel, in the fixed row order.  One JSON line.

    python tools/adaptive_rate.py [--reps 7] [--warmup 2]        (on the GPU box)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from loltracer_amd import gpu, scene as S  # noqa: E402

CONTRASTS = (0, 8, 16, 32, 255)
CONFIGS = (("scene4", 3840, 2160, 2), ("scene4", 3840, 2160, 4), ("scene", 1920, 1080, 2), ("scene", 1920, 1080, 4))


def run_config(torch, name, w, h, s, args):
    sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", f"{name}.lol"))
    r = gpu.Renderer(0)
    r.set_samples(s)                                      # before the upload: the module carries the supersampling kernels
    r.prepare(sc)
    r.set_tile_order("rows")
    stream = torch.cuda.Stream()
    fc = sc.frame_camera(w, h)
    buf = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    variants = [-1] + list(CONTRASTS)                     # -1: the full s x s frame
    ms = {v: [] for v in variants}
    passes = {v: [] for v in CONTRASTS}
    refined = {}
    kernels = {}
    torch.cuda.synchronize()
    for rep in range(args.warmup + args.reps):
        for v in variants:
            r.set_adaptive_samples(v)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            r.render_into(buf.data_ptr(), w, h, 256, stream=stream.cuda_stream, frame_camera=fc)
            e1.record(stream)
            e1.synchronize()
            kernels[v] = r.kernel_name()
            if rep < args.warmup:
                continue
            ms[v].append(e0.elapsed_time(e1))
            if v >= 0:
                passes[v].append(r.adaptive_pass_ms())
                refined[v] = r.adaptive_refined()
    key = r.kernel_key()
    r.close()
    full = statistics.median(ms[-1])
    out = {"scene": name, "w": w, "h": h, "s": s, "kernel_key": key,
           "full": {"kernel": kernels[-1], "median_ms": round(full, 4), "min_ms": round(min(ms[-1]), 4), "max_ms": round(max(ms[-1]), 4),
                    "mpixels_s": round(w * h / full / 1e3, 1)}}
    for T in CONTRASTS:
        med = statistics.median(ms[T])
        f = refined[T] / (w * h)
        split = [round(statistics.median(p[i] for p in passes[T]), 4) for i in range(3)]
        out[f"T{T}"] = {"kernel": kernels[T], "median_ms": round(med, 4), "min_ms": round(min(ms[T]), 4), "max_ms": round(max(ms[T]), 4),
                        "mpixels_s": round(w * h / med / 1e3, 1), "refined_fraction": round(f, 4),
                        "speedup_vs_full": round(full / med, 3), "model_1_over_(1/s2+f)": round(1.0 / (1.0 / (s * s) + f), 3),
                        "pass_ms_plain_classify_refine": split}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    res = [run_config(torch, *c, args) for c in CONFIGS]
    print(json.dumps({"tool": "adaptive_rate", "tile_order": "rows", "reps": args.reps, "warmup": args.warmup, "configs": res}))


if __name__ == "__main__":
    main()
