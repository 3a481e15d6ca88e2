"""What supersampling costs (lol_gpu_set_samples): scene4 at 1920x1080 with 2x2 samples and at 960x540 with 4x4, against the plain
3840x2160 frame — the same rays and the same wave shapes — all in the fixed row order and on the scene's own kernel (one module:
lol_render_spec and lol_render_spec_aa).  HIP-event median of the timed frames after a warm-up, both kernel_keys, one JSON line.

    python tools/aa_rate.py [--frames 40] [--warmup 16]        (on the GPU box)
    python tools/aa_rate.py --compile                           (no device: hipRTC time of the module with and without the
                                                                 supersampling kernel, scene4 and a 1024-op scene)
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from loltracer_amd import gpu, scene as S  # noqa: E402


def scene4():
    return S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", "scene4.lol"))


def union_tree(depth, seed=3):
    """one object: a balanced smooth-union tree of 2^depth spheres (2^(depth+1) ops)"""
    import numpy as np
    rng = np.random.default_rng(seed)

    def tree(d):
        if d == 0:
            return "sphere { point = (%.3f, %.3f, %.3f), radius = %.3f }" % (*(rng.normal(size=3) * [3, 1.5, 2] + [0, 0, -8]), rng.uniform(0.3, 0.9))
        return "smooth_union { smoothness = 0.5, a = %s, b = %s }" % (tree(d - 1), tree(d - 1))
    return S.Scene.parse_string(
        "materials { { shininess = 2, diffuse = (0,0,0), specular = (0,0,0), ambient = (.02,.02,.02) },"
        " { shininess = 8, diffuse = (.5,.5,.5), specular = (.2,.2,.2), ambient = (.1,.1,.1) } }\n"
        "scene { camera { point = (0, 1, 4), direction = (0, -0.1, -1), fov = 100 },"
        " point_light { point = (0,9,0), diffuse_intensity = (2,2,2), specular_intensity = (2,2,2) }, "
        + tree(depth).replace("{", "{ material = #1,", 1) + " }")


def compile_times():
    os.environ["LOL_GPU_CACHE_DIR"] = ""                  # no disk cache: every module is really compiled
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, sc in (("scene4", scene4()), ("tree1024", union_tree(9))):
            prog = sc.flatten()
            row = {"ops": prog.n_ops}
            for s in (1, 2):                              # (2 and 4 compile the same module)
                t0 = time.perf_counter()
                gpu.compile_offline_samples(prog, os.path.join(d, f"{name}_{s}"), s)
                row["plain_s" if s == 1 else "aa_s"] = round(time.perf_counter() - t0, 3)
            out[name] = row
    return out


def frame_times(args):
    import torch
    sc = scene4()
    r = gpu.Renderer(0)
    r.set_samples(2)                                      # before the upload: the module carries lol_render_spec_aa
    r.prepare(sc)
    r.set_tile_order("rows")
    stream = torch.cuda.Stream()
    res = {}
    with torch.cuda.stream(stream):
        for label, w, h, s in (("plain_3840x2160", 3840, 2160, 1), ("s2_1920x1080", 1920, 1080, 2), ("s4_960x540", 960, 540, 4),
                               ("plain_3840x2160_again", 3840, 2160, 1)):
            r.set_samples(s)
            fc = sc.frame_camera(w, h)
            buf = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            for _ in range(args.warmup):
                r.render_into(buf.data_ptr(), w, h, 256, stream=stream.cuda_stream, frame_camera=fc)
            torch.cuda.synchronize()
            ev = []
            for _ in range(args.frames):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                r.render_into(buf.data_ptr(), w, h, 256, stream=stream.cuda_stream, frame_camera=fc)
                e1.record(stream)
                ev.append((e0, e1))
            torch.cuda.synchronize()
            ms = [a.elapsed_time(b) for a, b in ev]
            res[label] = {"kernel": r.kernel_name(), "kernel_key": r.kernel_key(), "median_ms": round(statistics.median(ms), 4),
                          "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "frames": len(ms)}
    r.close()
    base = statistics.mean([res["plain_3840x2160"]["median_ms"], res["plain_3840x2160_again"]["median_ms"]])
    for k in ("s2_1920x1080", "s4_960x540"):
        res[k]["vs_plain_4k"] = round(res[k]["median_ms"] / base, 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--compile", action="store_true", help="hipRTC compile times only (no device needed)")
    args = ap.parse_args()
    if args.compile:
        print(json.dumps({"tool": "aa_rate", "compile_s": compile_times()}))
        return
    print(json.dumps({"tool": "aa_rate", "tile_order": "rows", "scene": "scene4", "frames": frame_times(args)}))


if __name__ == "__main__":
    main()
