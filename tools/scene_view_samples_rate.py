"""What an ANTIALIASED animation of the scene costs: 64 frames of scene4 at 128x128 in which one sphere moves (scene.tween), every
pixel with 2 x 2 samples, by four routes.
Arms, ALTERNATING in one process, every arm warmed up first:
    a  the only route without supersampled scene views: per frame, upload_program of that frame's scene and a supersampled
       render_into, on one context with set_samples(2) and specialisation off (no scene-compiler run is queued behind an upload
       nobody will render twice)
    b  one render_scene_views_into(..., samples=2) of the 64 scenes on the interpreter's kernel (render_interp_scene_batch_aa, every
       record on its own macro-op lists) of a context with specialisation off: plain square roots and divisions, no proven blend factor
    f  the same on the interpreter's kernel of a context with the proven fast paths (set_specialize 4: what a default context runs
       the call on without set_scene_view_samples, or until its structure module is loaded)
    c  the same on the structure module (set_scene_view_samples before the upload: lol_render_param_batch_aa)
All four write the same 64 frames, which is checked once, byte for byte, before anything is timed.  A window repeats its arm until it
lasts at least --window-s; a host clock around the window, which ends in a device synchronise (arm a waits on the host inside every
upload: device events would not see that); --windows windows per arm, median and range recorded, in milliseconds per 64 frames.
The programs and frame cameras are made before the windows: flattening a scene is the host's work in every arm.
With --shutter K the arms b, f and c are also timed as blends of K supersampled scenes per frame (there is no arm a for a blend: a
context has one scene).  One JSON document on stdout (or --out FILE).

    python tools/scene_view_samples_rate.py --out profiles/r19_scene_view_samples_rate.json                    (on the GPU box)
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from loltracer_amd import gpu, scene as S  # noqa: E402
from scene_views_rate import FRAMES, H, MAX_STEPS, W, fastest, moving_scenes, summary, window  # noqa: E402

SAMPLES = 2
KERNELS = {"b": ("render_interp_scene_batch_aa", "render_interp_scene_batch_aa_lin"),
           "f": ("render_interp_scene_batch_aa", "render_interp_scene_batch_aa_lin"),
           "c": ("lol_render_param_batch_aa", "lol_render_param_batch_aa_lin")}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--scene", default="scene4")
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--shutter", type=int, default=4, choices=(1, 2, 4, 8, 16))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "scene_view_samples_rate needs a GPU"
    sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", args.scene + ".lol"))
    n, s = args.frames, SAMPLES
    scenes = moving_scenes(sc, n, 1)
    progs = [x.flatten() for x in scenes]
    fc = sc.frame_camera(W, H)
    fcs = [fc] * n

    upload = gpu.Renderer(0, specialize=False)
    upload.prepare(sc)
    upload.set_tile_order("rows")
    upload.set_samples(s)
    interp = gpu.Renderer(0, specialize=False)
    interp.prepare(sc)
    fast = gpu.Renderer(0, specialize=4)
    fast.prepare(sc)
    assert interp.interp_fast_paths() == (0, 0, 0) and fast.interp_fast_paths()[0] == 3 and fast.interp_fast_paths()[1] >= 1
    struct = gpu.Renderer(0)
    struct.set_scene_view_samples(True)
    struct.prepare(sc)
    assert struct.scene_views_state() == 2, struct.specialize_log()
    ctx = {"b": interp, "f": fast, "c": struct}
    for a, r in ctx.items():
        assert (r.scene_view_samples_kernel_name(1, s), r.scene_view_samples_kernel_name(4, s)) == KERNELS[a], a

    out = {a: torch.zeros((n, H, W), dtype=torch.int32, device="cuda") for a in "abfc"}
    torch.cuda.synchronize()

    def arm_a():
        for f in range(n):
            upload.upload_program(progs[f], wait=False)
            upload.render_into(out["a"][f].data_ptr(), W, H, MAX_STEPS, frame_camera=fc)

    def one_call(a, items, cams, k):
        return lambda: ctx[a].render_scene_views_into(out[a].data_ptr(), cams, items, W, H, k, MAX_STEPS, samples=s)

    issue = {"a": arm_a, "b": one_call("b", progs, fcs, 1), "f": one_call("f", progs, fcs, 1), "c": one_call("c", progs, fcs, 1)}
    sync = {"a": upload.sync, "b": interp.sync, "f": fast.sync, "c": struct.sync}
    arms = "abfc"
    reps = {}
    for a in arms:                                        # warm-up, and how often a window repeats its arm
        window(sync[a], issue[a], 1)
        ms = window(sync[a], issue[a], 2)
        reps[a] = max(1, math.ceil(args.window_s * 1e3 / (ms / 2)))
    frames = {a: out[a].cpu().numpy() for a in arms}
    same = bool(all(np.array_equal(frames["a"], frames[x]) for x in "bfc"))
    assert same, "the four routes wrote different frames"
    distinct = len({frames["a"][f].tobytes() for f in range(n)})
    dev = {a: [] for a in arms}
    for _ in range(args.windows):
        for a in arms:                                    # alternating
            dev[a].append(window(sync[a], issue[a], reps[a]) / reps[a])
    doc = {"tool": "scene_view_samples_rate", "device": torch.cuda.get_device_name(0), "scene": args.scene, "w": W, "h": H, "frames": n,
           "samples": s, "max_steps": MAX_STEPS, "windows": args.windows, "window_s": args.window_s, "unit": "ms per %d frames" % n,
           "clock": "host clock around a window that ends in a device synchronise",
           "arms_are": {"a": "%d x (upload_program + render_into), one context with set_samples(%d), specialisation off" % (n, s),
                        "b": "1 x render_scene_views_into(samples=%d), interpreter (%s), specialisation off: plain arithmetic" % (s, KERNELS["b"][0]),
                        "f": "1 x render_scene_views_into(samples=%d), interpreter (%s) with the proven fast paths (set_specialize 4)" % (s, KERNELS["f"][0]),
                        "c": "1 x render_scene_views_into(samples=%d), structure module (%s)" % (s, KERNELS["c"][0])},
           "frames_equal_across_arms": same, "distinct_frames": distinct,
           "arms": {a: summary(dev[a], reps[a], n) for a in arms}}
    spread = max(doc["arms"][a]["max_ms"] - doc["arms"][a]["min_ms"] for a in arms)
    doc["largest_spread_ms"] = round(spread, 4)
    for x in "bfc":
        doc["a_over_" + x] = round(doc["arms"]["a"]["median_ms"] / doc["arms"][x]["median_ms"], 2)
        doc[x + "_faster_than_a_by_more_than_the_spread"] = bool(doc["arms"]["a"]["min_ms"] - doc["arms"][x]["max_ms"] > spread)
    doc["b_over_c"] = round(doc["arms"]["b"]["median_ms"] / doc["arms"]["c"]["median_ms"], 4)
    doc["f_over_c"] = round(doc["arms"]["f"]["median_ms"] / doc["arms"]["c"]["median_ms"], 4)
    doc["fastest_of_b_f_c"] = fastest(doc["arms"], "bfc")
    if args.shutter > 1:                                  # the blend over K supersampled scenes per frame: b, f and c alone
        k = args.shutter
        bprogs = [x.flatten() for x in moving_scenes(sc, n, k)]
        bfcs = [fc] * (n * k)
        bissue = {a: one_call(a, bprogs, bfcs, k) for a in "bfc"}
        breps = {}
        for a in "bfc":
            window(sync[a], bissue[a], 1)
            ms = window(sync[a], bissue[a], 2)
            breps[a] = max(1, math.ceil(args.window_s * 1e3 / (ms / 2)))
        bsame = bool(np.array_equal(out["b"].cpu().numpy(), out["c"].cpu().numpy()) and np.array_equal(out["f"].cpu().numpy(), out["c"].cpu().numpy()))
        assert bsame, "the kernels blended different frames"
        bdev = {a: [] for a in "bfc"}
        for _ in range(args.windows):
            for a in "bfc":
                bdev[a].append(window(sync[a], bissue[a], breps[a]) / breps[a])
        doc["blend"] = {"scenes_per_frame": k, "frames_equal_across_arms": bsame,
                        "kernels": {a: KERNELS[a][1] for a in "bfc"},
                        "arms": {a: summary(bdev[a], breps[a], n) for a in "bfc"}}
        doc["blend"]["f_over_c"] = round(doc["blend"]["arms"]["f"]["median_ms"] / doc["blend"]["arms"]["c"]["median_ms"], 4)
        doc["blend"]["fastest_of_b_f_c"] = fastest(doc["blend"]["arms"], "bfc")
        doc["blend"]["b_over_c"] = round(doc["blend"]["arms"]["b"]["median_ms"] / doc["blend"]["arms"]["c"]["median_ms"], 4)
    doc["kernel_keys"] = {"interpreter_context": interp.kernel_key(), "fast_interpreter_context": fast.kernel_key(),
                          "structure_context": struct.kernel_key()}
    doc["fast_interpreter_proofs"] = dict(zip(("sqrt_kind", "proven_blend_factors", "proven_without_fixup"), fast.interp_fast_paths()))
    for r in (upload, interp, fast, struct):
        r.close()
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
