"""What animating the SCENE costs: 64 frames of scene4 at 128x128 in which one sphere moves (scene.tween), by four routes.
Arms, ALTERNATING in one process, every arm warmed up first:
    a  the only route without scene views: per frame, upload_program of that frame's scene and render_into, on one context with
       specialisation off (no scene-compiler run is queued behind an upload nobody will render twice)
    b  one render_scene_views_into of the 64 scenes on the interpreter's kernels (every record on its own macro-op lists) of a
       context with specialisation off: plain square roots and divisions, no proven blend factor
    f  the same on the interpreter's kernels of a context with the proven fast paths (set_specialize 4: what a default context
       runs scene views on without set_scene_views, or until its structure module is loaded)
    c  the same on the structure module (set_scene_views before the upload: lol_render_param_batch)
All four write the same 64 frames, which is checked once, byte for byte, before anything is timed.  A window repeats its arm until it
lasts at least --window-s; a host clock around the window, which ends in a device synchronise (arm a waits on the host inside every
upload: device events would not see that); --windows windows per arm, median and range recorded, in milliseconds per 64 frames.
The programs and frame cameras are made before the windows: flattening a scene is the host's work in every arm.
With --shutter K the arms b, f and c are also timed as blends of K scenes per frame (there is no arm a for a blend: a context has one
scene).  With --small-batches REPS, what a CALL costs the host: REPS plain batches of 8 views at 64x36 back to back per window, a
host clock around the calls alone and around the calls and the synchronise behind them, in microseconds per call.  One JSON
document on stdout (or --out FILE).

    python tools/scene_views_rate.py --out profiles/r18_scene_views_rate.json                                  (on the GPU box)
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

W, H, FRAMES, MAX_STEPS = 128, 128, 64, 256


def moving_scenes(sc, frames, k):
    """frames x k scenes: the first sphere of the scene moves 3 units along x and 1 along y over the animation"""
    far = sc.clone()
    i = next(i for i in range(sc.c.n_nodes) if sc.c.nodes[i].type == S.NODE_SPHERE)
    far.c.nodes[i].point.x += 3.0
    far.c.nodes[i].point.y += 1.0
    return [S.tween(sc, far, t) for f in range(frames) for t in S.shutter_times(f, frames, k)]


def window(r_sync, issue, reps):
    r_sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        issue()
    r_sync()
    return (time.perf_counter() - t0) * 1e3


def summary(ms, reps, frames):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "windows": len(ms),
            "repeats_per_window": reps, "mpixels_per_s": round(frames * W * H / med / 1e3, 1)}


def fastest(arms, among):
    """the arm whose slowest window beats every other arm's fastest, or that no arm does"""
    for x in among:
        if all(arms[x]["max_ms"] < arms[y]["min_ms"] for y in among if y != x):
            return x
    return "none (windows overlap)"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--scene", default="scene4")
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--shutter", type=int, default=4, choices=(1, 2, 4, 8, 16))
    ap.add_argument("--small-batches", type=int, default=0, metavar="REPS",
                    help="also time REPS plain batches of 8 views at 64x36 per window, a host clock around the calls")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "scene_views_rate needs a GPU"
    sc = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", args.scene + ".lol"))
    n = args.frames
    scenes = moving_scenes(sc, n, 1)
    progs = [s.flatten() for s in scenes]
    fc = sc.frame_camera(W, H)
    fcs = [fc] * n

    upload = gpu.Renderer(0, specialize=False)
    upload.prepare(sc)
    upload.set_tile_order("rows")
    interp = gpu.Renderer(0, specialize=False)
    interp.prepare(sc)
    fast = gpu.Renderer(0, specialize=4)
    fast.prepare(sc)
    assert interp.interp_fast_paths() == (0, 0, 0) and fast.interp_fast_paths()[0] == 3 and fast.interp_fast_paths()[1] >= 1
    struct = gpu.Renderer(0)
    struct.set_scene_views(True)
    struct.prepare(sc)
    assert interp.scene_views_kernel_name(1) == "render_interp_scene_batch"
    assert struct.scene_views_kernel_name(1) == "lol_render_param_batch" and struct.scene_views_state() == 2, struct.specialize_log()

    out = {a: torch.zeros((n, H, W), dtype=torch.int32, device="cuda") for a in "abfc"}
    torch.cuda.synchronize()

    def arm_a():
        for f in range(n):
            upload.upload_program(progs[f], wait=False)
            upload.render_into(out["a"][f].data_ptr(), W, H, MAX_STEPS, frame_camera=fc)

    issue = {"a": arm_a,
             "b": lambda: interp.render_scene_views_into(out["b"].data_ptr(), fcs, progs, W, H, 1, MAX_STEPS),
             "f": lambda: fast.render_scene_views_into(out["f"].data_ptr(), fcs, progs, W, H, 1, MAX_STEPS),
             "c": lambda: struct.render_scene_views_into(out["c"].data_ptr(), fcs, progs, W, H, 1, MAX_STEPS)}
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
    doc = {"tool": "scene_views_rate", "device": torch.cuda.get_device_name(0), "scene": args.scene, "w": W, "h": H, "frames": n,
           "max_steps": MAX_STEPS, "windows": args.windows, "window_s": args.window_s, "unit": "ms per %d frames" % n,
           "clock": "host clock around a window that ends in a device synchronise",
           "arms_are": {"a": "%d x (upload_program + render_into), one context, specialisation off" % n,
                        "b": "1 x render_scene_views_into, interpreter (render_interp_scene_batch), specialisation off: plain arithmetic",
                        "f": "1 x render_scene_views_into, interpreter (render_interp_scene_batch) with the proven fast paths (set_specialize 4)",
                        "c": "1 x render_scene_views_into, structure module (lol_render_param_batch)"},
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
    if args.shutter > 1:                                  # the blend over K scenes per frame: b and c alone
        k = args.shutter
        bscenes = moving_scenes(sc, n, k)
        bprogs = [s.flatten() for s in bscenes]
        bfcs = [fc] * (n * k)
        bissue = {"b": lambda: interp.render_scene_views_into(out["b"].data_ptr(), bfcs, bprogs, W, H, k, MAX_STEPS),
                  "f": lambda: fast.render_scene_views_into(out["f"].data_ptr(), bfcs, bprogs, W, H, k, MAX_STEPS),
                  "c": lambda: struct.render_scene_views_into(out["c"].data_ptr(), bfcs, bprogs, W, H, k, MAX_STEPS)}
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
                        "arms": {a: summary(bdev[a], breps[a], n) for a in "bfc"}}
        doc["blend"]["f_over_c"] = round(doc["blend"]["arms"]["f"]["median_ms"] / doc["blend"]["arms"]["c"]["median_ms"], 4)
        doc["blend"]["fastest_of_b_f_c"] = fastest(doc["blend"]["arms"], "bfc")
        doc["blend"]["b_over_c"] = round(doc["blend"]["arms"]["b"]["median_ms"] / doc["blend"]["arms"]["c"]["median_ms"], 4)
    if args.small_batches:                                # what a CALL costs the host: plain batches too small to keep the device busy
        reps, k, bw, bh = args.small_batches, 8, 64, 36
        plain = gpu.Renderer(0)
        plain.set_view_batches(True)
        plain.prepare(sc)
        cams = [sc.frame_camera(bw, bh, c) for c in S.orbit_cameras(sc, k)]      # made before the windows, like the programs
        small = torch.zeros((k, bh, bw), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        queued, synced = [], []
        for i in range(args.windows + 1):                 # (the first window warms up)
            plain.sync()
            t0 = time.perf_counter()
            for _ in range(reps):                         # no synchronise in here: the clock is around the calls
                plain.render_views_into(small.data_ptr(), cams, bw, bh, MAX_STEPS)
            t1 = time.perf_counter()
            plain.sync()
            t2 = time.perf_counter()
            if i:
                queued.append((t1 - t0) * 1e6 / reps)
                synced.append((t2 - t0) * 1e6 / reps)
        spread = lambda us: {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}  # noqa: E731
        doc["small_batches"] = {"what": "%d x render_views_into of %d views at %dx%d back to back, no synchronise between them" % (reps, k, bw, bh),
                                "unit": "microseconds per call", "kernel": plain.view_samples_kernel_name(1, -1), "windows": args.windows,
                                "host_clock_around_the_calls": spread(queued), "and_the_synchronise_behind_them": spread(synced)}
        plain.close()
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
