"""What a scene query costs (lol_gpu_trace_scene_rays, lol_gpu_shade_scene_rays, lol_gpu_trace_scene_pixels) beside what a host had
to do without it.  scene4 with one sphere moving (scene.tween from the sphere at (0, 1, -6) to (1.5, 2, -5)): 64 records; the rays of
a 64 x 64 frame under the scene's camera as a list of 4096 rays that every record shares, and ONE pixel per record (the pick).
Contexts without the scene compiler (specialize 4: the interpreter with the upload's proven fast paths — what a scene query runs on
whatever the context is).  Arms, ALTERNATING in one process, every arm warmed up first:
    Q   one scene-query call over the 64 records
    U   64 x (upload_program of the record's scene + the single-scene query + sync): what it costs without scene queries
    S   64 single-scene interpreter queries on the prepared scene: the same amount of marching without the per-record reads,
        the records' copy and the launch over records
Before anything is timed Q's answers are held equal, bit for bit, to U's.  A window repeats its arm until it lasts at least
--window-s; HIP events around the window; --windows windows per arm; medians and ranges in milliseconds per 64 records.

    python tools/scene_queries_rate.py --out profiles/r26_scene_queries_rate.json                          (on the GPU box)
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
from shade_rate import camera_rays  # noqa: E402

RECORDS, SIDE = 64, 64
PICK = (34, 17)                          # a pixel the moving sphere shows in every record
MAX_STEPS = 256


def moving_scenes():
    path = os.path.join(ROOT, "tests", "golden", "scenes", "scene4.lol")
    text = open(path).read()
    assert "point\t\t= (0, 1, -6)" in text
    a, b = S.Scene.parse_file(path), S.Scene.parse_string(text.replace("point\t\t= (0, 1, -6)", "point\t\t= (1.5, 2, -5)"))
    return a, [S.tween(a, b, t) for f in range(RECORDS) for t in S.shutter_times(f, RECORDS, 1)]


def workloads(torch, base, scenes, q, u, handle_q, handle_u):
    """{name: (n, {arm: issue}, the tensors Q and U write)}"""
    n = SIDE * SIDE
    rays = camera_rays(torch, base, SIDE, SIDE)
    progs = [sc.flatten() for sc in scenes]
    fc = base.frame_camera(SIDE, SIDE)
    xy = torch.tensor(PICK, dtype=torch.int32, device="cuda")
    new = lambda count, k=1: [torch.zeros(count * k, dtype=torch.int32, device="cuda") for _ in range(2)]      # noqa: E731
    out = {}

    def per_record(ctx, call, upload):
        def issue():
            for rec in range(RECORDS):
                if upload:
                    ctx.upload_program(progs[rec], wait=False)
                call(ctx, rec)
                if upload:
                    ctx.sync()
        return issue

    # ---- a list of rays: geometry
    d_q, d_u = new(RECORDS * n)
    single = lambda t, h: lambda ctx, rec: ctx.trace_rays_into(rays.data_ptr(), n, MAX_STEPS, dist_ptr=t.data_ptr() + 4 * rec * n, stream=h)      # noqa: E731
    out["trace_rays"] = (n, {
        "Q": lambda: q.trace_scene_rays_into(progs, rays.data_ptr(), n, 0, MAX_STEPS, dist_ptr=d_q.data_ptr(), stream=handle_q),
        "U": per_record(u, single(d_u, handle_u), True),
        "S": per_record(q, single(d_u, handle_q), False)}, (d_q, d_u))
    # ---- a list of rays: colour
    p_q, p_u = new(RECORDS * n)
    single = lambda t, h: lambda ctx, rec: ctx.shade_rays_into(rays.data_ptr(), n, MAX_STEPS, pixel_ptr=t.data_ptr() + 4 * rec * n, stream=h)     # noqa: E731
    out["shade_rays"] = (n, {
        "Q": lambda: q.shade_scene_rays_into(progs, rays.data_ptr(), n, 0, MAX_STEPS, pixel_ptr=p_q.data_ptr(), stream=handle_q),
        "U": per_record(u, single(p_u, handle_u), True),
        "S": per_record(q, single(p_u, handle_q), False)}, (p_q, p_u))
    # ---- one pixel per record: the pick
    k_q, k_u = new(RECORDS)
    single = lambda t, h: lambda ctx, rec: ctx.trace_pixels_into(xy.data_ptr(), 1, SIDE, SIDE, MAX_STEPS, dist_ptr=t.data_ptr() + 4 * rec,      # noqa: E731
                                                                 stream=h, frame_camera=fc)
    out["pick"] = (1, {
        "Q": lambda: q.trace_scene_pixels_into(progs, xy.data_ptr(), 1, SIDE, SIDE, 0, MAX_STEPS, dist_ptr=k_q.data_ptr(), stream=handle_q,
                                               cameras=[fc] * RECORDS),
        "U": per_record(u, single(k_u, handle_u), True),
        "S": per_record(q, single(k_u, handle_q), False)}, (k_q, k_u))
    return out, (rays, progs, xy)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "scene_queries_rate needs a GPU"
    base, scenes = moving_scenes()
    q, u = gpu.Renderer(0, specialize=4), gpu.Renderer(0, specialize=4)
    q.prepare(base)
    u.prepare(base)
    assert q.trace_kernel_name() == "trace_interp" and q.shade_kernel_name() == "shade_interp" and q.miss_skip_active() == 7
    handle_q, handle_u = q.next_stream(), u.next_stream()
    streams = {"Q": torch.cuda.ExternalStream(handle_q), "U": torch.cuda.ExternalStream(handle_u), "S": torch.cuda.ExternalStream(handle_q)}
    loads, keep = workloads(torch, base, scenes, q, u, handle_q, handle_u)
    doc = {"tool": "scene_queries_rate", "device": torch.cuda.get_device_name(0), "scene": "scene4", "records": RECORDS, "windows": args.windows,
           "window_s": args.window_s, "unit": "ms per 64 records", "max_steps": MAX_STEPS,
           "arms_are": {"Q": "one scene-query call over the 64 records",
                        "U": "64 x (lol_gpu_upload_program + the single-scene query + sync), specialisation off (interpreter, proven fast paths)",
                        "S": "64 single-scene interpreter queries on the prepared scene, no upload, no sync between them"},
           "workloads": {}}
    for name, (n, issue, (t_q, t_u)) in loads.items():
        # the answers first: one call is the 64 uploads and queries, bit for bit
        issue["Q"]()
        issue["U"]()
        q.sync()
        u.sync()
        torch.cuda.synchronize()
        assert torch.equal(t_q, t_u), name + ": the scene query's answers are not the single-scene queries'"
        distinct = len({row.tobytes() for row in t_q.view(RECORDS, -1).cpu().numpy()})      # (the sphere moves: no two records answer alike)
        arms = list(issue)
        reps = {}
        for a in arms:                                        # warm-up, and the repeats
            window(torch, streams[a], issue[a], 2)
            ms = window(torch, streams[a], issue[a], 2)
            reps[a] = max(1, math.ceil(args.window_s * 1e3 / (ms / 2)))
        dev = {a: [] for a in arms}
        for _ in range(args.windows):
            for a in arms:                                    # alternating
                dev[a].append(window(torch, streams[a], issue[a], reps[a]) / reps[a])
        assert distinct > RECORDS // 2, name + ": the records answer alike"
        row = {"rays_per_record": n, "answers_equal_q_u": True, "distinct_records": distinct, "arms": {}}
        for a in arms:
            med = statistics.median(dev[a])
            row["arms"][a] = {"median_ms": round(med, 4), "min_ms": round(min(dev[a]), 4), "max_ms": round(max(dev[a]), 4),
                              "windows": len(dev[a]), "repeats_per_window": reps[a]}
        row["u_over_q"] = round(row["arms"]["U"]["median_ms"] / row["arms"]["Q"]["median_ms"], 2)
        row["q_over_s"] = round(row["arms"]["Q"]["median_ms"] / row["arms"]["S"]["median_ms"], 3)
        print(json.dumps({name: row}), file=sys.stderr, flush=True)
        doc["workloads"][name] = row
    doc["kernel_key"] = q.kernel_key()
    q.close()
    u.close()
    del keep
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
