"""What a capture and a relight over records cost (lol_gpu_light_scene_pixels, lol_gpu_relight_scenes) beside what a host had to do
without them.  scene4 with one sphere moving (scene.tween from the sphere at (0, 1, -6) to (1.5, 2, -5)): 64 records, every pixel of
a 128 x 128 frame under the scene's camera in each.  Contexts without the scene compiler (specialize 4: the interpreter with the
upload's proven fast paths — what a capture runs on whatever the context is).  Arms, ALTERNATING in one process, every arm warmed up
first:
    Q    one light_scene_pixels_into over the 64 records
    U    64 x (upload_program of the record's scene + light_pixels_into + sync): what an animation's capture cost before
    S    64 light_pixels_into on the prepared scene, into the planes of the whole: lol_gpu_light_views' loop (the same amount of
         marching without the per-record reads, the records' copy and the launch over records)
    R    one relight_scenes_into over Q's planes, every record under its own look
    R64  64 relight_into over the same bytes, record by record (the tween moves geometry alone, so the tables of every record's look
         are one look of the prepared scene: the 64 calls are accepted and answer what R answers)
Before anything is timed Q's planes are held equal, byte for byte, to U's, and R's pixels to R64's.  A window repeats its arm until it
lasts at least --window-s; HIP events around the window; --windows windows per arm; medians and ranges in milliseconds per 64 records.

    python tools/scene_light_rate.py --out profiles/r27_scene_light_rate.json                              (on the GPU box)
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
from loltracer_amd.__main__ import look_of  # noqa: E402
from ray_rate import window  # noqa: E402
from scene_queries_rate import RECORDS, moving_scenes  # noqa: E402

SIDE = 128
MAX_STEPS = 256
LOOK = dict(lights=[((.9, .2, .1), (.1, .8, .3)), ((2., 1.5, 1.), (1., 1.5, 2.))], ambient=(.35, .15, .6))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "scene_light_rate needs a GPU"
    base, scenes = moving_scenes()
    n, nl = SIDE * SIDE, len(base.lights())
    total = RECORDS * n
    q, u = gpu.Renderer(0, specialize=4), gpu.Renderer(0, specialize=4)
    q.prepare(base)
    u.prepare(base)
    assert q.miss_skip_active() == 7
    handle_q, handle_u = q.next_stream(), u.next_stream()
    streams = {a: torch.cuda.ExternalStream(handle_u if a == "U" else handle_q) for a in ("Q", "U", "S", "R", "R64")}
    progs = [sc.flatten() for sc in scenes]
    fc = base.frame_camera(SIDE, SIDE)
    base_look = base.with_look(**LOOK)
    look_progs = [look_of(sc, base_look).flatten() for sc in scenes]
    base_look_prog = base_look.flatten()
    zeros = lambda count: torch.zeros(count, dtype=torch.int32, device="cuda")      # noqa: E731
    f_q, f_u, id_q, id_u = zeros(4 * nl * total), zeros(4 * nl * total), zeros(total), zeros(total)
    px_r, px_64 = zeros(total), zeros(total)

    def per_record(ctx, t_f, t_id, handle, upload):
        def issue():
            for rec in range(RECORDS):
                if upload:
                    ctx.upload_program(progs[rec], wait=False)
                ctx.light_pixels_into(n, SIDE, SIDE, MAX_STEPS, factors_ptr=t_f.data_ptr() + 16 * rec * n, id_ptr=t_id.data_ptr() + 4 * rec * n,
                                      light_stride=total, stream=handle, frame_camera=fc)
                if upload:
                    ctx.sync()
        return issue

    def relight_64():
        for rec in range(RECORDS):
            q.relight_into(base_look_prog, n, factors_ptr=f_q.data_ptr() + 16 * rec * n, id_ptr=id_q.data_ptr() + 4 * rec * n,
                           pixel_ptr=px_64.data_ptr() + 4 * rec * n, light_stride=total, stream=handle_q)

    issue = {
        "Q": lambda: q.light_scene_pixels_into(progs, n, SIDE, SIDE, 0, MAX_STEPS, factors_ptr=f_q.data_ptr(), id_ptr=id_q.data_ptr(),
                                               stream=handle_q, cameras=[fc] * RECORDS),
        "U": per_record(u, f_u, id_u, handle_u, True),
        "S": per_record(q, f_u, id_u, handle_q, False),
        "R": lambda: q.relight_scenes_into(progs, look_progs, n, factors_ptr=f_q.data_ptr(), id_ptr=id_q.data_ptr(), pixel_ptr=px_r.data_ptr(),
                                           stream=handle_q),
        "R64": relight_64,
    }
    # the answers first: one capture is the 64 uploads and captures, one relight the 64 relights, bit for bit
    issue["Q"]()
    issue["U"]()
    q.sync()
    u.sync()
    torch.cuda.synchronize()
    assert torch.equal(f_q, f_u) and torch.equal(id_q, id_u), "the capture over records is not the 64 single-scene captures"
    distinct = len({row.tobytes() for row in f_q.view(nl, RECORDS, -1)[0].cpu().numpy()})      # (the sphere moves: no two records capture alike)
    assert distinct > RECORDS // 2, "the records capture alike"
    issue["R"]()
    issue["R64"]()
    q.sync()
    torch.cuda.synchronize()
    assert torch.equal(px_r, px_64), "the relight over records is not the 64 relights"
    arms = list(issue)
    reps = {}
    for a in arms:                                            # warm-up, and the repeats
        window(torch, streams[a], issue[a], 2)
        ms = window(torch, streams[a], issue[a], 2)
        reps[a] = max(1, math.ceil(args.window_s * 1e3 / (ms / 2)))
    dev = {a: [] for a in arms}
    for _ in range(args.windows):
        for a in arms:                                        # alternating
            dev[a].append(window(torch, streams[a], issue[a], reps[a]) / reps[a])
    # (S and the timed U have written f_u since: Q's planes are what R and R64 read, and nothing has written them again but Q)
    row = {"pixels_per_record": n, "lights": nl, "captures_equal_q_u": True, "relights_equal_r_r64": True, "distinct_records": distinct, "arms": {}}
    for a in arms:
        med = statistics.median(dev[a])
        row["arms"][a] = {"median_ms": round(med, 4), "min_ms": round(min(dev[a]), 4), "max_ms": round(max(dev[a]), 4),
                          "windows": len(dev[a]), "repeats_per_window": reps[a]}
    m = {a: row["arms"][a]["median_ms"] for a in arms}
    row["u_over_q"], row["q_over_s"], row["r64_over_r"] = round(m["U"] / m["Q"], 2), round(m["Q"] / m["S"], 3), round(m["R64"] / m["R"], 2)
    doc = {"tool": "scene_light_rate", "device": torch.cuda.get_device_name(0), "scene": "scene4", "records": RECORDS, "frame": [SIDE, SIDE],
           "windows": args.windows, "window_s": args.window_s, "unit": "ms per 64 records", "max_steps": MAX_STEPS,
           "arms_are": {"Q": "one light_scene_pixels_into over the 64 records",
                        "U": "64 x (lol_gpu_upload_program + light_pixels_into + sync), specialisation off (interpreter, proven fast paths)",
                        "S": "64 light_pixels_into on the prepared scene, no upload, no sync between them (lol_gpu_light_views' loop)",
                        "R": "one relight_scenes_into over the 64 records, a look per record",
                        "R64": "64 relight_into over the same planes, record by record"},
           "result": row, "kernel_key": q.kernel_key()}
    q.close()
    u.close()
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
