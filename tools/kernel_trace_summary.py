"""Reduce a `rocprofv3 --kernel-trace` run (its rocpd SQLite database, `*_results.db`) to what a document quotes: per kernel the
number of dispatches, median / min / max time, their sum, and the gaps between consecutive dispatches of the same kernel on the
same queue (start of one minus end of the one before; gaps of a millisecond or more — the host was doing something else — are
left out).  Microseconds.  No device needed: it reads the file.

    rocprofv3 --kernel-trace --stats -d out -o batch_ad -- python tools/batch_rate.py --scenes scene4 --shapes 128x128x256 \\
              --arms AD --windows 1 --window-s 0.05                                                  (on the GPU box)
    python tools/kernel_trace_summary.py out/batch_ad_results.db --kernels lol_render_spec,lol_render_spec_batch \\
              --min-blocks 256 --views lol_render_spec_batch=256 --what "..." > profiles/r9_batch_trace_128.json
"""
import argparse
import json
import sqlite3
import statistics


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("db")
    ap.add_argument("--kernels", required=True, help="kernel names (without arguments), comma separated")
    ap.add_argument("--min-blocks", type=int, default=0, help="leave out dispatches of fewer 64-lane blocks (warm-up and helper frames)")
    ap.add_argument("--views", default="", help="NAME=N,...: views per dispatch of a kernel, for a per-view figure")
    ap.add_argument("--what", default="")
    ap.add_argument("--tool", default="")
    args = ap.parse_args()
    views = dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in args.views.split(",") if kv)
    con = sqlite3.connect(args.db)
    rows = con.execute("select name, start, end, queue_id, grid_x, grid_y, grid_z, workgroup_x from kernels order by start").fetchall()
    out = {"tool": args.tool, "what": args.what, "reduced_by": "tools/kernel_trace_summary.py", "kernels": {}}
    for want in args.kernels.split(","):
        # (the trace gives grids in lanes)
        v = [(s, e, q) for n, s, e, q, gx, gy, gz, wx in rows
             if n.split("(")[0] == want and gx * gy * gz // max(1, wx) >= args.min_blocks]
        if not v:
            continue
        d = [(e - s) / 1e3 for s, e, _ in v]
        gaps = [(v[i + 1][0] - v[i][1]) / 1e3 for i in range(len(v) - 1) if v[i + 1][2] == v[i][2]]
        g = sorted(x for x in gaps if x < 1000) or [0.0]
        k = {"dispatches": len(v), "median_us": round(statistics.median(d), 2), "min_us": round(min(d), 2), "max_us": round(max(d), 2),
             "sum_ms": round(sum(d) / 1e3, 3), "median_gap_us": round(statistics.median(g), 2), "p90_gap_us": round(g[int(len(g) * 0.9)], 2),
             "views_per_dispatch": views.get(want, 1)}
        if views.get(want, 1) > 1:
            k["us_per_view"] = round(k["median_us"] / views[want], 3)
        out["kernels"][want] = k
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
