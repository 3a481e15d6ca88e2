"""A CPU model of the repeated-view schedule's tables (lol_sched.hip): which pixel every lane of every wave slot shades, and in
which order the wave slots go out.  Plain numpy; imports nothing from the library.

  deal_rectangles   the lane table of a view's recording frame: wave k of a region = its k-th 16 x 4 rectangle
  deal_by_cost      the lane table from the third frame on: a region's pixels sorted by what they cost, 64 to a wave
  longest_first     the counting sort of the waves by run time: bucket numbers, bucket starts, who must lie in which bucket
  lane_efficiency   what dealing is for: the work of the real lanes over the work the waves execute

The tables are compared ENTRY FOR ENTRY with the device's (tests/test_gpu_schedule.py): the sort keys are unique, so there is one
right lane table; only the order inside a bucket of the wave sort is free (the device ranks a bucket's members by atomics).
"""
import numpy as np

# ---- the layout, each with the line it restates ----
LANE_PADDING = 1 << 31        # lol_kernel.h: constexpr u32 LANE_PADDING = 1u << 31;
ROW_SHIFT = 16                # lol_sched.hip, deal_*_kernel: lane_pixels[i] = x | r << 16 | pad;
COLUMN_MASK, ROW_MASK = 0xFFFF, 0x7FFF      # lol_kernel.h, store_pixel: gx = e & 0xFFFFu, gr = e >> 16 & 0x7FFFu
REGION = (64, 16)             # lol_sched.hip: static RegionShape region_shape() { return { 64, 16 }; }
RECTANGLE = (16, 4)           # lol_sched.hip, deal_rectangles_kernel: (k % (REGION_W / 16)) * 16 + lane % 16, (k / (REGION_W / 16)) * 4 + lane / 16
WAVE = 64                     # lol_sched.hip, deal_rectangles_kernel: k = j / 64, lane = j % 64
LPT_BUCKETS = 1024            # lol_sched.hip: constexpr unsigned LPT_BUCKETS = 1024, ...
LPT_RESORT = 16               # lol_sched.hip: ... LPT_RESORT = 16
MAX_RUN_TIME_CODE = 703       # lol_kernel.h, store_pixel: at most 21 * 32 + 31 = 703


def regions_of(w, n_rows, region=REGION):
    """(regions per row of regions, rows of regions): lol_sched.hip, regions_x / regions_y"""
    return (w + region[0] - 1) // region[0], (n_rows + region[1] - 1) // region[1]


def n_waves(w, n_rows, region=REGION, wave=WAVE):
    rx, ry = regions_of(w, n_rows, region)
    return rx * ry * (region[0] * region[1] // wave)


def _entries(x, r, w, n_rows):
    """column | row << 16, clamped into the frame and flagged where the lane lies beyond it"""
    pad = (x >= w) | (r >= n_rows)
    return (np.minimum(x, w - 1) | np.minimum(r, n_rows - 1) << ROW_SHIFT | np.where(pad, LANE_PADDING, 0)).astype(np.uint32)


def unpack(lanes):
    """(column, row, is padding) of every entry"""
    lanes = np.asarray(lanes, dtype=np.uint32).astype(np.int64)
    return lanes & COLUMN_MASK, lanes >> ROW_SHIFT & ROW_MASK, (lanes & LANE_PADDING) != 0


def deal_rectangles(w, n_rows, region=REGION, rectangle=RECTANGLE):
    """The lane table of the recording frame, flat: region after region (row by row of regions), inside a region rectangle after
    rectangle (row by row of rectangles), inside a rectangle lane after lane (row by row of pixels)."""
    (RW, RH), (TW, TH) = region, rectangle
    assert RW % TW == 0 and RH % TH == 0
    rx, ry = regions_of(w, n_rows, region)
    per_region, per_wave = RW * RH, TW * TH
    i = np.arange(rx * ry * per_region, dtype=np.int64)
    reg, j = i // per_region, i % per_region
    k, lane = j // per_wave, j % per_wave
    x = (reg % rx) * RW + (k % (RW // TW)) * TW + lane % TW
    r = (reg // rx) * RH + (k // (RW // TW)) * TH + lane // TW
    return _entries(x, r, w, n_rows)


def deal_by_cost(cost, region=REGION):
    """The lane table dealt by `cost` (n_rows, w): the positions j = 0 ... of a region (row by row of ITS pixels) sorted ascending
    by (0 if beyond the frame's edge else cost + 1, j); wave k of the region is the k-th WAVE of them."""
    cost = np.asarray(cost)
    n_rows, w = cost.shape
    RW, RH = region
    rx, ry = regions_of(w, n_rows, region)
    per_region = RW * RH
    j = np.arange(per_region, dtype=np.int64)
    out = np.empty(rx * ry * per_region, dtype=np.uint32)
    for reg in range(rx * ry):
        x, r = (reg % rx) * RW + j % RW, (reg // rx) * RH + j // RW
        inside = (x < w) & (r < n_rows)
        key = np.where(inside, cost[np.minimum(r, n_rows - 1), np.minimum(x, w - 1)].astype(np.int64) + 1, 0)
        q = np.lexsort((j, key))                       # (last key first: by key, ties by position)
        out[reg * per_region:(reg + 1) * per_region] = _entries(x[q], r[q], w, n_rows)
    return out


def longest_first(cost, order_in):
    """The wave sort.  cost[i] = the run-time code of the wave at launch position i, order_in[i] = the wave slot that position
    shaded.  Returns (starts, keys, members): keys[i] = 1023 - min(cost[i], 1023) (bucket 0 = the longest), starts[b] = the launch
    position at which bucket b begins (exclusive prefix sum of the bucket sizes), members[b] = the sorted entries of order_in that
    must occupy positions starts[b] ... starts[b] + len(members[b]) - 1 of the new table, in whatever order."""
    cost = np.asarray(cost).astype(np.int64)
    order_in = np.asarray(order_in)
    assert cost.shape == order_in.shape and cost.ndim == 1
    keys = LPT_BUCKETS - 1 - np.minimum(cost, LPT_BUCKETS - 1)
    sizes = np.bincount(keys, minlength=LPT_BUCKETS)
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    by_bucket = np.argsort(keys, kind="stable")
    members = [np.sort(order_in[by_bucket[starts[b]:starts[b] + sizes[b]]]) for b in range(LPT_BUCKETS)]
    return starts.astype(np.uint32), keys.astype(np.uint32), members


def bucket_ranges_sorted(order_out, starts):
    """order_out with every bucket's range of launch positions sorted: equal to np.concatenate(members) iff every range holds
    exactly its multiset"""
    order_out = np.asarray(order_out)
    edges = np.concatenate((np.asarray(starts, dtype=np.int64), [len(order_out)]))
    out = order_out.copy()
    for b in range(len(edges) - 1):
        out[edges[b]:edges[b + 1]] = np.sort(order_out[edges[b]:edges[b + 1]])
    return out


def wave_work(lanes, cost, wave=WAVE):
    """(sum of the costs of the real lanes, sum over the waves of their dearest real lane): integers"""
    cost = np.asarray(cost).astype(np.int64)
    x, r, pad = unpack(lanes)
    c = np.where(pad, 0, cost[r, x]).reshape(-1, wave)
    return int(c.sum()), int(c.max(axis=1).sum())


def wave_maxima(lanes, cost, wave=WAVE):
    """per wave slot: the cost of its dearest real lane (0 for a wave of padding alone), and whether it has a real lane at all"""
    cost = np.asarray(cost).astype(np.int64)
    x, r, pad = unpack(lanes)
    c = np.where(pad, 0, cost[r, x]).reshape(-1, wave)
    return c.max(axis=1), ~pad.reshape(-1, wave).all(axis=1)


def lane_efficiency(lanes, cost, wave=WAVE):
    """the sum of the costs of the real lanes over `wave` x the sum of the wave maxima (1 for a frame that costs nothing)"""
    work, maxima = wave_work(lanes, cost, wave)
    return work / (wave * maxima) if maxima else 1.0


# ---- the inputs both sides of the suite are run on ----
FRAMES = [(1, 1), (16, 4), (64, 16), (65, 17), (37, 9), (100, 37), (333, 187)]
SYNTHETIC = ["constant", "zero", "saturated", "descending", "ties"]


def synthetic_cost(kind, w, n_rows):
    """(n_rows, w) uint16.  `descending` is strictly so in the frame's row-major order (every frame of FRAMES has fewer than 65536
    pixels); `ties` draws from 7 values, so every region of more than a few pixels sorts mostly by position."""
    n = w * n_rows
    assert n <= 0xFFFF
    if kind == "constant":
        c = np.full(n, 57)
    elif kind == "zero":
        c = np.zeros(n)
    elif kind == "saturated":
        c = np.full(n, 0xFFFF)
    elif kind == "descending":
        c = 0xFFFF - np.arange(n)
    elif kind == "ties":
        c = np.random.default_rng(1000 * w + n_rows).choice([0, 1, 2, 128, 129, 300, 0xFFFF], size=n)
    else:
        raise KeyError(kind)
    c = c.astype(np.uint16).reshape(n_rows, w)
    c.setflags(write=False)
    return c
