"""The tables of the repeated-view schedule (lol_sched.hip) held to a CPU model (tests/schedule_reference.py).

tests/test_gpu_parity.py proves that the lane table and the order table are PERMUTATIONS (every pixel is rendered exactly once
whatever they hold).  Here: WHICH permutations.
  the kernels alone    deal_rectangles / deal_by_cost and the three kernels of the wave sort, run by the library on scratch
                       (lol_gpu_testing_deal, lol_gpu_testing_sort_tiles): the lane table entry for entry, the bucket of every wave,
                       the start of every bucket, and every bucket's range of launch positions holding exactly its members;
  the live schedule    a still camera polled after every frame (lol_gpu_testing_schedule): fixed order, recording frame, dealt
                       frame, first sort, LPT_RESORT frames of rest, second sort — and again after the camera moved, the order was
                       set anew, the frame was resized and another scene was prepared;
  the cost's address   the run time a wave reports lands at the launch position the sort reads for it: the reported codes follow
                       the waves' dearest pixels more closely than any of 1000 shuffles of them does.
"""
import ctypes as C

import numpy as np
import pytest

import schedule_reference as M
from loltracer_amd import gpu
from loltracer_amd import scene as S

pytestmark = pytest.mark.gpu

KERNELS = {"spec": (1, "lol_render_spec"), "interp": (4, "render_interp")}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    """a context for the scratch runs: no scene, no frame"""
    r = gpu.Renderer(0)
    yield r
    r.close()


def open_renderer(sc, kernel):
    r = gpu.Renderer(0, specialize=KERNELS[kernel][0])
    r.prepare(sc)
    assert r.kernel_name() == KERNELS[kernel][1], r.specialize_log()
    return r


class Frames:
    """frames of one scene into one buffer, on the current stream"""

    def __init__(self, torch, r, w, h, rows=None):
        self.torch, self.r, self.w, self.h, self.rows = torch, r, w, h, rows
        self.n_rows = gpu.part_rows(h, rows)
        self.buf = torch.zeros((self.n_rows, w), dtype=torch.int32, device="cuda")

    def frame(self, camera=None):
        """one frame; what the accessor then says (None: the frame went out in a fixed order)"""
        self.r.render_into(self.buf.data_ptr(), self.w, self.h, camera=camera, rows=self.rows, stream=self.torch.cuda.current_stream().cuda_stream)
        return self.r.testing_schedule()


_real_cost = {}


def scene4_cost(torch, scenes, w, h):
    """what scene4's pixels cost at w x h (lol_gpu_testing_pixel_cost after the recording frame) — rendered once per size"""
    if (w, h) not in _real_cost:
        r = open_renderer(scenes["scene4"], "spec")
        try:
            f = Frames(torch, r, w, h)
            assert f.frame() is None and f.frame()["frames"] == 1
            cost = r.testing_pixel_cost(w, h)
        finally:
            r.close()
        assert len(np.unique(cost)) > 20, "scene4's pixels should differ in cost"
        cost.setflags(write=False)
        _real_cost[(w, h)] = cost
    return _real_cost[(w, h)]


# ---------------------------------------------------------------- the kernels alone

@pytest.mark.parametrize("w,n_rows", M.FRAMES)
def test_rectangles_are_the_models(ctx, w, n_rows):
    assert np.array_equal(ctx.testing_deal(None, w, n_rows), M.deal_rectangles(w, n_rows))


@pytest.mark.parametrize("w,n_rows", M.FRAMES)
@pytest.mark.parametrize("kind", M.SYNTHETIC)
def test_pixels_dealt_by_a_synthetic_cost_are_the_models(ctx, kind, w, n_rows):
    cost = M.synthetic_cost(kind, w, n_rows)
    got, want = ctx.testing_deal(cost, w, n_rows), M.deal_by_cost(cost)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} entries differ, the first at {int(np.flatnonzero(got != want)[0])}"


def test_pixels_dealt_by_scene4s_cost_are_the_models(torch_cuda, ctx, scenes):
    cost = scene4_cost(torch_cuda, scenes, 100, 37)
    got, want = ctx.testing_deal(cost, 100, 37), M.deal_by_cost(cost)
    assert np.array_equal(got, want)
    assert M.lane_efficiency(got, cost) > M.lane_efficiency(M.deal_rectangles(100, 37), cost)


def test_the_scratch_runs_refuse_a_table_of_another_size(ctx):
    out = np.zeros(1024, dtype=np.uint32)
    fn, lanes = gpu.gpu_lib().lol_gpu_testing_deal, out.ctypes.data_as(C.POINTER(C.c_uint32))
    assert fn(ctx._ctx, None, 65, 16, lanes, 1024) == -3                 # two regions
    assert fn(ctx._ctx, None, 0, 16, lanes, 1024) == -3
    assert fn(ctx._ctx, None, 64, 16, lanes, 1024) == 0
    with pytest.raises(gpu.GpuError):
        ctx.testing_sort_tiles(np.zeros(4, np.uint32), np.array([0, 1, 2, 4], np.uint32))      # names a wave slot beyond the table
    assert ctx.testing_schedule() is None                                # no frame yet


SORT_SIZES = [1, 7, 8, 9, 255, 256, 257, 1152, 4100]


def sort_costs(kind, n):
    rng = np.random.default_rng(7 * n + len(kind))
    if kind == "equal":                  # one bucket fed by many blocks
        return np.full(n, 300, dtype=np.uint32)
    if kind == "distinct":               # all distinct modulo 704: no bucket holds more than ceil(n / 704) waves
        return rng.permutation(n).astype(np.uint32) % 704
    if kind == "clamped":                # some above 1023, and the values around the clamp
        c = rng.integers(0, 3000, n).astype(np.uint32)
        c[:min(n, 5)] = np.array([1023, 1024, 1022, 0xFFFFFFFF, 0], dtype=np.uint32)[:min(n, 5)]
        return rng.permutation(c)
    if kind == "zero":
        return np.zeros(n, dtype=np.uint32)
    raise KeyError(kind)


def check_sort(order_out, keys, starts, cost, order_in):
    """one sort against the model: the buckets, their starts, a permutation, every bucket's range holds its members"""
    want_starts, want_keys, members = M.longest_first(cost, order_in)
    assert np.array_equal(keys, want_keys), f"{int((keys != want_keys).sum())} waves in another bucket"
    if starts is not None:
        assert np.array_equal(starts, want_starts), "bucket starts"
    assert np.array_equal(np.sort(order_out), np.sort(order_in)), "not a permutation of the old table"
    assert np.array_equal(M.bucket_ranges_sorted(order_out, want_starts), np.concatenate(members)), "a bucket's range holds other waves than its members"


@pytest.mark.parametrize("n", SORT_SIZES)
@pytest.mark.parametrize("kind", ["equal", "distinct", "clamped", "zero"])
def test_one_sort_is_the_models(ctx, kind, n):
    cost = sort_costs(kind, n)
    order_in = np.random.default_rng(n).permutation(n).astype(np.uint32)
    order_out, keys, starts = ctx.testing_sort_tiles(cost, order_in)
    check_sort(order_out, keys, starts, cost, order_in)


def test_a_sort_counts_a_wave_of_padding_as_nothing(ctx):
    """a wave slot whose lanes are all padding reports no run time: whatever lies at its launch position is another wave's"""
    w, n_rows = 333, 187
    lanes = M.deal_by_cost(M.synthetic_cost("ties", w, n_rows))
    n = M.n_waves(w, n_rows)
    assert n == 1152
    empty = ~M.wave_maxima(lanes, np.zeros((n_rows, w)))[1]
    assert 100 < int(empty.sum()) < n // 2
    rng = np.random.default_rng(5)
    cost, order_in = rng.integers(1, 704, n).astype(np.uint32), rng.permutation(n).astype(np.uint32)
    order_out, keys, starts = ctx.testing_sort_tiles(cost, order_in, lanes)
    check_sort(order_out, keys, starts, np.where(empty[order_in], 0, cost), order_in)
    assert (keys[empty[order_in]] == M.LPT_BUCKETS - 1).all() and (keys[~empty[order_in]] < M.LPT_BUCKETS - 1).all()


# ---------------------------------------------------------------- the live schedule

def check_geometry(s, w, n_rows):
    assert (s["region_w"], s["region_h"]) == M.REGION and (s["w"], s["n_rows"]) == (w, n_rows)
    assert s["n_tiles"] == M.n_waves(w, n_rows) and s["lanes"].size == 64 * s["n_tiles"]
    assert int(s["cost"].max()) <= M.MAX_RUN_TIME_CODE


def check_recording_frame(s, w, n_rows):
    check_geometry(s, w, n_rows)
    assert s["frames"] == 1
    assert np.array_equal(s["lanes"], M.deal_rectangles(w, n_rows)), "the recording frame's lanes are not the rectangles"
    assert np.array_equal(s["order"], np.arange(s["n_tiles"])), "the recording frame's waves do not go out in slot order"


def check_dealt_frame(s, pixel_cost, w, n_rows, label):
    """the third frame of a view; returns the lane efficiencies (rectangles, dealt) on the recorded costs"""
    check_geometry(s, w, n_rows)
    assert s["frames"] == 2
    want = M.deal_by_cost(pixel_cost)
    assert np.array_equal(s["lanes"], want), f"{int((s['lanes'] != want).sum())} lanes differ from the model's"
    assert np.array_equal(s["order"], np.arange(s["n_tiles"]))
    before, after = M.lane_efficiency(M.deal_rectangles(w, n_rows), pixel_cost), M.lane_efficiency(s["lanes"], pixel_cost)
    print(f"{label}: lane efficiency on the recorded costs {before:.4f} as rectangles, {after:.4f} dealt")
    assert after >= before and after == M.lane_efficiency(want, pixel_cost)
    return before, after


def check_sorted_frame(s, before, label):
    """a frame that a sort went ahead of, against what was polled after the frame before it"""
    n = s["n_tiles"]
    empty = s["lanes"].reshape(n, 64)[:, 63] >= M.LANE_PADDING          # (dealt: the padding of a region comes first)
    assert np.array_equal(empty, ~M.wave_maxima(s["lanes"], np.zeros((s["n_rows"], s["w"])))[1])
    assert np.array_equal(s["order_before"], before["order"]), "the sort read another table than the frame before it used"
    assert np.array_equal(s["lanes"], before["lanes"]), "a sort changed the lane table"
    empty_at = empty[before["order"]]                                    # by launch position of the frame before
    stale = int((before["cost"][empty_at] != 0).sum())
    ranked = int((s["keys"][empty_at] != M.LPT_BUCKETS - 1).sum())
    print(f"{label}: {int(empty.sum())} of {n} wave slots are empty; {stale} of them lie where another wave left a run time, {ranked} were ranked by it")
    assert ranked == 0, "a wave of padding alone was ranked by a stale run time"
    check_sort(s["order"], s["keys"], None, np.where(empty_at, 0, before["cost"]), before["order"])
    assert np.array_equal(np.sort(s["order"]), np.arange(n))
    # longest first, said once more without the model: the run times never increase along the launch positions, bucket by bucket
    where = np.empty(n, dtype=np.int64)
    where[before["order"]] = np.arange(n)
    ran = np.where(empty_at, 0, before["cost"])[where[s["order"]]]
    assert (np.diff(ran.astype(np.int64)) <= 0).all()


def run_still_view(f, r, label, camera=None, expect_fixed_first=True, through=18):
    """a camera that stands still, polled after every frame; returns the last poll"""
    w, n_rows = f.w, f.n_rows
    if expect_fixed_first:
        assert f.frame(camera) is None, "the first frame of a view went through a table"          # 1
    s = f.frame(camera)                                                                           # 2: records
    assert s is not None
    check_recording_frame(s, w, n_rows)
    sorts0 = s["sorts"]
    s = f.frame(camera)                                                                           # 3: dealt
    pixel_cost = r.testing_pixel_cost(w, n_rows)
    check_dealt_frame(s, pixel_cost, w, n_rows, label)
    assert s["sorts"] == sorts0
    if through < 4:
        return s
    before, s = s, f.frame(camera)                                                                # 4: after the first sort
    check_geometry(s, w, n_rows)
    assert s["frames"] == 3 and s["sorts"] == sorts0 + 1
    check_sorted_frame(s, before, label + ", first sort")
    for k in range(5, min(through, M.LPT_RESORT + 1) + 1):                                        # 5 ... 17: at rest
        before, s = s, f.frame(camera)
        check_geometry(s, w, n_rows)
        assert s["frames"] == k - 1 and s["sorts"] == sorts0 + 1, k
        assert np.array_equal(s["order"], before["order"]) and np.array_equal(s["lanes"], before["lanes"]), k
    if through >= M.LPT_RESORT + 2:
        before, s = s, f.frame(camera)                                                            # 18: after the second sort
        check_geometry(s, w, n_rows)
        assert s["frames"] == M.LPT_RESORT + 1 and s["sorts"] == sorts0 + 2
        check_sorted_frame(s, before, label + ", second sort")
        assert np.array_equal(r.testing_pixel_cost(w, n_rows), pixel_cost)
    return s


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("w,h,rows", [(333, 187, None), (100, 37, None), (200, 120, gpu.Rows(4, 12, 4))], ids=["333x187", "100x37", "band-of-200x120"])
def test_a_still_view_goes_through_the_models_tables_frame_by_frame(torch_cuda, scenes, kernel, w, h, rows):
    r = open_renderer(scenes["scene4"], kernel)
    try:
        assert r.tile_order()["mode"] == "lpt"
        f = Frames(torch_cuda, r, w, h, rows)
        assert f.n_rows == (h if rows is None else 40)
        s = run_still_view(f, r, f"scene4 {kernel} {w}x{f.n_rows}")
        assert s["sorts"] == 2 and r.tile_order()["decisions"] == 2
    finally:
        r.close()


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_the_tables_start_afresh_with_every_new_view(torch_cuda, scenes, kernel):
    """a moved camera, the order set anew, another size, another scene: the accessor refuses until a view repeats, and the frame
    that then records has the model's tables for ITS geometry"""
    sc = scenes["scene4"]
    r = open_renderer(sc, kernel)
    try:
        f = Frames(torch_cuda, r, 100, 37)
        run_still_view(f, r, f"scene4 {kernel} 100x37", through=5)
        cam = S.Camera()
        C.memmove(C.byref(cam), C.byref(sc.c.camera), C.sizeof(cam))
        cam.point.x += 0.4
        s = run_still_view(f, r, f"scene4 {kernel} 100x37, camera moved", camera=cam, through=4)
        assert s["sorts"] == 2
        # the order set anew: no table at once, and the next frame has no predecessor to repeat
        r.set_tile_order("lpt")
        assert r.testing_schedule() is None
        s = run_still_view(f, r, f"scene4 {kernel} 100x37, order set anew", camera=cam, through=4)
        # another size (the old camera, which this size has not seen)
        g = Frames(torch_cuda, r, 65, 17)
        s = run_still_view(g, r, f"scene4 {kernel} 65x17", through=4)
        assert s["n_tiles"] == 64
        # ... and back: the first size's tables are gone, not resumed
        run_still_view(f, r, f"scene4 {kernel} 100x37 again", through=3)
        # another scene
        r.prepare(scenes["scene"])
        run_still_view(f, r, f"scene {kernel} 100x37", through=4)
    finally:
        r.close()


# ---------------------------------------------------------------- the cost lands where the sort reads it

def ranks(v):
    """average ranks (ties share the mean of their places)"""
    v = np.asarray(v)
    _, inverse, counts = np.unique(v, return_inverse=True, return_counts=True)
    last = np.cumsum(counts)                              # one past the last place of every distinct value
    return ((last - counts + last - 1) / 2.0)[inverse]


def correlation(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_a_waves_run_time_lands_at_the_position_the_sort_reads_for_it(torch_cuda, scenes):
    """333 x 187: 1152 wave slots.  The dealt frame (the third of the view) goes out in slot order, so the run-time code at launch
    position i is wave slot i's; the wave ran as long as its dearest pixel.  Spearman's rank correlation of the two exceeds that of
    every one of 1000 shuffles of the codes: a build that wrote the codes to other positions than the sort reads would sit among
    the shuffles.  (No threshold of its own: nobody has measured this correlation here before; it is printed.)"""
    w, h = 333, 187
    r = open_renderer(scenes["scene4"], "spec")
    try:
        f = Frames(torch_cuda, r, w, h)
        assert f.frame() is None and f.frame()["frames"] == 1
        s = f.frame()
        pixel_cost = r.testing_pixel_cost(w, h)
    finally:
        r.close()
    assert s["frames"] == 2 and s["n_tiles"] == 1152 and np.array_equal(s["order"], np.arange(1152))
    assert np.array_equal(s["lanes"], M.deal_by_cost(pixel_cost))
    dearest, real = M.wave_maxima(s["lanes"], pixel_cost)
    a, b = ranks(dearest[real]), ranks(s["cost"][real])
    rho = correlation(a, b)
    rng = np.random.default_rng(2026)
    null = np.array([correlation(a, rng.permutation(b)) for _ in range(1000)])
    print(f"scene4 spec {w}x{h}: {int(real.sum())} waves with a real lane, {len(np.unique(s['cost'][real]))} distinct run-time codes; Spearman's rho of "
          f"run-time code against dearest pixel {rho:.4f}; 1000 shuffles: max {null.max():.4f}, min {null.min():.4f}, mean {null.mean():.4f}")
    assert rho > null.max()
