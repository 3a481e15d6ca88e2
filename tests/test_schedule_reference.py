"""The CPU model of the repeated-view schedule (tests/schedule_reference.py) held to what the tables are FOR, without a GPU: every
pixel is shaded exactly once, the padding of a region comes first, the costs along a region's lanes never decrease, and — on regions
small enough for brute force — no other way of dealing a region's pixels to its waves executes less.  tests/test_gpu_schedule.py
then holds the device's tables to this model entry for entry."""
import itertools

import numpy as np
import pytest

import schedule_reference as M

FRAMES, KINDS = M.FRAMES, M.SYNTHETIC
PER_REGION = M.REGION[0] * M.REGION[1]


def tables(kind, w, n_rows):
    cost = M.synthetic_cost(kind, w, n_rows)
    return cost, M.deal_rectangles(w, n_rows), M.deal_by_cost(cost)


@pytest.mark.parametrize("w,n_rows", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_real_pixel_appears_exactly_once(kind, w, n_rows):
    _, rect, dealt = tables(kind, w, n_rows)
    for name, lanes in (("rectangles", rect), ("by cost", dealt)):
        assert lanes.dtype == np.uint32 and lanes.size == M.n_waves(w, n_rows) * M.WAVE, name
        x, r, pad = M.unpack(lanes)
        seen = np.bincount((r * w + x)[~pad], minlength=w * n_rows)
        assert seen.size == w * n_rows and (seen == 1).all(), name
        # no bit beyond column | row << 16 | padding
        assert np.array_equal(lanes, (x | r << 16 | np.where(pad, M.LANE_PADDING, 0)).astype(np.uint32)), name


@pytest.mark.parametrize("w,n_rows", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_padding_comes_first_in_its_region_and_names_a_pixel_of_the_frame(kind, w, n_rows):
    _, rect, dealt = tables(kind, w, n_rows)
    rx, ry = M.regions_of(w, n_rows)
    for name, lanes in (("rectangles", rect), ("by cost", dealt)):
        x, r, pad = M.unpack(lanes)
        assert (x < w).all() and (r < n_rows).all(), name
        # as many lanes of padding as the regions reach beyond the frame
        assert int(pad.sum()) == rx * ry * PER_REGION - w * n_rows, name
    pad = M.unpack(dealt)[2].reshape(-1, PER_REGION)
    assert (np.diff(pad.astype(np.int8), axis=1) <= 0).all(), "a real lane before a lane of padding"
    # (a wave of the dealt table is empty exactly when its last lane is padding: what lpt_hist_kernel relies on)
    waves = M.unpack(dealt)[2].reshape(-1, M.WAVE)
    assert np.array_equal(waves.all(axis=1), waves[:, M.WAVE - 1])


@pytest.mark.parametrize("w,n_rows", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_costs_along_a_regions_lanes_never_decrease(kind, w, n_rows):
    cost, _, dealt = tables(kind, w, n_rows)
    x, r, pad = M.unpack(dealt)
    c = np.where(pad, -1, cost[r, x].astype(np.int64)).reshape(-1, PER_REGION)
    assert (np.diff(c, axis=1) >= 0).all()
    # ... and equal costs stay in the order of their position in the region (the keys are unique: one right table)
    pos = ((r % M.REGION[1]) * M.REGION[0] + x % M.REGION[0]).reshape(-1, PER_REGION)
    real = ~pad.reshape(-1, PER_REGION)
    tie = (np.diff(c, axis=1) == 0) & real[:, 1:] & real[:, :-1]
    assert (np.diff(pos, axis=1)[tie] > 0).all()
    if kind == "descending" and (w, n_rows) == (64, 16):
        assert np.array_equal(dealt, M.deal_by_cost(M.synthetic_cost("constant", w, n_rows))[::-1]), "a full region in reverse"


def pairings(items):
    """every way of splitting `items` into unordered pairs"""
    if not items:
        yield []
        return
    a = items[0]
    for i in range(1, len(items)):
        for rest in pairings(items[1:i] + items[i + 1:]):
            yield [(a, items[i])] + rest


@pytest.mark.parametrize("w,n_rows", [(4, 2), (8, 1), (7, 3), (3, 1), (9, 5), (1, 1)])
@pytest.mark.parametrize("seed", range(4))
def test_no_other_partition_of_a_small_region_executes_less(w, n_rows, seed):
    """the property the feature is for: regions of 4 x 2 pixels, waves of 2 lanes.  A wave executes its dearest lane's work on all
    its lanes, so a region costs the sum of its wave maxima; the dealt partition reaches the minimum over all 105 partitions."""
    region, wave = (4, 2), 2
    rng = np.random.default_rng(seed)
    cost = rng.choice([0, 1, 2, 3, 5, 8, 13, 40], size=(n_rows, w)).astype(np.uint16)
    dealt = M.deal_by_cost(cost, region=region)
    rect = M.deal_rectangles(w, n_rows, region=region, rectangle=(2, 1))
    assert dealt.size == rect.size == M.n_waves(w, n_rows, region, wave) * wave
    assert len(list(pairings(list(range(8))))) == 105
    for reg in range(dealt.size // 8):
        x, r, pad = M.unpack(dealt[8 * reg:8 * reg + 8])
        c = np.where(pad, 0, cost[r, x].astype(np.int64))
        got = int(c.reshape(-1, wave).max(axis=1).sum())
        best = min(sum(max(c[a], c[b]) for a, b in p) for p in pairings(list(range(8))))
        assert got == best, (reg, c)
        assert np.array_equal(np.sort(dealt[8 * reg:8 * reg + 8]), np.sort(rect[8 * reg:8 * reg + 8]))
    assert M.wave_work(dealt, cost, wave)[1] <= M.wave_work(rect, cost, wave)[1]
    assert M.lane_efficiency(dealt, cost, wave) >= M.lane_efficiency(rect, cost, wave)


@pytest.mark.parametrize("w,n_rows", FRAMES)
def test_a_constant_cost_deals_the_rectangles_pixels_in_another_order(w, n_rows):
    cost, rect, dealt = tables("constant", w, n_rows)
    a, b = rect.reshape(-1, PER_REGION), dealt.reshape(-1, PER_REGION)
    assert np.array_equal(np.sort(a, axis=1), np.sort(b, axis=1)), "not the same entries region by region"
    # a region is wider than one rectangle: row by row of the region is another order than rectangle by rectangle
    assert (a != b).any(axis=1).all()
    # ... and where a region IS one rectangle and lies inside the frame, the two are one table
    if w % 16 == 0 and n_rows % 4 == 0:
        assert np.array_equal(M.deal_rectangles(w, n_rows, region=M.RECTANGLE), M.deal_by_cost(cost, region=M.RECTANGLE))
    # nothing to gain from dealing a constant cost
    assert M.wave_work(rect, cost)[0] == M.wave_work(dealt, cost)[0] == 57 * w * n_rows
    assert M.lane_efficiency(dealt, cost) >= M.lane_efficiency(rect, cost)


@pytest.mark.parametrize("w,n_rows", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_dealing_never_lowers_the_lane_efficiency(kind, w, n_rows):
    cost, rect, dealt = tables(kind, w, n_rows)
    assert M.wave_work(rect, cost)[0] == M.wave_work(dealt, cost)[0] == int(cost.astype(np.int64).sum())
    assert M.wave_work(dealt, cost)[1] <= M.wave_work(rect, cost)[1]
    assert 0.0 < M.lane_efficiency(rect, cost) <= M.lane_efficiency(dealt, cost) <= 1.0


def test_lane_efficiency_by_hand():
    # one region of 4 x 2, waves of 2: costs 1 9 / 9 1 / ... dealt (1 1)(9 9) against rectangles (1 9)(9 1)
    cost = np.array([[1, 9, 9, 1]], dtype=np.uint16)
    rect = M.deal_rectangles(4, 1, region=(4, 1), rectangle=(2, 1))
    dealt = M.deal_by_cost(cost, region=(4, 1))
    assert rect.tolist() == [0, 1, 2, 3] and dealt.tolist() == [0, 3, 1, 2]
    assert M.wave_work(rect, cost, 2) == (20, 18) and M.wave_work(dealt, cost, 2) == (20, 10)
    assert M.lane_efficiency(rect, cost, 2) == 20 / 36 and M.lane_efficiency(dealt, cost, 2) == 1.0
    # a lane of padding counts nothing and a wave of padding alone runs nothing
    cost = np.array([[7]], dtype=np.uint16)
    dealt = M.deal_by_cost(cost, region=(4, 1))
    assert dealt.tolist() == [M.LANE_PADDING] * 3 + [0]
    assert M.wave_work(dealt, cost, 2) == (7, 7)
    maxima, real = M.wave_maxima(dealt, cost, 2)
    assert maxima.tolist() == [0, 7] and real.tolist() == [False, True]


@pytest.mark.parametrize("n", [1, 7, 8, 9, 255, 256, 257, 1152, 4100])
def test_longest_first_is_a_counting_sort_by_descending_cost(n):
    rng = np.random.default_rng(n)
    order_in = rng.permutation(n).astype(np.uint32)
    for cost in (np.full(n, 300), np.arange(n) % 704, rng.integers(0, 5000, n), np.zeros(n, dtype=np.int64)):
        starts, keys, members = M.longest_first(cost.astype(np.uint32), order_in)
        assert len(members) == M.LPT_BUCKETS == starts.size and keys.size == n
        assert np.array_equal(keys, 1023 - np.minimum(cost, 1023))
        assert starts[0] == 0 and (np.diff(starts.astype(np.int64)) == [len(m) for m in members[:-1]]).all()
        assert int(starts[-1]) + len(members[-1]) == n
        flat = np.concatenate(members)
        assert np.array_equal(np.sort(flat), np.arange(n))
        # the launch positions run from the longest waves to the shortest
        where = np.empty(n, dtype=np.int64)
        where[order_in] = np.arange(n)
        assert (np.diff(np.minimum(cost, 1023)[where[flat]]) <= 0).all()
        # a stable sort is one of the orders the device may produce; a reversed table is not (unless all costs are equal)
        stable = order_in[np.argsort(keys, kind="stable")]
        assert np.array_equal(M.bucket_ranges_sorted(stable, starts), flat)
        if len(np.unique(keys)) > 1:
            assert not np.array_equal(M.bucket_ranges_sorted(stable[::-1], starts), flat)
