"""The mask of adaptive supersampling (tests/adaptive_reference.py, include/lol_gpu.h lol_gpu_set_adaptive_samples) on hand-made
frames, and the restatement as a whole on the CPU oracle.  No GPU."""
import numpy as np
import pytest

import aa_reference as A
import adaptive_reference as R
import oracle_lib as O


def flat(h, w, c=(10, 20, 30), obj=1):
    return np.full((h, w), obj, dtype=np.int64), np.tile(np.array(c, dtype=np.int32), (h, w, 1))


def refined(m):
    return {(int(y), int(x)) for y, x in zip(*np.nonzero(m))}


def test_flat_frame_refines_nothing():
    ids, c8 = flat(5, 7)
    assert not R.mask(ids, c8, 0).any()


def test_single_pixel_frame_has_no_neighbours():
    for obj in (0, 3):
        ids, c8 = flat(1, 1, (255, 0, 255), obj)
        assert not R.mask(ids, c8, 0).any()


def test_corner_and_border_neighbourhoods():
    """neighbours outside the frame are ignored: a change in a corner refines that corner and its three neighbours"""
    ids, c8 = flat(4, 6)
    ids[0, 0] = 2
    assert refined(R.mask(ids, c8, 255)) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    ids, c8 = flat(4, 6)
    ids[3, 5] = 2
    assert refined(R.mask(ids, c8, 255)) == {(3, 5), (3, 4), (2, 5), (2, 4)}
    ids, c8 = flat(4, 6)
    ids[0, 3] = 2                                   # top border: six pixels
    assert refined(R.mask(ids, c8, 255)) == {(0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4)}
    ids, c8 = flat(5, 5)
    ids[2, 2] = 2                                   # inside: the whole 3 x 3 neighbourhood
    assert refined(R.mask(ids, c8, 255)) == {(y, x) for y in (1, 2, 3) for x in (1, 2, 3)}


@pytest.mark.parametrize("n", [1, 2, 5])
def test_one_row_and_one_column_frames(n):
    for k in range(n):
        ids, c8 = flat(1, n)
        ids[0, k] = 7
        want = {(0, x) for x in (k - 1, k, k + 1) if 0 <= x < n} if n > 1 else set()
        assert refined(R.mask(ids, c8, 0)) == want
        ids, c8 = flat(n, 1)
        c8[k, 0, 1] += 100
        want = {(y, 0) for y in (k - 1, k, k + 1) if 0 <= y < n} if n > 1 else set()
        assert refined(R.mask(ids, c8, 99)) == want
        assert not R.mask(ids, c8, 100).any()


@pytest.mark.parametrize("T", [0, 1, 16, 200, 254])
@pytest.mark.parametrize("ch", [0, 1, 2])
def test_a_difference_of_exactly_T_is_not_refined_and_T_plus_one_is(T, ch):
    for sign in (1, -1):
        ids, c8 = flat(3, 3, (0, 0, 0) if sign > 0 else (255, 255, 255))
        c8[1, 1, ch] += sign * T
        assert not R.mask(ids, c8, T).any()
        c8[1, 1, ch] += sign
        assert refined(R.mask(ids, c8, T)) == {(y, x) for y in range(3) for x in range(3)}


def test_an_id_change_with_equal_colours_is_refined():
    ids, c8 = flat(3, 4)
    ids[:, 2:] = 0                                  # an object and the sky, same colour
    assert refined(R.mask(ids, c8, 255)) == {(y, x) for y in range(3) for x in (1, 2)}


def test_at_255_only_ids_refine():
    ids, c8 = flat(4, 4, (0, 0, 0))
    c8[::2, ::2] = 255                              # every channel as far apart as it gets
    assert not R.mask(ids, c8, 255).any()
    assert R.mask(ids, c8, 254).all()
    ids[3, 3] = 9
    assert refined(R.mask(ids, c8, 255)) == {(2, 2), (2, 3), (3, 2), (3, 3)}


def test_diagonal_neighbours_count():
    ids, c8 = flat(3, 3)
    ids[0, 0] = 5
    assert (1, 1) in refined(R.mask(ids, c8, 0))
    assert (2, 2) not in refined(R.mask(ids, c8, 0))


@pytest.mark.parametrize("s", [2, 4])
def test_reference_is_the_full_frame_where_refined_and_the_plain_frame_elsewhere(scenes, s):
    sc = scenes["scene4"]
    w, h, T = 23, 13, 16
    full = A.render(sc, w, h, s)
    x, rgb, m = R.render(sc, w, h, s, T, full=full)
    plain_x, plain_rgb, _ = O.render(sc, w, h, want_rgb=True)
    assert m.any() and (~m).any()
    assert np.array_equal(x[m], full[0][m]) and np.array_equal(rgb[m].view(np.uint32), full[1][m].view(np.uint32))
    assert np.array_equal(x[~m], plain_x[~m]) and np.array_equal(rgb[~m].view(np.uint32), plain_rgb[~m].view(np.uint32))
    # the same rows computed alone (the sampled-rows route of the full-size test) agree
    rows = [0, 6, 12]
    xr, rgbr, mr = R.render(sc, w, h, s, T, rows=rows)
    assert np.array_equal(xr, x[rows]) and np.array_equal(mr, m[rows]) and np.array_equal(rgbr.view(np.uint32), rgb[rows].view(np.uint32))


def test_every_pixel_refined_is_the_full_frame(scenes):
    """a frame where every pixel is refined (a checkerboard of objects) equals aa_reference.render"""
    sc = scenes["scene"]
    w, h, s = 9, 7, 2
    full = A.render(sc, w, h, s)
    px, rgb, ids = R.plain(sc, w, h)
    ids = np.indices((h, w)).sum(axis=0) % 2      # (hand-made ids: every pixel has a neighbour of another object)
    m = R.mask(ids, R.channels(px), 255)
    assert m.all()
    x, r = R.combine(m, rgb, *full)
    assert np.array_equal(x, full[0]) and np.array_equal(r.view(np.uint32), full[1].view(np.uint32))
