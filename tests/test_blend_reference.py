"""Views averaged over K cameras, the part that needs no GPU: the contract restated on the oracle (tests/blend_reference.py) agrees
with the plain frame where it must, and the two camera generators (scene.shutter_cameras, scene.lens_cameras) do what they say."""
import math
import os
import sys

import numpy as np
import pytest

import blend_reference as B
import oracle_lib as O
from loltracer_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H = 37, 11
F32_EPS = 2.0 ** -24                     # half an ulp of a float in [1, 2): the relative error of one rounding to float


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", ["scene", "scene4"])
def test_one_camera_per_view_is_the_plain_frame(scenes, name):
    sc = scenes[name]
    cams = S.orbit_cameras(sc, 3)
    px, rgb = B.render(sc, cams, 1, W, H)
    for v, cam in enumerate(cams):
        ox, orgb, _ = O.render(sc, W, H, camera=cam, want_rgb=True)
        assert np.array_equal(px[v], ox), v
        assert np.array_equal(bits(rgb[v]), bits(orgb)), v


@pytest.mark.parametrize("k", [2, 4, 8, 16])
def test_equal_cameras_are_the_plain_frame_bit_for_bit(scenes, k):
    """doubling and a power-of-two scale are exact on [0, 1]: K copies of one camera are that camera's frame"""
    sc = scenes["scene4"]
    cams = S.orbit_cameras(sc, 3)
    one_px, one_rgb = B.render(sc, cams, 1, W, H)
    many = [B.copy_camera(c) for c in cams for _ in range(k)]
    px, rgb = B.render(sc, many, k, W, H)
    assert np.array_equal(px, one_px) and np.array_equal(bits(rgb), bits(one_rgb))


def test_the_mean_is_taken_before_gamma(scenes):
    """a blend of two different cameras is NOT the mean of the two packed frames wherever the two differ much: the contract averages
    linear light"""
    sc = scenes["scene4"]
    a, b = S.orbit_cameras(sc, 8)[:2]
    px, _ = B.render(sc, [a, b], 2, W, H)
    pa, _ = B.render(sc, [a], 1, W, H)
    pb, _ = B.render(sc, [b], 1, W, H)
    host = np.zeros_like(px[0])
    for sh in (16, 8, 0):
        host |= (((pa[0] >> sh & 0xFF) + (pb[0] >> sh & 0xFF)) // 2) << sh
    assert (px[0] != host).any()


def vec(v):
    return np.array(v.tuple(), dtype=np.float64)


def test_shutter_cameras(scenes):
    sc = scenes["scene4"]
    a, b = S.orbit_cameras(sc, 8)[:2]
    for k in (1, 2, 4, 16):
        cams = S.shutter_cameras(a, b, k)
        assert len(cams) == k
        for i, c in enumerate(cams):
            t = (i + 0.5) / k
            want = vec(a.point) + t * (vec(b.point) - vec(a.point))
            assert np.array_equal(vec(c.point), want.astype(np.float32).astype(np.float64)), (k, i)       # the midpoint, rounded to float
            d = vec(a.direction) + t * (vec(b.direction) - vec(a.direction))
            d /= math.sqrt(float(d @ d))
            assert np.array_equal(vec(c.direction), d.astype(np.float32).astype(np.float64)), (k, i)
            # a unit vector whose three components were rounded to float: |d|^2 is off by at most 2 eps (|dx| + |dy| + |dz|) eps-terms
            assert abs(float(vec(c.direction) @ vec(c.direction)) - 1.0) <= 2 * F32_EPS * math.sqrt(3.0) + 1e-12, (k, i)
            assert c.fov == a.fov
    # the shutter of a camera that does not move: that camera, k times over, bit for bit
    for k in (1, 2, 8):
        for c in S.shutter_cameras(a, a, k):
            assert bytes(memoryview(c).cast("B")) == bytes(memoryview(a).cast("B"))
    with pytest.raises(ValueError):
        S.shutter_cameras(a, b, 0)


def test_lens_cameras(scenes):
    sc = scenes["scene4"]
    cam = sc.camera
    one = S.lens_cameras(cam, 5.0, 0.3, 1)
    assert len(one) == 1 and bytes(memoryview(one[0]).cast("B")) == bytes(memoryview(cam).cast("B"))
    p, d = vec(cam.point), vec(cam.direction)
    d /= math.sqrt(float(d @ d))
    focus_distance, radius = 5.0, 0.3
    focus = p + focus_distance * d
    # positions are rounded to float: each coordinate moves by at most eps |coordinate|
    slack = F32_EPS * float(np.abs(p).max() + radius) * math.sqrt(3.0)
    for k in (2, 4, 8, 16):
        cams = S.lens_cameras(cam, focus_distance, radius, k)
        assert len(cams) == k
        seen = set()
        for i, c in enumerate(cams):
            off = vec(c.point) - p
            assert abs(float(off @ d)) <= slack, (k, i)                                        # in the lens plane
            r = math.sqrt(float(off @ off))
            assert r <= radius + slack, (k, i)                                                 # within the aperture
            assert abs(r - radius * math.sqrt((i + 0.5) / k)) <= slack, (k, i)                 # the stated pattern
            look = focus - vec(c.point)
            look /= math.sqrt(float(look @ look))
            # the direction was normalised in doubles from the unrounded position and rounded to float: it differs from the
            # direction from the ROUNDED position by the position's rounding over the focus distance, plus its own rounding
            assert np.abs(vec(c.direction) - look).max() <= slack / (focus_distance - radius) + F32_EPS, (k, i)
            assert c.fov == cam.fov
            seen.add(c.point.tuple())
        assert len(seen) == k                                                                  # k different positions
    up = S.Camera()
    up.point, up.direction, up.fov = S.V3(0, 0, 0), S.V3(0, 1, 0), cam.fov
    with pytest.raises(ValueError):
        S.lens_cameras(up, 5.0, 0.3, 4)
