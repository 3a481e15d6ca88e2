"""tests/light_views_reference.py held to the contracts it composes.  No GPU.

The relit averaged pixel — light_reference.reference on the leaves' rays, relit_reference under the look, tree_mean over the samples,
then over the cameras, powf and pack — IS the supersampled frame of the look's scene for K = 1 (aa_reference.render), its blend for
s = 1 (blend_reference.render) and its supersampled blend otherwise (blend_aa_reference.render), bit for bit: the yardstick the device
is held to in tests/test_gpu_light_views.py."""
import numpy as np
import pytest

import aa_reference as A
import blend_aa_reference as BA
import blend_reference as B
import light_views_reference as LV
import ray_reference as R
from loltracer_amd import scene as S
from test_light_reference import looks_of

W, H = 13, 5
SHAPES = [(2, 1), (4, 1), (1, 4), (2, 2)]             # (s, K)
LOOKS = (None, 0, 2, 4)                               # the scene itself, and looks a, c and e of looks_of: tinted, material 0 lit, NaN


def cameras_of(sc, k):
    """K cameras of one view: the scene's own for K = 1, else an exposure between two neighbours of an orbit of 8"""
    if k == 1:
        return [B.copy_camera(sc.camera)]
    orbit = S.orbit_cameras(sc, 8)
    return S.shutter_cameras(orbit[0], orbit[1], k)


@pytest.mark.parametrize("s,k", SHAPES)
@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_relit_views_are_the_views_of_the_look(scenes, name, s, k):
    sc = scenes[name]
    cams = cameras_of(sc, k)
    looks = looks_of(sc)
    for which in LOOKS:
        what, look = ("itself", sc) if which is None else looks[which]
        got = LV.render(sc, look, cams, k, W, H, s)
        if k == 1:
            px, rgb = A.render(look, W, H, s, camera=cams[0])
        elif s == 1:
            px, rgb = B.render(look, cams, k, W, H)
        else:
            px, rgb = BA.render(look, cams, k, s, W, H)
        assert R.same_bits(got["rgb"], np.ascontiguousarray(rgb.reshape(-1, 3))).all(), (what, "rgb")
        assert np.array_equal(got["pixel"], px.ravel()), (what, "pixel")
        assert ((got["rgb_linear"] >= 0) & (got["rgb_linear"] <= 1)).all(), what


def test_the_layout_is_view_camera_row_column():
    """resolve() takes leaf (v, k, Y, X) from element ((v K + k) s h + Y) s w + X, sums a pixel's samples in order j s + i, then the
    cameras in order of k, each tree with its own scale"""
    n, k, w, h, s = 2, 2, 3, 2, 2
    N = n * k * s * s * w * h
    leaves = np.zeros((N, 3), np.float32)
    leaves[:, 0] = np.arange(N, dtype=np.float32)
    got = LV.resolve(leaves, n, k, w, h, s)[:, 0].reshape(n, h, w)
    for v in range(n):
        for y in range(h):
            for x in range(w):
                m = []
                for c in range(k):
                    e = [(((v * k + c) * s * h + s * y + j) * s * w + s * x + i) for j in range(s) for i in range(s)]
                    m.append(np.float32(np.float32(np.float32(e[0]) + np.float32(e[1])) + np.float32(np.float32(e[2]) + np.float32(e[3]))) * np.float32(.25))
                assert got[v, y, x] == np.float32(m[0] + m[1]) * np.float32(.5), (v, y, x)
    # one sample and one camera: the leaves themselves, unscaled
    assert np.array_equal(LV.resolve(leaves, 1, 1, N, 1, 1), leaves)


def test_the_inputs_discriminate(scenes):
    """the relit views differ from the plain relit frame of camera 0 and, for K > 1, from camera 0's supersampled frame alone: a
    resolve that ignored the samples or the cameras would not pass"""
    sc = scenes["scene4"]
    look = looks_of(sc)[0][1]
    plain = LV.render(sc, look, cameras_of(sc, 1), 1, W, H, 1)["pixel"]
    for s, k in SHAPES:
        cams = cameras_of(sc, k)
        got = LV.render(sc, look, cams, k, W, H, s)["pixel"]
        assert (got != LV.render(sc, look, cams[:1], 1, W, H, 1)["pixel"]).any(), (s, k)
        if k > 1:
            assert (got != LV.render(sc, look, cams[:1], 1, W, H, s)["pixel"]).any(), (s, k)
        else:
            assert (got != plain).any(), (s, k)
