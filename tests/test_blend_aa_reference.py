"""Supersampled blends, the part that needs no GPU: the contract restated on the oracle (tests/blend_aa_reference.py) is the blend's
where s = 1, the supersampled frame's where K = 1 or the cameras are equal, and the inputs the GPU tests render tell a kernel that
ignores s, or all cameras but one, from a right one."""
import numpy as np
import pytest

import aa_reference as A
import blend_aa_reference as BA
import blend_reference as B
from loltracer_amd import scene as S

W, H, N = BA.W, BA.H, BA.N


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", ["scene", "scene4"])
def test_one_sample_is_the_blend(scenes, name):
    sc = scenes[name]
    for k in (1, 2, 4):
        cams = BA.shutter_groups(sc, N, k)
        px, rgb = BA.render(sc, cams, k, 1, W, H)
        bpx, brgb = B.render(sc, cams, k, W, H)
        assert np.array_equal(px, bpx) and np.array_equal(bits(rgb), bits(brgb)), k


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("name", ["scene", "scene4"])
def test_one_camera_is_the_supersampled_frame(scenes, name, s):
    sc = scenes[name]
    cams = S.orbit_cameras(sc, 8)[:N]
    px, rgb = BA.render(sc, cams, 1, s, W, H)
    for v, cam in enumerate(cams):
        apx, argb = A.render(sc, W, H, s, camera=cam)
        assert np.array_equal(px[v], apx) and np.array_equal(bits(rgb[v]), bits(argb)), v


@pytest.mark.parametrize("k", [2, 4, 8, 16])
def test_equal_cameras_are_the_supersampled_frame_bit_for_bit(scenes, k):
    """doubling and a power-of-two scale are exact on [0, 1]: K copies of one camera are that camera's supersampled frame"""
    sc = scenes["scene4"]
    cams = S.orbit_cameras(sc, 8)[:N]
    for s in (2, 4):
        one_px, one_rgb = BA.render(sc, cams, 1, s, W, H)
        px, rgb = BA.render(sc, [B.copy_camera(c) for c in cams for _ in range(k)], k, s, W, H)
        assert np.array_equal(px, one_px) and np.array_equal(bits(rgb), bits(one_rgb)), s


@pytest.mark.parametrize("name", ["scene", "scene4"])
def test_the_gpu_inputs_discriminate(scenes, name):
    """For every (cameras, K, s) the GPU tests render, the reference differs in a packed pixel of EVERY view from the blend with one
    sample per pixel (a kernel that ignores s would pass otherwise) and from the supersampled view under the group's first camera
    alone (... that ignores all cameras but one)."""
    sc = scenes[name]
    for what, cams, k, s in BA.gpu_cases(sc):
        px, _ = BA.render(sc, cams, k, s, W, H)
        one_sample, _ = B.render(sc, cams, k, W, H)
        first, _ = BA.render(sc, cams[::k], 1, s, W, H)
        for v in range(len(cams) // k):
            assert (px[v] != one_sample[v]).any(), (what, v, "equals the s = 1 blend")
            assert (px[v] != first[v]).any(), (what, v, "equals the supersampled view under camera 0 of the group")


def test_the_two_trees_are_not_one_tree():
    """the order of rounding the contract fixes — 1 / s^2 per camera, then the tree over the cameras — differs from one tree over
    K s^2 leaves on subnormal channels: the smallest subnormal under every sample of one camera, zero under the other"""
    tiny = np.float32(2.0 ** -149)
    leaves = np.zeros((2, 4, 3), dtype=np.float32)
    leaves[0] = tiny                                           # camera 0: four samples of 2^-149; camera 1: four of 0
    per_camera = A.tree_mean(A.tree_mean(leaves)[None])        # (4 tiny) / 4 = tiny exactly; (tiny + 0) / 2 rounds to even: 0
    one_tree = A.tree_mean(leaves.reshape(1, 8, 3))            # (4 tiny) / 8 = tiny / 2 rounds to even: 0
    assert bits(per_camera).tolist() == [[0, 0, 0]] and bits(one_tree).tolist() == [[0, 0, 0]]
    leaves[1, 0] = tiny                                        # ... and one sample of 2^-149 under camera 1
    per_camera = A.tree_mean(A.tree_mean(leaves)[None])        # m_1 = tiny / 4 -> 0; (tiny + 0) / 2 -> 0
    one_tree = A.tree_mean(leaves.reshape(1, 8, 3))            # (5 tiny) / 8 = 0.625 tiny -> tiny
    assert bits(per_camera).tolist() == [[0, 0, 0]] and bits(one_tree).tolist() == [[1, 1, 1]]
