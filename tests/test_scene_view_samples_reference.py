"""Supersampled scene views, the part that needs no GPU: the contract restated on the oracle (tests/scene_view_samples_reference.py) is
the scene views' where s = 1, the supersampled blend's where every record carries one scene, the supersampled frame's of a record's
own scene where K = 1 — and the inputs the GPU tests render tell a kernel that ignores s, the record's scene, or all records but
the first of a group, from a right one."""
import numpy as np
import pytest

import aa_reference as A
import blend_aa_reference as BA
import scene_view_samples_reference as R
import scene_views_reference as SVR
import test_gpu_scene_views as SV

W, H, MAX_STEPS = R.W, R.H, R.MAX_STEPS


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_one_sample_is_the_scene_views(scenes):
    scs, cams = R.single_case(scenes, "scene4")
    px, rgb = R.render(scs, cams, 1, 1, W, H, max_steps=MAX_STEPS)
    for v in range(3):
        f = SVR.frame(scs[v], cams[v], W, H, MAX_STEPS)
        assert np.array_equal(px[v], f["xrgb"]) and np.array_equal(bits(rgb[v]), bits(f["rgb"])), v
    for k in (2, 4):
        scs, cams = R.blend_case(scenes, "scene4", k)
        px, rgb = R.render(scs, cams, k, 1, W, H, max_steps=MAX_STEPS)
        bpx, brgb = SVR.render_blend(scs, cams, k, W, H, max_steps=MAX_STEPS)
        assert np.array_equal(px, bpx) and np.array_equal(bits(rgb), bits(brgb)), k


def test_equal_scenes_in_every_record_is_the_supersampled_blend(scenes):
    sc = scenes["scene4"]
    for k, s in ((2, 2), (2, 4)):
        cams = BA.shutter_groups(sc, 2, k)
        px, rgb = R.render([sc] * len(cams), cams, k, s, W, H, max_steps=MAX_STEPS)
        bpx, brgb = BA.render(sc, cams, k, s, W, H, max_steps=MAX_STEPS)
        assert np.array_equal(px, bpx) and np.array_equal(bits(rgb), bits(brgb)), (k, s)


@pytest.mark.parametrize("s", R.SINGLE_SAMPLES)
def test_one_record_is_the_supersampled_frame_of_its_own_scene(scenes, s):
    scs, cams = R.single_case(scenes, "scene4")
    px, rgb = R.render(scs, cams, 1, s, W, H, max_steps=MAX_STEPS)
    for v in range(3):
        apx, argb = A.render(scs[v], W, H, s, max_steps=MAX_STEPS, camera=cams[v])
        assert np.array_equal(px[v], apx) and np.array_equal(bits(rgb[v]), bits(argb)), v


@pytest.mark.parametrize("name", R.NAMES)
def test_the_gpu_inputs_discriminate(scenes, name):
    """For every case the GPU tests render and every view, the packed reference differs in a pixel from the s = 1 result (a kernel that
    ignores s would pass otherwise); for K = 1 from the supersampled frame of the UPLOADED base scene under the same camera (... that
    ignores the record's scene); for K > 1 from the supersampled frame of the group's first record alone (... all records but one)."""
    base = SV.base_scene(scenes, name)
    for what, scs, cams, k, s in R.gpu_cases(scenes, name):
        px, _ = R.render(scs, cams, k, s, W, H, max_steps=MAX_STEPS)
        one_sample, _ = R.render(scs, cams, k, 1, W, H, max_steps=MAX_STEPS)
        if k == 1:
            other, _ = R.render([base] * len(cams), cams, 1, s, W, H, max_steps=MAX_STEPS)
        else:
            other, _ = R.render(scs[::k], cams[::k], 1, s, W, H, max_steps=MAX_STEPS)
        for v in range(len(scs) // k):
            assert (px[v] != one_sample[v]).any(), (name, what, v, "equals the s = 1 result")
            assert (px[v] != other[v]).any(), (name, what, v, "equals the base scene's frame" if k == 1 else "equals the first record's frame")
