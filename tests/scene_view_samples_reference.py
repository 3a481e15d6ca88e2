"""The contract of lol_gpu_render_scene_views_samples (include/lol_gpu.h), restated on the CPU oracle.  Test infrastructure only.

Pixel (x, y) of view v of a call with K records per view and s x s samples per pixel:
  1. for each k, m_k is the linear mean of the supersampling contract taken on record v K + k's OWN Scene under its camera
     (blend_aa_reference.camera_mean: the s^2 clamped linear colours of pixels (s x + i, s y + j) of the reference's s w x s h
     frame of that scene, in order j s + i, as a balanced binary32 tree, times 1 / s^2);
  2. m_0 ... m_{K - 1} are summed as the same kind of tree and multiplied by 1 / K (aa_reference.tree_mean);
  3. the CPU's powf(c, 1 / 2.2f) (oracle_lib.powf) and the packing (aa_reference.pack).
Two trees, one after the other.  The means are cached per (scene object, camera bytes, s, size, max_steps) by camera_mean: keep the
Scene objects alive for as long as the cache is used (the inputs below are held by tests/test_gpu_scene_views.py's dictionary).

Also the inputs of tests/test_gpu_scene_view_samples.py, stated here so that tests/test_scene_view_samples_reference.py can hold them
to "they discriminate" on the CPU.
"""
from __future__ import annotations

import numpy as np

import aa_reference as A
import blend_aa_reference as BA
import oracle_lib as O
import test_gpu_scene_views as SV
import test_gpu_views as V

# 33 x 17 pixels: sample grids of 66 x 34 (s = 2) and 132 x 68 (s = 4) — partial 16 x 4 tiles in x for both, in y for s = 2 (with
# four rows to a tile, s = 4 can never be ragged in y)
W, H = 33, 17
MAX_STEPS = 256
NAMES = ("scene4", "scene", "shape")
SINGLE_SAMPLES = (2, 4)                              # K = 1: variants() under three_cameras()
BLENDS = ((2, 2), (4, 2), (2, 4))                    # (K, s): moving(name, 2, K) under the base camera


def render(scenes, cams, k: int, s: int, w: int, h: int, fmt=None, max_steps: int = 256):
    """(packed [n, h, w] uint32, rgb [n, h, w, 3] float32 after gamma) of the n = len(scenes) / k views"""
    scenes, cams = list(scenes), list(cams)
    assert k >= 1 and len(scenes) == len(cams) and len(scenes) % k == 0
    n = len(scenes) // k
    means = np.zeros((n, h, w, k, 3), dtype=np.float32)
    for v in range(n):
        for j in range(k):
            means[v, :, :, j, :] = BA.camera_mean(scenes[v * k + j], cams[v * k + j], s, w, h, max_steps)
    mean = A.tree_mean(means)
    post = O.powf(mean, np.full(mean.shape, A.GAMMA, dtype=np.float32))
    return A.pack(post, fmt), post


def single_case(scenes, name):
    """(scenes, cameras) of the K = 1 cases: three records, every one under a scene and a camera of its own"""
    return SV.variants(scenes, name), SV.three_cameras(SV.base_scene(scenes, name))


def blend_case(scenes, name, k):
    """(scenes, cameras) of a K > 1 case: two views, each the exposure of k scenes of a moving object, under the base camera"""
    scs = SV.moving(scenes, name, 2, k)
    return scs, [V.copy_camera(SV.base_scene(scenes, name).camera)] * len(scs)


def gpu_cases(scenes, name):
    """[(what, scenes, cameras, K, s)]: what the GPU tests render of the scene called `name`"""
    out = [("K=1 s=%d" % s,) + single_case(scenes, name) + (1, s) for s in SINGLE_SAMPLES]
    out += [("K=%d s=%d" % (k, s),) + blend_case(scenes, name, k) + (k, s) for k, s in BLENDS]
    return out
