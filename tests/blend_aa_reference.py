"""The contract of lol_gpu_render_views_blend_samples (include/lol_gpu.h), restated on the CPU oracle.  Test infrastructure only.

Pixel (x, y) of view v of a blend with K cameras per view and s x s samples per pixel:
  1. for each k, m_k is the linear mean of the supersampling contract under cams[v K + k]: the s^2 clamped LINEAR colours of the
     pixels (s x + i, s y + j) of the reference's s w x s h frame (aa_reference.sample_colours), in order j s + i, summed per
     channel in float32 as a balanced binary tree and multiplied by 1 / s^2 (aa_reference.tree_mean);
  2. m_0 ... m_{K - 1}, in order of k, are summed as the same kind of tree and multiplied by 1 / K (aa_reference.tree_mean again);
  3. the result goes through the CPU's powf(c, 1 / 2.2f) (oracle_lib.powf), (Uint8)(c * 255) and SDL_MapRGB's packing
     (aa_reference.pack).
Two trees, one after the other, each with its own scale: NOT one tree over K s^2 leaves.
"""
from __future__ import annotations

import numpy as np

import aa_reference as A
import oracle_lib as O
from loltracer_amd import scene as S

_means = {}


def camera_mean(scene, cam, s: int, w: int, h: int, max_steps: int = 256) -> np.ndarray:
    """[h, w, 3] float32: step 1, the linear mean m of every pixel's s x s samples under `cam`.  Cached per (scene, camera bytes, s,
    size, max_steps): computed once, shared by every test that needs it, left unchanged by every caller."""
    key = (id(scene), bytes(memoryview(cam).cast("B")), s, w, h, max_steps)
    if key not in _means:
        m = A.tree_mean(A.sample_colours(scene, w, h, s, range(h), max_steps, camera=cam))
        m.setflags(write=False)
        _means[key] = m
    return _means[key]


def render(scene, cams, k: int, s: int, w: int, h: int, fmt=None, max_steps: int = 256):
    """(packed [n, h, w] uint32, rgb [n, h, w, 3] float32 after gamma) of the n = len(cams) / k views"""
    cams = list(cams)
    assert k >= 1 and len(cams) % k == 0
    n = len(cams) // k
    means = np.zeros((n, h, w, k, 3), dtype=np.float32)
    for v in range(n):
        for j in range(k):
            means[v, :, :, j, :] = camera_mean(scene, cams[v * k + j], s, w, h, max_steps)
    mean = A.tree_mean(means)
    post = O.powf(mean, np.full(mean.shape, A.GAMMA, dtype=np.float32))
    return A.pack(post, fmt), post


# ---- the inputs of tests/test_gpu_view_blend_samples.py, stated here so that tests/test_blend_aa_reference.py can hold them to
# "they discriminate" on the CPU: 37 x 11 pixels (sample grids of 74 x 22 and 148 x 44, ragged against the 16 x 4 tile on both axes)
# and three views (the view in the grid's z, more than one group of cameras)
W, H, N = 37, 11, 3
SHUTTERS = ((2, 2), (4, 2), (2, 4))      # (K, s) of the shutter groups
LENS = (16, 2)                           # ... and of the lens: one view
LENS_FOCUS, LENS_RADIUS = 6.0, 0.25


def shutter_groups(sc, n, k, first=0):
    """n views, each the exposure between two neighbours of an orbit of 8: n k cameras (test_gpu_view_blends.shutter_groups)"""
    orbit = S.orbit_cameras(sc, 8)
    cams = []
    for v in range(n):
        cams += S.shutter_cameras(orbit[(first + v) % 8], orbit[(first + v + 1) % 8], k)
    return cams


def gpu_cases(sc):
    """[(what, cameras, K, s)]: what the GPU tests render of scene `sc`"""
    out = [("shutter K=%d s=%d" % (k, s), shutter_groups(sc, N, k), k, s) for k, s in SHUTTERS]
    out.append(("lens K=%d s=%d" % LENS, S.lens_cameras(sc.camera, LENS_FOCUS, LENS_RADIUS, LENS[0]), LENS[0], LENS[1]))
    return out
