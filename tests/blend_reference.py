"""The contract of lol_gpu_render_views_blend (include/lol_gpu.h), restated on the CPU oracle.  Test infrastructure only.

Pixel (x, y) of view v of a blend with K cameras per view: sample k is pixel (x, y) of the reference's w x h frame under
cams[v K + k], taken as the clamped LINEAR colour get_light() returns (lol_oracle_probe.rgb_linear); the K samples, in order of k,
are summed per channel in float32 as a balanced binary tree and multiplied by 1 / K (aa_reference.tree_mean); the mean goes through
the CPU's powf(c, 1 / 2.2f), (Uint8)(c * 255) and SDL_MapRGB's packing (aa_reference.pack).  With K = 1 this is the plain frame
(checked against oracle_lib.render in tests/test_blend_reference.py).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import aa_reference as A
import oracle_lib as O

_linear = {}


def linear_frame(scene, cam, w: int, h: int, max_steps: int = 256) -> np.ndarray:
    """[h, w, 3] float32: the clamped linear colour of every pixel of the reference's frame under `cam`.  Cached per (scene, camera
    bytes, size, max_steps): left unchanged by every caller."""
    key = (id(scene), bytes(memoryview(cam).cast("B")), w, h, max_steps)
    if key not in _linear:
        out = np.zeros((h, w, 3), dtype=np.float32)
        for y in range(h):
            for x in range(w):
                out[y, x] = np.array(O.probe(scene, w, h, x, y, max_steps, cam).rgb_linear, dtype=np.float32)
        out.setflags(write=False)
        _linear[key] = out
    return _linear[key]


def render(scene, cams, k: int, w: int, h: int, fmt=None, max_steps: int = 256):
    """(packed [n, h, w] uint32, rgb [n, h, w, 3] float32 after gamma) of the n = len(cams) / k views"""
    cams = list(cams)
    assert k >= 1 and len(cams) % k == 0
    n = len(cams) // k
    samples = np.zeros((n, h, w, k, 3), dtype=np.float32)
    for v in range(n):
        for j in range(k):
            samples[v, :, :, j, :] = linear_frame(scene, cams[v * k + j], w, h, max_steps)
    mean = A.tree_mean(samples)
    post = O.powf(mean, np.full(mean.shape, A.GAMMA, dtype=np.float32))
    return A.pack(post, fmt), post


def copy_camera(c):
    out = type(c)()
    C.memmove(C.byref(out), C.byref(c), C.sizeof(c))
    return out
