"""The contract of lol_gpu_render_scene_views (include/lol_gpu.h), restated on the CPU oracle.  Test infrastructure only.

Record r of a call is the reference's frame of scenes[r] under cams[r].  With K = 1 a view is that frame (oracle_lib.render_rows and
probe on the record's own Scene).  With K > 1 it is blend_reference.render generalised to per-record scenes: sample k of view v is
the clamped linear colour of record v K + k, the K samples go through aa_reference.tree_mean, the CPU's powf and the packing.
Frames are cached per (scene object, camera bytes, size, max_steps) and left unchanged by every caller: keep the Scene objects alive
for as long as the cache is used (the tests hold them in module-level dictionaries).
"""
from __future__ import annotations

import numpy as np

import aa_reference as A
import blend_reference as B
import oracle_lib as O

_frames = {}


def frame(scene, cam, w: int, h: int, max_steps: int = 256) -> dict:
    """xrgb [h, w], rgb [h, w, 3] after gamma, id [h, w] and dist [h, w] of the reference's frame of `scene` under `cam`"""
    key = (id(scene), bytes(memoryview(cam).cast("B")), w, h, max_steps)
    if key not in _frames:
        ox, orgb, osteps = O.render_rows(scene, w, h, 0, h, max_steps, camera=cam, want_steps=True)
        dist = np.zeros((h, w), dtype=np.float32)
        for y in range(h):
            for x in range(w):
                dist[y, x] = O.probe(scene, w, h, x, y, max_steps, camera=cam).hit_dist
        out = dict(xrgb=ox, rgb=orgb, id=osteps[..., 2].astype(np.uint32), dist=dist)
        for a in out.values():
            a.setflags(write=False)
        _frames[key] = out
    return _frames[key]


def render_blend(scenes, cams, k: int, w: int, h: int, fmt=None, max_steps: int = 256):
    """(packed [n, h, w] uint32, rgb [n, h, w, 3] float32 after gamma) of the n = len(scenes) / k views of a blend over records"""
    scenes, cams = list(scenes), list(cams)
    assert k >= 1 and len(scenes) == len(cams) and len(scenes) % k == 0
    n = len(scenes) // k
    samples = np.zeros((n, h, w, k, 3), dtype=np.float32)
    for v in range(n):
        for j in range(k):
            samples[v, :, :, j, :] = B.linear_frame(scenes[v * k + j], cams[v * k + j], w, h, max_steps)
    mean = A.tree_mean(samples)
    post = O.powf(mean, np.full(mean.shape, A.GAMMA, dtype=np.float32))
    return A.pack(post, fmt), post
