"""The supersampling contract of lol_gpu_set_samples (include/lol_gpu.h), restated on the CPU oracle. Test infrastructure only.

Pixel (x, y) of a w x h frame with s x s samples: sample (i, j) is pixel (s x + i, s y + j) of the reference's s w x s h frame,
taken as the clamped LINEAR colour get_light() returns (lol_oracle_probe.rgb_linear); the samples, in order k = j s + i, are
summed per channel in float32 as a balanced binary tree and multiplied by 1 / s^2; the mean goes through the CPU's powf(c,
1 / 2.2f), (Uint8)(c * 255) and SDL_MapRGB's packing.  With s = 1 this is the plain frame (checked against oracle_lib.render).
"""
from __future__ import annotations

import numpy as np

import oracle_lib as O

GAMMA = np.float32(1.0) / np.float32(2.2)


def sample_colours(scene, w: int, h: int, s: int, rows, max_steps: int = 256, camera=None) -> np.ndarray:
    """[len(rows), w, s*s, 3] float32: the linear colours of every pixel's samples, in order k = j s + i."""
    out = np.zeros((len(rows), w, s * s, 3), dtype=np.float32)
    for a, y in enumerate(rows):
        for j in range(s):
            for x in range(w):
                for i in range(s):
                    p = O.probe(scene, s * w, s * h, s * x + i, s * y + j, max_steps, camera)
                    out[a, x, j * s + i] = np.array(p.rgb_linear, dtype=np.float32)
    return out


def tree_mean(v: np.ndarray) -> np.ndarray:
    """Mean over axis -2 (s*s samples, a power of two) in float32: pairs of neighbours first ((v0 + v1) + (v2 + v3) ...), then
    the sum times 1 / s^2."""
    n = v.shape[-2]
    acc = v.astype(np.float32)
    while acc.shape[-2] > 1:
        acc = (acc[..., 0::2, :] + acc[..., 1::2, :]).astype(np.float32)
    return (acc[..., 0, :] * np.float32(1.0 / n)).astype(np.float32)


def pack(post: np.ndarray, fmt=None) -> np.ndarray:
    """(Uint8)(c * 255) per channel, then SDL_MapRGB for a non-palettised 32-bit format (None = XRGB8888)."""
    c8 = (post.astype(np.float32) * np.float32(255.0)).astype(np.uint32) & np.uint32(0xFF)
    if fmt is None:
        shifts, losses, amask = (16, 8, 0), (0, 0, 0), 0
    else:
        shifts, losses, amask = (fmt.r_shift, fmt.g_shift, fmt.b_shift), (fmt.r_loss, fmt.g_loss, fmt.b_loss), fmt.a_mask
    px = np.full(post.shape[:-1], np.uint32(amask), dtype=np.uint32)
    for ch in range(3):
        px |= (c8[..., ch] >> np.uint32(losses[ch])) << np.uint32(shifts[ch])
    return px


def render(scene, w: int, h: int, s: int, rows=None, fmt=None, max_steps: int = 256, camera=None):
    """(xrgb [len(rows), w] uint32, rgb [len(rows), w, 3] float32 after gamma) of the frame rows `rows` (default: all)."""
    rows = list(range(h)) if rows is None else list(rows)
    mean = tree_mean(sample_colours(scene, w, h, s, rows, max_steps, camera))
    post = O.powf(mean, np.full(mean.shape, GAMMA, dtype=np.float32))
    return pack(post, fmt), post
