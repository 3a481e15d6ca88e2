"""The adaptive supersampling contract of lol_gpu_set_adaptive_samples (include/lol_gpu.h), restated on the CPU oracle. Test
infrastructure only.

P is the plain frame (oracle_lib.render_rows: its packed XRGB8888 pixels, and its hit ids in steps[..., 2]).  Pixel (x, y) is
refined when one of its 8 neighbours inside the frame has another id, or differs from it by more than T in one of the three
8-bit channels of P.  A refined pixel is the s x s pixel of aa_reference.render; any other pixel is P's, packed by
aa_reference.pack in the requested format.  Nothing here depends on the order in which refined pixels are computed.
"""
from __future__ import annotations

import numpy as np

import aa_reference as A
import oracle_lib as O


def channels(xrgb: np.ndarray) -> np.ndarray:
    """[..., 3] int32: the 8-bit channels r, g, b of XRGB8888 pixels"""
    x = xrgb.astype(np.uint32)
    return np.stack([(x >> 16) & 0xFF, (x >> 8) & 0xFF, x & 0xFF], axis=-1).astype(np.int32)


def mask(ids: np.ndarray, c8: np.ndarray, T: int) -> np.ndarray:
    """[h, w] bool: the refined pixels of a frame with object ids `ids` [h, w] and 8-bit channels `c8` [h, w, 3]"""
    ids = np.asarray(ids).astype(np.int64)
    c8 = np.asarray(c8).astype(np.int32)
    h, w = ids.shape
    m = np.zeros((h, w), dtype=bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            ys0, ys1 = max(0, -dy), min(h, h - dy)          # pixels whose neighbour (x + dx, y + dy) lies inside the frame
            xs0, xs1 = max(0, -dx), min(w, w - dx)
            if ys0 >= ys1 or xs0 >= xs1:
                continue
            here_id, there_id = ids[ys0:ys1, xs0:xs1], ids[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
            here_c, there_c = c8[ys0:ys1, xs0:xs1], c8[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
            m[ys0:ys1, xs0:xs1] |= (here_id != there_id) | (np.abs(here_c - there_c) > T).any(axis=-1)
    return m


def plain(scene, w: int, h: int, y0: int = 0, y1: int | None = None, max_steps: int = 256, camera=None):
    """(xrgb [h, w], rgb after gamma [h, w, 3], ids [h, w]) of P; only rows [y0, y1) are filled"""
    x1, rgb1, steps = O.render_rows(scene, w, h, y0, h if y1 is None else y1, max_steps, camera, want_steps=True)
    return x1, rgb1, steps[..., 2].astype(np.int64)


def combine(mask_: np.ndarray, plain_rgb, aa_x, aa_rgb, fmt=None):
    """the adaptive frame from its parts: the s x s pixels aa_x (already packed in `fmt`) / aa_rgb where mask_ is set; elsewhere
    P's colour after gamma, packed by aa_reference.pack ((Uint8)(c * 255) of the same floats gives P's 8-bit channels)"""
    px = np.where(mask_, aa_x, A.pack(plain_rgb, fmt))
    rgb = np.where(mask_[..., None], aa_rgb, plain_rgb)
    return px.astype(np.uint32), rgb.astype(np.float32)


def render(scene, w: int, h: int, s: int, T: int, fmt=None, max_steps: int = 256, camera=None, rows=None, full=None):
    """(packed [len(rows), w] uint32, rgb after gamma [len(rows), w, 3] float32, mask [len(rows), w] bool) of the adaptive frame's
    rows `rows` (default: all).  `full`: the whole s x s frame (aa_reference.render(scene, w, h, s, fmt=fmt)) where the caller has
    it."""
    if rows is None:
        rows = list(range(h))
        px, rgb, ids = plain(scene, w, h, 0, h, max_steps, camera)
        m = mask(ids, channels(px), T)
    else:                                       # only P's rows the mask of these rows reads: y - 1 ... y + 1
        rows = list(rows)
        px, rgb, m = np.zeros((len(rows), w), np.uint32), np.zeros((len(rows), w, 3), np.float32), np.zeros((len(rows), w), bool)
        for a, y in enumerate(rows):
            y0, y1 = max(0, y - 1), min(h, y + 2)
            x1, rgb1, ids1 = plain(scene, w, h, y0, y1, max_steps, camera)
            px[a], rgb[a] = x1[y], rgb1[y]
            m[a] = mask(ids1[y0:y1], channels(x1[y0:y1]), T)[y - y0]
    if full is None:
        aa_x, aa_rgb = A.render(scene, w, h, s, rows=rows, fmt=fmt, max_steps=max_steps, camera=camera)
    else:
        aa_x, aa_rgb = full[0][rows], full[1][rows]
    x, r = combine(m, rgb, aa_x, aa_rgb, fmt)
    return x, r, m
