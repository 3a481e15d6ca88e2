"""The contract of lol_gpu_light_views / lol_gpu_relight_views (include/lol_gpu.h, "Relit views"), restated on the CPU oracle.  Not a
test file.

The planes hold one element per LEAF: sample column X < s w, sample row Y < s h under cams[v K + k] is element
((v K + k) s h + Y) s w + X — record r = v K + k is light_reference.reference on the camera rays of the s w x s h frame under its camera.
A pixel is then: per leaf light_reference.relit_reference's rgb_linear under the look; per camera aa_reference.tree_mean over its s^2
leaves in order j s + i (s = 1: the leaf, unscaled); tree_mean over the K cameras in order of k (K = 1: m_0); oracle_lib.powf and
aa_reference.pack.  tests/test_light_views_reference.py holds this to aa_reference.render, blend_reference.render and
blend_aa_reference.render of the look's scene.
"""
import numpy as np

import aa_reference as A
import light_reference as LR
import oracle_lib as O
import ray_reference as R


def leaf_rays(sc, cams, w, h, s):
    """the rays of every leaf, in the order of the planes: per camera the camera rays of its s w x s h frame, row-major"""
    return np.concatenate([R.camera_rays(sc, s * w, s * h, camera=c) for c in cams])


def planes(sc, cams, w, h, s, max_steps=256):
    """light_reference.reference of every leaf, in the layout of the capture's planes"""
    return LR.reference(sc, leaf_rays(sc, cams, w, h, s), max_steps)


def resolve(leaves, n_views, k, w, h, s):
    """[n_views * h * w, 3] float32: steps 2 and 3 of the contract on the leaves' clamped linear colours ([N, 3], in the planes' order)"""
    a = np.ascontiguousarray(leaves, dtype=np.float32).reshape(n_views, k, h, s, w, s, 3)           # [v, k, y, j, x, i]
    a = a.transpose(0, 2, 4, 1, 3, 5, 6).reshape(n_views, h, w, k, s * s, 3)                        # [v, y, x, k, j s + i]
    m = A.tree_mean(a) if s > 1 else a[..., 0, :]                                                   # [v, y, x, k]
    out = A.tree_mean(m) if k > 1 else m[..., 0, :]
    return np.ascontiguousarray(out.reshape(-1, 3))


def finish(mean, fmt=None):
    """dict(rgb_linear, rgb [n, 3] f32, pixel [n] u32) of the means before gamma: step 4"""
    post = O.powf(mean, np.full(mean.shape, A.GAMMA, dtype=np.float32))
    return dict(rgb_linear=mean, rgb=post, pixel=A.pack(post, fmt))


def render(sc, look, cams, k, w, h, s, fmt=None, max_steps=256):
    """the outputs of lol_gpu_relight_views(look) over planes captured from `sc` under `cams`: dict(rgb_linear, rgb, pixel), dense
    over [view, y, x]"""
    cams = list(cams)
    assert len(cams) % k == 0
    leaves = LR.relit_reference(planes(sc, cams, w, h, s, max_steps), look)["rgb_linear"]
    return finish(resolve(leaves, len(cams) // k, k, w, h, s), fmt)
