"""The fixed point the kernels' stationary exit rests on (lol_kernel.h, soft_shadow), replayed on the CPU: no GPU.

A turn of the reference's shadow march maps (t, res) to (fl(t + s), min(res, 50 s / t)) with s = sdf(fl(ro + dir t)).  Once
fl(t + s) == t, the next turn reads what this one read, so (t, res) never change again and the factor after 128 turns is the factor
at that turn.  The rays are recorded ones (tests/golden/stationary_shadow_rays.json: 64 of scene4 and 64 of scene3 that the oracle
marches for all 128 turns at 160 x 90, evenly spaced over all of them), given as float32 bit patterns, so nothing is reconstructed;
a second test ties the record to the oracle's own pixels.
"""
import numpy as np
import pytest

import oracle_lib as O
import shadow_replay as SR


@pytest.fixture(scope="module")
def golden():
    return SR.load_golden()


@pytest.mark.parametrize("name", ["scene4", "scene3"])
def test_a_ray_that_has_stopped_never_moves_again(scenes, golden, name):
    _, _, rays = golden
    g = rays[name]
    assert len(g["ro"]) >= 64
    rep = SR.replay(scenes[name], g["ro"], g["dir"], g["max_dist"])
    assert (rep["count"] == SR.TURNS).all(), "a recorded ray is not one the reference runs to 128 turns"
    k = rep["still"]
    stationary = k > 0
    print(f"{name}: {int(stationary.sum())} of {len(k)} rays become stationary; first at turn {int(k[stationary].min())}, "
          f"last at turn {int(k[stationary].max())}, mean {float(k[stationary].mean()):.1f}")
    assert stationary.mean() >= 0.8, f"only {int(stationary.sum())} of {len(k)} recorded rays become stationary"
    t, res = rep["t"].view(np.uint32), rep["res"].view(np.uint32)
    for i in np.flatnonzero(stationary):
        # columns k ... 128: the state after turns k, k + 1, ..., 128 — bit for bit the state after turn k
        assert (t[i, k[i]:] == t[i, k[i]]).all(), (name, i, int(k[i]))
        assert (res[i, k[i]:] == res[i, k[i]]).all(), (name, i, int(k[i]))
        at_k = np.float32(rep["res"][i, k[i]])
        factor_at_k = at_k if at_k > 0 else np.float32(0)                     # maxf(res, 0)
        assert np.float32(factor_at_k).view(np.uint32) == np.float32(rep["factor"][i]).view(np.uint32), (name, i, int(k[i]))
        assert rep["t"][i, k[i]] != 0, "a ray that never left its origin (the t == 0 fix-up's case) is not what is recorded here"
    # what a kernel runs: the turns up to k, never more than the reference's
    ex = SR.executed(rep)
    assert (ex[stationary] == np.minimum(k, rep["settled"])[stationary]).all() and (ex <= rep["count"]).all()


@pytest.mark.parametrize("name", ["scene4", "scene3"])
def test_the_recorded_rays_are_the_oracles(scenes, golden, name):
    """every recorded ray is the shadow ray of its pixel and light as the oracle builds it, the oracle counts 128 turns for it, and
    the replay's count and factor are the oracle's"""
    w, h, rays = golden
    g = rays[name]
    sc = scenes[name]
    _, _, osteps = O.render_rows(sc, w, h, 0, h, 256, want_steps=True)
    every = SR.rays_run_to_the_end(osteps, sc.c.n_lights)
    assert len(every) >= 200 and set(g["pixels"]) <= set(every)
    ro, rd, md = SR.shadow_rays(sc, w, h, g["pixels"])
    for got, want in ((ro, g["ro"]), (rd, g["dir"]), (md, g["max_dist"])):
        assert np.array_equal(SR.bits(got), SR.bits(want))
    rep = SR.replay(sc, ro, rd, md)
    for i, (x, y, li) in enumerate(g["pixels"]):
        p = O.probe(sc, w, h, x, y)
        assert p.shadow_steps[li] == rep["count"][i] == osteps[y, x, 4 + li] == SR.TURNS
        assert osteps[y, x, 8 + li] == rep["settled"][i]
        assert np.float32(p.shadow[li]).view(np.uint32) == np.float32(rep["factor"][i]).view(np.uint32), (x, y, li)
