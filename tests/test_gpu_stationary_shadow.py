"""The stationary exit of the shadow march on the device (lol_kernel.h, soft_shadow): a lane whose ray has stopped moving —
fl(t + s) == t — leaves the loop, and the turns it leaves out are counted apart.

Three things are held here, at 160 x 90, where every scene used has some hundreds of shadow rays that run all 128 turns:
  pixels and counts   the frame is the oracle's bit for bit and the REPORTED march and shadow step counts are the oracle's on every
                      pixel — both kernels (the scene's own and the interpreter), the fixed order and the repeated view after its
                      tables have settled; a shaded list query and a light pass report the same counts;
  executed steps      what the pixels are dealt by (lol_gpu_testing_pixel_cost) is at most what is reported, and on every pixel
                      that runs some light to 128 turns it is what a CPU replay of the march predicts (tests/shadow_replay.py).
Every test first asserts from the oracle that its frame holds at least 200 pixels with a per-light settled count of 128, so that it
cannot pass on a frame where the exit never fires.
"""
import os

import numpy as np
import pytest

import oracle_lib as O
import scene_shapes as C
import shadow_replay as SR
from loltracer_amd import gpu
from loltracer_amd import scene as S
from test_gpu_light import capture_pixels
from test_gpu_parity import HOST_LIBM_IS_FMA_VARIANT, check_against_oracle, gpu_render
from test_gpu_shades import all_pixels, shade_pixels

pytestmark = pytest.mark.gpu

W, H = 160, 90
NAMES = ["scene2", "scene3", "scene4", "three_lights"]
KERNELS = {"spec": (1, "lol_render_spec"), "interp": (4, "render_interp")}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_cache = {}


def scene_and_oracle(scenes, name):
    """(scene, the oracle's step planes at W x H, the pixels that run some light to 128 turns) — computed once per scene"""
    if name not in _cache:
        sc = scenes[name] if name in scenes else S.Scene.parse_file(os.path.join(C.SCENES_DIR, name + ".lol"))
        _, _, osteps = O.render_rows(sc, W, H, 0, H, 256, want_steps=True)
        osteps.setflags(write=False)
        full = (osteps[..., 8:12] == SR.TURNS).any(axis=-1)
        assert int(full.sum()) >= 200, f"{name}: only {int(full.sum())} pixels with a per-light settled count of 128"
        _cache[name] = (sc, osteps, full)
    return _cache[name]


def open_renderer(sc, kernel):
    r = gpu.Renderer(0, specialize=KERNELS[kernel][0])
    r.want_kernel = KERNELS[kernel][1]
    return r


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", NAMES)
def test_pixels_and_reported_counts_are_the_oracles(torch_cuda, scenes, name, kernel):
    sc, osteps, full = scene_and_oracle(scenes, name)
    r = open_renderer(sc, kernel)
    try:
        for what, repeat in (("fixed order", 1), ("repeated view", 5)):
            g = gpu_render(torch_cuda, r, sc, W, H, repeat=repeat)
            assert (r.tile_order()["order"] == "lpt") == (repeat > 1), (what, r.tile_order())
            mism = check_against_oracle(g, sc, W, H)          # march and shadow step counts of every pixel, colours, packed pixels
            assert mism == 0 if HOST_LIBM_IS_FMA_VARIANT else mism <= max(4, W * H // 2000), f"{name} {kernel} {what}: {mism} packed pixels differ"
    finally:
        r.close()


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", ["scene4", "three_lights"])
def test_a_list_query_and_a_light_pass_report_the_same_counts(torch_cuda, scenes, name, kernel):
    sc, osteps, full = scene_and_oracle(scenes, name)
    r = gpu.Renderer(0, specialize=KERNELS[kernel][0])
    try:
        r.set_shade_queries(True)
        r.prepare(sc)
        g = gpu_render(torch_cuda, r, sc, W, H)
        check_against_oracle(g, sc, W, H)
        got = shade_pixels(torch_cuda, r, all_pixels(W, H), W, H, want=("steps",))
        assert np.array_equal(got["steps"].reshape(H, W), g["steps"]), "a shaded list of every pixel reports other counts than the frame"
        # the light pass marches every light of every pixel (no dark or miss skip) up to the settled exit: per light, the oracle's
        # settled count
        assert r.miss_skip_active() & 4
        _, planes = capture_pixels(torch_cuda, r, W, H)
        nl = min(sc.c.n_lights, 4)
        assert np.array_equal(planes["steps"].reshape(H, W), osteps[..., 0])
        for li in range(nl):
            assert np.array_equal(planes["shadow_steps"][:, li].reshape(H, W), osteps[..., 8 + li]), f"light {li}"
        assert (planes["shadow_steps"][:, :nl].reshape(H, W, nl)[full] == SR.TURNS).any(axis=-1).all()
    finally:
        r.close()


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", ["scene4", "scene3"])
def test_executed_steps_are_the_replays(torch_cuda, scenes, name, kernel):
    """the table the pixels are dealt by holds what each pixel's lane RAN: never more than it reports, and for the pixels with a
    light that the oracle runs to 128 turns exactly the march steps plus, per light, the turns up to the settled exit or up to the
    turn after which the replayed ray stands still"""
    sc, osteps, full = scene_and_oracle(scenes, name)
    r = open_renderer(sc, kernel)
    try:
        g = gpu_render(torch_cuda, r, sc, W, H, repeat=3)       # the second frame records, the third is dealt by the record
        assert r.tile_order()["order"] == "lpt"
        skip = r.miss_skip_active()
        assert skip == 7
        cost = r.testing_pixel_cost(W, H).astype(np.int64)
        reported = (g["steps"] & 0xFFFF).astype(np.int64) + (g["steps"] >> 16).astype(np.int64)
        assert (cost <= reported).all()
        # per light: dark lights and escaped pixels are not marched at all; a settled count below 128 is an exit the replay need
        # not find (a ray that stood still would have run to 128); the others are replayed
        rays = SR.rays_run_to_the_end(osteps, sc.c.n_lights)
        rep = SR.replay(sc, *SR.shadow_rays(sc, W, H, rays))
        assert (rep["count"] == SR.TURNS).all() and (rep["settled"] == SR.TURNS).all(), "the replay does not reproduce the oracle's counts"
        ran = SR.executed(rep)
        want = osteps[..., 0].astype(np.int64)
        hit = osteps[..., 2] != 0
        for li in range(min(sc.c.n_lights, 4)):
            dark = ((osteps[..., 3] >> li) & 1) != 0
            want = want + np.where(hit & ~dark, osteps[..., 8 + li].astype(np.int64), 0)
        for (x, y, li), k in zip(rays, ran):
            want[y, x] -= SR.TURNS - int(k)
        some = full & hit
        saved = int((reported - cost)[some].sum())
        print(f"{name} {kernel}: {int(some.sum())} pixels run a light to 128 turns; {len(rays)} such rays, {int((ran < SR.TURNS).sum())} stationary; "
              f"turns left out {saved} of {int(reported[some].sum())} reported on those pixels")
        assert np.array_equal(cost[some], want[some]), f"{int((cost[some] != want[some]).sum())} pixels ran other counts than the replay"
        assert np.array_equal(cost[hit], want[hit]) and np.array_equal(cost[~hit], osteps[..., 0].astype(np.int64)[~hit])
        assert saved > 0
    finally:
        r.close()
