"""tests/shade_reference.py held to the oracle, and the populations the GPU tests of shading queries rely on.  No GPU.

lol_oracle_probe_pixel follows naive_renderer.c:217-235 for one pixel; shade_reference.shade follows :225-229 for one ray with the eye
at the ray's origin.  Fed the probe's own ray (probe.rd from the camera's position) the two must agree field by field, bit for bit:
hit_dist, hit_id, march_steps, shadow[], shadow_steps[] and rgb_linear — and gamma() / pack() give the probe's rgb and xrgb."""
import glob
import os

import numpy as np
import pytest

import oracle_lib as O
import ray_reference as R
import shade_reference as SR
from loltracer_amd import gpu
from loltracer_amd import scene as S

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTILE_FILE = sorted(glob.glob(os.path.join(HERE, "golden", "hostile", "*.lol")))[0]
SIZES = ((13, 5, 256), (16, 9, 7))
SEED = 20261018


def hold_to_probe(sc, w, h, max_steps):
    """every pixel of the frame; returns per pixel (id, [shadow factor per light])"""
    rays = R.camera_rays(sc, w, h)
    ref = SR.reference(sc, rays, max_steps)
    n_lights = min(len(sc.lights()), O.PROBE_LIGHTS)
    seen = []
    for y in range(h):
        for x in range(w):
            p, i = O.probe(sc, w, h, x, y, max_steps), y * w + x
            s = SR.shade(sc, rays[i, :3], rays[i, 3:], max_steps)
            want = dict(dist=np.float32(p.hit_dist), id=np.uint32(p.hit_id), steps=np.uint32(p.march_steps),
                        shadow=np.array(p.shadow[:n_lights], np.float32), shadow_steps=np.array(p.shadow_steps[:n_lights], np.uint32),
                        rgb_linear=np.array(tuple(p.rgb_linear), np.float32))
            got = dict(dist=s["dist"], id=np.uint32(s["id"]), steps=np.uint32(s["steps"]), shadow=np.array(s["shadow"][:n_lights], np.float32),
                       shadow_steps=np.array(s["shadow_steps"][:n_lights], np.uint32), rgb_linear=np.array(s["rgb_linear"], np.float32))
            for f in want:
                assert R.same_bits(got[f], want[f]).all(), (x, y, max_steps, f, got[f], want[f])
            # ... and the outputs' layout: gamma, packing, the two step counts in one word
            assert R.same_bits(ref["rgb_linear"][i], want["rgb_linear"]).all() and R.same_bits(ref["rgb"][i], np.array(tuple(p.rgb), np.float32)).all()
            assert ref["pixel"][i] == p.xrgb, (x, y, hex(ref["pixel"][i]), hex(p.xrgb))
            if len(sc.lights()) <= O.PROBE_LIGHTS:
                assert ref["steps"][i] == (p.march_steps & 0xFFFF) | (sum(p.shadow_steps[:n_lights]) << 16)
            seen.append((int(p.hit_id), [float(v) for v in s["shadow"]]))
    return seen


@pytest.mark.parametrize("w,h,max_steps", SIZES)
@pytest.mark.parametrize("name", ["scene", "scene2", "scene3", "scene4"])
def test_example_scenes_are_the_probe(scenes, name, w, h, max_steps):
    hold_to_probe(scenes[name], w, h, max_steps)


@pytest.mark.parametrize("w,h,max_steps", SIZES)
def test_the_hostile_scene_is_the_probe(w, h, max_steps):
    hold_to_probe(S.Scene.parse_file(HOSTILE_FILE), w, h, max_steps)


def populations(seen):
    escaped = sum(1 for i, _ in seen if i == 0)
    hits = [sh for i, sh in seen if i != 0]
    zero = sum(1 for sh in hits if any(v == 0.0 for v in sh))
    partial = sum(1 for sh in hits if any(0.0 < v < 1.0 for v in sh))
    full = sum(1 for sh in hits if any(v == 1.0 for v in sh))
    return escaped, zero, partial, full


def test_the_populations_the_gpu_tests_rely_on(scenes):
    """the 13 x 5 frames hold escaped rays, rays in full shadow, in none — and scene4 rays in partial shadow (scene.lol has none at
    that size, so none is demanded of it)"""
    escaped, zero, partial, full = populations(hold_to_probe(scenes["scene4"], 13, 5, 256))
    assert escaped > 0 and zero > 0 and partial > 0 and full > 0, (escaped, zero, partial, full)
    escaped, zero, partial, full = populations(hold_to_probe(scenes["scene"], 13, 5, 256))
    assert escaped > 0 and zero > 0 and full > 0, (escaped, zero, partial, full)


def test_shade_ray_set_holds_what_it_says(scenes):
    for name in ("scene4", "scene"):
        sc = scenes[name]
        rays = SR.shade_ray_set(sc, SEED)
        base = R.ray_set(sc, SEED)
        assert rays.dtype == np.float32 and rays.shape[1] == 6 and not rays.flags.writeable and SR.shade_ray_set(sc, SEED) is rays
        assert len(rays) % 64 == 0 and len(rays) >= len(base) + 128
        assert np.array_equal(rays[:len(base)].view(np.uint32), base.view(np.uint32))
        ids = SR.reference(sc, rays)["id"]
        w = SR.waves(ids)
        assert any(all_escaped for all_escaped, _ in w), "no wave of escaped rays alone"
        assert any(mixed for _, mixed in w), "no wave that mixes escaped rays and hits"
        assert w[-2] == (True, False) and w[-1] == (False, True)
        assert (ids[-64::2] == 0).all() and (ids[-63::2] != 0).all()         # (f)'s second half alternates


def test_pack_follows_the_pixel_format():
    rgb = np.array([[1.0, 0.5, 0.0], [0.25, 0.75, 0.999]], np.float32)
    assert SR.pack(rgb).tolist() == [0xFF7F00, (63 << 16) | (191 << 8) | 254]
    fmt = gpu.PixelFormat(11, 5, 0, 3, 2, 3, 4, 0, 0xFF000000)               # RGB565's shifts and losses in 32 bits, with an alpha mask
    assert SR.pack(rgb, fmt).tolist() == [0xFF000000 | (31 << 11) | (31 << 5), 0xFF000000 | (7 << 11) | (47 << 5) | 31]
