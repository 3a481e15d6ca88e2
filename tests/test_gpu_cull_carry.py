"""The culling bound carried along a ray (lol_codegen.hip, carry_constants) changes no pixel: whole frames against the oracle — scene4 at
the C3 size in the repeated view and in a fixed tile order, scene.lol at the C2 size with the carry forced on — and random scenes of
tests/tools/soak.py (plain and stress) with the carry forced on.  The bound itself is proven in tests/test_cull_carry_bound.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from loltracer_amd import gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4


def whole_frame(torch, r, sc, w, h, steps, frames):
    r.prepare(sc)
    assert r.kernel_name() == "lol_render_spec", r.specialize_log()
    buf = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    for _ in range(frames):
        r.render_into(buf.data_ptr(), w, h, steps)
    r.sync()
    return buf.cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("carry", [None, "1"], ids=["default", "forced"])
def test_whole_frames_equal_the_oracle(scenes, monkeypatch, carry):
    import torch
    if carry is not None:
        monkeypatch.setenv("LOL_GPU_TUNING", "1")          # (the library honours A/B switches only beside this)
        monkeypatch.setenv("LOL_GPU_CULL_CARRY", carry)
    cases = [("scene4", 3840, 2160, 256)] if carry is None else [("scene", 1920, 1080, 128)]
    for name, w, h, steps in cases:
        sc = scenes[name]
        want, _, _ = O.render(sc, w, h, steps, threads=THREADS)
        r = gpu.Renderer(0)
        got = whole_frame(torch, r, sc, w, h, steps, 5)            # the repeated view: pixels dealt by cost, waves longest first
        assert r.tile_order()["order"] == "lpt"
        assert np.array_equal(got, want), f"{name} {w}x{h} repeated view: {(got != want).sum()} pixels differ"
        r.set_tile_order("rows")
        got = whole_frame(torch, r, sc, w, h, steps, 1)            # a fixed order
        assert np.array_equal(got, want), f"{name} {w}x{h} rows: {(got != want).sum()} pixels differ"
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [[], ["stress"], ["still", "stress"]], ids=["plain", "stress", "still-stress"])
def test_random_scenes_with_the_carry_forced_on(mode):
    env = dict(os.environ, LOL_GPU_TUNING="1", LOL_GPU_CULL_CARRY="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "soak.py"), "12", "7707"] + mode,
                         cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:]
    assert "total 12 bad 0" in out.stdout, out.stdout[-3000:]
