"""Supersampling (lol_gpu_set_samples) without a device: the CPU restatement of the contract anchors itself to the oracle, the
C ABI declares and exports the new entry points, and the scene compiler's module gains lol_render_spec_aa only when asked."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aa_reference as A
import oracle_lib as O
from loltracer_amd import gpu, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ["scene", "scene2", "scene3", "scene4"]
ERR_ARG = -3                    # LOL_GPU_ERR_ARG (include/lol_gpu.h)


def load(name):
    return S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol"))


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("size", [(23, 17), (16, 9)])
def test_one_sample_is_the_oracle_frame(name, size):
    """s = 1 of the restatement is the reference's frame, packed pixels and colours after gamma, bit for bit."""
    sc = load(name)
    w, h = size
    xrgb, rgb = A.render(sc, w, h, 1)
    ox, orgb, _ = O.render(sc, w, h, want_rgb=True)
    assert np.array_equal(xrgb, ox)
    assert np.array_equal(rgb.view(np.uint32), orgb.view(np.uint32))


def test_tree_mean_is_the_pairwise_order():
    v = np.array([[1e8, 1.0, -1e8, 1.0]], dtype=np.float32)[..., None]
    got = A.tree_mean(v)[0, 0]
    want = (np.float32(np.float32(1e8) + np.float32(1.0)) + np.float32(np.float32(-1e8) + np.float32(1.0))) * np.float32(0.25)
    assert got == want
    assert got != np.float32(0.5)                  # (a left-to-right sum would keep both ones)


def test_samples_are_the_reference_pixels_of_the_larger_frame():
    """A sample is a pixel of the s w x s h frame: with every sample equal to the mean, s = 2 would be that frame's pixel."""
    sc = load("scene4")
    w, h, s = 9, 7, 2
    v = A.sample_colours(sc, w, h, s, [3])
    p = O.probe(sc, s * w, s * h, s * 4 + 1, s * 3 + 1)
    assert np.array_equal(v[0, 4, 1 * s + 1], np.array(p.rgb_linear, dtype=np.float32))


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(lol_[a-z0-9_]+)\s*\(", text))


def test_new_entry_points_are_declared_and_exported():
    lib = C.CDLL(os.path.join(S.LIB_DIR, "liblol_gpu.so"))
    pub = {"lol_gpu_set_samples", "lol_gpu_samples", "lol_gpu_multi_set_samples"}
    assert pub <= declared("lol_gpu.h")
    assert "lol_gpu_compile_offline_samples" in declared("lol_gpu_diag.h")
    for n in pub | {"lol_gpu_compile_offline_samples"}:
        assert getattr(lib, n) is not None


def test_samples_entry_points_refuse_without_a_context():
    lib = gpu.gpu_lib()
    assert lib.lol_gpu_set_samples(None, 2) == ERR_ARG
    assert lib.lol_gpu_multi_set_samples(None, 2) == ERR_ARG


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("name", ["scene4", "scene"])
def test_offline_module_with_and_without_supersampling(name, tmp_path):
    prog = load(name).flatten()
    plain = str(tmp_path / "plain")
    gpu.compile_offline(prog, plain)
    one = str(tmp_path / "one")
    gpu.compile_offline_samples(prog, one, 1)
    # samples = 1: exactly lol_gpu_compile_offline's source and code object
    assert _read(one + ".hip") == _read(plain + ".hip")
    assert _read(one + ".co") == _read(plain + ".co")
    assert b"lol_render_spec_aa" not in _read(plain + ".co")
    base = _read(plain + ".hip")
    for s in (2, 4):
        out = str(tmp_path / f"aa{s}")
        gpu.compile_offline_samples(prog, out, s)
        src = _read(out + ".hip")
        assert src.startswith(base) and len(src) > len(base)
        tail = src[len(base):].decode()
        assert tail.startswith('#include "lol_kernel_aa.h"\n')
        assert "lol_render_spec_aa" in tail and "lol_render_spec(" not in tail
        co = _read(out + ".co")
        assert co[:4] == b"\x7fELF" and b"lol_render_spec_aa" in co
        for k in (b"lol_render_spec\x00", b"lol_sdf_spec"):
            assert k in co
    # s = 2 and s = 4 compile the same module: s is read at run time
    assert _read(str(tmp_path / "aa2") + ".hip") == _read(str(tmp_path / "aa4") + ".hip")


def test_offline_refuses_other_sample_counts(tmp_path):
    prog = load("scene4").flatten()
    lib = gpu.gpu_lib()
    log = C.create_string_buffer(256)
    for s in (0, 3, 5, 8, -1):
        st = lib.lol_gpu_compile_offline_samples(C.byref(prog), b"gfx950", os.fsencode(str(tmp_path / "x")), 0, s, log, len(log))
        assert st == ERR_ARG
    assert not os.path.exists(str(tmp_path / "x.hip"))
