"""Every kernel family on every interpreter rung and every form of the scene compiler (tests/scene_shapes.py).

The families beside the plain frame — supersampled frames (`_aa`), the refine pass of adaptive frames (`_aa_list`), batches of views
(`_batch`), supersampled and adaptive batches (`_batch_aa`, `_batch_aa_list`) — exist once per rung of the interpreter's ladder (eight
rungs, lol_gpu.hip interp_rung) and once per form of the scene's own module (SDF inlined or out of line, tables in LDS or in global
memory).  Each case here renders one shape of the catalogue through one family and

  * compares as the family's own test file does (test_gpu_parity / _supersample / _adaptive / _views / _view_samples: their helpers,
    imported; array equality on bit patterns, with the host-libm proviso of the file that has one; no tolerance of its own),
  * asks the LIBRARY which kernel and rung ran (kernel_name, view_samples_kernel_name, interp_variant, specialize_state and the scene
    compiler's log) and holds that to what the catalogue declares: a case that falls back to another kernel fails.

Oracle frames are cached per (shape, view, size, s) for the whole module: the shapes are sized by what the oracle costs.
"""
import numpy as np
import pytest

import aa_reference as A
import adaptive_reference as D
import scene_shapes as C
import test_gpu_adaptive as AD
import test_gpu_supersample as AA
import test_gpu_view_samples as VS
import test_gpu_views as V
from loltracer_amd import gpu
from test_gpu_parity import check_against_oracle, gpu_render

pytestmark = pytest.mark.gpu

PAD = 5                                  # pixels of padding in every pitch; PAD + 3 more pixels between the views of a batch


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


class Target:
    """where a shape runs: an interpreter mode (4: with the proven fast paths, 0: plain) or a form of the scene compiler"""

    def __init__(self, shape, specialize, form=None):
        self.shape, self.specialize, self.form = shape, specialize, form
        self.own = form is not None
        self.id = form.name if form else "%s-interp%d" % (shape.name, specialize)

    def open(self, families=True):
        """a renderer with the scene uploaded and — families — every family asked for BEFORE the upload, so that a scene module
        carries them all (one module per scene and form: the compiler's in-process cache serves the later cases)"""
        r = gpu.Renderer(0, specialize=self.specialize)
        try:
            if families:
                r.set_samples(2)
                r.set_view_samples(True)
            r.prepare(C.scene_of(self.shape))
            r.set_samples(1)
            self.assert_identity(r, families)
        except BaseException:
            r.close()
            raise
        return r

    def assert_identity(self, r, families=True):
        log = r.specialize_log()
        if not self.own:
            assert r.interp_variant() == self.shape.rung, (r.interp_variant(), self.shape.rung)
            assert r.kernel_name() == "render_interp" and r.specialize_state()[0] == 0, log
            return
        assert r.specialize_state()[0] == 2 and r.kernel_name() == "lol_render_spec", (r.specialize_state(), log)
        if self.form.second_tier:
            assert "form: SDF out of line" in log and "second tier (SDF inlined): " in log, log
        else:
            assert "form: SDF " + self.form.form in log and "second tier" not in log, log
        assert "not to be had" not in log, log
        if families:
            assert r.view_samples

    def names(self):
        p = "lol_render_spec" if self.own else "render_interp"
        return dict(plain=p, aa=p + "_aa", aa_list=p + "_aa_list", batch=p + "_batch", batch_aa=p + "_batch_aa", batch_aa_list=p + "_batch_aa_list")


INTERP = [Target(sh, mode) for sh in C.RUNG_SHAPES for mode in (4, 0)]
FORMS = [Target(f.shape, f.specialize, f) for f in C.FORMS]
TARGETS = INTERP + FORMS
PLAIN = [t for t in INTERP if t.shape.name in ("tree5", "tree9-tables", "tree12-tables")]
ids = lambda t: t.id                     # noqa: E731


def test_every_rung_and_form_has_its_cases():
    assert {t.shape.rung for t in INTERP} == C.ALL_RUNGS and {t.specialize for t in INTERP} == {4, 0}
    assert {t.shape.rung for t in PLAIN} == {(7, False), (11, True), (63, True)}
    assert [t.form.name for t in FORMS] == ["inline-small", "mid-out-of-line", "mid-inlined", "big-out-of-line", "tables-global"]


# ---------------------------------------------------------------------------------------------------------------- oracle frames
_full, _adaptive = {}, {}


def oracle(name, sc, view, cam, w, h, s, T, max_steps=256):
    """(packed, rgb, mask or None): aa_reference's s x s frame, or adaptive_reference's at contrast T; view: a key for `cam`"""
    k = (name, view, w, h, s, max_steps)
    if k not in _full:
        _full[k] = A.render(sc, w, h, s, max_steps=max_steps, camera=cam)
    if T < 0:
        return _full[k][0], _full[k][1], None
    if k + (T,) not in _adaptive:
        _adaptive[k + (T,)] = D.render(sc, w, h, s, T, max_steps=max_steps, camera=cam, full=_full[k])
    return _adaptive[k + (T,)]


def layout(w, h):
    pitch_px = w + PAD
    return pitch_px, h * pitch_px + PAD + 3


# ----------------------------------------------------------------------------------------------------- the families, one by one
def frame_aa(torch, t, r, name, sc, w, h, samples=C.SAMPLES, max_steps=256):
    for s in samples:
        r.set_samples(s)
        r.set_adaptive_samples(-1)
        x, rgb = AA.render_aa(torch, r, sc, w, h, s, pitch_px=w + PAD, prepare=False, max_steps=max_steps)      # (checks the padding)
        assert r.kernel_name() == t.names()["aa"], r.specialize_log()
        want_x, want_rgb, _ = oracle(name, sc, "own", None, w, h, s, -1, max_steps)
        AA.assert_equal_to_reference(x, rgb, want_x, want_rgb)


def frame_adaptive(torch, t, r, name, sc, w, h, T, samples=C.SAMPLES, max_steps=256, some=True):
    for s in samples:
        r.set_samples(s)
        r.set_adaptive_samples(T)
        x, rgb = AD.render_adaptive(torch, r, sc, w, h, s, T, pitch_px=w + PAD, prepare=False, max_steps=max_steps)
        assert r.kernel_name() == t.names()["aa_list"], r.specialize_log()
        want_x, want_rgb, m = oracle(name, sc, "own", None, w, h, s, T, max_steps)
        if some:                                       # (held on the CPU too: tests/test_scene_shapes.py)
            assert 0 < int(m.sum()) < w * h
        assert r.adaptive_refined() == int(m.sum())
        AD.assert_equal_to_reference(x, rgb, want_x, want_rgb)
    r.set_adaptive_samples(-1)


def batch_plain(torch, t, r, r2, name, sc, w, h):
    cams = C.cameras(sc)
    pitch_px, stride_px = layout(w, h)
    assert r.view_samples_kernel_name(1, -1) == t.names()["batch"], r.specialize_log()
    b = V.render_batch(torch, r, cams, w, h, pitch_px=pitch_px, stride_px=stride_px)
    assert V.untouched_outside_views(b, len(cams), w, h, pitch_px, stride_px)
    for v, cam in enumerate(cams):
        what = f"{t.id} {w}x{h} view {v}"
        V.assert_view_is_frame(b, v, V.render_single(torch, r2, cam, w, h), what)
        V.assert_view_is_oracle(b, v, V.oracle_view(name, sc, v, cam, w, h), what)
    b = V.render_batch(torch, r, cams, w, h, pitch_px=pitch_px, stride_px=stride_px, debug=False)      # the non-counting kernel
    assert V.untouched_outside_views(b, len(cams), w, h, pitch_px, stride_px)
    for v, cam in enumerate(cams):
        assert np.array_equal(b["xrgb"][v], V.oracle_view(name, sc, v, cam, w, h)["xrgb"]), v


def batch_samples(torch, t, r, r2, name, sc, w, h, T, samples=C.SAMPLES, max_steps=256, some=True):
    """T = -1: `_batch_aa`; else the adaptive batch, whose refine pass is `_batch_aa_list`"""
    cams = C.cameras(sc)
    pitch_px, stride_px = layout(w, h)
    for s in samples:
        assert r.view_samples_kernel_name(s, T) == t.names()["batch_aa" if T < 0 else "batch_aa_list"], r.specialize_log()
        b = VS.render_batch(torch, r, cams, w, h, s, T, pitch_px=pitch_px, stride_px=stride_px, max_steps=max_steps)
        assert b["outside_untouched"]
        refined = 0
        for v, cam in enumerate(cams):
            what = f"{t.id} {w}x{h} s={s} T={T} max_steps={max_steps} view {v}"
            VS.assert_view(b, v, VS.render_single(torch, r2, cam, w, h, s, T, max_steps), what)
            ox, orgb, m = oracle(name, sc, v, cam, w, h, s, T, max_steps)
            assert np.array_equal(b["xrgb"][v], ox), f"{what}: pixels differ from the oracle"
            assert np.array_equal(VS.bits(b["rgb"][v]), VS.bits(orgb)), f"{what}: rgb differs from the oracle"
            refined += int(m.sum()) if m is not None else 0
        if T >= 0:
            if some:
                assert 0 < refined < len(cams) * w * h
            assert r.views_refined() == refined, (t.id, s, T)
    r2.set_samples(1)
    r2.set_adaptive_samples(-1)


# ----------------------------------------------------------------------------------------------- rungs and forms x families
@pytest.mark.parametrize("t", PLAIN, ids=ids)
def test_plain_frame(torch_cuda, t):
    """pixels, float colours, ids, distances and both step counts on the rungs no plain-frame test reached"""
    sc, (w, h) = C.scene_of(t.shape), t.shape.size
    r = gpu.Renderer(0, specialize=t.specialize)
    try:
        r.want_kernel = "render_interp"
        g = gpu_render(torch_cuda, r, sc, w, h)
        t.assert_identity(r, families=False)
        check_against_oracle(g, sc, w, h)
    finally:
        r.close()


@pytest.mark.parametrize("t", TARGETS, ids=ids)
def test_aa(torch_cuda, t):
    r = t.open()
    try:
        frame_aa(torch_cuda, t, r, t.shape.name, C.scene_of(t.shape), *t.shape.size)
    finally:
        r.close()


@pytest.mark.parametrize("t", TARGETS, ids=ids)
def test_aa_list(torch_cuda, t):
    r = t.open()
    try:
        frame_adaptive(torch_cuda, t, r, t.shape.name, C.scene_of(t.shape), *t.shape.size, t.shape.contrast)
    finally:
        r.close()


@pytest.mark.parametrize("t", TARGETS, ids=ids)
def test_batch(torch_cuda, t):
    r = t.open()
    try:
        r2 = t.open(families=False)
        try:
            r2.set_tile_order("rows")
            batch_plain(torch_cuda, t, r, r2, t.shape.name, C.scene_of(t.shape), *t.shape.size)
        finally:
            r2.close()
    finally:
        r.close()


@pytest.mark.parametrize("t", TARGETS, ids=ids)
def test_batch_aa(torch_cuda, t):
    r = t.open()
    try:
        r2 = t.open()
        try:
            batch_samples(torch_cuda, t, r, r2, t.shape.name, C.scene_of(t.shape), *t.shape.size, -1)
        finally:
            r2.close()
    finally:
        r.close()


@pytest.mark.parametrize("t", TARGETS, ids=ids)
def test_batch_aa_list(torch_cuda, t):
    r = t.open()
    try:
        r2 = t.open()
        try:
            batch_samples(torch_cuda, t, r, r2, t.shape.name, C.scene_of(t.shape), *t.shape.size, t.shape.contrast)
        finally:
            r2.close()
    finally:
        r.close()


def test_declining_the_second_tier_keeps_the_out_of_line_kernel(torch_cuda):
    """lol_gpu_set_specialize(ctx, 5) on a scene of 257 ... 1024 ops: the kernel in use is the FIRST tier's — the SDF as one
    out-of-line function, which the scene compiler delivers 3 - 6 times sooner — and nothing is compiled behind it.  (Before this
    test the library compiled the inlined form in its place: the slow compile the host had declined.)  With 1 the same scene ends
    on the inlined form, through the out-of-line one."""
    sc = C.scene_of(C.MID)
    for specialize, first, second in ((5, "form: SDF out of line", False), (1, "form: SDF out of line", True)):
        r = gpu.Renderer(0, specialize=specialize)
        try:
            r.prepare(sc)
            log = r.specialize_log()
            assert r.specialize_state()[0] == 2 and r.kernel_name() == "lol_render_spec", log
            assert first in log and ("second tier (SDF inlined): " in log) == second and "form: SDF inlined" not in log, log
        finally:
            r.close()
    r = gpu.Renderer(0)                                     # ... and a small scene has one form, inlined
    try:
        r.prepare(C.scene_of(C.RUNG["scene4"]))
        assert "form: SDF inlined" in r.specialize_log() and "out of line" not in r.specialize_log()
    finally:
        r.close()


def test_interp_variant_needs_a_program(torch_cuda):
    r = gpu.Renderer(0)
    try:
        with pytest.raises(gpu.GpuError) as e:
            r.interp_variant()
        assert e.value.status == -4                     # LOL_GPU_ERR_NO_PROGRAM
        r.prepare(C.scene_of(C.RUNG["scene4"]))
        assert r.interp_variant() == (3, False)         # (what the interpreter WOULD run: the scene has its own kernel)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------- fuzz and degenerate shapes
class _Anon:
    """a catalogue entry for a scene that has no Shape of its own"""

    def __init__(self, name, sc, size):
        self.name, self.sc, self.size = name, sc, size


def _all_five(torch, name, sc, w, h, T, specialize, some):
    shape = _Anon(name, sc, (w, h))
    t = Target(shape, specialize, form=None)
    t.own = specialize == 1

    def open_():
        r = gpu.Renderer(0, specialize=specialize)
        try:
            r.set_samples(2)
            r.set_view_samples(True)
            r.prepare(sc)
            r.set_samples(1)
            if t.own:
                assert r.specialize_state()[0] == 2 and r.kernel_name() == "lol_render_spec", r.specialize_log()
            else:
                assert r.specialize_state()[0] == 0 and r.kernel_name() == "render_interp"
        except BaseException:
            r.close()
            raise
        return r
    r = open_()
    try:
        r2 = open_()
        try:
            frame_aa(torch, t, r, name, sc, w, h)
            frame_adaptive(torch, t, r, name, sc, w, h, T, some=some)
            r.set_samples(1)
            r2.set_tile_order("rows")
            batch_plain(torch, t, r, r2, name, sc, w, h)
            r2.set_tile_order("lpt")
            batch_samples(torch, t, r, r2, name, sc, w, h, -1)
            batch_samples(torch, t, r, r2, name, sc, w, h, T, some=False)
        finally:
            r2.close()
    finally:
        r.close()


@pytest.mark.parametrize("specialize", [4, 1], ids=["interp4", "scene-kernel"])
@pytest.mark.parametrize("i", range(C.N_FUZZ))
def test_fuzz_scene_through_all_five(torch_cuda, i, specialize):
    sc = C.fuzz_scenes()[i]
    try:
        _all_five(torch_cuda, "fuzz%d" % i, sc, *C.FUZZ_SIZE, C.FUZZ_CONTRAST, specialize, some=True)
    except AssertionError as e:
        raise AssertionError(f"fuzz scene {i} failed: {e}\n{C.fuzz_texts()[i]}") from e


@pytest.mark.parametrize("specialize", [4, 1], ids=["interp4", "scene-kernel"])
@pytest.mark.parametrize("i", range(6), ids=C.DEGENERATE_NAMES)
def test_degenerate_input_through_all_five(torch_cuda, i, specialize):
    sc = C.degenerate_scenes()[i]
    _all_five(torch_cuda, "degenerate%d" % i, sc, *C.DEGENERATE_SIZE, C.DEGENERATE_CONTRAST, specialize, some=C.DEGENERATE_REFINES_SOME[i])


# ------------------------------------------------------------------------------------------------------------------ max_steps
@pytest.mark.parametrize("specialize", [4, 1], ids=["interp4", "scene-kernel"])
@pytest.mark.parametrize("max_steps", C.MAX_STEPS)
def test_max_steps(torch_cuda, max_steps, specialize):
    """the supersampled and adaptive families march max_steps steps like the plain frame (scene4, contrast 16)"""
    shape = C.MAX_STEPS_SHAPE
    sc, (w, h) = C.scene_of(shape), C.MAX_STEPS_SIZE
    t = Target(shape, specialize, form=C.FORMS[0] if specialize == 1 else None)
    some = max_steps > 0                               # (no step marched: every ray escapes, nothing to refine)
    r = t.open()
    try:
        r2 = t.open()
        try:
            frame_aa(torch_cuda, t, r, shape.name, sc, w, h, max_steps=max_steps)
            frame_adaptive(torch_cuda, t, r, shape.name, sc, w, h, 16, max_steps=max_steps, some=some)
            r.set_samples(1)
            batch_samples(torch_cuda, t, r, r2, shape.name, sc, w, h, -1, max_steps=max_steps)
            batch_samples(torch_cuda, t, r, r2, shape.name, sc, w, h, 16, max_steps=max_steps, some=some)
        finally:
            r2.close()
    finally:
        r.close()
