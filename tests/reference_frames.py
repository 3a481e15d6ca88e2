"""What tests/golden/ref_renderer_frames.npz records, and how to read it.  Not a test file.

The fixture holds frames that the reference's OWN render_thread (naive_renderer.c, compiled unmodified into oracle/_ref/liblol_ref.so:
oracle/Makefile, oracle/ref_render.c, oracle/sdl_standin/SDL.h) stored, in XRGB8888, for the scenes and cameras cases() lists — and,
for the hostile scenes under their own camera, what tests/golden/make_golden.py's RefPipeline composes from the reference's compiled
primitives: hit ids, hit distances, march steps, post-gamma colours and per-light shadow steps.  The reference's MAX_STEPS is a
constant: every frame is 256 steps.

tests/golden/make_golden.py writes the file from cases(); tests/test_reference_renderer.py (CPU) and
tests/test_gpu_reference_frames.py (GPU) read it through load() and never need the reference.
"""
import hashlib
import io
import json
import os
import zipfile
from dataclasses import dataclass, field
from typing import Callable, List, Tuple

import numpy as np

import scene_shapes as C
from loltracer_amd import scene as S

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_renderer_frames.npz")
EXAMPLES = ("scene", "scene2", "scene3", "scene4")
EXAMPLE_SIZE = (64, 36)
MAX_LEFT_OUT = 2


@dataclass(frozen=True)
class Case:
    key: str                            # the arrays of the case are `<key>_xrgb` [K, h, w], `<key>_cams` [K, 7] (+ the composition's)
    group: str                          # example | shape | fuzz | degenerate | hostile | tie | exit
    text: Callable[[], str] = field(repr=False, compare=False)
    size: Tuple[int, int]
    n_ops: int = 0                      # (shapes only: what decides which GPU kernels a case is worth)
    composed: bool = False              # RefPipeline's ids, distances, steps and colours are recorded too (own camera)


# The march ends with `dist >= MAX_DIST` → id 0 (naive_renderer.c:65).  dist == 100 EXACTLY is reachable: from the origin, looking
# down -z, a sphere of radius 1 at (0, 0, -101) is 100 away; the central ray of an odd-sized frame is (0, 0, -1) exactly, its first
# step makes dist 100 (not > 100: the loop goes on), its second finds the surface (0 < EPSILON) and ends it with dist == 100: the
# reference calls that a miss, and `>` in place of `>=` would call it a hit, in another material's colour.
MARCH_EXIT_KEY = "march-exit-at-100"
MARCH_EXIT_TEXT = C.tie_text(("sphere { material = #1, point = (0, 0, -101), radius = 1 }",))


def cam_at(x, y, z, dx, dy, dz, fov=90.0):
    """a camera the way tests/test_gpu_parity.py makes them: the direction normalised in floats like scene.c does"""
    cam = S.Camera()
    cam.point = S.V3(x, y, z)
    d = np.array([dx, dy, dz], dtype=np.float32)
    n = np.float32(1.0) / np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1]) + np.float32(d[2] * d[2]), dtype=np.float32)
    cam.direction = S.V3(*(float(np.float32(v * n)) for v in d))
    cam.fov = float(np.float32(np.float32(fov) / np.float32(180) * np.pi))
    return cam


def first_step_cameras():
    """the seven of test_gpu_parity.test_first_step_is_given_or_taken, in its order"""
    return [cam_at(-2.0, 6.0, 3.0, 0.2, -0.5, -1.0), cam_at(-0.0, 6.0, 3.0, 0.0, -0.5, -1.0), cam_at(0.0, 6.0, -0.0, 0.0, -0.5, -1.0),
            cam_at(0.0, 1.0, -6.0, 0.0, 0.0, -1.0), cam_at(0.0, -0.9995, 3.0, 0.0, 0.1, -1.0), cam_at(0.0, 150.0, 0.0, 0.0, -1.0, -0.01),
            cam_at(0.0, 99.0, 0.0, 0.0, -1.0, -0.01)]


def copy_camera(c):
    return S.Camera.from_buffer_copy(bytes(c))


def tie_cameras(sc):
    """the three of test_gpu_hostile.tie_cameras: given, minus-zero, insane"""
    given, taken = copy_camera(sc.camera), copy_camera(sc.camera)
    taken.point.x = -0.0
    insane = S.Camera()
    insane.point = S.V3(1.0e16, 3.0, 2.5)
    insane.direction = S.V3(-1.0, 0.0, 0.0)
    insane.fov = float(np.float32(np.float32(60.0) / np.float32(180) * np.pi))
    return [("given", given), ("minus-zero", taken), ("insane", insane)]


def cam7(cam):
    return np.array(cam.point.tuple() + cam.direction.tuple() + (cam.fov,), dtype=np.float32)


def camera_of(row):
    cam = S.Camera()
    cam.point, cam.direction, cam.fov = S.V3(*map(float, row[:3])), S.V3(*map(float, row[3:6])), float(row[6])
    return cam


def cases() -> List[Case]:
    out = [Case(n, "example", (lambda n=n: open(os.path.join(C.SCENES_DIR, n + ".lol")).read()), EXAMPLE_SIZE) for n in EXAMPLES]
    out += [Case("shape-" + s.name, "shape", s.text, C.MAX_STEPS_SIZE, n_ops=s.n_ops) for s in C.RUNG_SHAPES + [C.MID, C.BIG]]
    out += [Case("fuzz%d" % i, "fuzz", (lambda i=i: C.fuzz_texts()[i]), C.FUZZ_SIZE) for i in range(C.N_FUZZ)]
    out += [Case("degenerate-" + n, "degenerate", (lambda t=t: t), C.DEGENERATE_SIZE) for n, t in zip(C.DEGENERATE_NAMES, C.DEGENERATE_CASES)]
    out += [Case("hostile-" + e.name, "tie" if e.tie else "hostile", (lambda e=e: e.text), e.size, composed=True) for e in C.HOSTILE]
    out += [Case(MARCH_EXIT_KEY, "exit", (lambda: MARCH_EXIT_TEXT), C.HOSTILE_SIZE, composed=True)]
    return out


def cameras_of(case: Case, sc) -> List[Tuple[str, "S.Camera"]]:
    """every camera the case is recorded under, the scene's own first"""
    cams = [("own", copy_camera(sc.camera))]
    if case.group != "example":
        cams += [("orbit%d" % i, c) for i, c in enumerate(C.cameras(sc))]
    if case.group == "tie":
        cams += tie_cameras(sc)
    if case.key == "scene4":
        cams += [("first-step%d" % i, c) for i, c in enumerate(first_step_cameras())]
    return cams


def sha256(text: str) -> str:
    return hashlib.sha256(text.encode()).hexdigest()


# ---- a .npz written the same way every time (numpy's savez stamps every member with the time of day)
def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


_loaded = None


def load():
    """(meta, arrays): meta is the fixture's own table of contents — libm variant, cases (key, group, size, sha256 of the text,
    camera names) and the scenes left out with the reason; the arrays are read-only"""
    global _loaded
    if _loaded is None:
        z = np.load(FIXTURE)
        arrays = {k: z[k] for k in z.files}
        for a in arrays.values():
            a.setflags(write=False)
        _loaded = (json.loads(bytes(arrays.pop("meta")).decode()), arrays)
    return _loaded


def dominant_channel(rgb):
    """0, 1, 2 = red, green, blue; None where no channel is above both others"""
    rgb = [float(v) for v in rgb]
    top = max(rgb)
    return rgb.index(top) if rgb.count(top) == 1 else None


def assert_recorded_tie_goes_to_the_first(e):
    """In the REFERENCE's own frame of tie scene `e` (render_thread's pixels, its own camera) the centre pixel wears the colour of
    the FIRST tied object's material and not the second's — the tied objects wear materials of three different hues under a white
    light (scene_shapes.TIE_MATERIALS), so the hue names the winner —, and in the composition recorded beside it (whose packed
    pixels the generator held to render_thread's) the centre pixel's id is the first's and no other tied id shows anywhere.
    (tie-camera is tied on the first step only: the reference marches 256 steps, its centre pixel shows the sphere ahead.  Its
    frames are recorded and held like all others; its first-step id is the oracle's and the device's to show.)"""
    _, arrays = load()
    sc = C.hostile_scene(e)
    w, h = e.size
    first = min(e.tie.tied)
    mats = sc.materials()
    worn = [mats[sc.nodes()[sc.roots()[i - 1]].material] for i in e.tie.tied]          # in the order of e.tie.tied: the first first
    hues = [dominant_channel(m.diffuse.tuple()) for m in worn]
    assert None not in hues and len(set(hues)) == len(hues), hues
    px = int(arrays["hostile-" + e.name + "_xrgb"][0, h // 2, w // 2])
    ids = arrays["hostile-" + e.name + "_hit_id"]
    if not e.tie.along_ray:
        assert ids[h // 2, w // 2] != 0
        return
    seen = dominant_channel([px >> 16 & 255, px >> 8 & 255, px & 255])
    assert seen == hues[0] and seen not in hues[1:], (e.name, hex(px), hues)
    assert ids[h // 2, w // 2] == first
    assert first in ids and not (set(e.tie.tied) - {first}) & set(ids.ravel().tolist())


def one_colour_by_input(sc) -> bool:
    """no light reaches any pixel's colour — there is none, or every material's diffuse and specular are 0 — and ambient x
    material.ambient is one value over all materials: every pixel of every view is that colour, whatever is hit"""
    mats = sc.materials()
    unlit = len(sc.lights()) == 0 or all(m.diffuse.tuple() == (0, 0, 0) == m.specular.tuple() for m in mats)
    amb = sc.c.ambient_color.tuple()
    return unlit and len({tuple(np.float32(a) * np.float32(b) for a, b in zip(amb, m.ambient.tuple())) for m in mats}) == 1


def recorded():
    """[(case, meta entry)] of every case of cases() that the fixture holds, in cases()' order"""
    meta, _ = load()
    by = {m["key"]: m for m in meta["cases"]}
    return [(c, by[c.key]) for c in cases() if c.key in by]
