"""ctypes mirror of include/lol_scene.h — the `.lol` reader, scene model and flattener.

The work is done by loltracer_amd/lib/liblol_scene.so (plain C,
loltracer_amd/csrc/lol_scene.c); this module only declares the structs and
wraps the entry points so tests and bench.py can drive them.  Names follow the
reference's scene.h / scene-parser.y (scene_parse → Scene.parse_file,
scene_validate_materials → Scene.validate_materials).
"""
from __future__ import annotations

import ctypes as C
import math
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

# sanity caps of include/lol_scene.h (a program is as large as its scene; counts beyond these are taken for corruption)
LOL_MAX_OPS = 1 << 20
LOL_MAX_LIGHTS = 1 << 16
LOL_MAX_MATERIALS = 1 << 20
LOL_MAX_STACK = 64

(LOL_OK, LOL_ERR_IO, LOL_ERR_SYNTAX, LOL_ERR_PROPERTY, LOL_ERR_TYPE, LOL_ERR_COMPONENT,
 LOL_ERR_MATERIAL, LOL_ERR_NOMEM, LOL_ERR_UNSUPPORTED) = range(9)

NODE_SPHERE, NODE_BOX, NODE_PLANE, NODE_SMOOTH_UNION = range(4)
OP_SPHERE, OP_RBOX, OP_PLANE, OP_SMIN, OP_SMIN_R, OP_TOP = range(6)


class V3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def tuple(self):
        return (self.x, self.y, self.z)


class Material(C.Structure):
    _fields_ = [("shininess", C.c_float), ("diffuse", V3), ("specular", V3), ("ambient", V3)]


class Light(C.Structure):
    _fields_ = [("point", V3), ("diffuse_intensity", V3), ("specular_intensity", V3)]


class Camera(C.Structure):
    _fields_ = [("point", V3), ("direction", V3), ("fov", C.c_float)]


class Node(C.Structure):
    _fields_ = [("type", C.c_int32), ("material", C.c_uint32), ("point", V3), ("radius", C.c_float),
                ("half_extent", V3), ("smoothness", C.c_float), ("a", C.c_int32), ("b", C.c_int32)]


class SceneStruct(C.Structure):
    _fields_ = [("materials", C.POINTER(Material)), ("n_materials", C.c_size_t),
                ("lights", C.POINTER(Light)), ("n_lights", C.c_size_t),
                ("nodes", C.POINTER(Node)), ("n_nodes", C.c_size_t),
                ("roots", C.POINTER(C.c_int32)), ("n_roots", C.c_size_t),
                ("ambient_color", V3), ("camera", Camera)]


class Op(C.Structure):
    _fields_ = [("op", C.c_uint32), ("id", C.c_uint32), ("f", C.c_float * 7), ("_pad", C.c_uint32)]


class Program(C.Structure):
    """lol_program: counts + pointers to the four tables (allocated by lol_scene_flatten, released with the object)."""
    _fields_ = [("n_ops", C.c_uint32), ("n_lights", C.c_uint32), ("n_materials", C.c_uint32),
                ("n_roots", C.c_uint32), ("max_stack", C.c_uint32), ("ambient_color", V3),
                ("ops", C.POINTER(Op)), ("lights", C.POINTER(Light)),
                ("materials", C.POINTER(Material)), ("root_material", C.POINTER(C.c_uint32))]

    def tables(self) -> bytes:
        """Everything the program says, as bytes (two programs are the same scene iff these are equal)."""
        head = bytes(memoryview(self).cast("B")[:C.sizeof(C.c_uint32) * 5 + C.sizeof(V3)])
        parts = [head]
        for ptr, n, t in ((self.ops, self.n_ops, Op), (self.lights, self.n_lights, Light),
                          (self.materials, self.n_materials, Material), (self.root_material, self.n_roots, C.c_uint32)):
            parts.append(C.string_at(ptr, n * C.sizeof(t)) if n else b"")
        return b"".join(parts)

    def free(self):
        if getattr(self, "_owned", False):
            self._owned = False
            host_lib().lol_program_free(C.byref(self))

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class FrameCamera(C.Structure):
    _fields_ = [("origin", V3), ("dir", V3), ("right", V3), ("up", V3),
                ("width", C.c_float), ("height", C.c_float)]


class SceneError(Exception):
    def __init__(self, status: int, message: str):
        super().__init__(f"[{status}] {message}")
        self.status = status
        self.message = message


def _bind_prototypes(lib, *tables):
    """Declare to ctypes every function of `tables` (name -> (restype, argtypes)) that `lib` has.  One it lacks — an older build of
    the library — stays as it is: calling it raises ctypes' AttributeError."""
    for table in tables:
        for name, (restype, argtypes) in table.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes


# The C prototypes of include/lol_scene.h: function -> (restype, argtypes).  tests/test_cabi_prototypes.py holds them, and the
# struct mirrors above, to the header's text.
_P = C.POINTER
_LOL_SCENE_H = {
    "lol_scene_parse_file": (C.c_int, [C.c_char_p, _P(_P(SceneStruct)), C.c_char_p, C.c_size_t]),
    "lol_scene_parse_string": (C.c_int, [C.c_char_p, C.c_size_t, _P(_P(SceneStruct)), C.c_char_p, C.c_size_t]),
    "lol_scene_free": (None, [_P(SceneStruct)]),
    "lol_scene_clone": (C.c_int, [_P(SceneStruct), _P(_P(SceneStruct))]),
    "lol_scene_new": (_P(SceneStruct), []),
    "lol_scene_validate_materials": (C.c_int, [_P(SceneStruct)]),
    "lol_scene_flatten": (C.c_int, [_P(SceneStruct), _P(Program)]),
    "lol_program_free": (None, [_P(Program)]),
    "lol_frame_camera_init": (None, [_P(FrameCamera), _P(Camera), C.c_int, C.c_int]),
    "lol_status_str": (C.c_char_p, [C.c_int]),
}

_lib = None


def host_lib() -> C.CDLL:
    """liblol_scene.so; raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is None:
        path = os.path.join(LIB_DIR, "liblol_scene.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run __graft_entry__.build() (or make -C loltracer_amd/csrc)")
        lib = C.CDLL(path)
        _bind_prototypes(lib, _LOL_SCENE_H)
        _lib = lib
    return _lib


class Scene:
    """Owning handle of a parsed `lol_scene*`."""

    def __init__(self, ptr):
        self._ptr = ptr

    @classmethod
    def parse_file(cls, path: str) -> "Scene":
        lib = host_lib()
        out = C.POINTER(SceneStruct)()
        err = C.create_string_buffer(256)
        st = lib.lol_scene_parse_file(os.fsencode(path), C.byref(out), err, len(err))
        if st != LOL_OK:
            raise SceneError(st, err.value.decode() or lib.lol_status_str(st).decode())
        return cls(out)

    @classmethod
    def parse_string(cls, text) -> "Scene":
        lib = host_lib()
        data = text.encode() if isinstance(text, str) else bytes(text)
        out = C.POINTER(SceneStruct)()
        err = C.create_string_buffer(256)
        st = lib.lol_scene_parse_string(data, len(data), C.byref(out), err, len(err))
        if st != LOL_OK:
            raise SceneError(st, err.value.decode() or lib.lol_status_str(st).decode())
        return cls(out)

    def clone(self) -> "Scene":
        """lol_scene_clone: a deep copy — equal counts, equal bytes in every table — that is this object's own to change."""
        lib = host_lib()
        out = C.POINTER(SceneStruct)()
        st = lib.lol_scene_clone(self._ptr, C.byref(out))
        if st != LOL_OK:
            raise SceneError(st, lib.lol_status_str(st).decode())
        return Scene(out)

    def with_look(self, lights=None, materials=None, ambient=None) -> "Scene":
        """A clone with another LOOK: only the numbers lol_gpu_relight lets a look differ in are replaced, so same_geometry(self,
        clone) holds by construction.  lights: one entry per light, (diffuse_intensity, specular_intensity), each a 3-tuple or None
        (keep); materials: one entry per material, (diffuse, specular, ambient) likewise; ambient: a 3-tuple.  A whole entry, or the
        whole argument, may be None.  The numbers are stored as floats whatever they are: NaN and infinities included."""
        out = self.clone()
        c = out.c

        def put(dst, v):
            if v is not None:
                dst.x, dst.y, dst.z = (float(t) for t in v)

        if lights is not None:
            if len(lights) != c.n_lights:
                raise ValueError("with_look: one entry per light")
            for i, e in enumerate(lights):
                if e is not None:
                    put(c.lights[i].diffuse_intensity, e[0])
                    put(c.lights[i].specular_intensity, e[1])
        if materials is not None:
            if len(materials) != c.n_materials:
                raise ValueError("with_look: one entry per material")
            for i, e in enumerate(materials):
                if e is not None:
                    put(c.materials[i].diffuse, e[0])
                    put(c.materials[i].specular, e[1])
                    put(c.materials[i].ambient, e[2])
        put(c.ambient_color, ambient)
        return out

    def with_lighting(self, points=None, shininess=None) -> "Scene":
        """A clone with other LIGHTING GEOMETRY: what a light update (Renderer.light_update_*_into) lets a look differ in beyond
        with_look's numbers.  points: one entry per light, a 3-tuple or None (keep); shininess: one entry per material, a number or
        None.  Either argument may be None.  The numbers are stored as floats whatever they are: NaN and infinities included."""
        out = self.clone()
        c = out.c
        if points is not None:
            if len(points) != c.n_lights:
                raise ValueError("with_lighting: one entry per light")
            for i, e in enumerate(points):
                if e is not None:
                    c.lights[i].point.x, c.lights[i].point.y, c.lights[i].point.z = (float(t) for t in e)
        if shininess is not None:
            if len(shininess) != c.n_materials:
                raise ValueError("with_lighting: one entry per material")
            for i, e in enumerate(shininess):
                if e is not None:
                    c.materials[i].shininess = float(e)
        return out

    def tables(self) -> bytes:
        """Everything the scene says, as bytes: counts, ambient colour and camera, then nodes, roots, materials and lights."""
        c = self.c
        head = b"".join(int(n).to_bytes(8, "little") for n in (c.n_materials, c.n_lights, c.n_nodes, c.n_roots))
        head += bytes(memoryview(c.ambient_color).cast("B")) + bytes(memoryview(c.camera).cast("B"))
        parts = [head]
        for ptr, n, t in ((c.nodes, c.n_nodes, Node), (c.roots, c.n_roots, C.c_int32), (c.materials, c.n_materials, Material),
                          (c.lights, c.n_lights, Light)):
            parts.append(C.string_at(ptr, n * C.sizeof(t)) if n else b"")
        return b"".join(parts)

    @property
    def ptr(self):
        return self._ptr

    @property
    def c(self) -> SceneStruct:
        return self._ptr.contents

    @property
    def camera(self) -> Camera:
        return self.c.camera

    def validate_materials(self) -> bool:
        return bool(host_lib().lol_scene_validate_materials(self._ptr))

    def flatten(self) -> Program:
        prog = Program()
        st = host_lib().lol_scene_flatten(self._ptr, C.byref(prog))
        if st != LOL_OK:
            raise SceneError(st, host_lib().lol_status_str(st).decode())
        prog._owned = True                  # its tables belong to this object (lol_program_free when it goes)
        return prog

    def frame_camera(self, w: int, h: int, camera: Camera | None = None) -> FrameCamera:
        fc = FrameCamera()
        cam = camera if camera is not None else self.c.camera
        host_lib().lol_frame_camera_init(C.byref(fc), C.byref(cam), w, h)
        return fc

    def nodes(self):
        return [self.c.nodes[i] for i in range(self.c.n_nodes)]

    def roots(self):
        return [self.c.roots[i] for i in range(self.c.n_roots)]

    def materials(self):
        return [self.c.materials[i] for i in range(self.c.n_materials)]

    def lights(self):
        return [self.c.lights[i] for i in range(self.c.n_lights)]

    def close(self):
        if self._ptr:
            host_lib().lol_scene_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def same_structure(a: "Scene", b: "Scene") -> bool:
    """Do a and b differ in numbers alone?  Equal counts of nodes, roots, materials and lights, equal roots, and equal type and
    children node by node.  Such scenes flatten to programs of equal counts, opcodes and ids: what
    Renderer.render_scene_views_into asks of the scenes of one call.  Which material an object wears is a number here, as it is
    there (root_material may differ per record)."""
    ca, cb = a.c, b.c
    if (ca.n_nodes, ca.n_roots, ca.n_materials, ca.n_lights) != (cb.n_nodes, cb.n_roots, cb.n_materials, cb.n_lights):
        return False
    for i in range(ca.n_roots):
        if ca.roots[i] != cb.roots[i]:
            return False
    for i in range(ca.n_nodes):
        x, y = ca.nodes[i], cb.nodes[i]
        if (x.type, x.a, x.b) != (y.type, y.a, y.b):
            return False
    return True


def geometry_difference(a, b, lighting=True):
    """The first thing in which b differs from a that a LOOK may not differ in, as a sentence, or None: what lol_gpu_relight checks
    of a look against the uploaded program (include/lol_gpu.h), in its order.  a, b: Scene objects (flattened here) or Programs.
    Equal must be, bit for bit: the counts of ops, lights, materials and roots and max_stack; every op's opcode, id and numbers;
    every light's point; every material's shininess (a NaN shininess equals itself); every root's material index.  Free are the
    lights' intensities, the materials' three colours and the ambient colour.  lighting=False leaves the lights' points and the
    shininesses free too: what a light update checks of its look (light_changes)."""
    pa = a if isinstance(a, Program) else a.flatten()
    pb = b if isinstance(b, Program) else b.flatten()
    for f in ("n_ops", "n_lights", "n_materials", "n_roots", "max_stack"):
        if getattr(pa, f) != getattr(pb, f):
            return f"{f} differs: {getattr(pa, f)} and {getattr(pb, f)}"
    for i in range(pa.n_ops):
        x, y = pa.ops[i], pb.ops[i]
        if (x.op, x.id) != (y.op, y.id):
            return f"op {i} differs in opcode or id"
        if bytes(memoryview(x.f).cast("B")) != bytes(memoryview(y.f).cast("B")):
            return f"op {i} (object {x.id}) differs in a number: {list(x.f)} and {list(y.f)}"
    for i in range(pa.n_lights if lighting else 0):
        if bytes(memoryview(pa.lights[i].point).cast("B")) != bytes(memoryview(pb.lights[i].point).cast("B")):
            return f"light {i} stands at {pa.lights[i].point.tuple()} and at {pb.lights[i].point.tuple()}"
    for i in range(pa.n_materials if lighting else 0):
        if C.string_at(C.addressof(pa.materials[i]), 4) != C.string_at(C.addressof(pb.materials[i]), 4):
            return f"material {i} has shininess {pa.materials[i].shininess} and {pb.materials[i].shininess}"
    for i in range(pa.n_roots):
        if pa.root_material[i] != pb.root_material[i]:
            return f"object {i + 1} wears material {pa.root_material[i]} and {pb.root_material[i]}"
    return None


def same_geometry(a, b) -> bool:
    """Is b a LOOK of a — the scene with other light intensities, material colours or ambient colour, and nothing else changed?
    The predicate lol_gpu_relight's host check implements (geometry_difference says what differs)."""
    return geometry_difference(a, b) is None


def light_changes(held, look):
    """(march_mask, specular_mask) of the light update that brings planes holding `held` to `look` (Renderer.light_update_*_into;
    Scene objects or Programs).  Bit l of the first mask: light l's point differs, as bits — its whole factor is computed again.  If
    any material's shininess differs, as bits, every other light goes into the second mask: its specular incidence alone.  Anything
    else of the geometry that differs raises ValueError with geometry_difference's sentence; lights from the 64th on cannot be
    updated and raise too."""
    pa = held if isinstance(held, Program) else held.flatten()
    pb = look if isinstance(look, Program) else look.flatten()
    why = geometry_difference(pa, pb, lighting=False)
    if why is not None:
        raise ValueError(why)
    moved = [i for i in range(pa.n_lights)
             if bytes(memoryview(pa.lights[i].point).cast("B")) != bytes(memoryview(pb.lights[i].point).cast("B"))]
    shiny = any(C.string_at(C.addressof(pa.materials[i]), 4) != C.string_at(C.addressof(pb.materials[i]), 4) for i in range(pa.n_materials))
    if (moved and moved[-1] >= 64) or (shiny and pa.n_lights > 64):
        raise ValueError("lights from the 64th on cannot be updated: capture again")
    march = sum(1 << i for i in moved)
    return march, (((1 << pa.n_lights) - 1) & ~march) if shiny else 0


def _lerp32(a, b, t):
    """a + (b - a) * t, every operation a binary32 operation (numpy float32 scalars or arrays: no double in between)"""
    import numpy as np
    with np.errstate(all="ignore"):
        return np.float32(a) + (np.float32(b) - np.float32(a)) * np.float32(t)


def tween(a: "Scene", b: "Scene", t: float) -> "Scene":
    """The scene between a (t = 0) and b (t = 1): a clone of a in which every float of the nodes (point, radius, half_extent,
    smoothness), of the lights, of the materials and of the ambient colour is a + (b - a) * t, each operation in float32 with t
    rounded to float32 first.  The structure — node types, children, roots —, the material indices and the camera are a's; a and b must
    have the same structure (same_structure), else ValueError.  tween(a, b, 0) is a's numbers and tween(a, b, 1) b's wherever
    b - a is exact, which it is for the numbers scenes are written with."""
    if not same_structure(a, b):
        raise ValueError("tween: the two scenes differ in structure")
    import numpy as np
    t = np.float32(t)
    out = a.clone()
    ca, cb, co = a.c, b.c, out.c

    def blend(dst, x, y, cls):
        n = C.sizeof(cls) // 4
        fx = np.frombuffer(bytes(memoryview(x).cast("B")), dtype=np.float32)
        fy = np.frombuffer(bytes(memoryview(y).cast("B")), dtype=np.float32)
        C.memmove(C.byref(dst), np.ascontiguousarray(_lerp32(fx, fy, t), dtype=np.float32).tobytes(), 4 * n)

    for i in range(ca.n_nodes):
        x, y, o = ca.nodes[i], cb.nodes[i], co.nodes[i]
        blend(o.point, x.point, y.point, V3)
        blend(o.half_extent, x.half_extent, y.half_extent, V3)
        o.radius = float(_lerp32(x.radius, y.radius, t))
        o.smoothness = float(_lerp32(x.smoothness, y.smoothness, t))
    for i in range(ca.n_lights):
        blend(co.lights[i], ca.lights[i], cb.lights[i], Light)
    for i in range(ca.n_materials):
        blend(co.materials[i], ca.materials[i], cb.materials[i], Material)
    blend(co.ambient_color, ca.ambient_color, cb.ambient_color, V3)
    return out


def shutter_times(frame: int, frames: int, k: int) -> list:
    """The times of the k scenes of frame `frame` of `frames` frames that run from t = 0 to t = 1, each frame's exposure one of
    `frames` equal parts of that interval: scene i of the frame stands at the midpoint of the i-th of k equal parts of its exposure,
    the way shutter_cameras spreads its cameras.  k = 1: the middle of the frame's part."""
    if frames < 1 or k < 1 or not 0 <= frame < frames:
        raise ValueError("shutter_times: frames and k must be at least 1 and 0 <= frame < frames")
    return [(frame + (i + 0.5) / k) / frames for i in range(k)]


def orbit_cameras(scene: "Scene", n: int) -> list:
    """n cameras on a circle round the scene: what a contact sheet or a ring of thumbnails wants (Renderer.render_views_into).

    The circle is horizontal (constant y), at the scene camera's height, about the vertical axis through the PIVOT: the point on
    the scene camera's axis nearest to the mean of the centres of the scene's spheres and boxes (one unit ahead of the camera when
    the scene has none, or when that point lies behind it).  Camera i stands at angle 2 pi i / n from the scene camera's own
    position — camera 0 is there — and looks at the pivot with the scene's field of view.  A camera straight above or below the
    pivot has no circle to go round: every camera is then the scene's own.  Positions are computed in doubles and rounded to float."""
    if n < 1:
        raise ValueError("orbit_cameras: n must be at least 1")
    cam = scene.camera
    p = [float(v) for v in cam.point.tuple()]
    d = [float(v) for v in cam.direction.tuple()]
    norm = math.sqrt(sum(v * v for v in d)) or 1.0
    d = [v / norm for v in d]
    centres = [nd.point.tuple() for nd in scene.nodes() if nd.type in (0, 1)]      # LOL_NODE_SPHERE, LOL_NODE_BOX
    t = 1.0
    if centres:
        mean = [sum(c[k] for c in centres) / len(centres) for k in range(3)]
        along = sum((mean[k] - p[k]) * d[k] for k in range(3))
        if along > 0.0 and math.isfinite(along):
            t = along
    pivot = [p[k] + t * d[k] for k in range(3)]
    rx, rz = p[0] - pivot[0], p[2] - pivot[2]
    radius, phase = math.hypot(rx, rz), math.atan2(rx, rz)
    out = []
    for i in range(n):
        c = Camera()
        if radius > 0.0:
            th = phase + 2.0 * math.pi * i / n
            pos = [pivot[0] + radius * math.sin(th), p[1], pivot[2] + radius * math.cos(th)]
        else:
            pos = list(p)
        look = [pivot[k] - pos[k] for k in range(3)]
        ln = math.sqrt(sum(v * v for v in look))
        c.point = V3(*pos)
        c.direction = V3(*([v / ln for v in look] if ln > 0.0 else d))
        c.fov = cam.fov
        out.append(c)
    return out


def _copy_camera(cam: Camera) -> Camera:
    out = Camera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(Camera))
    return out


def shutter_cameras(a: Camera, b: Camera, k: int) -> list:
    """k cameras of one exposure, for motion blur (Renderer.render_blended_views_into): the shutter opens at camera a and closes at
    camera b, and camera i (0 <= i < k) stands at the midpoint t = (i + 1/2) / k of the i-th of k equal parts of that interval.

    Position and direction are a + t (b - a), interpolated in doubles; the direction is then normalised and everything rounded to
    float.  Where a and b look the same way the direction is a's, as it is (nothing to interpolate, nothing to normalise), so
    shutter_cameras(a, a, k) is a, k times over.  Two directions that cancel at some t leave a's direction there.  The fov is a's."""
    if k < 1:
        raise ValueError("shutter_cameras: k must be at least 1")
    pa, pb = [float(v) for v in a.point.tuple()], [float(v) for v in b.point.tuple()]
    da, db = [float(v) for v in a.direction.tuple()], [float(v) for v in b.direction.tuple()]
    out = []
    for i in range(k):
        t = (i + 0.5) / k
        c = _copy_camera(a)
        c.point = V3(*[pa[j] + t * (pb[j] - pa[j]) for j in range(3)])
        if da != db:
            d = [da[j] + t * (db[j] - da[j]) for j in range(3)]
            ln = math.sqrt(sum(v * v for v in d))
            if ln > 0.0 and math.isfinite(ln):
                c.direction = V3(*[v / ln for v in d])
        out.append(c)
    return out


GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))


def lens_cameras(camera: Camera, focus_distance: float, aperture_radius: float, k: int) -> list:
    """k cameras on a lens, for depth of field (Renderer.render_blended_views_into).  k = 1 is the camera itself: a pinhole.

    Otherwise the k positions lie on the lens disc through the camera's position, spanned by the right and up vectors the reference's
    host moves its camera by (right = normalize(direction x (0, 1, 0)), up = normalize(right x direction)), in a fixed pattern:
    position i at radius R sqrt((i + 1/2) / k) and angle i times the golden angle — equal areas of the disc, no two on one spoke.
    Every camera looks at the focus point, point + focus_distance * direction, with the camera's fov; whatever lies at that distance
    stays sharp, the rest is averaged over the lens.  This is the TOE-IN approximation of a thin lens: the cameras are turned towards
    the focus point, where a thin lens would keep their image planes parallel and shift them; the plane of focus is therefore only
    approximately a plane (exact on the axis), which for apertures small against the focus distance is what a viewer expects.
    Computed in doubles and rounded to float.  A camera looking straight up or down has no right vector: ValueError."""
    if k < 1:
        raise ValueError("lens_cameras: k must be at least 1")
    if k == 1:
        return [_copy_camera(camera)]
    p = [float(v) for v in camera.point.tuple()]
    d = [float(v) for v in camera.direction.tuple()]
    ln = math.sqrt(sum(v * v for v in d))
    if not (ln > 0.0 and math.isfinite(ln)):
        raise ValueError("lens_cameras: the camera has no direction")
    d = [v / ln for v in d]

    def cross(u, v):
        return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]

    right = cross(d, [0.0, 1.0, 0.0])
    rn = math.sqrt(sum(v * v for v in right))
    if not rn > 0.0:
        raise ValueError("lens_cameras: a camera looking straight up or down has no lens plane of this kind")
    right = [v / rn for v in right]
    up = cross(right, d)
    un = math.sqrt(sum(v * v for v in up))
    up = [v / un for v in up]
    focus = [p[j] + float(focus_distance) * d[j] for j in range(3)]
    out = []
    for i in range(k):
        rad, th = float(aperture_radius) * math.sqrt((i + 0.5) / k), i * GOLDEN_ANGLE
        pos = [p[j] + rad * (math.cos(th) * right[j] + math.sin(th) * up[j]) for j in range(3)]
        look = [focus[j] - pos[j] for j in range(3)]
        lk = math.sqrt(sum(v * v for v in look))
        c = _copy_camera(camera)
        c.point = V3(*pos)
        if lk > 0.0 and math.isfinite(lk):
            c.direction = V3(*[v / lk for v in look])
        out.append(c)
    return out


def panorama_rays(camera: Camera, w: int, h: int):
    """The rays of a w x h equirectangular panorama from the camera's position, for Renderer.shade_rays_into: float32 [h w, 6],
    row-major, each {ox, oy, oz, dx, dy, dz}.

    Pixel (x, y) looks along longitude ((x + .5) / w * 2 - 1) pi and latitude (.5 - (y + .5) / h) pi:
    cos(lat) sin(lon) right + sin(lat) up + cos(lat) cos(lon) dir, in the basis lol_frame_camera_init gives the camera (dir
    normalised here) — the image's centre looks where the camera does, its left and right edges meet behind it, its top row looks
    up.  Computed in doubles, normalised, then rounded to float: the rays are data, a shading query's contract starts at their bits.
    The field of view plays no part."""
    import numpy as np
    if w < 1 or h < 1:
        raise ValueError("panorama_rays: w and h must be at least 1")
    fc = FrameCamera()
    host_lib().lol_frame_camera_init(C.byref(fc), C.byref(camera), w, h)
    d, right, up = (np.array(v.tuple(), np.float64) for v in (fc.dir, fc.right, fc.up))
    d, right, up = (v / (np.linalg.norm(v) or 1.0) for v in (d, right, up))
    lon = ((np.arange(w, dtype=np.float64) + .5) / w * 2. - 1.) * math.pi
    lat = (.5 - (np.arange(h, dtype=np.float64) + .5) / h) * math.pi
    lon, lat = np.meshgrid(lon, lat)                                # [h, w]
    rd = ((np.cos(lat) * np.sin(lon))[..., None] * right + np.sin(lat)[..., None] * up + (np.cos(lat) * np.cos(lon))[..., None] * d)
    rd /= np.linalg.norm(rd, axis=-1, keepdims=True)
    rays = np.empty((h * w, 6), np.float32)
    rays[:, :3] = np.array(camera.point.tuple(), np.float32)
    rays[:, 3:] = rd.reshape(-1, 3).astype(np.float32)
    return rays
