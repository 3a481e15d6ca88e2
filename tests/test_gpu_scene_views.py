"""Scene views (lol_gpu_render_scene_views): record r of a call IS the frame a context renders under cams[r] after uploading
scenes[r] — packed pixels, float colours, hit distances and ids EQUAL to the CPU oracle's on that record's own Scene, bit for bit,
step counts equal to a fresh context's — and a blend over records is the contract of lol_gpu_render_views_blend with per-record
scenes (tests/scene_views_reference.py).

Every case runs on three arms: the interpreter's kernels in plain arithmetic (Renderer(specialize=0)), the interpreter's kernels with
the fast paths the upload proved (specialize=4: the proven root's instantiations, proven blend factors in the records' lists, the
list without v_div_fixup for finite records under sane cameras — what a default context runs scene views on without the setter) and
the structure module (set_scene_views before the upload, the kernel's name checked after specialize_wait), and for three scenes: scene4 (a blob of nested smooth unions and a
plane), scene.lol (four top-level objects: the structure module's march asks for the id once, ids in file order) and the first
scene of tests/scene_shapes.py's fuzz catalogue that has a rounded box, a plane and nested smooth unions (the first case also for
that catalogue's small scene whose tables are too large for LDS: every record's tables are then read where they lie).  Frames are 33 x 17 —
partial tiles on both axes, three tiles by five — with max_steps 256.  Reference frames are cached for the whole module and shared
between the arms.
"""
import ctypes as C

import numpy as np
import pytest

import scene_shapes as SH
import scene_views_reference as R
import test_gpu_views as V
from loltracer_amd import gpu, scene as S

pytestmark = pytest.mark.gpu

W, H, MAX_STEPS = 33, 17, 256
ERR_HIP, ERR_ARG, ERR_UNSUPPORTED = -2, -3, -5
ARMS = ("interpreter", "interpreter-fast", "structure-module")
SPECIALIZE = {"interpreter": 0, "interpreter-fast": 4, "structure-module": 1}
NAMES = ("scene4", "scene", "shape")
KERNEL = {"interpreter": ("render_interp_scene_batch", "render_interp_scene_batch_lin"),
          "interpreter-fast": ("render_interp_scene_batch", "render_interp_scene_batch_lin"),
          "structure-module": ("lol_render_param_batch", "lol_render_param_batch_lin")}
PATTERN = 0x5CE7E5A7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


bits = V.bits
_kept = {}           # every Scene a reference frame was cached for stays alive (the caches key on id(scene))


def shape_scene():
    """the first fuzz scene with a rounded box, a plane, nested smooth unions, several objects and several materials"""
    for sc in SH.fuzz_scenes():
        nodes = sc.nodes()
        types = {n.type for n in nodes}
        nested = any(n.type == S.NODE_SMOOTH_UNION and S.NODE_SMOOTH_UNION in (nodes[n.a].type, nodes[n.b].type) for n in nodes)
        if {S.NODE_BOX, S.NODE_PLANE} <= types and nested and sc.c.n_roots >= 2 and sc.c.n_materials >= 2 and sc.c.n_lights >= 1:
            return sc
    raise AssertionError("no fuzz scene has a rounded box, a plane and nested smooth unions")


def base_scene(scenes, name):
    if name == "tables-global":              # 110 materials: the tables are read where they lie (lol_kernel.h, TABLES_LDS_MAX_DWORDS)
        return SH.scene_of(SH.RUNG["tree2-tables"])
    return shape_scene() if name == "shape" else scenes[name]


def first_node(sc, *types):
    return next(i for i in range(sc.c.n_nodes) if sc.c.nodes[i].type in types)


def variants(scenes, name):
    """three mutually different scenes of the base scene's structure: between them a moved object, a changed radius, a smoothness
    no upload ever proved, a moved light, a changed material colour and root material, and a changed ambient colour"""
    key = ("variants", name)
    if key not in _kept:
        base = base_scene(scenes, name)
        a, b, c = base.clone(), base.clone(), base.clone()
        solid = first_node(base, S.NODE_SPHERE, S.NODE_BOX)
        a.c.nodes[solid].point.x += 0.375
        a.c.nodes[solid].point.y += 0.25
        a.c.ambient_color.x += 0.125
        b.c.nodes[solid].radius = b.c.nodes[solid].radius * 1.25 + 0.0625
        unions = [i for i in range(base.c.n_nodes) if base.c.nodes[i].type == S.NODE_SMOOTH_UNION]
        if unions:
            b.c.nodes[unions[0]].smoothness = 2.7182817              # (no scene of the suite has it: never proven at the upload)
        b.c.lights[0].point.x -= 1.5
        b.c.lights[0].point.y += 1.0
        m = c.c.n_materials - 1
        c.c.materials[m].diffuse.y = 0.8125
        c.c.materials[m].ambient.z = 0.3125
        root = c.c.roots[0]
        c.c.nodes[root].material = (c.c.nodes[root].material + 1) % c.c.n_materials
        c.c.ambient_color.z = 0.4375
        _kept[key] = [a, b, c]
    return _kept[key]


def three_cameras(sc):
    orbit = S.orbit_cameras(sc, 8)
    return [V.copy_camera(sc.camera), orbit[1], orbit[6]]


def has_unions(sc):
    return any(n.type == S.NODE_SMOOTH_UNION for n in sc.nodes())


def open_renderer(sc, arm, wait=True):
    r = gpu.Renderer(0, specialize=SPECIALIZE[arm])
    try:
        r.set_scene_views(arm == "structure-module")
        r.prepare(sc, wait=wait)
        kind, proven, no_fixup = r.interp_fast_paths()
        if arm == "interpreter":
            assert (kind, proven, no_fixup) == (0, 0, 0)
        else:                                # the proven root, and a proven blend factor for a scene that has a smooth union
            assert kind == 3 and no_fixup <= proven and (proven >= 1) == has_unions(sc), (kind, proven, no_fixup)
        if wait:
            assert r.scene_views_state() == (2 if arm == "structure-module" else 0), r.specialize_log()
            assert (r.scene_views_kernel_name(1), r.scene_views_kernel_name(4)) == KERNEL[arm]
    except BaseException:
        r.close()
        raise
    return r


def queue(r, out, cams, scs, k=1, stream=None):
    n, w, h, pitch_px, stride_px = out["geom"]
    assert len(scs) == len(cams) == n * k
    r.render_scene_views_into(out["frame"].data_ptr(), cams, scs, w, h, k, MAX_STEPS, pitch_bytes=pitch_px * 4,
                              view_stride_bytes=stride_px * 4, debug=out["dbg"], stream=stream)


def render(torch, r, cams, scs, k=1, debug=True, stream=None):
    out = V.alloc_batch(torch, len(scs) // k, W, H, None, None, debug)
    torch.cuda.synchronize()                 # torch's fills run on ITS stream; the batch on the renderer's own
    queue(r, out, cams, scs, k, stream)
    r.sync()
    return V.collect(out, *out["geom"])


def fresh_steps(torch, sc, cam, key):
    """what a fresh context that uploaded `sc` reports as the step counts of the frame under `cam` (cached: both arms ask)"""
    if key not in _kept:
        r = gpu.Renderer(0, specialize=False)
        try:
            r.prepare(sc)
            _kept[key] = V.render_batch(torch, r, [cam], W, H, MAX_STEPS)["steps"][0]
        finally:
            r.close()
    return _kept[key]


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name", NAMES + ("tables-global",))
def test_three_views_are_three_frames_of_three_scenes(torch_cuda, scenes, name, arm):
    base = base_scene(scenes, name)
    scs, cams = variants(scenes, name), three_cameras(base)
    r = open_renderer(base, arm)
    try:
        b = render(torch_cuda, r, cams, scs)
        assert V.untouched_outside_views(b, 3, W, H, W, H * W)
        for v in range(3):
            V.assert_view_is_oracle(b, v, R.frame(scs[v], cams[v], W, H, MAX_STEPS), f"{name} view {v} ({arm})")
            want = fresh_steps(torch_cuda, scs[v], cams[v], ("steps", name, v))
            assert np.array_equal(b["steps"][v] & 0xFFFF, want & 0xFFFF), f"{name} view {v} ({arm}): march steps"
            assert np.array_equal(b["steps"][v] >> 16, want >> 16), f"{name} view {v} ({arm}): shadow steps"
        assert not np.array_equal(b["xrgb"][0], b["xrgb"][1]) and not np.array_equal(b["xrgb"][1], b["xrgb"][2])
    finally:
        r.close()


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name", NAMES)
def test_the_uploaded_scene_in_every_record_is_the_plain_batch(torch_cuda, scenes, name, arm):
    base = base_scene(scenes, name)
    cams = three_cameras(base)
    r = open_renderer(base, arm)
    try:
        plain = V.render_batch(torch_cuda, r, cams, W, H, MAX_STEPS)
        b = render(torch_cuda, r, cams, [base] * 3)
        assert np.array_equal(b["raw"], plain["raw"])                            # byte for byte
        for d in V.DIAGNOSTICS:
            assert np.array_equal(bits(b[d]), bits(plain[d])), d
        groups = []
        orbit = S.orbit_cameras(base, 8)
        for v in range(3):
            groups += S.shutter_cameras(orbit[v], orbit[v + 1], 4)
        out = V.alloc_batch(torch_cuda, 3, W, H, None, None, ("rgb",))
        torch_cuda.cuda.synchronize()
        r.render_blended_views_into(out["frame"].data_ptr(), groups, 4, W, H, MAX_STEPS, debug=out["dbg"])
        r.sync()
        blend = V.collect(out, *out["geom"])
        b4 = render(torch_cuda, r, groups, [base] * 12, 4, debug=("rgb",))
        assert np.array_equal(b4["raw"], blend["raw"]) and np.array_equal(bits(b4["rgb"]), bits(blend["rgb"]))
    finally:
        r.close()


def moving(scenes, name, n, k):
    """n k scenes between the base scene and its first variant moved further: the exposures of n frames, k scenes each"""
    key = ("moving", name, n, k)
    if key not in _kept:
        base = base_scene(scenes, name)
        far = variants(scenes, name)[0].clone()
        solid = first_node(base, S.NODE_SPHERE, S.NODE_BOX)
        far.c.nodes[solid].point.x += 1.0
        far.c.nodes[solid].point.z -= 0.5
        _kept[key] = [S.tween(base, far, t) for f in range(n) for t in S.shutter_times(f, n, k)]
    return _kept[key]


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name", NAMES)
def test_blends_over_moving_objects_equal_the_reference(torch_cuda, scenes, name, arm):
    base = base_scene(scenes, name)
    r = open_renderer(base, arm)
    try:
        for k in (2, 4):
            scs = moving(scenes, name, 2, k)
            cams = [V.copy_camera(base.camera)] * len(scs)
            b = render(torch_cuda, r, cams, scs, k, debug=("rgb",))
            px, rgb = R.render_blend(scs, cams, k, W, H, max_steps=MAX_STEPS)
            assert np.array_equal(b["xrgb"], px), f"{name} K={k} ({arm}): pixels differ from the reference"
            assert np.array_equal(bits(b["rgb"]), bits(rgb)), f"{name} K={k} ({arm}): rgb differs from the reference"
            assert V.untouched_outside_views(b, 2, W, H, W, H * W)
            for d in ("dist", "id", "steps"):                                    # refused, as for any blend
                out = V.alloc_batch(torch_cuda, 2, W, H, None, None, (d,))
                torch_cuda.cuda.synchronize()
                with pytest.raises(gpu.GpuError) as e:
                    queue(r, out, cams, scs, k)
                assert e.value.status == ERR_UNSUPPORTED
                r.sync()
                assert (V.collect(out, *out["geom"])["raw"] == V.SENTINEL).all()
    finally:
        r.close()


def hostile_scene(scenes, name):
    key = ("hostile", name)
    if key not in _kept:
        sc = base_scene(scenes, name).clone()
        n = sc.c.nodes[first_node(sc, S.NODE_SPHERE, S.NODE_BOX)]
        n.point.x = float("nan")
        n.radius = float("inf")
        _kept[key] = sc
    return _kept[key]


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name", NAMES)
def test_a_hostile_record_is_its_own_business(torch_cuda, scenes, name, arm):
    base = base_scene(scenes, name)
    sane, cams = variants(scenes, name), three_cameras(base)
    bad, insane = hostile_scene(scenes, name), V.insane_camera()
    scs = [sane[0], bad, sane[1], sane[2], sane[2]]
    all_cams = [cams[0], cams[1], cams[1], insane, cams[2]]
    r = open_renderer(base, arm)
    try:
        b = render(torch_cuda, r, all_cams, scs)
        alone = render(torch_cuda, r, cams, sane)
        for v, u in ((0, 0), (2, 1), (4, 2)):
            assert np.array_equal(b["xrgb"][v], alone["xrgb"][u]), (v, u)
            for d in V.DIAGNOSTICS:
                assert np.array_equal(bits(b[d][v]), bits(alone[d][u])), (d, v, u)
        for v in (1, 3):
            o = R.frame(scs[v], all_cams[v], W, H, MAX_STEPS)
            what = f"{name} hostile view {v} ({arm})"
            assert np.array_equal(b["xrgb"][v], o["xrgb"]), what
            assert np.array_equal(bits(b["rgb"][v]), bits(o["rgb"])), what
            assert np.array_equal(b["id"][v], o["id"]), what
            assert np.array_equal(b["dist"][v], o["dist"], equal_nan=True), what      # (a NaN is a NaN: payloads are not the contract)
    finally:
        r.close()


@pytest.mark.parametrize("arm", ARMS)
def test_the_context_is_left_as_it_was(torch_cuda, scenes, arm):
    base = scenes["scene4"]
    scs, cams = variants(scenes, "scene4"), three_cameras(base)
    r = open_renderer(base, arm)
    other = gpu.Renderer(0, specialize=SPECIALIZE[arm])
    try:
        other.prepare(base)                                                      # the same scene without set_scene_views
        assert not other.scene_views and other.scene_views_state() == 0
        assert other.kernel_key() == r.kernel_key() and other.kernel_name() == r.kernel_name()
        for _ in range(3):                                                       # (a repeated view: the tile-order state has something to lose)
            before = V.render_single(torch_cuda, r, cams[1], W, H, MAX_STEPS)
        key, order, name = r.kernel_key(), r.tile_order(), r.kernel_name()
        render(torch_cuda, r, cams, scs)
        render(torch_cuda, r, cams + cams[:1], scs + scs[:1], 2, debug=("rgb",))
        assert (r.kernel_key(), r.tile_order(), r.kernel_name()) == (key, order, name)
        after = V.render_single(torch_cuda, r, cams[1], W, H, MAX_STEPS)
        for d in ("xrgb",) + V.DIAGNOSTICS:
            assert np.array_equal(bits(after[d]), bits(before[d])), d
    finally:
        other.close()
        r.close()


def changed_program(prog, what):
    """a copy of `prog` (its op list copied: `keep` holds the memory) with one thing about its STRUCTURE changed"""
    out = S.Program()
    C.memmove(C.byref(out), C.byref(prog), C.sizeof(S.Program))
    ops = (S.Op * prog.n_ops)()
    C.memmove(ops, prog.ops, C.sizeof(ops))
    out.ops = C.cast(ops, C.POINTER(S.Op))
    out._keep = (ops, prog)
    tops = [i for i in range(prog.n_ops) if ops[i].op == S.OP_TOP]
    smins = [i for i in range(prog.n_ops) if ops[i].op in (S.OP_SMIN, S.OP_SMIN_R)]
    if what == "opcode":
        i = smins[-1]
        ops[i].op = S.OP_SMIN_R if ops[i].op == S.OP_SMIN else S.OP_SMIN
    elif what == "id":
        ops[tops[-1]].id, ops[tops[0]].id = ops[tops[0]].id, ops[tops[-1]].id
    elif what == "n_lights":
        out.n_lights = prog.n_lights - 1
    elif what == "max_stack":
        out.max_stack = prog.max_stack + 1
    elif what == "root_material":
        rm = (C.c_uint32 * prog.n_roots)(*[prog.root_material[i] for i in range(prog.n_roots)])
        rm[prog.n_roots - 1] = prog.n_materials
        out.root_material = C.cast(rm, C.POINTER(C.c_uint32))
        out._keep += (rm,)
    elif what == "null-table":
        out.lights = C.POINTER(S.Light)()
    return out


@pytest.mark.parametrize("arm", ARMS)
def test_refusals_write_nothing_and_leave_the_context_usable(torch_cuda, scenes, arm):
    base = scenes["scene4"]
    scs, cams = variants(scenes, "scene4"), three_cameras(base)
    progs = [sc.flatten() for sc in scs]
    r = open_renderer(base, arm)
    try:
        dev = torch_cuda.device("cuda:0")
        frame = torch_cuda.full((3 * H * W,), PATTERN, dtype=torch_cuda.int32, device=dev)
        torch_cuda.cuda.synchronize()

        def refused(cameras, items, k, status):
            with pytest.raises(gpu.GpuError) as e:
                r.render_scene_views_into(frame.data_ptr(), cameras, items, W, H, k, MAX_STEPS)
            assert e.value.status == status, e.value
            r.sync()
            assert (frame.cpu().numpy().view(np.uint32) == PATTERN).all()

        for what in ("opcode", "id", "n_lights", "max_stack", "root_material", "null-table"):
            for at in (0, 2):                                                    # anywhere in the list
                items = list(progs)
                items[at] = changed_program(progs[at], what)
                refused(cams, items, 1, ERR_ARG)
        refused(cams, progs, 3, ERR_ARG)                                         # K outside the set
        r.testing_fail_view_scratch(1)                                           # an injected scratch failure
        refused(cams * 2, progs * 2, 2, ERR_HIP)
        # ... and the context still renders: the same blend, and a batch equal to the oracle
        frame2 = torch_cuda.full((3 * H * W,), PATTERN, dtype=torch_cuda.int32, device=dev)
        torch_cuda.cuda.synchronize()
        r.render_scene_views_into(frame2.data_ptr(), cams * 2, progs * 2, W, H, 2, MAX_STEPS)
        r.sync()
        assert not (frame2.cpu().numpy().view(np.uint32) == PATTERN).any()
        b = render(torch_cuda, r, cams, scs)
        for v in range(3):
            assert np.array_equal(b["xrgb"][v], R.frame(scs[v], cams[v], W, H, MAX_STEPS)["xrgb"]), v
    finally:
        r.close()
    # no program: refused as such
    empty = gpu.Renderer(0, specialize=False)
    try:
        with pytest.raises(gpu.GpuError) as e:
            empty.scene = base
            empty.render_scene_views_into(frame.data_ptr(), cams, progs, W, H, 1, MAX_STEPS)
        assert e.value.status == -4
    finally:
        empty.close()


@pytest.mark.parametrize("streams", (1, 4), ids=("one-stream", "four-streams"))
@pytest.mark.parametrize("arm", ARMS)
def test_ten_calls_back_to_back(torch_cuda, scenes, arm, streams):
    """the ring of record sets has 8: calls nine and ten wait for, and reuse, the sets of calls one and two"""
    base = scenes["scene4"]
    scs = moving(scenes, "scene4", 10, 1)
    cam = V.copy_camera(base.camera)
    r = open_renderer(base, arm)
    try:
        r.set_frames_in_flight(streams)
        outs = [V.alloc_batch(torch_cuda, 1, W, H, None, None, False) for _ in scs]
        torch_cuda.cuda.synchronize()
        for out, sc in zip(outs, scs):
            queue(r, out, [cam], [sc])
        r.sync()
        for i, (out, sc) in enumerate(zip(outs, scs)):
            assert np.array_equal(V.collect(out, *out["geom"])["xrgb"][0], R.frame(sc, cam, W, H, MAX_STEPS)["xrgb"]), i
    finally:
        r.close()


@pytest.mark.parametrize("arm", ARMS)
def test_blends_of_views_and_of_scene_views_share_one_scratch_ring(torch_cuda, scenes, arm):
    """Three blends of views and three blends of scene views (K = 2, 2 views of 16 x 8 each), alternating, queued back to back with
    NO wait between them on one context with two streams: six uses of the scratch ring both calls take their sets from, which has
    4 — the fifth and sixth take a set whose last user, a call of the OTHER kind, may still be running.  Each of the six is its own
    reference.  Queued once."""
    base = scenes["scene4"]
    w, h, k = 16, 8, 2
    orbit = S.orbit_cameras(base, 16)
    moved = moving(scenes, "scene4", 6, k)                                     # 12 scenes: four for each call of scene views
    calls = []
    for i in range(6):
        cams = [orbit[(2 * i + j) % 16] for j in range(2 * k)]                   # no two calls under the same cameras
        calls.append((cams, moved[4 * (i // 2):4 * (i // 2) + 4] if i % 2 else [base] * (2 * k)))
    r = open_renderer(base, arm)
    try:
        r.set_frames_in_flight(2)
        outs = [V.alloc_batch(torch_cuda, 2, w, h, w + 3, h * (w + 3) + 5, ("rgb",)) for _ in calls]
        torch_cuda.cuda.synchronize()
        for i, (out, (cams, scs)) in enumerate(zip(outs, calls)):
            if i % 2:
                r.render_scene_views_into(out["frame"].data_ptr(), cams, scs, w, h, k, MAX_STEPS, pitch_bytes=(w + 3) * 4,
                                          view_stride_bytes=(h * (w + 3) + 5) * 4, debug=out["dbg"])
            else:
                r.render_blended_views_into(out["frame"].data_ptr(), cams, k, w, h, MAX_STEPS, pitch_bytes=(w + 3) * 4,
                                            view_stride_bytes=(h * (w + 3) + 5) * 4, debug=out["dbg"])
        r.sync()
        for i, (out, (cams, scs)) in enumerate(zip(outs, calls)):
            b = V.collect(out, *out["geom"])
            px, rgb = R.render_blend(scs, cams, k, w, h, max_steps=MAX_STEPS)
            assert np.array_equal(b["xrgb"], px), f"call {i} ({arm}): pixels differ from the reference"
            assert np.array_equal(bits(b["rgb"]), bits(rgb)), f"call {i} ({arm}): rgb differs from the reference"
            assert V.untouched_outside_views(b, 2, w, h, w + 3, h * (w + 3) + 5), f"call {i}"
    finally:
        r.close()


@pytest.mark.parametrize("arm", ARMS)
def test_the_first_step_of_a_record_is_the_frames(torch_cuda, scenes, arm):
    """Two records whose camera decides the primary march's first step in a way of its own: an origin with a negative zero in x (the
    step is not given: every lane takes it), and an origin inside scene4's blob (the first value lies below EPSILON: the step is
    not given either, and ends the march).  Hit distance, hit id and both step counts of each record equal those of the frame a
    fresh context renders under that camera after uploading that record's scene."""
    base = scenes["scene4"]
    a, _, c = variants(scenes, "scene4")                                        # (c differs from scene4 in materials alone: the blob is where it was)
    scs = [a, c]
    cams = [V.cam_at(-0.0, 6.0, 3.0, 0.0, -0.5, -1.0), V.cam_at(0.0, 1.0, -6.0, 0.0, 0.0, -1.0)]
    r = open_renderer(base, arm)
    try:
        b = render(torch_cuda, r, cams, scs)
        for v in range(2):
            fresh = gpu.Renderer(0, specialize=False)
            try:
                fresh.prepare(scs[v])
                g = V.render_single(torch_cuda, fresh, cams[v], W, H, MAX_STEPS)
            finally:
                fresh.close()
            V.assert_view_is_frame(b, v, g, f"record {v} ({arm})")
        inside = b["dist"][1]
        assert (b["steps"][1] & 0xFFFF).max() == 1 and float(inside.max()) < 0.001, "the second camera is not inside the blob"
    finally:
        r.close()


def test_a_call_before_the_structure_module_is_loaded(torch_cuda, scenes):
    """a context that asked for the module renders from the first call on: on the interpreter's kernels (with the upload's fast paths)
    while the module is being compiled, on the module once a call's boundary or specialize_wait has loaded it — the same frames"""
    base = scenes["scene4"]
    scs, cams = variants(scenes, "scene4"), three_cameras(base)
    r = open_renderer(base, "structure-module", wait=False)
    try:
        assert r.scene_views and r.scene_views_state() == 1                      # nothing is loaded outside a boundary
        names = set()
        for _ in range(2):
            b = render(torch_cuda, r, cams, scs)
            names.add(r.scene_views_kernel_name(1))
            assert r.scene_views_state() == (2 if r.scene_views_kernel_name(1) == KERNEL["structure-module"][0] else 1)
            for v in range(3):
                V.assert_view_is_oracle(b, v, R.frame(scs[v], cams[v], W, H, MAX_STEPS), f"view {v} ({r.scene_views_kernel_name(1)})")
        r.specialize_wait()
        assert r.scene_views_state() == 2 and r.scene_views_kernel_name(2) == KERNEL["structure-module"][1]
        b = render(torch_cuda, r, cams, scs)
        for v in range(3):
            V.assert_view_is_oracle(b, v, R.frame(scs[v], cams[v], W, H, MAX_STEPS), f"view {v} (after the wait)")
        assert names <= {KERNEL["interpreter"][0], KERNEL["structure-module"][0]}
    finally:
        r.close()
