"""Scene records whose culling plans differ (tests/scene_records.py) through the three call families that take a scene per record —
scene views, supersampled scene views, scene queries: every record of a call IS what a context that uploaded that record's scene
computes, and the oracle's frame of that scene, whatever scene was uploaded, in whatever order and company the records come.

The host builds an interpreter list per record (lol_gpu.hip, build_scene_records): which objects have a bound, the order of
evaluation, the tie flags, the test records and their jump distances and the list's length are the RECORD's, and so are the three
exact skips, FINITE, SANE and the first step.  The records here differ in all of these (tests/test_scene_records.py holds that on the
CPU), so that a record run with another record's list length, flags or first step, or a tie that lost its MOP_TIE in a re-ordering,
shows as a wrong pixel, id or step count.

Every comparison is equality of bit patterns, with the families' own helpers: V.assert_view_is_oracle, scene_views_reference.frame and
render_blend, scene_view_samples_reference.render, ray_reference / shade_reference (same_bits: two NaNs are the same).  The one
latitude is the header's: for lists of RAYS with the exact skips on, the shadow half of `steps` is compared with the skips off alone,
as in tests/test_gpu_scene_queries.py.  Frames are 23 x 13 with max_steps 256; oracle frames, CPU references and the answers of the
fresh contexts (ONE per record, asked everything at once) are cached for the module and shared between the arms.
"""
import numpy as np
import pytest

import hostile_rays as HR
import ray_reference as R
import reference_frames as RF
import scene_records as SR
import scene_view_samples_reference as SVR
import scene_views_reference as F
import shade_reference as SHR
import test_gpu_rays as TR
import test_gpu_scene_queries as SQ
import test_gpu_scene_views as SV
import test_gpu_shades as TS
import test_gpu_views as V
from loltracer_amd import gpu

pytestmark = pytest.mark.gpu

W, H = SR.SIZE
MAX_STEPS = 256
PITCH, STRIDE = W + 5, H * (W + 5) + 8                  # a pitch and a view stride larger than the frame
N, LIST_STRIDE = 70, 75                                 # rays per record: one full wave and a tail; the lists' distance where each has its own
ARMS = SV.ARMS
INTERP_ARMS = ("interpreter", "interpreter-fast")
KINDS = SQ.KINDS
REF = {"trace": R, "shade": SHR}
bits = V.bits
ids = lambda rs: rs.name                 # noqa: E731
_kept = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module", autouse=True)
def modules():
    """the structure modules: one upload per set for the whole module, closed when it is done"""
    yield
    for key in [k for k in _kept if k[0] == "module"]:
        _kept.pop(key).close()


def scenes_and_cameras(recs):
    return [r.scene for r in recs], [r.camera for r in recs]


def open_renderer(sc, arm):
    """a context that uploaded `sc`.  The structure module is made with set_scene_view_samples: all four kernels, so that one upload
    per set serves the plain and the supersampled calls"""
    r = gpu.Renderer(0, specialize=SV.SPECIALIZE[arm])
    try:
        r.set_scene_view_samples(arm == "structure-module")
        r.prepare(sc)
        kind, proven, no_fixup = r.interp_fast_paths()
        if arm == "interpreter":
            assert (kind, proven, no_fixup) == (0, 0, 0)
        else:
            assert kind == 3 and no_fixup <= proven, (kind, proven, no_fixup)
        assert r.scene_views_state() == (2 if arm == "structure-module" else 0), r.specialize_log()
        assert (r.scene_views_kernel_name(1), r.scene_views_kernel_name(4)) == SV.KERNEL[arm]
        if arm == "structure-module":
            assert (r.scene_view_samples_kernel_name(1, 2), r.scene_view_samples_kernel_name(4, 4)) == ("lol_render_param_batch_aa", "lol_render_param_batch_aa_lin")
    except BaseException:
        r.close()
        raise
    return r


class renderer:
    """with renderer(rs, arm) as r: the set's uploaded scene on one of the three arms (the structure module's context is kept)"""

    def __init__(self, rs, arm, upload=None):
        self.key = ("module", rs.name) if arm == "structure-module" and upload is None else None
        if self.key and self.key in _kept:
            self.r = _kept[self.key]
        else:
            self.r = open_renderer(SR.uploaded(rs) if upload is None else SR.record(rs, upload).scene, arm)
            if self.key:
                _kept[self.key] = self.r

    def __enter__(self):
        return self.r

    def __exit__(self, *exc):
        if not self.key:
            self.r.close()


def render(torch, r, recs, k=1, s=1, debug=True):
    scs, cams = scenes_and_cameras(recs)
    out = V.alloc_batch(torch, len(scs) // k, W, H, PITCH, STRIDE, debug)
    torch.cuda.synchronize()                 # torch's fills run on ITS stream; the call on the renderer's own
    r.render_scene_views_into(out["frame"].data_ptr(), cams, scs, W, H, k, MAX_STEPS, pitch_bytes=PITCH * 4, view_stride_bytes=STRIDE * 4,
                              debug=out["dbg"], samples=s)
    r.sync()
    b = V.collect(out, *out["geom"])
    assert V.untouched_outside_views(b, len(scs) // k, W, H, PITCH, STRIDE), "memory outside the views was written"
    return b


def same_planes(a, va, b, vb, what):
    """view va of call a and view vb of call b: every output plane, byte for byte, steps included"""
    assert np.array_equal(a["xrgb"][va], b["xrgb"][vb]), f"{what}: pixels"
    for d in V.DIAGNOSTICS:
        assert np.array_equal(bits(a[d][va]), bits(b[d][vb])), f"{what}: {d}"


def oracle_frame(rec):
    return F.frame(rec.scene, rec.camera, W, H, MAX_STEPS)


# ------------------------------------------------------------------------------------------------------------- lists of rays
def ray_list(rec, seed):
    """70 rays for one record: aimed and grazing rays made from THAT record's culling bounds and the rays straight down for its
    objects without one (hostile_rays.bound_rays), filled up with its own camera's rays, the eight special rays inside the list"""
    key = ("rays", id(rec.scene), seed)
    if key not in _kept:
        parts, _, _ = HR.bound_rays(rec.scene, [SR.SEED, seed])
        own = np.concatenate(parts).astype(np.float32)
        own = own[np.isfinite(own).all(axis=1)]
        cam = R.camera_rays(rec.scene, 13, 5, rec.camera)
        specials = R.special_rays(cam[len(cam) // 2, :3], cam[len(cam) // 2, 3:])
        n_own = min(len(own), 44)
        take = own[np.linspace(0, len(own) - 1, n_own).astype(int)] if n_own else own[:0]
        n_cam = N - len(specials) - n_own
        rays = list(take) + list(cam[np.linspace(0, len(cam) - 1, n_cam).astype(int)])
        for at, s in zip((3, 11, 19, 27, 35, 43, 65, 67), specials):               # six inside the full wave, two inside the tail
            rays.insert(at, s)
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        assert rays.shape == (N, 6) and np.isnan(rays).any() and np.isinf(rays).any() and n_own >= 16
        rays.setflags(write=False)
        _kept[key] = (rec, rays)
    return _kept[key][1]


def shared_list(rs):
    return ray_list(SR.records(rs)[0], 0)


def own_list(rs, rec):
    return ray_list(rec, 1 + SR.records(rs).index(rec))


def all_pixels():
    return TR.all_pixels(W, H)


def cpu_reference(kind, rs, rec, what):
    """ray_reference / shade_reference on the record's own Scene: what = "pixels" (every pixel under its camera), "shared", "own" """
    key = ("cpu", kind, id(rec.scene), what)
    if key not in _kept:
        rays = R.camera_rays(rec.scene, W, H, rec.camera) if what == "pixels" else shared_list(rs) if what == "shared" else own_list(rs, rec)
        _kept[key] = (rec, REF[kind].reference(rec.scene, rays, MAX_STEPS))
    return _kept[key][1]


def fresh(torch, rs, rec):
    """everything a fresh context that uploaded the record answers, asked once: its frame with all planes, and both single-scene
    queries over every pixel, the shared list and the record's own list, with the exact skips on and off"""
    key = ("fresh", id(rec.scene))
    if key not in _kept:
        out = {}
        r = gpu.Renderer(0, specialize=False)
        try:
            r.prepare(rec.scene)
            assert r.kernel_name() == "render_interp"
            g = V.render_batch(torch, r, [rec.camera], W, H, MAX_STEPS)
            out["frame"] = {d: g[d][0] for d in ("xrgb",) + V.DIAGNOSTICS}
            out["skips"] = r.miss_skip_active()
            for skips in (7, 0):
                r.set_exact_skips(skips)
                for kind, rays_fn, pixels_fn in (("trace", TR.trace_rays, TR.trace_pixels), ("shade", TS.shade_rays, TS.shade_pixels)):
                    out[kind, "pixels", skips] = pixels_fn(torch, r, all_pixels(), W, H, camera=rec.camera, max_steps=MAX_STEPS)
                    out[kind, "shared", skips] = rays_fn(torch, r, shared_list(rs), max_steps=MAX_STEPS)
                    out[kind, "own", skips] = rays_fn(torch, r, own_list(rs, rec), max_steps=MAX_STEPS)
        finally:
            r.close()
        _kept[key] = (rec, out)
    return _kept[key][1]


# ------------------------------------------------------------------------------------------------------------------ scene views
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("rs", SR.SETS, ids=ids)
def test_every_record_is_its_own_frame(torch_cuda, rs, arm):
    """one call, K = 1, all records of the set: pixels, rgb, dist and id are the oracle's frame of that record's scene and camera, both
    step counts a fresh context's that uploaded the record; nothing outside the views is written (pitch w + 5, stride + 8)"""
    recs = SR.records(rs)
    with renderer(rs, arm) as r:
        b = render(torch_cuda, r, recs)
    for v, rec in enumerate(recs):
        what = f"{rs.name} {rec.label} ({arm})"
        V.assert_view_is_oracle(b, v, oracle_frame(rec), what)
        want = fresh(torch_cuda, rs, rec)["frame"]["steps"]
        assert np.array_equal(b["steps"][v] & 0xFFFF, want & 0xFFFF), f"{what}: march steps"
        assert np.array_equal(b["steps"][v] >> 16, want >> 16), f"{what}: shadow steps"
    # (the records differ: a kernel that rendered one record's list for another would show)
    assert len({b["xrgb"][v].tobytes() for v in range(len(recs))}) == len(recs)


@pytest.mark.parametrize("arm", INTERP_ARMS)
@pytest.mark.parametrize("rs", SR.SETS, ids=ids)
def test_which_scene_is_uploaded_changes_nothing(torch_cuda, rs, arm):
    """the records rendered on contexts that uploaded three different records of the set (the most and the least bounded of
    bound-flips, the record 1000 times the size of other-scale among them): every output plane is byte-equal between the uploads,
    steps included — whatever the upload proved, a record's list is built from the record"""
    recs = SR.records(rs)
    first = None
    for label in rs.uploads:
        with renderer(rs, arm, upload=label) as r:
            b = render(torch_cuda, r, recs)
        if first is None:
            first = b
            for v, rec in enumerate(recs):
                V.assert_view_is_oracle(b, v, oracle_frame(rec), f"{rs.name} {rec.label} ({arm}, {label} uploaded)")
            continue
        assert np.array_equal(b["raw"], first["raw"]), f"{rs.name} ({arm}): pixels differ between uploading {rs.uploads[0]} and {label}"
        for v, rec in enumerate(recs):
            same_planes(b, v, first, v, f"{rs.name} {rec.label} ({arm}): {label} uploaded instead of {rs.uploads[0]}")


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("rs", SR.SETS, ids=ids)
def test_order_and_company_change_nothing(torch_cuda, rs, arm):
    """the records reversed, each alone, and one record repeated between and behind two others: the planes of the first call"""
    recs = SR.records(rs)
    n = len(recs)
    with renderer(rs, arm) as r:
        first = render(torch_cuda, r, recs)
        back = render(torch_cuda, r, recs[::-1])
        for v in range(n):
            same_planes(back, n - 1 - v, first, v, f"{rs.name} {recs[v].label} ({arm}): reversed")
        for v in range(n):
            alone = render(torch_cuda, r, [recs[v]])
            same_planes(alone, 0, first, v, f"{rs.name} {recs[v].label} ({arm}): alone")
        x = n // 2
        company = [0, x, x, n - 1, x]
        again = render(torch_cuda, r, [recs[i] for i in company])
        for at, v in enumerate(company):
            same_planes(again, at, first, v, f"{rs.name} {recs[v].label} ({arm}): at {at} of {company}")


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("rs", [rs for rs in SR.SETS if rs.blends], ids=ids)
def test_blends_over_records_with_different_plans(torch_cuda, rs, arm):
    recs = SR.records(rs)
    groups = {2: recs[:6], 4: [recs[0], recs[2], recs[4], recs[5]] + recs[1:5]}   # three views of two, two views of four
    with renderer(rs, arm) as r:
        for k, group in groups.items():
            scs, cams = scenes_and_cameras(group)
            b = render(torch_cuda, r, group, k, debug=("rgb",))
            px, rgb = F.render_blend(scs, cams, k, W, H, max_steps=MAX_STEPS)
            assert np.array_equal(b["xrgb"], px), f"{rs.name} K={k} ({arm}): pixels differ from the reference"
            assert np.array_equal(bits(b["rgb"]), bits(rgb)), f"{rs.name} K={k} ({arm}): rgb differs from the reference"


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("rs,s", [(rs, s) for rs in SR.SETS for s in rs.samples], ids=lambda x: x.name if hasattr(x, "name") else "s%d" % x)
def test_supersampled_records(torch_cuda, rs, s, arm):
    """s x s samples under every record's own scene: scene_view_samples_reference on the records' Scenes"""
    recs = SR.records(rs)
    scs, cams = scenes_and_cameras(recs)
    with renderer(rs, arm) as r:
        b = render(torch_cuda, r, recs, 1, s, debug=("rgb",))
    px, rgb = SVR.render(scs, cams, 1, s, W, H, max_steps=MAX_STEPS)
    for v, rec in enumerate(recs):
        assert np.array_equal(b["xrgb"][v], px[v]), f"{rs.name} {rec.label} s={s} ({arm}): pixels differ from the reference"
        assert np.array_equal(bits(b["rgb"][v]), bits(rgb[v])), f"{rs.name} {rec.label} s={s} ({arm}): rgb differs from the reference"


# ---------------------------------------------------------------------------------------------------------------- scene queries
@pytest.mark.parametrize("specialize", (0, 4), ids=("plain", "fast"))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rs", SR.SETS, ids=ids)
def test_every_pixel_of_every_record(torch_cuda, rs, kind, specialize):
    """all 23 x 13 pixels under each record's own camera and scene: the single-scene query of a context that uploaded the record
    (every field, all 32 bits of `steps`, skips on and off), the CPU reference on the record's Scene and, shaded, the frame of
    render_scene_views_into on the same context, which is the oracle's"""
    recs = SR.records(rs)
    scs, cams = scenes_and_cameras(recs)
    xy = all_pixels()
    r = SQ.open_fresh(SR.uploaded(rs), specialize)
    try:
        for skips in (7, 0):
            r.set_exact_skips(skips)
            got = SQ.scene_query(torch_cuda, r, kind, scs, len(xy), xy=xy, size=(W, H), cameras=cams, max_steps=MAX_STEPS)
            frames = render(torch_cuda, r, recs) if kind == "shade" else None
            for v, rec in enumerate(recs):
                what = f"{rs.name} {rec.label}: {kind} pixels, skips {skips}, specialize {specialize}"
                SQ.assert_same(kind, got[v], fresh(torch_cuda, rs, rec)[kind, "pixels", skips], what + ": the fresh context")
                SQ.assert_same(kind, got[v], cpu_reference(kind, rs, rec, "pixels"), what + ": the CPU reference", march_steps_only=skips != 0,
                               fields=tuple(got[v]))
                if kind == "shade":
                    frame = dict(pixel=frames["xrgb"][v].ravel(), rgb=frames["rgb"][v].reshape(-1, 3), dist=frames["dist"][v].ravel(),
                                 id=frames["id"][v].ravel(), steps=frames["steps"][v].ravel())
                    SQ.assert_same(kind, got[v], frame, what + ": the frame of render_scene_views_into")
                    if skips == 7:
                        V.assert_view_is_oracle(frames, v, oracle_frame(rec), what)
    finally:
        r.close()


@pytest.mark.parametrize("specialize", (0, 4), ids=("plain", "fast"))
@pytest.mark.parametrize("lists", ["shared", "own"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rs", SR.SETS, ids=ids)
def test_ray_lists_of_every_record(torch_cuda, rs, kind, lists, specialize):
    """70 rays per record, the special rays among them: one list for every record (list_stride = 0), and a list per record — aimed
    and grazing rays made from that record's OWN culling bounds — 75 rays apart, NaN rays in the gaps"""
    recs = SR.records(rs)
    scs, _ = scenes_and_cameras(recs)
    own = [own_list(rs, rec) for rec in recs]
    assert len({a.tobytes() for a in own}) == len(own)
    buf, stride = (shared_list(rs), 0) if lists == "shared" else (SQ.with_gaps(own, LIST_STRIDE, np.float32(np.nan)), LIST_STRIDE)
    r = SQ.open_fresh(SR.uploaded(rs), specialize)
    try:
        for skips in (0, 7):
            r.set_exact_skips(skips)
            got = SQ.scene_query(torch_cuda, r, kind, scs, N, rays=buf, stride=stride, max_steps=MAX_STEPS)
            for v, rec in enumerate(recs):
                what = f"{rs.name} {rec.label}: {kind} rays ({lists}), skips {skips}, specialize {specialize}"
                SQ.assert_same(kind, got[v], fresh(torch_cuda, rs, rec)[kind, lists, skips], what + ": the fresh context", march_steps_only=skips != 0)
                SQ.assert_same(kind, got[v], cpu_reference(kind, rs, rec, lists), what + ": the CPU reference", march_steps_only=skips != 0,
                               fields=tuple(got[v]))
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------- the host's decisions
def test_the_skips_are_each_records_own(torch_cuda):
    """what a fresh context that uploaded a record of skip-flips reports as its active skips (lol_gpu_miss_skip_active: bit 0 escaped
    waves, bit 1 zero incidence, bit 2 settled shadows) is what tests/scene_records.py declares for that record"""
    assert bytes(SR.record(SR.SKIPS, "camera-insane").camera) == bytes(SR.insane_camera()) == bytes(V.insane_camera())      # the families' own
    for rec in SR.records(SR.SKIPS):
        miss, dark, settle = SR.SKIPS_DECLARED[rec.label][:3]
        assert fresh(torch_cuda, SR.SKIPS, rec)["skips"] == (1 if miss else 0) | (2 if dark else 0) | (4 if settle else 0), rec.label
    # ... and the step counts show it: the sane record and the one whose material #0 has a diffuse colour are one scene to the march,
    # and differ in the shadow steps of escaped rays alone
    lit, sane = (fresh(torch_cuda, SR.SKIPS, SR.record(SR.SKIPS, k))["frame"] for k in ("diffuse-0", "sane"))
    assert np.array_equal(lit["steps"] & 0xFFFF, sane["steps"] & 0xFFFF) and np.array_equal(lit["id"], sane["id"])
    more = (lit["steps"] >> 16) != (sane["steps"] >> 16)
    assert more.any() and (lit["id"][more] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------ ties
TIES = [(rs, rec) for rs in SR.SETS for rec in SR.records(rs) if rec.tied]


@pytest.mark.parametrize("rs,rec", TIES, ids=lambda x: getattr(x, "label", None) or x.name)
def test_ties_go_to_the_lowest_id_in_every_family(torch_cuda, rs, rec):
    """the central pixel of a tie record: the lowest tied id, in that object's material's hue, on every arm of the scene views, in
    the supersampled views (where the tied objects are one shape) and in both scene queries — with other records round it"""
    recs = SR.records(rs)
    at = recs.index(rec)
    first = min(rec.tied)
    mats = rec.scene.materials()
    hue = RF.dominant_channel(mats[SR.root_node(rec.scene, first).material].diffuse.tuple())
    others = {RF.dominant_channel(mats[SR.root_node(rec.scene, i).material].diffuse.tuple()) for i in rec.tied if i != first}
    assert hue is not None and hue not in others
    cx, cy = W // 2, H // 2
    xy = np.array([(cx, cy)], np.uint32)
    for arm in ARMS:
        with renderer(rs, arm) as r:
            b = render(torch_cuda, r, recs)
            assert b["id"][at, cy, cx] == first, f"{rec.label} ({arm}): the tie went to id {b['id'][at, cy, cx]}"
            assert RF.dominant_channel(b["rgb"][at, cy, cx]) == hue, f"{rec.label} ({arm}): the colour is another material's"
            if rec.coincide:
                for s in rs.samples:
                    aa = render(torch_cuda, r, recs, 1, s, debug=("rgb",))
                    assert RF.dominant_channel(aa["rgb"][at, cy, cx]) == hue, f"{rec.label} s={s} ({arm}): the colour is another material's"
            if arm == "structure-module":
                continue
            scs, cams = scenes_and_cameras(recs)
            hit = SQ.scene_query(torch_cuda, r, "trace", scs, 1, xy=xy, size=(W, H), cameras=cams, max_steps=MAX_STEPS)[at]
            shade = SQ.scene_query(torch_cuda, r, "shade", scs, 1, xy=xy, size=(W, H), cameras=cams, max_steps=MAX_STEPS)[at]
            assert hit["id"][0] == first and shade["id"][0] == first, f"{rec.label} ({arm}): the queries' tie"
            assert RF.dominant_channel(shade["rgb"][0]) == hue, f"{rec.label} ({arm}): the shading query's colour"
            # ... and straight down the central ray as a ray of a list, a tie at every step of its march
            ray = np.array([[0, 0, 0, 0, 0, -1]], np.float32)
            hit = SQ.scene_query(torch_cuda, r, "trace", scs, 1, rays=ray, max_steps=MAX_STEPS)[at]
            assert hit["id"][0] == first, f"{rec.label} ({arm}): the central ray of a list"
