"""tests/scene_records.py is what it claims, on the CPU: every record has the uploaded scene's structure; the interpreter lists the
scene-record calls would build (lol_gpu_interp_list_info: no device) differ between the records of a set in order, tie flags, test
records, unbounded objects and length as declared; the ties are exact and go to the lowest id in another colour; the three exact skips,
FINITE, SANE and the first step differ between the records of skip-flips as declared; and the oracle's pictures are not degenerate
and differ between any two records of a set."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import scene_records as SR
import scene_shapes as SH
from loltracer_amd import gpu, scene as S

ids = lambda rs: rs.name                 # noqa: E731
_kept = {}


def info(rec, cull=True):
    key = (id(rec.scene), cull)
    if key not in _kept:
        _kept[key] = (rec, gpu.interp_list_info(rec.scene.flatten(), cull))
    return _kept[key][1]


def oracle_ids(rec, size, camera=None):
    """(packed pixels, hit ids) of the oracle's frame of a record, under its own camera or `camera`"""
    w, h = size
    px, _, steps = O.render_rows(rec.scene, w, h, 0, h, 256, camera=rec.camera if camera is None else camera, want_steps=True)
    return px, steps[..., 2]


def oracle_sdf(sc, p):
    oid = ctypes.c_uint32()
    d = O.lib().lol_oracle_sdf(sc.ptr, float(p[0]), float(p[1]), float(p[2]), ctypes.byref(oid))
    return np.float32(d), oid.value


def test_the_catalogue_is_the_five_sets():
    assert [rs.name for rs in SR.SETS] == ["crowd-regrouped", "bound-flips", "other-scale", "skip-flips", "deep"]
    for rs in SR.SETS:
        labels = [r.label for r in SR.records(rs)]
        assert 5 <= len(labels) <= 8 and len(set(labels)) == len(labels), rs.name
        assert len(rs.uploads) >= 3 and set(rs.uploads) <= set(labels), rs.name
        assert rs.size == SH.HOSTILE_SIZE
    assert SR.CROWD.blends and SR.FLIPS.blends and SR.CROWD.samples == (2, 4) and all(2 in rs.samples for rs in SR.SETS)
    assert {"all-bounded", "none-bounded"} <= set(SR.FLIPS.uploads) and "scale-1000" in SR.SCALES.uploads
    # three rungs of the interpreter's ladder between them
    assert [SH.rung_of(SR.uploaded(rs).flatten()) for rs in SR.SETS] == [(1, False), (3, False), (1, False), (3, False), (7, False)]


@pytest.mark.parametrize("rs", SR.SETS, ids=ids)
def test_every_record_has_the_uploaded_structure(rs):
    up = SR.uploaded(rs)
    p = up.flatten()
    for rec in SR.records(rs):
        assert S.same_structure(up, rec.scene), rec.label
        q = rec.scene.flatten()
        assert (q.n_ops, q.n_lights, q.n_materials, q.n_roots, q.max_stack) == (p.n_ops, p.n_lights, p.n_materials, p.n_roots, p.max_stack)
        assert [(q.ops[i].op, q.ops[i].id) for i in range(q.n_ops)] == [(p.ops[i].op, p.ops[i].id) for i in range(p.n_ops)], rec.label


def test_the_list_info_of_a_plain_scene():
    """scene4: a plane and one blob — two objects, the plane first (it has no bound), one test in front of the blob, no tie flag on
    the first object; without culling, file order and no test.  Bad arguments are refused."""
    sc = S.Scene.parse_file(SH.SCENES_DIR + "/scene4.lol")
    p = sc.flatten()
    on, off = gpu.interp_list_info(p, True), gpu.interp_list_info(p, False)
    assert sorted(on["order"]) == list(off["order"]) == list(range(1, p.n_roots + 1))
    assert off["n_tests"] == 0 and off["n_unbounded"] == p.n_roots and not any(off["tie"])
    assert on["n_mops"] == off["n_mops"] + on["n_tests"] and on["n_tests"] >= 1 and on["n_unbounded"] == 1
    assert on["tie"][0] == 0
    lib = gpu.gpu_lib()
    assert lib.lol_gpu_interp_list_info(None, 1, None, None, None, None, None, 0) == -3
    assert lib.lol_gpu_interp_list_info(ctypes.byref(p), 1, None, None, None, None, None, 4) == -3       # a capacity and no arrays
    assert lib.lol_gpu_interp_list_info(ctypes.byref(p), 1, None, None, None, None, None, 0) == p.n_roots
    one, flag = (ctypes.c_uint32 * 1)(), (ctypes.c_uint32 * 1)()
    assert lib.lol_gpu_interp_list_info(ctypes.byref(p), 1, None, None, None, one, flag, 1) == p.n_roots and one[0] == on["order"][0]


@pytest.mark.parametrize("rs", SR.SETS, ids=ids)
def test_the_tie_flag_is_the_order(rs):
    """MOP_TIE as the list carries it: exactly on the objects evaluated after one with a higher id; n_mops = objects' records + tests"""
    for rec in SR.records(rs):
        for cull in (True, False):
            i = info(rec, cull)
            n = rec.scene.c.n_roots
            assert sorted(i["order"]) == list(range(1, n + 1)), rec.label
            seen, want = 0, []
            for obj in i["order"]:
                want.append(int(obj < seen))
                seen = max(seen, obj)
            assert list(i["tie"]) == want, (rec.label, cull)
            assert i["n_mops"] - i["n_tests"] == info(rec, False)["n_mops"], rec.label
            assert list(i["order"][:i["n_unbounded"]]) == sorted(i["order"][:i["n_unbounded"]]), rec.label     # the unbounded ones first, in file order


@pytest.mark.parametrize("rs", SR.SETS, ids=ids)
def test_without_culling_every_record_has_the_files_list(rs):
    recs = SR.records(rs)
    n = recs[0].scene.c.n_roots
    assert len({info(r, False)["n_mops"] for r in recs}) == 1
    for r in recs:
        i = info(r, False)
        assert i["order"] == tuple(range(1, n + 1)) and not any(i["tie"]) and i["n_tests"] == 0 and i["n_unbounded"] == n, r.label


def test_the_plans_differ_as_declared():
    crowd = [info(r) for r in SR.records(SR.CROWD)]
    assert len({i["order"] for i in crowd}) >= 4 and len({i["tie"] for i in crowd}) >= 3
    flips = [info(r) for r in SR.records(SR.FLIPS)]
    assert len({i["n_mops"] for i in flips}) >= 4
    assert {1, SR.FLIPS_N} <= {i["n_unbounded"] for i in flips} and any(i["n_tests"] == 0 for i in flips)
    by = {r.label: info(r) for r in SR.records(SR.FLIPS)}
    assert [by[k]["n_unbounded"] for k in ("all-bounded", "minus-1", "minus-3", "minus-5", "none-bounded", "minus-2", "negative-radius")] == [1, 2, 4, 6, 9, 3, 1]
    assert by["all-bounded"]["order"][0] == SR.FLIPS_PLANE and by["none-bounded"]["order"] == tuple(range(1, 10))
    assert len({i["n_mops"] for i in (info(r) for r in SR.records(SR.DEEP))}) >= 2
    # the sets built on bound-flips' scene and on tie-crowd upload what they say
    assert SR.uploaded(SR.CROWD).tables() == SH.hostile_scene(SH.HOSTILE_BY_NAME["tie-crowd"]).tables()
    assert SR.uploaded(SR.SKIPS).tables() == SR.uploaded(SR.FLIPS).tables()


def test_bound_flips_is_the_scene_it_describes():
    sc = SR.uploaded(SR.FLIPS)
    nodes, roots = sc.nodes(), sc.roots()
    kinds = [nodes[r].type for r in roots]
    assert 8 <= len(roots) <= 10 and kinds.index(S.NODE_PLANE) > 0 and kinds.count(S.NODE_PLANE) == 1
    assert kinds.count(S.NODE_SPHERE) >= 2 and kinds.count(S.NODE_BOX) >= 2
    sizes = sorted(len(SR.leaves(sc, r)) for r in roots if nodes[r].type == S.NODE_SMOOTH_UNION)
    assert sizes == [2, 3, 4]                                                    # two and three spheres, and the nested union of four
    assert sc.c.n_lights == 2 and len({nodes[r].material for r in roots} - {0}) >= 2
    negative = SR.record(SR.FLIPS, "negative-radius")
    prog = negative.scene.flatten()
    c, r = (ctypes.c_float * 3)(), ctypes.c_float()
    assert gpu.gpu_lib().lol_gpu_cull_bounds(ctypes.byref(prog), 8 - 1, c, ctypes.byref(r)) == 1 and r.value < 1e-3       # bounded, tiny


def test_other_scale_is_what_it_says():
    by = {r.label: r for r in SR.records(SR.SCALES)}
    base = by["scale-1"].scene
    proven = {n.smoothness for n in base.nodes() if n.type == S.NODE_SMOOTH_UNION}
    ks = lambda label: [n.smoothness for n in by[label].scene.nodes() if n.type == S.NODE_SMOOTH_UNION]      # noqa: E731
    assert len(proven) == 4 and not set(ks("unproven")) & proven
    assert set(ks("mixed")) & proven and set(ks("mixed")) - proven
    assert not set(ks("scale-1000")) & proven and max(ks("scale-30")) == 1800.0
    assert 0 < SR.root_node(by["tiny-radius"].scene, 8).radius < 2.0 ** -20
    for label, f in (("scale-30", 30.0), ("scale-1000", 1000.0)):
        sc = by[label].scene
        assert sc.camera.point.y == float(np.float32(base.camera.point.y) * np.float32(f))
        assert SR.root_node(sc, 8).radius == 0.5 * f and SR.root_node(sc, 2).point.y == -f


def test_deep_is_rung_seven_with_tests_between_stack_users():
    sc = SR.uploaded(SR.DEEP)
    p = sc.flatten()
    assert SH.rung_of(p) == (7, False) and p.max_stack == 5
    assert [len(SR.leaves(sc, sc.roots()[t - 1])) for t in SR.DEEP_TREES] == [16, 16]
    i = info(SR.records(SR.DEEP)[0])
    trees = [i["order"].index(t) for t in SR.DEEP_TREES]
    assert min(trees) >= 1 and i["n_tests"] >= 4                                 # each tree behind another object: a test in front of it
    sharp = SR.record(SR.DEEP, "smoothness-0")
    assert info(sharp)["n_unbounded"] == 2 and all(sharp.scene.c.nodes[u].smoothness == 0.0 for u in SR.unions(sharp.scene, sharp.scene.roots()[1]))
    assert all(sharp.scene.c.nodes[leaf].radius > 0 for leaf in SR.leaves(sharp.scene, sharp.scene.roots()[4]))
    shrunk = SR.record(SR.DEEP, "negative-radii")
    assert all(shrunk.scene.c.nodes[leaf].radius < 0 for leaf in SR.leaves(shrunk.scene, shrunk.scene.roots()[4]))


# ---------------------------------------------------------------------------------------------------------------------- ties
def alone(sc, obj_id):
    """the scene with every top-level object but `obj_id` out of reach (spheres and planes: crowd-regrouped has nothing else)"""
    out = sc.clone()
    for k in range(1, sc.c.n_roots + 1):
        n = SR.root_node(out, k)
        assert n.type in (S.NODE_SPHERE, S.NODE_PLANE)
        if k != obj_id:
            n.point.y = -1e19
    return out


TIE_RECORDS = [(rs, rec) for rs in SR.SETS for rec in SR.records(rs) if rec.tied]


@pytest.mark.parametrize("rs,rec", TIE_RECORDS, ids=lambda x: getattr(x, "label", None) or x.name)
def test_ties_are_exact_and_go_to_the_lowest_id(rs, rec):
    sc = rec.scene
    w, h = rs.size
    first = min(rec.tied)
    assert sc.camera.point.tuple() == (0.0, 0.0, 0.0) and sc.camera.direction.tuple() == (0.0, 0.0, -1.0)
    centre = O.probe(sc, w, h, w // 2, h // 2, camera=rec.camera)
    assert tuple(centre.rd) == (0.0, 0.0, -1.0)
    pts = [(0.0, 0.0, 0.0)] + [(0.0, 0.0, -float(np.float32(t))) for t in (0.5, 1.0, 1.7, 2.25, 3.1, float(centre.hit_dist) - 0.5, float(centre.hit_dist))]
    singles = [alone(sc, i) for i in rec.tied]
    for p in pts:
        values = {oracle_sdf(one, p)[0].view(np.uint32).item() for one in singles}
        assert len(values) == 1, (rec.label, p, values)                          # bit-equal: the tie is real
        d, oid = oracle_sdf(sc, p)
        assert (d.view(np.uint32).item(), oid) == (values.pop(), first), (rec.label, p, oid)      # ... the scene's minimum, and the lowest id wins
    _, hit = oracle_ids(rec, rs.size)
    assert hit[h // 2, w // 2] == first == centre.hit_id
    if rec.coincide:
        assert first in hit and not (set(rec.tied) - {first}) & set(hit.ravel().tolist())
    else:                                # mirror images: the other one shows on its own side, and the whole central row is tied
        assert set(rec.tied) <= set(hit.ravel().tolist()) and not (set(rec.tied) - {first}) & set(hit[h // 2].tolist())
    # a winner of the wrong id would wear another material, of another colour
    mats = sc.materials()
    mine = SR.root_node(sc, first).material
    for other in set(rec.tied) - {first}:
        m = SR.root_node(sc, other).material
        assert m != mine and mats[m].diffuse.tuple() != mats[mine].diffuse.tuple(), (rec.label, other)


def test_the_ties_sit_where_the_set_says():
    by = {r.label: r for r in SR.records(SR.CROWD)}
    assert by["file"].tied == by["permuted-1"].tied == by["permuted-2"].tied == (3, 9, 14) and by["apart"].tied == ()
    assert by["pair-5-12"].tied == (5, 12) and len(by["heap"].tied) == 15 and min(by["heap"].tied) == 1
    assert by["mirror-4-13"].tied == (4, 13) and not by["mirror-4-13"].coincide
    # pulled apart, the three are no tie: three different values at the camera
    assert len({oracle_sdf(alone(by["apart"].scene, i), (0, 0, 0))[0].item() for i in (3, 9, 14)}) == 3
    # the tie flag has moved with the order: the lowest tied id is evaluated AFTER a higher tied id in at least one record
    late = 0
    for r in by.values():
        order = info(r)["order"]
        if r.tied and order.index(min(r.tied)) > min(order.index(t) for t in r.tied if t != min(r.tied)):
            late += 1
            assert info(r)["tie"][order.index(min(r.tied))] == 1, r.label
    assert late >= 2


# ------------------------------------------------------------------------------------------------------------- skip-flips
def test_skip_flips_switch_each_decision_off_alone():
    w, h = SR.SKIPS.size
    got = {}
    for rec in SR.records(SR.SKIPS):
        sc = rec.scene
        got[rec.label] = (SR.miss_skip_ok(sc), SR.dark_skip_ok(sc), SR.shadow_settle_ok(sc), SR.camera_sane(sc, w, h),
                          SR.first_step_given(sc, w, h, lambda s, p: oracle_sdf(s, p)[0]))
    assert got == SR.SKIPS_DECLARED
    labels = [r.label for r in SR.records(SR.SKIPS)]
    assert 0 < labels.index("sane") < len(labels) - 1 and SR.SKIPS_DECLARED["sane"] == (True,) * 5
    for k in range(5):                   # each decision is off in some record and on in others
        assert {v[k] for v in SR.SKIPS_DECLARED.values()} == {True, False}, k
    assert sum(v == (False, True, True, True, True) for v in got.values()) == 1          # the miss skip alone
    assert sum(v == (True, False, True, True, True) for v in got.values()) == 1          # the dark skip alone
    # every other set: all records finite and sane but those that hold a 1e19
    for rs in (SR.CROWD, SR.SCALES, SR.DEEP):
        assert all(SR.shadow_settle_ok(r.scene) and SR.camera_sane(r.scene, w, h) for r in SR.records(rs)), rs.name
    finite = {r.label: SR.shadow_settle_ok(r.scene) for r in SR.records(SR.FLIPS)}
    assert finite == {"all-bounded": True, "minus-1": True, "minus-3": True, "minus-5": False, "none-bounded": False, "minus-2": False,
                      "negative-radius": True}


# --------------------------------------------------------------------------------------------------------------- pictures
@pytest.mark.parametrize("rs", SR.SETS, ids=ids)
def test_no_degenerate_pictures(rs):
    """at most one record of a set shows a single id; every other frame has at least two ids, hits and escapes"""
    single = 0
    for rec in SR.records(rs):
        _, hit = oracle_ids(rec, rs.size)
        seen = set(hit.ravel().tolist())                                         # (an escaped ray's id is 0: it counts as one)
        if len(seen) == 1:
            single += 1
        else:
            assert 0 in seen and seen - {0}, (rec.label, seen)
    assert single <= 1, rs.name


@pytest.mark.parametrize("rs", SR.SETS, ids=ids)
def test_any_two_records_differ_in_a_pixel(rs):
    recs = SR.records(rs)
    cam = recs[0].camera
    frames = [oracle_ids(r, rs.size, cam)[0] for r in recs]
    for i in range(len(recs)):
        for j in range(i):
            assert not np.array_equal(frames[i], frames[j]), (recs[i].label, recs[j].label)
