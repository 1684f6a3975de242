"""Instanced triangle-intersection queries on the GPU (include/shader_ray_instance_intersect.h) against the restatement
(tests/instance_intersect_ref.py): every triangle index, every instance index and every count, on the host path, the device
path and the device path without an instance buffer (the scratch path above K = 8), for K in {0, 1, 2, 3, 4, 5, 8, 9, 64} with
and without counts, for SHRAY_INTERSECT_ANY and with SHRAY_INTERSECT_SKIP_SHARED, with 1, 63, 64, 65 and 768 queries.  One
identity instance against Scene.intersecting_triangles (indices, counts and its three counters) and, in the instance form,
against Scene.self_intersections; the nine-instance set of tests/instance_intersect_cases.py in the item form and, for every
instance, in the instance form with and without SHRAY_INTERSECT_SKIP_OWN_INSTANCE; the placed lattice, where only the in-plane
axes separate; two scenes of different heights and 301 instances of the tiny scenes; the counters of the nine-instance set
against instance_intersect_ref.walk_counters with the stored boxes as read back; a refit, a device update and both device
forms on one stream, and a host update followed by the queries; a count split over two launches; the refusals."""
import ctypes as C

import numpy as np
import pytest

import instance_intersect_cases as XC
import instance_intersect_ref as II
import instance_point_cases as IC
import instance_point_ref as IP
import intersect_cases as TC
import intersect_ref as IR
import refit_ref
import test_gpu_instance_point as G
from test_gpu_instance_overlap import stored_boxes
from test_gpu_instance_point import build, member
from test_gpu_ray_query import loaded

pytestmark = pytest.mark.gpu

F = np.float32
EYE = IC.EYE
KS = (0, 1, 2, 3, 4, 5, 8, 9, 64)
SMALL_COUNTS = (1, 63, 64, 65)
PATHS = ("host", "device", "no instance buffer")
COUNTERS = ("node_visits", "leaf_visits", "triangle_tests", "traversals")
_answers = {}


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    if "flat" in _answers:
        _answers["flat"][2].close()
        _answers["flat"][0].close()
    _answers.clear()
    for s in G._sets:
        s.close()
    G._sets.clear()
    for _, sc in G._members.values():
        sc.close()
    G._members.clear()


def dev_triangles(queries):
    import torch
    return torch.from_numpy(IR.make_triangles(queries).view(F).reshape(-1, 12).copy()).cuda()


def restate(positions, of, maps, queries, k=64, skip_shared=False):
    member_, first = II.membership(positions, of, maps, queries, skip_shared)
    return II.from_membership(member_, first, k)


def query(s, queries, k, counts, path, any_only=False, skip_shared=False):
    """(triangles [n, k], instances [n, k], counts [n]) as numpy, None for what is not returned.  Paths: the blocking host form;
    the device form through intersecting_triangles on the current torch stream; the device form without an instance buffer."""
    import torch
    n = len(queries)
    if path == "host":
        tri, inst, cnt = s.intersecting_triangles(queries, max_triangles=k, counts=counts, any_only=any_only, skip_shared=skip_shared)
        assert (tri is None) == (k == 0) and (inst is None) == (k == 0) and (cnt is None) == (not counts)
        if k:
            assert tri.dtype == np.int32 and tri.shape == (n, k) and inst.dtype == np.int32 and inst.shape == (n, k)
        return tri, inst, cnt
    if path == "device":
        tri, inst, cnt = s.intersecting_triangles(dev_triangles(queries), max_triangles=k, counts=counts, any_only=any_only,
                                                  skip_shared=skip_shared)
        torch.cuda.current_stream().synchronize()
        assert (tri is None) == (k == 0) and (inst is None) == (k == 0) and (cnt is None) == (not counts)
        if k:
            assert tri.dtype == torch.int32 and tuple(tri.shape) == (n, k) and tuple(inst.shape) == (n, k) and inst.is_cuda
        return (tri.cpu().numpy() if k else None), (inst.cpu().numpy() if k else None), (cnt.cpu().numpy() if counts else None)
    assert path == "no instance buffer"
    d = dev_triangles(queries)
    out = torch.full((n, max(k, 1)), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    s.intersecting_triangles_into(d.data_ptr(), n, out.data_ptr() if k else 0, 0, cnt.data_ptr() if counts else 0, k, any_only, skip_shared,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    return (out.cpu().numpy() if k else None), None, (cnt.cpu().numpy() if counts else None)


def own_query(s, q, k, counts, path, any_only=False, skip_shared=False, skip_own=True, first=0, count=None):
    """the instance form on the same three paths"""
    import torch
    if path == "host":
        return s.instance_intersections(q, max_triangles=k, counts=counts, any_only=any_only, skip_shared=skip_shared, skip_own=skip_own,
                                        first=first, count=count)
    if path == "device":
        got = s.instance_intersections(q, max_triangles=k, counts=counts, any_only=any_only, skip_shared=skip_shared, skip_own=skip_own,
                                       first=first, count=count, device=True)
        torch.cuda.current_stream().synchronize()
        assert all(g is None or (g.is_cuda and g.dtype == torch.int32) for g in got)
        return tuple(None if g is None else g.cpu().numpy() for g in got)
    n = s.triangle_count(q) - first if count is None else count
    out = torch.full((max(n, 1), max(k, 1)), -7, dtype=torch.int32, device="cuda")      # (an empty tensor has no pointer)
    cnt = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    s.instance_intersections_into(q, first, n, out.data_ptr() if k else 0, 0, cnt.data_ptr() if counts else 0, k, any_only, skip_shared,
                                  skip_own, torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    assert bool((out[n:] == -7).all()) and bool((cnt[n:] == -7).all()), "nothing is written past the range"
    return (out[:n].cpu().numpy() if k else None), None, (cnt[:n].cpu().numpy() if counts else None)


def assert_answer(got, want64, k, counts, what):
    tri, inst, cnt = got
    w_tri, w_inst, w_cnt = want64
    if k:
        bad = np.nonzero((tri != w_tri[:len(tri), :k]).any(1))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {len(tri)} queries differ, first {bad[:5]}: got {tri[bad[:3]]} want {w_tri[bad[:3], :k]}"
        if inst is not None:
            assert np.array_equal(inst, w_inst[:len(inst), :k]), (what, np.nonzero((inst != w_inst[:len(inst), :k]).any(1))[0][:5])
    else:
        assert tri is None and inst is None, what
    if counts:
        assert cnt.dtype == np.int32 and np.array_equal(cnt, w_cnt[:len(cnt)]), (what, np.nonzero(cnt != w_cnt[:len(cnt)])[0][:5])
    else:
        assert cnt is None, what


def check_every_form(s, queries, want64, want64_shared, what):
    """every K with and without counts and the ANY form on the three paths at all the queries, without and with SKIP_SHARED, the
    two short forms, and the small counts (where the last wave is partial, full, and one lane over) at the Ks on either side of
    the register slots' edge; K = 0 without counts is refused by the binding"""
    import torch
    for skip_shared, want in ((False, want64), (True, want64_shared)):
        if want is None:
            continue
        met = (want[2] > 0).astype(np.int32)
        for k in KS:
            for counts in (True, False):
                if k == 0 and not counts:
                    with pytest.raises(ValueError):
                        s.intersecting_triangles(queries, max_triangles=0, counts=False)
                    continue
                for path in PATHS:
                    assert_answer(query(s, queries, k, counts, path, skip_shared=skip_shared), want, k, counts,
                                  f"{what}, K = {k}, counts = {counts}, SKIP_SHARED = {skip_shared}, {path}")
        for path in PATHS:
            got = query(s, queries, 0, True, path, any_only=True, skip_shared=skip_shared)
            assert got[0] is None and got[1] is None and got[2].dtype == np.int32 and np.array_equal(got[2], met), f"{what}, ANY, {path}"
        assert np.array_equal(s.intersection_counts(queries, skip_shared=skip_shared), want[2]), what
        assert np.array_equal(s.triangles_intersected(queries, skip_shared=skip_shared), met != 0), what
        on_device = s.triangles_intersected(dev_triangles(queries), skip_shared=skip_shared)
        assert on_device.dtype == torch.bool and np.array_equal(on_device.cpu().numpy(), met != 0), what
    for count in SMALL_COUNTS:
        for k, counts in ((1, False), (8, True), (9, False), (64, True)):
            for path in PATHS:
                assert_answer(query(s, queries[:count], k, counts, path), want64, k, counts,
                              f"{what}, {count} queries, K = {k}, counts = {counts}, {path}")


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_trisrc", "lobed_528", "one triangle", "11-triangle leaf"])
def test_one_identity_instance_is_the_triangle_intersection_query(pkg, gpu, name):
    """Consequence 1: Scene.intersecting_triangles' indices and counts with instance 0 on every held slot, and its three
    counters, the ANY form's too: the root of a one-instance set is not tested, and an identity map's image boxes are the
    boxes.  Consequence 7: the instance form without SKIP_OWN_INSTANCE is Scene.self_intersections."""
    positions, sc = member(pkg, name)
    s = build(pkg, [name], EYE[None], name)
    queries = TC.make_queries({"vertex_positions": positions}, XC.NINE_QUERIES, seed=len(name))
    want64 = {}
    for skip_shared in (False, True):
        tri, cnt = sc.intersecting_triangles(queries, max_triangles=64, skip_shared=skip_shared)
        want, want_cnt = IR.intersect(queries, positions, 64, skip_shared)
        assert np.array_equal(tri, want) and np.array_equal(cnt, want_cnt), "the plain query is the restatement"
        want64[skip_shared] = (tri, np.where(tri >= 0, 0, -1).astype(np.int32), cnt)
    cnt = want64[False][2]
    assert (cnt == 0).mean() > 0.04 and (cnt > 0).mean() > 0.3
    check_every_form(s, queries, want64[False], want64[True], f"{name}, identity")
    walked = int(IR.walked(queries).sum())
    for k, counts, any_only, skip_shared in ((8, True, False, False), (0, True, False, True), (64, False, False, False), (0, True, True, False),
                                             (0, True, True, True)):
        plain = sc.intersecting_triangles(queries, max_triangles=k, counts=counts, counters=True, any_only=any_only, skip_shared=skip_shared)[-1]
        got = s.intersecting_triangles(queries, max_triangles=k, counts=counts, counters=True, any_only=any_only, skip_shared=skip_shared)
        if any_only:
            assert np.array_equal(got[2], (want64[skip_shared][2] > 0).astype(np.int32))
        else:
            assert_answer(got[:3], want64[skip_shared], k, counts, f"{name}, counting form, K = {k}")
        tally = got[3]
        for c in ("node_visits", "leaf_visits", "triangle_tests", "samples"):
            assert tally[c] == plain[c], (name, k, any_only, c, tally, plain)
        assert tally["traversals"] == walked and tally["shaded_hits"] == tally["env_lookups"] == tally["bad_hits"] == 0
    # the instance form against the self form
    triangles = len(positions) // 9
    assert s.triangle_count(0) == triangles == sc.triangle_count()
    for skip_shared in (False, True):
        for k, counts in ((8, True), (64, False), (0, True)):
            self_tri, self_cnt = sc.self_intersections(max_triangles=k, counts=counts, skip_shared=skip_shared)
            want = (self_tri, None if self_tri is None else np.where(self_tri >= 0, 0, -1).astype(np.int32), self_cnt)
            for path in PATHS:
                got = own_query(s, 0, k, counts, path, skip_shared=skip_shared, skip_own=False)
                assert_answer(got, (want[0], want[1], want[2]), k, counts, f"{name}, instance form against self form, K = {k}, {path}")
        met = sc.self_intersections(max_triangles=0, any_only=True, skip_shared=skip_shared)[1]
        assert np.array_equal(own_query(s, 0, 0, True, "host", any_only=True, skip_shared=skip_shared, skip_own=False)[2], met)
    with_flag = s.instance_intersections(0, max_triangles=8)
    assert (with_flag[0] == -1).all() and (with_flag[1] == -1).all() and (with_flag[2] == 0).all(), "one instance: nothing but its own"
    assert not s.instances_colliding().any()
    if triangles > 3:
        lo, n = triangles - 3, 3
        sub = sc.self_intersections(max_triangles=8, skip_shared=False, first=lo, count=n)
        got = s.instance_intersections(0, max_triangles=8, skip_own=False, first=lo, count=n)
        assert np.array_equal(got[0], sub[0]) and np.array_equal(got[2], sub[1]), "a sub-range with the last triangle"


# 2 ---------------------------------------------------------------------------------------------------------------------------
def nine(pkg):
    """(names, distinct positions, scene of every instance, maps, the set, queries, the restatement at K = 64 without and with
    SKIP_SHARED, first-axis codes)"""
    if "nine" not in _answers:
        positions, of, maps, kinds, names = XC.nine_instances(lambda name: member(pkg, name)[0])
        assert kinds[4] == "duplicate of 1" and names[4] == names[1] and np.array_equal(maps[4].view(np.uint32), maps[1].view(np.uint32))
        s = build(pkg, names, maps, "nine instances")
        queries = XC.world_queries(positions, of, maps)
        merged, first = IP.merged_positions(positions, of, maps)
        code = IR.first_axis(queries, merged)
        shared = IR.first_axis(queries, merged, True)
        _answers["nine"] = (names, positions, of, maps, s, queries, II.from_membership(code == IR.INTERSECT, first, 64),
                            II.from_membership(shared == IR.INTERSECT, first, 64), code)
    return _answers["nine"]


def test_the_nine_instance_set(pkg, gpu):
    names, positions, of, maps, s, queries, want64, want64_shared, code = nine(pkg)
    print(XC.assert_mixed(queries, want64[1], want64[2], code, "nine instances"))
    assert (want64_shared[2] < want64[2]).mean() > 0.1, "SKIP_SHARED removes members"
    check_every_form(s, queries, want64, want64_shared, "nine instances")
    inst = want64[1]
    assert ((inst == 1).sum(1) >= (inst == 4).sum(1)).all() and (inst == 4).sum() > 100, "the duplicate sorts behind its original"


@pytest.mark.parametrize("q", range(9))
def test_the_instance_form_on_the_nine_instance_set(pkg, gpu, q):
    """Consequence 6 for every instance: the instance form equals the item form fed with instance q's rows of the merged scene;
    with SKIP_OWN_INSTANCE the pairs of instance q are gone and n is less by their number.  Sub-ranges, the last triangle
    among them."""
    names, positions, of, maps, s, *_ = nine(pkg)
    triangles = s.triangle_count(q)
    assert triangles == len(positions[of[q]]) // 9
    rows = II.own_queries(positions, of, maps, q)
    item = query(s, rows, 64, True, "host")
    for skip_own in (False, True):
        want = II.intersect_instance(positions, of, maps, q, 64, skip_own=skip_own)
        if not skip_own:
            assert_answer(item, want, 64, True, f"instance {q}: the item form on its own rows")
            assert (want[2] >= 1).all()
        else:
            assert not (want[1] == q).any()
        for path in PATHS:
            for k, counts in ((64, True), (8, False), (9, False), (0, True), (3, True)):
                assert_answer(own_query(s, q, k, counts, path, skip_own=skip_own), want, k, counts,
                              f"instance {q}, SKIP_OWN_INSTANCE = {skip_own}, K = {k}, counts = {counts}, {path}")
            got = own_query(s, q, 0, True, path, any_only=True, skip_own=skip_own)
            assert np.array_equal(got[2], (want[2] > 0).astype(np.int32)), f"instance {q}, ANY, {path}"
    shared = II.intersect_instance(positions, of, maps, q, 64, skip_shared=True)
    assert_answer(own_query(s, q, 64, True, "device", skip_shared=True), shared, 64, True, f"instance {q}, SKIP_SHARED on world corners")
    want = II.intersect_instance(positions, of, maps, q, 64)
    for first, count in ((triangles - 1, 1), (triangles // 3, min(70, triangles - triangles // 3)), (0, 0), (triangles, 0)):
        part = tuple(w[first:first + count] for w in want)
        for path in PATHS:
            assert_answer(own_query(s, q, 8, True, path, first=first, count=count), part, 8, True, f"instance {q}, [{first}, +{count}), {path}")
    whole = s.instance_intersections(q, first=triangles // 2)
    assert len(whole[0]) == triangles - triangles // 2 and np.array_equal(whole[0], want[0][triangles // 2:, :8])


def test_the_facts_of_the_nine_instance_set_and_instances_colliding(pkg, gpu):
    names, positions, of, maps, s, *_ = nine(pkg)
    met = {}
    for q in range(9):
        tri, inst, n = s.instance_intersections(q, max_triangles=64)
        met[q] = (int((n > 0).sum()), int(n.max()), sorted(set(inst[inst >= 0].tolist())))
    assert met[5] == (0, 0, [])
    assert met[1][:2] == (528, 29) and met[4][:2] == (528, 29) and met[1][2] == [4] and met[4][2] == [1]
    assert met[0][0] == 306 and met[0][2] == [6, 8]
    assert len(met[8][2]) == 5 and met[8][1] == 169
    colliding = s.instances_colliding()
    assert colliding.dtype == np.bool_ and colliding.tolist() == [q != 5 for q in range(9)]
    assert colliding.tolist() == II.colliding(positions, of, maps).tolist()


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 7])
def test_the_placed_lattice(pkg, gpu, tmp_path_factory, seed):
    """Three exact placements of the flat lattice, integer queries: the in-plane axes 12 to 17 are each first to separate some
    pair, and every index, instance and count is the restatement's, which tests/test_instance_intersect_reference.py holds
    against the exact clip."""
    if "flat" not in _answers:
        tris = TC.flat_lattice()
        path = str(tmp_path_factory.mktemp("instance_intersect") / "flat_lattice.obj")
        pkg.scenes.write_obj(path, tris.reshape(-1, 3).astype(np.float64), np.arange(3 * len(tris)).reshape(-1, 3))
        world = pkg.World(path)
        pos = np.asarray(world.arrays()["vertex_positions"], F).copy()
        assert len(pos) == tris.size and (pos == np.round(pos)).all()
        _answers["flat"] = (world, pos, pkg.Scene(world.flatten()))
    _, pos, scene = _answers["flat"]
    maps = XC.lattice_maps()
    s = pkg.tracer.InstanceSet([scene] * 3, maps)
    try:
        queries = XC.lattice_queries(seed)
        merged, first = IP.merged_positions([pos], [0, 0, 0], maps)
        assert np.array_equal(merged, np.rint(merged))
        code = IR.first_axis(queries, merged)
        per_axis = np.bincount(code[(code >= IR.AXIS0) & (code < IR.UNWALKED)].astype(np.int64) - IR.AXIS0, minlength=IR.AXES)
        assert min(per_axis[11:]) >= 1, per_axis.tolist()
        want = II.from_membership(code == IR.INTERSECT, first, 64)
        assert set(want[1][want[1] >= 0].tolist()) == {0, 1, 2}
        world = merged.reshape(-1, 3, 3)
        for j in np.nonzero(want[2] > 0)[0][:40]:
            for t, i in zip(want[0][j], want[1][j]):
                if t >= 0:
                    assert TC.exact_intersects(queries[j], world[first[i] + t]), (j, i, t)
        shared = II.from_membership(IR.first_axis(queries, merged, True) == IR.INTERSECT, first, 64)
        for path in PATHS:
            for k, counts in ((64, True), (8, False), (0, True)):
                assert_answer(query(s, queries, k, counts, path), want, k, counts, f"lattice, seed {seed}, K = {k}, {path}")
            assert_answer(query(s, queries, 64, True, path, skip_shared=True), shared, 64, True, f"lattice, SKIP_SHARED, {path}")
            assert np.array_equal(query(s, queries, 0, True, path, any_only=True)[2], (want[2] > 0).astype(np.int32))
        for q in range(3):                                   # the instance form: the lattice's sheets cross each other in place
            got = s.instance_intersections(q, max_triangles=64, skip_own=False)
            assert_answer(got, II.intersect_instance([pos], [0, 0, 0], maps, q, 64, skip_own=False), 64, True, f"lattice, instance {q}")
    finally:
        s.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["two scenes of different heights", "301 tiny instances"])
def test_sets_equal_the_restatement(pkg, gpu, which):
    names, maps, kinds = G.the_set(pkg, which)
    s = build(pkg, names, maps, which)
    distinct = sorted(set(names))
    positions, of = [member(pkg, d)[0] for d in distinct], [distinct.index(x) for x in names]
    queries = XC.world_queries(positions, of, maps, XC.NINE_QUERIES, seed=len(names) + 7)
    want64 = restate(positions, of, maps, queries)
    cnt, inst = want64[2], want64[1]
    print(which, np.bincount(np.minimum(cnt, 65)))
    assert (cnt == 0).mean() > 0.05 and (cnt > 0).mean() > 0.2 and (cnt > 8).mean() > 0.04, (which, np.bincount(np.minimum(cnt, 65)))
    assert len(set(inst[inst >= 0].tolist())) >= min(len(names), 12), "the held pairs come from many instances"
    check_every_form(s, queries, want64, None, which)
    for q in (0, len(names) - 1, len(names) // 2):
        want = II.intersect_instance(positions, of, maps, q, 64)
        for path in PATHS:
            assert_answer(own_query(s, q, 64, True, path), want, 64, True, f"{which}, instance {q}, {path}")
            assert_answer(own_query(s, q, 8, False, path), want, 8, False, f"{which}, instance {q}, pruned, {path}")


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_the_counters_of_the_nine_instance_set(pkg, gpu):
    """node_visits, leaf_visits, triangle_tests and traversals of the counting form, equal to the sum over the instances of
    instance_intersect_ref.walk_counters on the member's own tree, with the box the set's top level stores for the instance: a
    lane walks an instance exactly when no guarded axis separates that box from its query's vertex box."""
    names, positions, of, maps, s, queries, want64, want64_shared, _ = nine(pkg)
    queries = queries[:384]
    stored = stored_boxes(pkg, s, 9)
    world = loaded(pkg, "lobed_528")[0]
    desc = world.export_tree()
    lobed_tree = refit_ref.TreeArrays.of(desc)
    vd = np.ctypeslib.as_array(desc.vertex_data, shape=(desc.vertex_count * 9,)).reshape(-1, 9)
    lobed_corners = np.ascontiguousarray(vd[lobed_tree.triangle_vertices][:, :, :3])
    assert np.array_equal(lobed_corners.reshape(-1).view(np.uint32), positions[0].view(np.uint32)), "the scene's triangles are in the tree's order"
    i32 = lambda *v: np.array(v, np.int32)
    trees = {}
    for name, p in zip(("lobed_528", "one triangle", "11-triangle leaf"), positions):
        corners = p.reshape(-1, 3, 3)
        if name == "lobed_528":
            trees[name] = (lobed_tree, lobed_tree.box, corners)
        else:
            v = corners.reshape(-1, 3)
            box = np.concatenate([v.min(0) - 1e-5, v.max(0) + 1e-5]).astype(F)[None]        # helpers.single_leaf_scene's
            trees[name] = (refit_ref.TreeArrays(i32(-1), i32(-1), i32(-1), None, None, i32(0), i32(len(corners)), None), box, corners)
    walked = int(IR.walked(queries).sum())
    for skip_shared, want in ((False, want64), (True, want64_shared)):
        total = dict.fromkeys(COUNTERS, 0)
        members = np.zeros(len(queries), np.int64)
        for i, name in enumerate(names):
            tree, node_boxes, corners = trees[name]
            w = II.walk_counters(tree, node_boxes, corners, maps[i], queries, top_box=stored[i], skip_shared=skip_shared)
            assert (w["members"][w["traversals"] == 0] == 0).all(), "no pair is behind a culled instance"
            for c in COUNTERS:
                total[c] += int(w[c].sum())
            members += w["members"]
        assert np.array_equal(members * IR.walked(queries), want[2][:len(queries)]), "the counting walk finds every member"
        assert walked < total["traversals"] < 9 * walked, "the top level culls some instances and not all"
        for k, counts in ((8, True), (64, False), (0, True)):
            got = s.intersecting_triangles(queries, max_triangles=k, counts=counts, counters=True, skip_shared=skip_shared)
            assert_answer(got[:3], want, k, counts, f"nine instances, counting form, K = {k}")
            for c in COUNTERS:
                assert got[3][c] == total[c], (k, c, got[3], total)
            assert got[3]["samples"] == len(queries)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_refit_update_and_query_on_one_stream_and_after_a_host_update(pkg, gpu):
    """A device refit of a member, a device update with moved maps and both device forms, enqueued on one side stream with
    nothing between them; then a host update with other maps followed by the queries on all paths.  Each against the
    restatement of the state the query must see: the instance form's queries are the moved mesh under the new map."""
    import torch
    world, _, _ = loaded(pkg, "lobed_528")
    own = pkg.Scene(world.flatten())            # a scene of its own: it is refit below
    small_positions, small = member(pkg, "small_trisrc")
    before = np.asarray(own.geometry()["vertex_positions"], F).reshape(-1)
    names = ["lobed_528", "small_trisrc", "lobed_528", "lobed_528", "small_trisrc"]
    members = [own if x == "lobed_528" else small for x in names]
    of = [0 if x == "lobed_528" else 1 for x in names]
    kinds = ["rotation_nonuniform", "shear", "mirror", "translation", "rotation_uniform"]
    maps = [IC.make_set([before, small_positions], of, seed=70 + k, spread=0.8, kinds=kinds[k:] + kinds[:k])[1] for k in range(3)]
    s = pkg.tracer.InstanceSet(members, maps[0])
    K, Q = 8, 0
    try:
        moved = (before.reshape(-1, 3) * F(1.3) + F(0.2)).astype(F)
        now = [moved.reshape(-1), small_positions]
        queries = XC.world_queries(now, of, maps[1], XC.NINE_QUERIES, seed=71)
        first = query(s, queries, K, True, "host")
        first_own = own_query(s, Q, K, True, "host")
        triangles = s.triangle_count(Q)
        d_moved, d_maps, d_q = torch.from_numpy(moved).cuda(), torch.from_numpy(maps[1]).cuda(), dev_triangles(queries)
        new = lambda n, *shape: torch.full((n, *shape), -7, dtype=torch.int32, device="cuda")
        d_out, d_inst, d_cnt = new(len(queries), K), new(len(queries), K), new(len(queries))
        o_out, o_inst, o_cnt = new(triangles, K), new(triangles, K), new(triangles)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            own.refit(d_moved, stream_ptr=side.cuda_stream)
            s.update_into(d_maps.data_ptr(), side.cuda_stream)
            s.intersecting_triangles_into(d_q.data_ptr(), len(queries), d_out.data_ptr(), d_inst.data_ptr(), d_cnt.data_ptr(), K,
                                          stream_ptr=side.cuda_stream)
            s.instance_intersections_into(Q, 0, triangles, o_out.data_ptr(), o_inst.data_ptr(), o_cnt.data_ptr(), K,
                                          stream_ptr=side.cuda_stream)
        side.synchronize()
        assert s.update_status() == -1
        want = restate(now, of, maps[1], queries)
        assert (first[0] != want[0][:, :K]).any(1).sum() > 100, "the refit and the update moved something"
        assert_answer((d_out.cpu().numpy(), d_inst.cpu().numpy(), d_cnt.cpu().numpy()), want, K, True, "one stream")
        want_own = II.intersect_instance(now, of, maps[1], Q, 64)
        assert (first_own[2] != want_own[2]).sum() > 50 and (want_own[2] > 0).sum() > 20, "the instance form sees the moved mesh"
        assert_answer((o_out.cpu().numpy(), o_inst.cpu().numpy(), o_cnt.cpu().numpy()), want_own, K, True, "one stream, the instance form")
        # a host update: the device copy of the maps is behind it until the next query stages them on its stream
        s.update(maps[2])
        want2 = restate(now, of, maps[2], queries)
        assert (want2[0] != want[0]).any(1).sum() > 100, "the host update moved something"
        want2_own = II.intersect_instance(now, of, maps[2], Q, 64)
        for path in PATHS:
            assert_answer(query(s, queries, K, True, path), want2, K, True, f"after a host update, {path}")
            assert_answer(query(s, queries, 9, False, path), want2, 9, False, f"after a host update, K = 9, {path}")
            assert_answer(own_query(s, Q, K, True, path), want2_own, K, True, f"after a host update, the instance form, {path}")
            assert_answer(own_query(s, Q, 9, False, path), want2_own, 9, False, f"after a host update, the instance form, K = 9, {path}")
    finally:
        s.close()
        own.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_a_count_split_over_two_launches(pkg, gpu):
    """2^24 + 3000 queries (one launch holds 2^24) on the one-triangle scene placed twice, K = 2: a tile of 1,000 distinct
    queries repeated on the device, the answer compared there with the restatement's tile.  Slot query * K of the last queries
    lies beyond 2^25 indices: indexed in 64 bits.  The launch split, not a workload."""
    import torch
    positions, _ = member(pkg, "one triangle")
    names = ["one triangle", "one triangle"]
    _, maps, _ = IC.make_set([positions], [0, 0], seed=5, spread=0.3, kinds=["rotation_nonuniform", "mirror"])
    s = build(pkg, names, maps, "one triangle, twice")
    n, K, TILE = (1 << 24) + 3000, 2, 1000
    tile = XC.world_queries([positions], [0, 0], maps, TILE, seed=33)
    want = restate([positions], [0, 0], maps, tile, K)
    assert (want[2] == 2).sum() > 20 and (want[2] == 1).sum() > 20 and (want[2] == 0).sum() > 50, np.bincount(want[2])
    repeats = (n + TILE - 1) // TILE
    d = dev_triangles(tile).repeat(repeats, 1)[:n].contiguous()
    d_out = torch.empty((n, K), dtype=torch.int32, device="cuda")
    d_inst = torch.empty((n, K), dtype=torch.int32, device="cuda")
    d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    s.intersecting_triangles_into(d.data_ptr(), n, d_out.data_ptr(), d_inst.data_ptr(), d_cnt.data_ptr(), K,
                                  stream_ptr=torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    del d
    for got, w in ((d_out, want[0]), (d_inst, want[1]), (d_cnt, want[2])):
        w = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        whole = (n // TILE) * TILE
        assert bool((got[:whole].reshape(n // TILE, *w.shape) == w[None]).all()), "every whole tile"
        assert torch.equal(got[whole:], w[:n - whole]), "the last launch's tail"


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops(pkg, gpu):
    import torch
    s = build(pkg, ["lobed_528", "one triangle"], np.stack([EYE, EYE]), "refusals")
    tri, inst, cnt = s.intersecting_triangles(np.zeros((0, 9), F))
    assert tri.shape == (0, 8) and inst.shape == (0, 8) and len(cnt) == 0
    assert len(s.intersection_counts(np.zeros((0, 12), F))) == 0
    sheet = np.array([[-1e3, -1e3, 0.01, 1e3, -1e3, 0.013, 0, 1e3, 0.017]] * 4, F)
    n = II.intersect_over_instances([member(pkg, "lobed_528")[0], member(pkg, "one triangle")[0]], [0, 1], np.stack([EYE, EYE]), sheet, 0)[2]
    assert n[0] > 8 and np.array_equal(s.intersection_counts(sheet), n)
    assert torch.equal(s.intersection_counts(torch.from_numpy(sheet).cuda()).cpu(), torch.from_numpy(n))
    assert s.triangles_intersected(sheet).all()
    with pytest.raises(ValueError):
        s.intersecting_triangles(torch.zeros((4, 5), device="cuda"))
    with pytest.raises(ValueError):
        s.intersecting_triangles(torch.zeros((4, 9), device="cuda"), counters=True)
    with pytest.raises(ValueError):
        s.intersecting_triangles(sheet, max_triangles=0, counts=False)
    with pytest.raises(ValueError):
        s.instance_intersections(0, max_triangles=0, counts=False)
    with pytest.raises(ValueError):
        s.triangle_count(2)
    for k in (-1, 65):
        with pytest.raises(pkg._native.ShrayError) as err:
            s.intersecting_triangles(sheet, max_triangles=k)
        assert err.value.code == -1
    with pytest.raises(pkg._native.ShrayError):
        s.intersecting_triangles(sheet, max_triangles=8, any_only=True)
    # the instance form's own refusals: an instance outside the set, then a range beyond its scene's triangles
    error = lambda: pkg._native.load_hip().shray_last_error().decode()
    for instance in (-1, 2):
        with pytest.raises(pkg._native.ShrayError) as err:
            s.instance_intersections(instance)
        assert err.value.code == -1 and "is not among the set's 2" in str(err.value)
    for first, count in ((0, 529), (528, 1), (529, 0), (100, 1 << 40)):
        for device in (False, True):
            with pytest.raises(pkg._native.ShrayError) as err:
                s.instance_intersections(0, first=first, count=count, device=device)
            assert err.value.code == -1 and "are not all among the 528" in str(err.value)
    with pytest.raises(pkg._native.ShrayError) as err:
        s.instance_intersections(1, first=1, count=1)
    assert "are not all among the 1 of instance 1" in str(err.value)
    with pytest.raises(pkg._native.ShrayError) as err:
        s.instance_intersections(0, first=-1, count=1)
    assert "negative first triangle" in str(err.value)
    assert len(s.instance_intersections(0, first=528, count=0)[2]) == 0, "an empty range at the end is a no-op"
    lib = pkg._native.load_instance_intersect()
    d = torch.zeros((64, 12), dtype=torch.int32, device="cuda")
    call, own, V = lib.shray_intersect_triangles_instances_device, lib.shray_intersect_instance_device, C.c_void_p
    op = pkg.tracer._set_intersect_params(1)
    base = d.data_ptr()
    assert call(s._handle, C.byref(op), V(base + 4), 1, V(base + 48), None, None, None) == -1
    assert call(s._handle, C.byref(op), V(base), 1, V(base + 50), None, None, None) == -1
    assert call(s._handle, C.byref(op), V(base), 1, V(base + 48), V(base + 98), None, None) == -1
    assert call(s._handle, C.byref(op), V(base), 1, V(base + 48), None, V(base + 98), None) == -1
    assert call(s._handle, C.byref(op), V(base), 1, None, None, V(base + 100), None) == -1          # K = 1 without indices
    assert call(s._handle, C.byref(op), V(base), 1, V(base + 52), V(base + 100), V(base + 104), None) == 0
    assert call(s._handle, C.byref(op), V(base), 0, V(base + 48), None, None, None) == 0
    # the order: the instance before the count, the alignment before the range
    assert own(s._handle, C.byref(op), 7, 0, -1, V(base), None, None, None) == -1 and "is not among the set's 2" in error()
    assert own(s._handle, C.byref(op), 0, 0, -1, V(base), None, None, None) == -1 and "negative triangle count" in error()
    assert own(s._handle, C.byref(op), 0, 0, 600, V(base + 2), None, None, None) == -1 and "aligned" in error()
    assert own(s._handle, C.byref(op), 0, 0, 600, V(base), None, None, None) == -1 and "are not all among" in error()
    assert own(s._handle, C.byref(op), 0, 520, 8, V(base), V(base + 64), V(base + 128), None) == 0
    flagged = pkg.tracer._set_intersect_params(1, skip_own=True)
    assert call(s._handle, C.byref(flagged), V(base), 1, V(base + 48), None, None, None) == -1 and "flags 0x4" in error()
    torch.cuda.synchronize()
