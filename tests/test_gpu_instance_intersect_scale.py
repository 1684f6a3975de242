"""Instanced triangle-intersection queries on the GPU at the cells of tests/instance_intersect_scale_cases.py (world, scene and
cancelling scales, far translations, ill-conditioned maps, negative zeros, the cells where every world coordinate underflows
and no query is walked, the NaN-corner cell): every triangle index, every instance index and every count against the
brute-force restatement on the members' own positions, for K in {0, 1, 2, 4, 5, 7, 8, 9, 64} with and without counts and for
SHRAY_INTERSECT_ANY on the three paths (host, device, device without an instance buffer: the scratch path at K = 9 and 64),
five of those forms and ANY again with SHRAY_INTERSECT_SKIP_SHARED, with 1, 63, 64, 65 and all queries; the top-level nodes
and the four counters under a
cancelling scale; the negative zeros against the positive; the four counters against the sum of
instance_intersect_ref.walk_counters with the stored boxes as read back on an ill and a far cell; the instance form of
instances 1, 3 and 8 with and without SHRAY_INTERSECT_SKIP_OWN_INSTANCE over sub-ranges that hold the last triangle, on two
world cells, a far cell and an ill cell; the draws at 2^-147; a device update from the k = 0 maps to the k = 40 maps and a host
update back.  tests/test_instance_intersect_scale_reference.py pins the cells on the CPU.

The members and sets are made as tests/test_gpu_instance_point_scale.py makes them (its module doc), and every restatement here
is on the members' own positions."""
import numpy as np
import pytest

import instance_intersect_ref as II
import instance_intersect_scale_cases as TS
import intersect_ref as IR
import test_gpu_instance_point as G
import test_gpu_instance_point_scale as PS
from test_gpu_instance_intersect import COUNTERS, assert_answer, dev_triangles, own_query, query
from test_gpu_instance_overlap import stored_boxes
from test_gpu_instance_overlap_scale import member_trees, one_corner_scene
from test_gpu_instance_point_scale import members_of, normal_or_zero, read_nodes
import test_gpu_instance_overlap_scale as XG

pytestmark = pytest.mark.gpu

F = np.float32
KS = (0, 1, 2, 4, 5, 7, 8, 9, 64)
SMALL_COUNTS = (1, 63, 64, 65)
SMALL_FORMS = ((1, False), (4, False), (5, True), (8, True), (9, False), (64, True))
PATHS = ("host", "device", "no instance buffer")
SHARED_FORMS = ((0, True), (1, False), (8, True), (9, False), (64, True))      # the forms that also run with SKIP_SHARED
COUNTER_QUERIES = 256
FORM_RANGE = 160
_sets = []
_memo = {}


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    _memo.clear()
    for s in _sets + XG._sets + PS._sets + G._sets:
        s.close()
    _sets.clear()
    XG._sets.clear()
    PS._sets.clear()
    G._sets.clear()
    for sc in XG._hand:
        sc.close()
    XG._hand.clear()
    for _, scene, world in PS._scenes.values():
        scene.close()
        if world is not None:
            world.close()
    PS._scenes.clear()
    for _, sc in G._members.values():
        sc.close()
    G._members.clear()


def restate(members, of, maps, queries, skip_shared=False):
    """(triangles [n, 64], instances [n, 64], counts [n]) on the members' own positions"""
    return II.intersect_over_instances([m[0] for m in members], of, maps, queries, 64, skip_shared)


def make_set(pkg, members, of, maps, what):
    """an InstanceSet over the members, kept until the module ends; the containment where every mapped corner is normal or 0"""
    s = pkg.tracer.InstanceSet([members[k][1] for k in of], maps)
    _sets.append(s)
    if normal_or_zero(members, of, maps):
        G.assert_contained(pkg, s, [members[k][0] for k in of], maps, what)
    return s


def check_every_form(s, queries, want64, want64_shared, what):
    """every K of KS with and without counts and the ANY form on the three paths at all the queries; SHARED_FORMS and the ANY
    form again with SKIP_SHARED; 1, 63, 64 and 65 queries at SMALL_FORMS"""
    for skip_shared, want in ((False, want64), (True, want64_shared)):
        met = (want[2] > 0).astype(np.int32)
        for k in KS:
            for counts in (True, False):
                if (k == 0 and not counts) or (skip_shared and (k, counts) not in SHARED_FORMS):
                    continue
                for path in PATHS:
                    assert_answer(query(s, queries, k, counts, path, skip_shared=skip_shared), want, k, counts,
                                  f"{what}, K = {k}, counts = {counts}, SKIP_SHARED = {skip_shared}, {path}")
        for path in PATHS:
            got = query(s, queries, 0, True, path, any_only=True, skip_shared=skip_shared)
            assert got[0] is None and got[1] is None and np.array_equal(got[2], met), f"{what}, ANY, SKIP_SHARED = {skip_shared}, {path}"
    for count in SMALL_COUNTS:
        for k, counts in SMALL_FORMS:
            for path in PATHS:
                assert_answer(query(s, queries[:count], k, counts, path), want64, k, counts,
                              f"{what}, {count} queries, K = {k}, counts = {counts}, {path}")


def cell_run(pkg, key):
    """(cell, members, set, the restatement at K = 64 without and with SKIP_SHARED) of a cell, once per module"""
    if key not in _memo:
        c = TS.cell(pkg, key)
        members = members_of(pkg, c)
        s = make_set(pkg, members, c.of, c.maps, str(c))
        _memo[key] = (c, members, s) + TS.restate_both([m[0] for m in members], c.of, c.maps, c.queries)
    return _memo[key]


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", TS.CELLS, ids=lambda k: f"{k[0]} {k[1]}")
def test_a_cell_equals_the_restatement(pkg, gpu, key):
    c, members, s, want64, shared64 = cell_run(pkg, key)
    check_every_form(s, c.queries, want64, shared64, str(c))
    go = IR.walked(c.queries)
    for k in (8, 0):
        got = s.intersecting_triangles(c.queries, max_triangles=k, counts=True, counters=True)
        assert_answer(got[:3], want64, k, True, f"{c}, counting form, K = {k}")
        assert got[3]["samples"] == len(go) and got[3]["traversals"] <= int(go.sum()) * len(c.of), (c, k, got[3])
        assert (got[3]["traversals"] > 0) == bool(go.any()), (c, k, got[3])
    if key in TS.ALL_ZERO or key[0] == "guard":
        assert not go.any() and (want64[2] == 0).all(), f"{c}: every normal underflows: no query is walked"
    if key == TS.NAN_CELL:
        for path in PATHS:
            tri8, inst8, n8 = query(s, c.queries, 8, True, path)
            tri64, inst64, n64 = query(s, c.queries, 64, True, path)
            assert np.array_equal(tri8, tri64[:, :8]) and np.array_equal(n8, n64), (c, path)
            assert inst8 is None or np.array_equal(inst8, inst64[:, :8]), (c, path)
    twin = TS.expected_cell(key)
    if twin and key[0] == "negzero":
        t_want64 = cell_run(pkg, twin)[3]
        for k, counts in ((64, True), (7, False)):
            assert_answer(query(s, c.queries, k, counts, "device"), t_want64, k, counts, f"{c} against {twin}")


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", TS.SC.CANCEL_EXPONENTS)
def test_a_cancelling_scale_keeps_every_bit(pkg, gpu, a):
    """The scenes at 2^a under linear parts x 2^-a, against the a = 0 set made the same way: the indices, the instance indices,
    the counts, the top-level nodes as read back and the counting form's four counters are equal, bit for bit."""
    c, members, s, want64, _ = cell_run(pkg, ("cancel", a))
    if ("cancel", 0) not in _memo:
        c0 = TS.cell(pkg, ("world", 0))
        members0 = members_of(pkg, c0, trees=True)
        s0 = make_set(pkg, members0, c0.of, c0.maps, "the a = 0 twin")
        _memo[("cancel", 0)] = (c0, members0, s0, restate(members0, c0.of, c0.maps, c0.queries))
    c0, members0, s0, want0 = _memo[("cancel", 0)]
    assert_answer(want64, want0, 64, True, f"{c}: the restatement against a = 0's")
    nodes, nodes0 = read_nodes(pkg, s), read_nodes(pkg, s0)
    assert np.array_equal(nodes, nodes0), f"{c}: {(nodes != nodes0).any(1).sum()} of {len(nodes)} top-level nodes differ from a = 0's"
    for k, counts, any_only in ((8, True, False), (0, True, False), (64, False, False), (0, True, True)):
        got = s.intersecting_triangles(c.queries, max_triangles=k, counts=counts, counters=True, any_only=any_only)
        got0 = s0.intersecting_triangles(c0.queries, max_triangles=k, counts=counts, counters=True, any_only=any_only)
        if any_only:
            assert np.array_equal(got[2], got0[2]) and np.array_equal(got[2], (want0[2] > 0).astype(np.int32)), (c, "ANY")
        else:
            assert_answer(got[:3], got0[:3], k, counts, f"{c} against the a = 0 set, K = {k}")
            assert_answer(got[:3], want0, k, counts, f"{c} against a = 0's restatement, K = {k}")
        for name in COUNTERS:
            assert got[3][name] == got0[3][name] > 0, (c, k, any_only, name, got[3], got0[3])


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("ill", 12), ("far", 20)], ids=lambda k: f"{k[0]} {k[1]}")
def test_the_counters_are_the_restated_walk_s(pkg, gpu, key):
    """node_visits, leaf_visits, triangle_tests and traversals of the counting form, equal to the sum over the instances of
    instance_intersect_ref.walk_counters on the member's own tree with the box the set's top level stores for the instance as
    read back."""
    c, members, s, want64, _ = cell_run(pkg, key)
    queries = c.queries[:COUNTER_QUERIES]
    stored = stored_boxes(pkg, s, len(c.of))
    trees = member_trees(pkg, c)
    total = dict.fromkeys(COUNTERS, 0)
    found = np.zeros(len(queries), np.int64)
    for i, k in enumerate(c.of):
        tree, node_boxes, corners = trees[k]
        w = II.walk_counters(tree, node_boxes, corners, c.maps[i], queries, top_box=stored[i])
        assert (w["members"][w["traversals"] == 0] == 0).all(), f"{c}: a pair is behind a culled instance"
        for name in COUNTERS:
            total[name] += int(w[name].sum())
        found += w["members"]
    assert np.array_equal(found * IR.walked(queries), want64[2][:len(queries)]), "the counting walk finds every member"
    for k, counts in ((8, True), (0, True)):
        got = s.intersecting_triangles(queries, max_triangles=k, counts=counts, counters=True)
        assert_answer(got[:3], want64, k, counts, f"{c}, counting form, K = {k}")
        for name in COUNTERS:
            assert got[3][name] == total[name], (c, k, name, got[3], total)
        assert got[3]["samples"] == len(queries)


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", TS.FORM_CELLS, ids=lambda k: f"{k[0]} {k[1]}")
def test_the_instance_form(pkg, gpu, key):
    """Instances 1 (whose duplicate is 4), 3 (a general map) and 8 (the shear), the last FORM_RANGE triangles and the last
    triangle alone, with and without SHRAY_INTERSECT_SKIP_OWN_INSTANCE: the query is instance q's own world corners, bit for
    bit, also where they collapse on the float grid."""
    c, members, s, *_ = cell_run(pkg, key)
    positions = [m[0] for m in members]
    for q in TS.FORM_INSTANCES:
        triangles = s.triangle_count(q)
        assert triangles == len(positions[c.of[q]]) // 9
        first = triangles - FORM_RANGE
        member, starts = II.own_membership(positions, c.of, c.maps, q, skip_own=False, first_triangle=first, count=FORM_RANGE)
        for skip_own in (False, True):
            if skip_own:
                member = member.copy()
                member[:, starts[q]:starts[q + 1]] = False
            want = II.from_membership(member, starts, 64)
            assert skip_own or key != ("world", 0) or (want[2] >= 1).all(), "a triangle meets itself"
            for path in PATHS:
                for k, counts in ((64, True), (8, False), (9, False), (0, True)):
                    assert_answer(own_query(s, q, k, counts, path, skip_own=skip_own, first=first, count=FORM_RANGE), want, k, counts,
                                  f"{c}, instance {q}, SKIP_OWN_INSTANCE = {skip_own}, K = {k}, counts = {counts}, {path}")
                last = tuple(w[FORM_RANGE - 1:] for w in want)
                assert_answer(own_query(s, q, 8, True, path, skip_own=skip_own, first=triangles - 1, count=1), last, 8, True,
                              f"{c}, instance {q}, the last triangle, {path}")
                got = own_query(s, q, 0, True, path, any_only=True, skip_own=skip_own, first=first, count=FORM_RANGE)
                assert np.array_equal(got[2], (want[2] > 0).astype(np.int32)), f"{c}, instance {q}, ANY, {path}"


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_the_draws_are_not_walked(pkg, gpu):
    """("draws", -147): query i is the triangle whose three corners are draw i's fp32 world corner.  Its normal is (0, 0, 0), so
    the header does not walk it, and every triangle of the set is degenerate: n = 0 and -1 everywhere, on every path.  (The
    guard cannot show in this query on a world this small; tests/test_gpu_instance_overlap_scale.py shows it in the box query,
    which compiles the same stored_overlaps.)"""
    c = TS.draws_cell(pkg)
    positions = c.positions(pkg)
    members = [(positions[i], one_corner_scene(pkg, positions[i][:3])) for i in range(len(positions))]
    s = pkg.tracer.InstanceSet([m[1] for m in members], c.maps)
    _sets.append(s)
    want64 = restate(members, c.of, c.maps, c.queries)
    assert (want64[2] == 0).all() and not IR.walked(c.queries).any()
    check_every_form(s, c.queries, want64, want64, str(c))


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_a_device_update_across_magnitudes_and_a_host_update_back(pkg, gpu):
    """One set goes from the k = 0 maps to the k = 40 maps by update_into on a side stream with intersecting_triangles_into
    behind it on that stream (K = 9, no instance buffer, no counts: the pruning form through the scratch), and back by the host
    update, then queried on the three paths: each state against its restatement."""
    import torch
    c0, c40 = TS.cell(pkg, ("world", 0)), TS.cell(pkg, ("world", 40))
    members = members_of(pkg, c0)
    s = make_set(pkg, members, c0.of, c0.maps, "before the updates")
    n, K = len(c40.queries), 9
    d_maps, d_q = torch.from_numpy(c40.maps).cuda(), dev_triangles(c40.queries)
    d_out = torch.full((n, K), -7, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.update_into(d_maps.data_ptr(), side.cuda_stream)
        s.intersecting_triangles_into(d_q.data_ptr(), n, d_out.data_ptr(), 0, 0, K, False, False, side.cuda_stream)
    side.synchronize()
    assert s.update_status() == -1
    want40 = restate(members, c40.of, c40.maps, c40.queries)
    assert_answer((d_out.cpu().numpy(), None, None), want40, K, False, "after the device update to 2^40")
    G.assert_contained(pkg, s, [members[k][0] for k in c40.of], c40.maps, "after the device update to 2^40")
    s.update(c0.maps)
    want0 = restate(members, c0.of, c0.maps, c0.queries)
    assert (want0[0] != want40[0]).any(1).sum() > 100, "the two states answer differently"
    check_every_form(s, c0.queries, want0, restate(members, c0.of, c0.maps, c0.queries, True), "after the host update back to 2^0")
    G.assert_contained(pkg, s, [members[k][0] for k in c0.of], c0.maps, "after the host update back to 2^0")
