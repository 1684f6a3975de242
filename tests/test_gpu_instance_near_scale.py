"""Instanced within-radius queries on the GPU at the cells of tests/instance_near_scale_cases.py (world, scene and cancelling
scales, far translations, ill-conditioned maps, negative zeros, the two cells where every dist2 is 0): every byte of every
record, every instance index and every count against the restatement, for K in {0, 1, 2, 4, 5, 7, 8, 9, 64} (the 4-slot
register instance full, the 8-slot one part-full) with and without counts on the three paths, with 1, 63, 64, 65 and all
points; the rim pairs (a radius exactly on a pair's dist2 and one step under it) count as the restatement does; where every
dist2 is 0, on the nine-instance set and on the small set whose first keys span five instances, nothing is culled and the
records are the first K keys in (instance, triangle) order; the top-level nodes and the four counters under a cancelling scale;
the negative zeros against the positive; a device update from the k = 0 maps to the k = 40 maps and a host update back.
tests/test_instance_near_scale_reference.py pins the cells on the CPU.

The members and sets are made as tests/test_gpu_instance_point_scale.py makes them (its module doc: a scene cell loads its
scenes at that scale, a cancel cell scales the unscaled scenes' own trees), and every restatement here is on the members' own
positions."""
import numpy as np
import pytest

import instance_near_ref as IN
import instance_near_scale_cases as NS
import near_ref as NR
import test_gpu_instance_point as G
import test_gpu_instance_point_scale as PS
from helpers import single_leaf_scene
from test_gpu_instance_near import COUNTERS, assert_answer, query, records
from test_gpu_instance_point import dev_points
from test_gpu_instance_point_scale import assert_no_stored_bound_above_a_dist2, loaded, members_of, normal_or_zero, read_nodes

pytestmark = pytest.mark.gpu

F = np.float32
KS = (0, 1, 2, 4, 5, 7, 8, 9, 64)
SMALL_COUNTS = (1, 63, 64, 65)
SMALL_FORMS = ((1, False), (4, False), (5, True), (8, True), (9, False), (64, True))
PATHS = ("host", "device", "no instance buffer")
_sets = []
_hand = {}
_memo = {}


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    _memo.clear()
    for s in _sets + PS._sets + G._sets:
        s.close()
    _sets.clear()
    PS._sets.clear()
    G._sets.clear()
    for sc in _hand.values():
        sc[1].close()
    _hand.clear()
    for _, scene, world in PS._scenes.values():
        scene.close()
        if world is not None:
            world.close()
    PS._scenes.clear()
    for _, sc in G._members.values():
        sc.close()
    G._members.clear()


def restate(members, of, maps, pts):
    """(records [n, 64], instances [n, 64], counts [n]) on the members' own positions, the pairs on the device"""
    return IN.near_over_instances([m[0] for m in members], of, maps, pts, 64, device="cuda")


def check_the_boxes(pkg, s, members, of, maps, pts, what):
    """the containment where every mapped corner is normal or 0, the cull's own property everywhere"""
    if normal_or_zero(members, of, maps):
        G.assert_contained(pkg, s, [members[k][0] for k in of], maps, what)
    assert_no_stored_bound_above_a_dist2(pkg, s, members, of, maps, pts, what)


def make_set(pkg, members, of, maps, pts, what):
    """an InstanceSet over the members, kept until the module ends, its stored boxes checked"""
    s = pkg.tracer.InstanceSet([members[k][1] for k in of], maps)
    _sets.append(s)
    check_the_boxes(pkg, s, members, of, maps, pts, what)
    return s


def check_every_form(s, pts, want64, what):
    """every K of KS with and without counts on the three paths at all the points; 1, 63, 64 and 65 points at SMALL_FORMS"""
    for k in KS:
        for counts in (True, False):
            if k == 0 and not counts:
                continue
            for path in PATHS:
                assert_answer(query(s, pts, k, counts, path), want64, k, counts, f"{what}, K = {k}, counts = {counts}, {path}")
    for count in SMALL_COUNTS:
        for k, counts in SMALL_FORMS:
            for path in PATHS:
                assert_answer(query(s, pts[:count], k, counts, path), want64, k, counts,
                              f"{what}, {count} points, K = {k}, counts = {counts}, {path}")


def cell_run(pkg, key):
    """(cell, members, set, the restatement at K = 64) of a cell, once per module"""
    if key not in _memo:
        c = NS.cell(pkg, key)
        members = members_of(pkg, c)
        s = make_set(pkg, members, c.of, c.maps, c.points, str(c))
        _memo[key] = (c, members, s, restate(members, c.of, c.maps, c.points))
    return _memo[key]


def assert_nothing_culled_and_the_first_keys(pkg, c, members, s, want64, what):
    """where every dist2 is 0: every walked point counts every triangle of the set, holds the first K keys in (instance,
    triangle) order with dist2 0, and the counting form walks every instance and tests every triangle"""
    total = sum(len(members[k][0]) // 9 for k in c.of)
    go = NS.walked(c.points)
    walked = int(go.sum())
    assert walked > 0.75 * len(go) and (want64[2][go] == total).all() and (want64[2][~go] == 0).all(), what
    inst64 = np.concatenate([np.full(len(members[k][0]) // 9, i, np.int32) for i, k in enumerate(c.of)])[:64]
    tri64 = np.concatenate([np.arange(len(members[k][0]) // 9, dtype=np.int32) for k in c.of])[:64]
    for k, counts in ((8, True), (0, True), (64, True)):
        rec, inst, cnt, tally = s.triangles_within(c.points, max_near=k, counts=counts, counters=True)
        assert_answer((rec, inst, cnt), want64, k, counts, f"{what}, counting form, K = {k}")
        assert (cnt[go] == total).all() and (cnt[~go] == 0).all(), what
        if k:
            assert (inst[go] == inst64[:k]).all() and (rec["triangle"][go] == tri64[:k]).all() and (rec["dist2"][go] == 0).all(), what
            assert (inst[~go] == -1).all() and (rec["triangle"][~go] == -1).all(), what
        assert tally["samples"] == len(go), tally
        assert tally["triangle_tests"] == walked * total, (what, k, tally, walked, total)
        assert tally["traversals"] == walked * len(c.of), (what, k, tally, walked)
    for k in (1, 8, 9):         # the pruning form: a reach of 0 from the K-th record on, and still nothing lost
        for path in PATHS:
            rec, inst, _ = query(s, c.points, k, False, path)
            assert (rec["triangle"][go] == tri64[:k]).all() and (rec["dist2"][go] == 0).all(), (what, k, path)
            assert inst is None or (inst[go] == inst64[:k]).all(), (what, k, path)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", NS.CELLS, ids=lambda k: f"{k[0]} {k[1]}")
def test_a_cell_equals_the_restatement(pkg, gpu, key):
    c, members, s, want64 = cell_run(pkg, key)
    part = IN.near_over_instances([m[0] for m in members], c.of, c.maps, c.points[:96], 64)
    assert_answer(part, want64, 64, True, f"{c}: the torch restatement against numpy")
    check_every_form(s, c.points, want64, str(c))
    go = NS.walked(c.points)
    for k in (8, 0):
        got = s.triangles_within(c.points, max_near=k, counts=True, counters=True)
        assert_answer(got[:3], want64, k, True, f"{c}, counting form, K = {k}")
        assert got[3]["samples"] == len(go) and 0 < got[3]["traversals"] <= int(go.sum()) * len(c.of), (c, k, got[3])
    # the rim pairs: the radius on a pair's dist2 and one step under it, on the same point
    first, second, j = c.rim.T
    w_at, w_under = NS.rim_counts(c, want64[2])
    assert (w_at >= j).all() and (w_under < j).all() and (w_under <= w_at).all(), f"{c}: the restatement at the rim"
    for path in PATHS:
        for k in (0, 4, 64):
            cnt = query(s, c.points, k, True, path)[2]
            g_at, g_under = NS.rim_counts(c, cnt)
            for name, g, w in (("on", g_at, w_at), ("one step under", g_under, w_under)):
                bad = np.nonzero(g != w)[0]
                assert len(bad) == 0, (f"{c}, {path}, K = {k}: the inclusive bound against max_dist2: {len(bad)} rim points with max_dist2 {name} "
                                       f"the dist2 of their j-th nearest pair count otherwise: first pair (points {first[bad[0]]}, {second[bad[0]]}, "
                                       f"j = {j[bad[0]]}) counts {g[bad[0]]}, the restatement {w[bad[0]]}")
            split = np.nonzero((w_at != w_under) & (g_at == g_under))[0]
            assert len(split) == 0, (f"{c}, {path}, K = {k}: the inclusive bound against max_dist2: pair (points {first[split[:1]]}, "
                                     f"{second[split[:1]]}) counts the same on the dist2 and one step under it")
    if key in NS.ALL_ZERO:
        assert_nothing_culled_and_the_first_keys(pkg, c, members, s, want64, str(c))
    twin = NS.expected_cell(key)
    if twin and key[0] == "negzero":
        t_want64 = cell_run(pkg, twin)[3]
        for k, counts in ((64, True), (7, False)):
            assert_answer(query(s, c.points, k, counts, "device"), t_want64, k, counts, f"{c} against {twin}")


# 2 ---------------------------------------------------------------------------------------------------------------------------
def small_members(pkg, c):
    """[(positions, scene)] of the small set's three distinct members at the cell's scale: the two tiny ones as single leaves
    over their scaled positions, lobed_528 loaded at that scale"""
    out = []
    for name, positions in zip(("one triangle", "11-triangle leaf"), c.positions(pkg)):
        if (name, c.scene_exp) not in _hand:
            _hand[(name, c.scene_exp)] = (positions, pkg.Scene(single_leaf_scene(positions.reshape(-1, 3, 3)).desc))
        out.append(_hand[(name, c.scene_exp)])
    return out + [loaded(pkg, "lobed_528", c.scene_exp)]


@pytest.mark.parametrize("key", NS.ALL_ZERO, ids=lambda k: f"{k[0]} {k[1]}")
def test_the_small_set_where_every_dist2_is_zero(pkg, gpu, key):
    """one triangle, 11-triangle leaf, one triangle, 11-triangle leaf, lobed_528: the first 64 keys span five instances and the
    first 8 span two, so the held keys are carried from instance to instance with a reach of 0"""
    c = NS.small_cell(pkg, key)
    members = small_members(pkg, c)
    s = make_set(pkg, members, c.of, c.maps, c.points, str(c))
    want64 = restate(members, c.of, c.maps, c.points)
    go = NS.walked(c.points)
    assert (want64[1][go][:, :8] == [0, 1, 1, 1, 1, 1, 1, 1]).all() and set(want64[1][go][0].tolist()) == {0, 1, 2, 3, 4}
    check_every_form(s, c.points, want64, str(c))
    assert_nothing_culled_and_the_first_keys(pkg, c, members, s, want64, str(c))


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", NS.SC.CANCEL_EXPONENTS)
def test_a_cancelling_scale_keeps_every_bit(pkg, gpu, a):
    """The scenes at 2^a under linear parts x 2^-a, against the a = 0 set made the same way: the records, the instance indices,
    the counts, the top-level nodes as read back and the counting form's four counters are equal, bit for bit."""
    c, members, s, want64 = cell_run(pkg, ("cancel", a))
    if ("cancel", 0) not in _memo:
        c0 = NS.cell(pkg, ("world", 0))
        members0 = members_of(pkg, c0, trees=True)
        s0 = make_set(pkg, members0, c0.of, c0.maps, c0.points, "the a = 0 twin")
        _memo[("cancel", 0)] = (c0, members0, s0, restate(members0, c0.of, c0.maps, c0.points))
    c0, members0, s0, want0 = _memo[("cancel", 0)]
    assert_answer(want64, want0, 64, True, f"{c}: the restatement against a = 0's")
    nodes, nodes0 = read_nodes(pkg, s), read_nodes(pkg, s0)
    assert np.array_equal(nodes, nodes0), f"{c}: {(nodes != nodes0).any(1).sum()} of {len(nodes)} top-level nodes differ from a = 0's"
    for k, counts in ((8, True), (0, True), (64, False)):
        got = s.triangles_within(c.points, max_near=k, counts=counts, counters=True)
        got0 = s0.triangles_within(c0.points, max_near=k, counts=counts, counters=True)
        assert_answer(got[:3], got0[:3], k, counts, f"{c} against the a = 0 set, K = {k}")
        assert_answer(got[:3], want0, k, counts, f"{c} against a = 0's restatement, K = {k}")
        for name in COUNTERS:
            assert got[3][name] == got0[3][name] > 0, (c, k, name, got[3], got0[3])


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_a_device_update_across_magnitudes_and_a_host_update_back(pkg, gpu):
    """One set goes from the k = 0 maps to the k = 40 maps by update_into on a side stream with triangles_within_into behind it
    on that stream (K = 9, no instance buffer, no counts: the pruning form through the scratch), and back by the host update, then queried on the three paths: each state
    against its restatement, the boxes checked after each."""
    import torch
    c0, c40 = NS.cell(pkg, ("world", 0)), NS.cell(pkg, ("world", 40))
    members = members_of(pkg, c0)
    s = make_set(pkg, members, c0.of, c0.maps, c0.points, "before the updates")
    n, K = len(c40.points), 9
    d_maps, d_pts = torch.from_numpy(c40.maps).cuda(), dev_points(c40.points)
    d_out = torch.full((n, K, 8), -7, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.update_into(d_maps.data_ptr(), side.cuda_stream)
        s.triangles_within_into(d_pts.data_ptr(), n, d_out.data_ptr(), 0, 0, K, side.cuda_stream)
    side.synchronize()
    assert s.update_status() == -1
    want40 = restate(members, c40.of, c40.maps, c40.points)
    assert_answer((records(d_out, K), None, None), want40, K, False, "after the device update to 2^40")
    check_the_boxes(pkg, s, members, c40.of, c40.maps, c40.points, "after the device update to 2^40")
    s.update(c0.maps)
    want0 = restate(members, c0.of, c0.maps, c0.points)
    assert (NR.as_bits(want0[0]) != NR.as_bits(want40[0])).any(1).sum() > 500
    check_every_form(s, c0.points, want0, "after the host update back to 2^0")
    check_the_boxes(pkg, s, members, c0.of, c0.maps, c0.points, "after the host update back to 2^0")
