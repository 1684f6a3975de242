"""Instanced box-overlap queries on the GPU at the cells of tests/instance_overlap_scale_cases.py (world, scene and cancelling
scales, far translations, ill-conditioned maps, negative zeros, the two cells where every world coordinate underflows, the world
at 2^100, the worlds about the top level's guard 2^-109, the NaN-corner cell): every triangle index, every instance index and
every count against the brute-force restatement on the members' own positions, for K in {0, 1, 2, 4, 5, 7, 8, 9, 64} with and
without counts and for SHRAY_OVERLAP_ANY on the three paths (host, device, device without an instance buffer: the scratch path at
K = 9 and 64), with 1, 63, 64, 65 and all boxes; the top-level nodes and the four counters under a cancelling scale; the negative
zeros against the positive; the four counters against the sum of instance_overlap_ref.walk_counters with the stored boxes as read
back, on the guard cells (which pins the threshold from both sides), an ill cell and a far cell; the draws at 2^-147 whose fp32
corner lies outside its stored box; the prefix rule at the NaN-corner cell; a device update from the k = 0 maps to the k = 40
maps and a host update back.  tests/test_instance_overlap_scale_reference.py pins the cells on the CPU.

The members and sets are made as tests/test_gpu_instance_point_scale.py makes them (its module doc), and every restatement here
is on the members' own positions."""
import numpy as np
import pytest

import instance_overlap_ref as IO
import instance_overlap_scale_cases as XS
import overlap_ref as OR
import refit_ref
import test_gpu_instance_point as G
import test_gpu_instance_point_scale as PS
from helpers import END, HandScene
from test_gpu_instance_overlap import COUNTERS, assert_answer, dev_boxes, query, stored_boxes
from test_gpu_instance_point_scale import loaded, members_of, normal_or_zero, read_nodes

pytestmark = pytest.mark.gpu

F = np.float32
KS = (0, 1, 2, 4, 5, 7, 8, 9, 64)
SMALL_COUNTS = (1, 63, 64, 65)
SMALL_FORMS = ((1, False), (4, False), (5, True), (8, True), (9, False), (64, True))
PATHS = ("host", "device", "no instance buffer")
COUNTER_BOXES = 384
_sets = []
_hand = []
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
    for sc in _hand:
        sc.close()
    _hand.clear()
    for _, scene, world in PS._scenes.values():
        scene.close()
        if world is not None:
            world.close()
    PS._scenes.clear()
    for _, sc in G._members.values():
        sc.close()
    G._members.clear()


def restate(members, of, maps, boxes):
    """(triangles [n, 64], instances [n, 64], counts [n]) on the members' own positions"""
    return IO.overlap_over_instances([m[0] for m in members], of, maps, boxes, 64)


def make_set(pkg, members, of, maps, what):
    """an InstanceSet over the members, kept until the module ends; the containment where every mapped corner is normal or 0"""
    s = pkg.tracer.InstanceSet([members[k][1] for k in of], maps)
    _sets.append(s)
    if normal_or_zero(members, of, maps):
        G.assert_contained(pkg, s, [members[k][0] for k in of], maps, what)
    return s


def check_every_form(s, boxes, want64, what):
    """every K of KS with and without counts and the ANY form on the three paths at all the boxes; 1, 63, 64 and 65 boxes at
    SMALL_FORMS"""
    touched = (want64[2] > 0).astype(np.int32)
    for k in KS:
        for counts in (True, False):
            if k == 0 and not counts:
                continue
            for path in PATHS:
                assert_answer(query(s, boxes, k, counts, path), want64, k, counts, f"{what}, K = {k}, counts = {counts}, {path}")
    for path in PATHS:
        got = query(s, boxes, 0, True, path, any_only=True)
        assert got[0] is None and got[1] is None and np.array_equal(got[2], touched), f"{what}, ANY, {path}"
    for count in SMALL_COUNTS:
        for k, counts in SMALL_FORMS:
            for path in PATHS:
                assert_answer(query(s, boxes[:count], k, counts, path), want64, k, counts,
                              f"{what}, {count} boxes, K = {k}, counts = {counts}, {path}")


def cell_run(pkg, key):
    """(cell, members, set, the restatement at K = 64) of a cell, once per module"""
    if key not in _memo:
        c = XS.cell(pkg, key)
        members = members_of(pkg, c)
        s = make_set(pkg, members, c.of, c.maps, str(c))
        _memo[key] = (c, members, s, restate(members, c.of, c.maps, c.boxes))
    return _memo[key]


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", XS.CELLS, ids=lambda k: f"{k[0]} {k[1]}")
def test_a_cell_equals_the_restatement(pkg, gpu, key):
    c, members, s, want64 = cell_run(pkg, key)
    check_every_form(s, c.boxes, want64, str(c))
    go = OR.walked(c.boxes)
    for k in (8, 0):
        got = s.triangles_in_boxes(c.boxes, max_triangles=k, counts=True, counters=True)
        assert_answer(got[:3], want64, k, True, f"{c}, counting form, K = {k}")
        assert got[3]["samples"] == len(go) and 0 < got[3]["traversals"] <= int(go.sum()) * len(c.of), (c, k, got[3])
    if key in XS.ALL_ZERO:
        assert (want64[2] > 64).mean() > 0.25, f"{c}: the underflowed world still answers richly"
    if key == XS.NAN_CELL:
        # the prefix rule where corners are NaN: K = 8 holds the first 8 of K = 64, n is the same, ANY is n > 0
        for path in PATHS:
            tri8, inst8, n8 = query(s, c.boxes, 8, True, path)
            tri64, inst64, n64 = query(s, c.boxes, 64, True, path)
            assert np.array_equal(tri8, tri64[:, :8]) and np.array_equal(n8, n64), (c, path)
            assert inst8 is None or np.array_equal(inst8, inst64[:, :8]), (c, path)
            assert np.array_equal(query(s, c.boxes, 0, True, path, any_only=True)[2], (n64 > 0).astype(np.int32)), (c, path)
        assert (want64[2][go] > 0).all(), f"{c}: every walked box holds a pair"
    twin = XS.expected_cell(key)
    if twin and key[0] == "negzero":
        t_want64 = cell_run(pkg, twin)[3]
        for k, counts in ((64, True), (7, False)):
            assert_answer(query(s, c.boxes, k, counts, "device"), t_want64, k, counts, f"{c} against {twin}")


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", XS.SC.CANCEL_EXPONENTS)
def test_a_cancelling_scale_keeps_every_bit(pkg, gpu, a):
    """The scenes at 2^a under linear parts x 2^-a, against the a = 0 set made the same way: the indices, the instance indices,
    the counts, the top-level nodes as read back and the counting form's four counters are equal, bit for bit."""
    c, members, s, want64 = cell_run(pkg, ("cancel", a))
    if ("cancel", 0) not in _memo:
        c0 = XS.cell(pkg, ("world", 0))
        members0 = members_of(pkg, c0, trees=True)
        s0 = make_set(pkg, members0, c0.of, c0.maps, "the a = 0 twin")
        _memo[("cancel", 0)] = (c0, members0, s0, restate(members0, c0.of, c0.maps, c0.boxes))
    c0, members0, s0, want0 = _memo[("cancel", 0)]
    assert_answer(want64, want0, 64, True, f"{c}: the restatement against a = 0's")
    nodes, nodes0 = read_nodes(pkg, s), read_nodes(pkg, s0)
    assert np.array_equal(nodes, nodes0), f"{c}: {(nodes != nodes0).any(1).sum()} of {len(nodes)} top-level nodes differ from a = 0's"
    for k, counts, any_only in ((8, True, False), (0, True, False), (64, False, False), (0, True, True)):
        got = s.triangles_in_boxes(c.boxes, max_triangles=k, counts=counts, counters=True, any_only=any_only)
        got0 = s0.triangles_in_boxes(c0.boxes, max_triangles=k, counts=counts, counters=True, any_only=any_only)
        if any_only:
            assert np.array_equal(got[2], got0[2]) and np.array_equal(got[2], (want0[2] > 0).astype(np.int32)), (c, "ANY")
        else:
            assert_answer(got[:3], got0[:3], k, counts, f"{c} against the a = 0 set, K = {k}")
            assert_answer(got[:3], want0, k, counts, f"{c} against a = 0's restatement, K = {k}")
        for name in COUNTERS:
            assert got[3][name] == got0[3][name] > 0, (c, k, any_only, name, got[3], got0[3])


# 3 ---------------------------------------------------------------------------------------------------------------------------
def member_trees(pkg, c):
    """(refit_ref.TreeArrays, node boxes, object corners in the tree's order) of the cell's two member scenes as loaded"""
    out = []
    for name in XS.SCENES:
        positions, _ = loaded(pkg, name, c.scene_exp)
        world = PS._scenes[(name, c.scene_exp, "loaded")][2]
        desc = world.export_tree()
        tree = refit_ref.TreeArrays.of(desc)
        vd = np.ctypeslib.as_array(desc.vertex_data, shape=(desc.vertex_count * 9,)).reshape(-1, 9)
        corners = np.ascontiguousarray(vd[tree.triangle_vertices][:, :, :3])
        assert np.array_equal(corners.reshape(-1).view(np.uint32), positions.view(np.uint32)), "the scene's triangles are in the tree's order"
        out.append((tree, tree.box, corners))
    return out


@pytest.mark.parametrize("key", XS.GUARD_CELLS + [("ill", 12), ("far", 20)], ids=lambda k: f"{k[0]} {k[1]}")
def test_the_counters_are_the_restated_walk_s(pkg, gpu, key):
    """node_visits, leaf_visits, triangle_tests and traversals of the counting form, equal to the sum over the instances of
    instance_overlap_ref.walk_counters on the member's own tree with the box the set's top level stores for the instance as
    read back: a lane walks an instance exactly when no axis separates that box from its query box with the stored end and
    the query end not both under 2^-109.  On the guard cells the stored ends lie on both sides of that threshold."""
    c, members, s, want64 = cell_run(pkg, key)
    boxes = c.boxes if key[0] == "guard" else c.boxes[:COUNTER_BOXES]
    stored = stored_boxes(pkg, s, len(c.of))
    if key[0] == "guard":
        # (at 2^-112 every stored end is under the guard and the far boxes' ends alone are over it)
        go = OR.walked(boxes)
        ends = np.abs(np.concatenate([np.concatenate(b) for b in stored.values()] + [boxes["lo"][go].ravel(), boxes["hi"][go].ravel()]))
        assert (ends < IO.GUARD).any() and (ends >= IO.GUARD).any(), f"{c}: stored and query ends on both sides of the guard"
    trees = member_trees(pkg, c)
    total = dict.fromkeys(COUNTERS, 0)
    touching = np.zeros(len(boxes), np.int64)
    for i, k in enumerate(c.of):
        tree, node_boxes, corners = trees[k]
        w = IO.walk_counters(tree, node_boxes, corners, c.maps[i], boxes, top_box=stored[i])
        assert (w["touching"][w["traversals"] == 0] == 0).all(), f"{c}: a pair is behind a culled instance"
        for name in COUNTERS:
            total[name] += int(w[name].sum())
        touching += w["touching"]
    assert np.array_equal(touching * OR.walked(boxes), want64[2][:len(boxes)]), "the counting walk finds every member"
    if key[0] == "guard":
        # the traversals that a guard of 2^-110 or 2^-108 would give, from the same stored boxes: where the CPU measurement says a
        # neighbour begins another number of walks (XS.GUARD_SEPARATES), it does here, so the equality below tells them apart
        lo, hi = OR.lo_hi(boxes)
        walks = {g: sum(int((go & ~IO.guarded_misses(stored[i][0][None], stored[i][1][None], lo, hi, guard=F(2.0 ** g))).sum())
                        for i in range(len(c.of))) for g in (-110, -109, -108)}
        assert walks[-109] == total["traversals"]
        print(f"{c}: traversals {walks[-109]}, with the guard at 2^-110 {walks[-110]}, at 2^-108 {walks[-108]}")
        below, above = XS.GUARD_SEPARATES[key[1]]
        assert (not below or walks[-110] < walks[-109]) and (not above or walks[-108] > walks[-109]), (c, walks)
    for k, counts in ((8, True), (0, True)):
        got = s.triangles_in_boxes(boxes, max_triangles=k, counts=counts, counters=True)
        assert_answer(got[:3], want64, k, counts, f"{c}, counting form, K = {k}")
        for name in COUNTERS:
            assert got[3][name] == total[name], (c, k, name, got[3], total)
        assert got[3]["samples"] == len(boxes)


# 4 ---------------------------------------------------------------------------------------------------------------------------
def one_corner_scene(pkg, v):
    """a resident scene of one triangle whose three corners are v, in a root box that is v itself (helpers.single_leaf_scene
    pads its box by 1e-5, which would hold every subnormal)"""
    pts = np.tile(np.asarray(v, F), (3, 1))
    hm = np.full((8, 1, 2), END, dtype=F)
    sc = pkg.Scene(HandScene(pts, np.zeros((3, 3), F), [pts[0]], [pts[0]], hm, [[0, 1]], 0).desc)
    _hand.append(sc)
    return sc


def test_the_draws_whose_corner_leaves_its_stored_box(pkg, gpu):
    """("draws", -147): one instance per draw, a one-corner scene under the draw's map; box i is the zero-extent box on draw i's
    fp32 world corner, which lies outside the box the top level stores for instance i.  The pair (i, 0) is in box i's answer on
    every path and in every form, and the whole answer is the restatement's."""
    c = XS.draws_cell(pkg)
    positions = c.positions(pkg)
    members = [(positions[i], one_corner_scene(pkg, positions[i][:3])) for i in range(len(positions))]
    s = pkg.tracer.InstanceSet([m[1] for m in members], c.maps)
    _sets.append(s)
    stored = stored_boxes(pkg, s, len(c.of))
    w = c.boxes["lo"]
    outside = sum(bool(((w[i] < stored[i][0]) | (w[i] > stored[i][1])).any()) for i in range(len(w)))
    assert outside == len(w), f"{outside} of {len(w)} corners lie outside the box read back for their instance"
    want64 = restate(members, c.of, c.maps, c.boxes)
    rows = np.arange(len(w))
    assert ((want64[1] == rows[:, None]) & (want64[0] == 0)).any(1).all(), "the restatement holds (i, 0) in box i"
    check_every_form(s, c.boxes, want64, str(c))
    for path in PATHS:
        tri, inst, n = query(s, c.boxes, 64, True, path)
        assert (n >= 1).all(), path
        if inst is not None:
            assert ((inst == rows[:, None]) & (tri == 0)).any(1).all(), path


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_a_device_update_across_magnitudes_and_a_host_update_back(pkg, gpu):
    """One set goes from the k = 0 maps to the k = 40 maps by update_into on a side stream with triangles_in_boxes_into behind it
    on that stream (K = 9, no instance buffer, no counts: the pruning form through the scratch), and back by the host update,
    then queried on the three paths: each state against its restatement."""
    import torch
    c0, c40 = XS.cell(pkg, ("world", 0)), XS.cell(pkg, ("world", 40))
    members = members_of(pkg, c0)
    s = make_set(pkg, members, c0.of, c0.maps, "before the updates")
    n, K = len(c40.boxes), 9
    d_maps, d_boxes = torch.from_numpy(c40.maps).cuda(), dev_boxes(c40.boxes)
    d_out = torch.full((n, K), -7, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.update_into(d_maps.data_ptr(), side.cuda_stream)
        s.triangles_in_boxes_into(d_boxes.data_ptr(), n, d_out.data_ptr(), 0, 0, K, False, side.cuda_stream)
    side.synchronize()
    assert s.update_status() == -1
    want40 = restate(members, c40.of, c40.maps, c40.boxes)
    assert_answer((d_out.cpu().numpy(), None, None), want40, K, False, "after the device update to 2^40")
    G.assert_contained(pkg, s, [members[k][0] for k in c40.of], c40.maps, "after the device update to 2^40")
    s.update(c0.maps)
    want0 = restate(members, c0.of, c0.maps, c0.boxes)
    check_every_form(s, c0.boxes, want0, "after the host update back to 2^0")
    G.assert_contained(pkg, s, [members[k][0] for k in c0.of], c0.maps, "after the host update back to 2^0")
