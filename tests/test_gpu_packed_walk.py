"""The twelve one-lane-per-item queries that walk a scene's packed tree, each with its own copy of one of two loops (nearest
first: closest point, within radius, triangle distance, their instanced forms, instanced signed distance; touching: box
overlap, triangle intersection, their instanced forms, the collision matrix), on the smallest trees that
have the branches those copies share: leaf_root (the root is a leaf:
the walk goes straight to a pop on an empty stack), one_branch (one push, one pop) and tree_shapes.WALK_SHAPES' spine3 (two
entries on the stack at once, and a pop that returns a branch whose own sibling still waits).  Every result is compared as
bits with the restatement that query's own GPU test uses, and the work counters with that restatement's walk_counters, which
restate the counting walk one item at a time: for the plain queries, for the one-instance sets, and for the counting forms of
the three-instance sets as the sum over the instances behind the boxes the top level stores (the forms that prune or stop at a
member carry state from one instance into the next in the top level's order, which no per-instance restatement predicts); for
the collision matrix in its counts mode and its ANY mode.

Items per query: 1, 63, 65 and 129 (a partial last wave), and a layout whose first wave has no walking lane (64 items that are
non-finite, inverted, degenerate or have a negative max_dist2) ahead of 65 others.  The instanced forms run over sets of one
instance (the identity: the set never consults its top level, so the counters are the restated walk's) and of three, the third
an exact duplicate of the first, so that a lane's reach and its K best carry from one member into the next and every key ties
across two instances.

The "reach has dropped" pop: on spine3 a point (or query triangle) on the last triangle, which lies in the root's positive
leaf, under max_dist2 = +inf.  Both of the root's children are in reach when the negative one, the branch N1, is pushed; the
leaf gives dist2 = 0; N1's bound is above 0 when it is popped.  The rechecking walks skip it there and the counting forms must
not: the closest-point walk visits 3 nodes and 1 leaf, the counting within-radius and triangle-distance walks all 7 nodes and 4
leaves, both as instance_point_ref / instance_near_ref / instance_clearance_ref.walk_counters predict (so no golden file of
counters is needed for it: 3 < 7 is the restatement's own statement, and it held on the commit before the walks were shared).
For the name-only stacks (within-radius, triangle distance) this pop is the one place the recomputed bound is compared; K = 1
and K = 2 (pruned: no counts) are compared as bits there.

The ANY forms: on spine3 the box of the whole tree finds its first member in the first leaf it reaches, the deepest on the
negative side, while two entries wait on the stack; the walk must stop there (5 nodes and 1 leaf, against the counting walk's
7 and 4, as instance_overlap_ref.walk_counters restates it), and the flag must be the restatement's.  The ANY forms of the
other four touching queries and of the two triangle-distance queries are compared with their restated ANY walks' counters on
every layout."""
import numpy as np
import pytest

import clearance_ref as CR
import instance_clearance_ref as XR
import instance_intersect_ref as II
import instance_near_ref as IN
import instance_overlap_ref as IO
import instance_pairs_ref as PR
import instance_point_ref as IP
import instance_sdf_ref as IS
import intersect_ref as IR
import intersect_shape_cases as TSH
import near_cases
import near_ref as NR
import overlap_ref as OR
import overlap_shape_cases as BSH
import point_query_ref as PQ
import sdf_ref as S
import test_gpu_clearance as GC
import test_gpu_instance_clearance as GXC
import test_gpu_instance_intersect as GXI
import test_gpu_instance_near as GXN
import test_gpu_instance_overlap as GXO
import test_gpu_instance_point as GXP
import test_gpu_intersect as GI
import test_gpu_overlap as GO
from test_gpu_instance_pairs import assert_cells, run as pairs_run, wanted
from test_gpu_instance_sdf import assert_values
from test_gpu_point_query import assert_bits, make_points
from test_gpu_signed_distance import assert_same_floats
from test_gpu_tree_shapes import Shape

pytestmark = pytest.mark.gpu

F = np.float32
INF = F(np.inf)
SHAPES = ("leaf_root", "one_branch", "spine3")
SIZES = (1, 63, 65, 129)
COUNTERS = ("node_visits", "leaf_visits", "triangle_tests", "traversals")
WALK = COUNTERS[:3]
IDENTITY = np.eye(3, 4, dtype=F)


@pytest.fixture(scope="module")
def shapes(pkg, gpu):
    """shapes(name): one resident scene per shape for this module (test_gpu_tree_shapes.Shape), closed at its end"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = Shape(pkg, name)
        return made[name]

    yield get
    for s in made.values():
        s.close()


def layouts(items, walked):
    """(what, items) of SIZES' counts, each starting with a walked item, and of the layout whose first wave walks nothing"""
    w, u = items[walked], items[~walked]
    assert len(w) >= 129 and len(u) >= 1, (len(w), len(u))
    mixed = np.concatenate([w[:1], items[:128]])
    for n in SIZES:
        yield f"{n} items", np.ascontiguousarray(mixed[:n])
    yield "an unwalked first wave", np.ascontiguousarray(np.concatenate([u[np.arange(64) % len(u)], w[:65]]))


def sets_of(s):
    """(what, scenes, scene_of_instance, maps): one instance under the identity; three, the second moved by two pitches along the
    tree's axis and half a unit across it, the third an exact duplicate of the first"""
    moved = IDENTITY.copy()
    moved[:, 3] = (0.4, 0.5, -0.25)
    return (("one instance", [s.scene], [0], IDENTITY[None].copy()),
            ("three instances, one a duplicate", [s.scene] * 3, [0, 0, 0], np.stack([IDENTITY, moved, IDENTITY])))


def same_counters(got, want, names, what):
    for c in names:
        assert got[c] == int(np.sum(want[c])), (what, c, {x: got[x] for x in names}, {x: int(np.sum(want[x])) for x in names})


def summed(walk, maps, stored):
    """the counters of a counting form over a set: the sum over the instances of walk(M, top_box), the restated walk of one
    instance behind the box the set's top level stores for it (a lane's walks of two instances do not interact in a form that
    neither prunes nor stops at a member)"""
    total = dict.fromkeys(COUNTERS, 0)
    for i, M in enumerate(maps):
        w = walk(M, stored[i])
        for c in COUNTERS:
            total[c] += int(np.sum(w[c]))
    return total


def pairs_any(pkg, iset):
    """(cells bool [n, n], counters) of the collision matrix's ANY mode through its counting entry"""
    import ctypes as C
    N = pkg._native
    cells = np.empty((iset.count, iset.count), np.int64)
    op = pkg.tracer._pairs_params(0, iset.count, True, False, False)
    tally = N.Counters()
    N.check(N.load_instance_pairs().shray_instance_pairs_intersect_counters(iset._handle, C.byref(op), None, cells.ctypes.data_as(C.c_void_p),
                                                                            C.byref(tally)))
    return cells != 0, tally.as_dict()


def geometry(s):
    corners = s.corners()
    return corners, corners.reshape(-1), s.tree.box


# nearest first ----------------------------------------------------------------------------------------------------------------
def points_of(pkg, xyz, md=None):
    return pkg.tracer.make_points(np.asarray(xyz, F).reshape(-1, 3), md)


@pytest.mark.parametrize("name", SHAPES)
def test_closest_points_and_signed_distances(pkg, gpu, shapes, name):
    s = shapes(name)
    corners, positions, boxes = geometry(s)
    every = make_points(s.arrays, 400, seed=11 + len(name))
    derived = S.derive(np.asarray(positions, F))
    for what, pts in layouts(every, NR.walked(every)):
        what = f"{name}, {what}"
        want = PQ.closest(positions, pts)
        got, tally = s.scene.closest_points(pts, counters=True)
        assert_bits(got, want, what + ": closest points, counting form")
        assert_bits(s.scene.closest_points(pts), want, what + ": closest points")
        w = IP.walk_counters(s.tree, boxes, corners, IDENTITY, pts)
        same_counters(tally, w, WALK, what + ": closest points")
        assert_same_floats(s.scene.signed_distance(pts), S.signed(pts, want, derived["sign_data"]), what + ": signed distance")
        for label, scenes, of, maps in sets_of(s):
            iset = pkg.tracer.InstanceSet(scenes, maps)
            try:
                tag = f"{what}, {label}"
                w_rec, w_inst = IP.closest_over_instances([positions], of, maps, pts)
                got, inst, c = iset.closest_points(pts, counters=True)
                GXP.assert_answer(got, inst, w_rec, w_inst, tag + ": instanced closest points, counting form")
                got, inst = iset.closest_points(pts)
                GXP.assert_answer(got, inst, w_rec, w_inst, tag + ": instanced closest points")
                if len(of) == 1:
                    same_counters(c, w, COUNTERS, tag + ": instanced closest points")
                else:
                    assert (w_inst[w_inst >= 0] != 2).all(), "a tie between an instance and its duplicate goes to the lower"
                W = iset.world_to_object()
                want_signed = IS.signed_over_instances([positions], of, maps, W, pts)[0]
                assert_values(iset.signed_distance(pts), want_signed, tag + ": instanced signed distance")
            finally:
                iset.close()


def test_the_pop_that_skips_what_the_reach_has_dropped_below(pkg, gpu, shapes):
    s = shapes("spine3")
    corners, positions, boxes = geometry(s)
    pts = points_of(pkg, corners[-1].astype(np.float64).mean(0))
    want = PQ.closest(positions, pts)
    assert want["triangle"][0] == len(corners) - 1 and want["dist2"][0] < 1e-8
    # the closest-point walk (uint2 entries, always rechecked) skips the popped branch ...
    got, tally = s.scene.closest_points(pts, counters=True)
    assert_bits(got, want, "closest point")
    pruned = IP.walk_counters(s.tree, boxes, corners, IDENTITY, pts)
    same_counters(tally, pruned, WALK, "closest point")
    assert (tally["node_visits"], tally["leaf_visits"]) == (3, 1), tally
    # ... the counting within-radius walk (name-only entries, no recheck) must not ...
    want64 = NR.near(positions, pts, 64)
    for k in (1, 2, 8, 64):
        rec, n, tally = s.scene.triangles_within(pts, max_near=k, counters=True)
        assert np.array_equal(NR.as_bits(rec), NR.as_bits(want64[0][:, :k])) and np.array_equal(n, want64[1]), k
        counted = IN.walk_counters(s.tree, boxes, corners, IDENTITY, pts)
        same_counters(tally, counted, WALK, f"within radius, counting form, K = {k}")
        assert (tally["node_visits"], tally["leaf_visits"]) == (7, 4) and tally["node_visits"] > pruned["node_visits"].sum(), tally
    # ... and its pruned forms (no counts), where the recomputed bound is compared, give the same K nearest
    for k in (1, 2):
        rec, n = s.scene.triangles_within(pts, max_near=k, counts=False)
        assert n is None and np.array_equal(NR.as_bits(rec), NR.as_bits(want64[0][:, :k])), k
    # the same point as a degenerate-free query triangle: the last triangle itself
    q = np.ascontiguousarray(corners[-1:])
    queries, d2, shared = GC.table(("packed walk", "spine3", "dropped reach"), q, positions)
    GC.check_forms(GC.item_run(s.scene, queries, INF), queries, positions, d2, shared, INF, False, "triangle distance", ks=(0, 1, 2, 8))
    for any_only in (False, True):
        counted = XR.walk_counters(s.tree, boxes, corners, IDENTITY, queries, INF, any_only=any_only)
        tally = s.scene.triangle_distances(queries, INF, max_pairs=0, counters=True, any_only=any_only)[2]
        same_counters(tally, counted, WALK, f"triangle distance, counting form, ANY {any_only}")
        assert (tally["node_visits"], tally["leaf_visits"]) == ((3, 1) if any_only else (7, 4)), (any_only, tally)
    for label, scenes, of, maps in sets_of(s):
        iset = pkg.tracer.InstanceSet(scenes, maps)
        try:
            want_n = GXN.restate([positions], of, maps, pts)
            for k, counts in ((1, False), (2, False), (8, True), (64, True)):
                GXN.assert_answer(GXN.query(iset, pts, k, counts, "host"), want_n, k, counts, f"{label}: within radius, K = {k}")
            table = GXC.table_of([positions], of, maps, queries)
            want_c = XR.from_merged_table(table, queries, 64, INF)
            for k, counts in ((1, False), (2, False), (8, True)):
                GXC.assert_answer(GXC.query(iset, queries, k, counts, "host", INF), want_c, k, counts, f"{label}: triangle distance, K = {k}")
        finally:
            iset.close()


@pytest.mark.parametrize("name", SHAPES)
def test_within_radius(pkg, gpu, shapes, name):
    s = shapes(name)
    corners, positions, boxes = geometry(s)
    every = near_cases.make_points(s.arrays, 400, seed=21 + len(name))
    for what, pts in layouts(every, NR.walked(every)):
        what = f"{name}, {what}"
        want64 = NR.near(positions, pts, 64)
        for k, counts in ((1, False), (8, False), (8, True), (64, True), (0, True)):
            rec, n = s.scene.triangles_within(pts, max_near=k, counts=counts)
            if k:
                assert np.array_equal(NR.as_bits(rec), NR.as_bits(want64[0][:, :k])), f"{what}: within radius, K = {k}, counts = {counts}"
            assert n is None if not counts else np.array_equal(n, want64[1]), f"{what}: counts, K = {k}"
        w = IN.walk_counters(s.tree, boxes, corners, IDENTITY, pts)
        same_counters(s.scene.triangles_within(pts, max_near=8, counters=True)[2], w, WALK, what + ": within radius")
        for label, scenes, of, maps in sets_of(s):
            iset = pkg.tracer.InstanceSet(scenes, maps)
            try:
                want = GXN.restate([positions], of, maps, pts)
                for k, counts in ((1, False), (8, False), (8, True), (64, True), (0, True)):
                    GXN.assert_answer(GXN.query(iset, pts, k, counts, "host"), want, k, counts, f"{what}, {label}: K = {k}, counts = {counts}")
                got = iset.triangles_within(pts, max_near=8, counters=True)
                GXN.assert_answer(got[:3], want, 8, True, f"{what}, {label}: counting form")
                if len(of) == 1:
                    same_counters(got[3], w, COUNTERS, f"{what}, {label}: within radius")
                else:
                    stored = GXO.stored_boxes(pkg, iset, len(of))
                    same_counters(got[3], summed(lambda M, top: IN.walk_counters(s.tree, boxes, corners, M, pts, top_box=top), maps, stored),
                                  COUNTERS, f"{what}, {label}: within radius")
            finally:
                iset.close()


@pytest.mark.parametrize("name", SHAPES)
def test_triangle_distances(pkg, gpu, shapes, name):
    s = shapes(name)
    corners, positions, boxes = geometry(s)
    every = TSH.shape_triangles(s.tree, corners, boxes, 31 + len(name), small=100, own=60)
    md = F((5 * 0.2) ** 2)
    for j, (what, queries) in enumerate(layouts(every, CR.walked(every, md))):
        what = f"{name}, {what}"
        queries, d2, shared = GC.table(("packed walk", name, j), queries, positions)
        GC.check_forms(GC.item_run(s.scene, queries, md), queries, positions, d2, shared, md, False, what, ks=(0, 1, 8, 64), paths=("host",))
        GC.check_forms(GC.item_run(s.scene, queries, INF), queries, positions, d2, shared, INF, False, what + ", +inf", ks=(1, 2), paths=("host",))
        for label, scenes, of, maps in sets_of(s):
            iset = pkg.tracer.InstanceSet(scenes, maps)
            try:
                table = GXC.table_of([positions], of, maps, queries)
                want = XR.from_merged_table(table, queries, 64, md)
                for k, counts in ((1, False), (8, False), (8, True), (0, True)):
                    GXC.assert_answer(GXC.query(iset, queries, k, counts, "host", md), want, k, counts, f"{what}, {label}: K = {k}, counts = {counts}")
                met = GXC.query(iset, queries, 0, True, "host", md, any_only=True)[2]
                assert np.array_equal(met, (want[2] > 0).astype(np.int32)), f"{what}, {label}: ANY"
                if len(of) == 1:
                    for any_only in (False, True):
                        w = XR.walk_counters(s.tree, boxes, corners, IDENTITY, queries, md, any_only=any_only, d2s=table[2])
                        got = iset.triangle_distances(queries, md, max_pairs=0, counters=True, any_only=any_only)
                        same_counters(got[3], w, COUNTERS, f"{what}, {label}: triangle distance, ANY {any_only}")
                        plain = s.scene.triangle_distances(queries, md, max_pairs=0, counters=True, any_only=any_only)[2]
                        same_counters(plain, w, WALK, f"{what}: triangle distance, ANY {any_only}")
                else:   # (the ANY form of a larger set stops at a member of whichever instance its top level reaches first)
                    stored = GXO.stored_boxes(pkg, iset, len(of))
                    got = iset.triangle_distances(queries, md, max_pairs=0, counters=True)
                    same_counters(got[3], summed(lambda M, top: XR.walk_counters(s.tree, boxes, corners, M, queries, md, top_box=top), maps, stored),
                                  COUNTERS, f"{what}, {label}: triangle distance")
            finally:
                iset.close()


# touching ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_box_overlaps(pkg, gpu, shapes, name):
    s = shapes(name)
    corners, positions, boxes_of_nodes = geometry(s)
    every = BSH.shape_boxes(s.tree, corners, boxes_of_nodes, 41 + len(name), small=100)
    whole = OR.make_boxes(np.asarray(boxes_of_nodes, F)[:1, :3], np.asarray(boxes_of_nodes, F)[:1, 3:])   # the root's own box
    every = np.concatenate([whole, every])
    for what, boxes in layouts(every, OR.walked(every)):
        what = f"{name}, {what}"
        member = OR.overlaps(positions, boxes)
        GO.check_every_k(s.scene, boxes, member, what, paths=("host",))
        touched = s.scene.triangles_in_boxes(boxes, max_triangles=0, any_only=True)[1]
        assert np.array_equal(touched, member.any(1).astype(np.int32)), what + ": ANY"
        for label, scenes, of, maps in sets_of(s):
            iset = pkg.tracer.InstanceSet(scenes, maps)
            try:
                want = GXO.restate([positions], of, maps, boxes)
                for k, counts in ((0, True), (1, True), (8, True), (8, False), (64, True)):
                    GXO.assert_answer(GXO.query(iset, boxes, k, counts, "host"), want, k, counts, f"{what}, {label}: K = {k}, counts = {counts}")
                met = GXO.query(iset, boxes, 0, True, "host", any_only=True)[2]
                assert np.array_equal(met, (want[2] > 0).astype(np.int32)) and met.any(), f"{what}, {label}: ANY"
                if len(of) == 1:
                    for any_only in (False, True):
                        w = IO.walk_counters(s.tree, boxes_of_nodes, corners, IDENTITY, boxes, any_only=any_only)
                        got = iset.triangles_in_boxes(boxes, max_triangles=0, counters=True, any_only=any_only)
                        same_counters(got[3], w, COUNTERS, f"{what}, {label}: box overlap, ANY {any_only}")
                        plain = s.scene.triangles_in_boxes(boxes, max_triangles=0, counters=True, any_only=any_only)[2]
                        same_counters(plain, w, WALK, f"{what}: box overlap, ANY {any_only}")
                        if name == "spine3":   # the whole box: ANY stops in the first leaf it reaches, two entries waiting
                            at = 64 if "unwalked" in what else 0
                            assert (w["leaf_visits"][at], w["node_visits"][at]) == ((1, 5) if any_only else (4, 7)), (any_only, w)
                else:   # (the ANY form of a larger set stops at a member of whichever instance its top level reaches first)
                    stored = GXO.stored_boxes(pkg, iset, len(of))
                    got = iset.triangles_in_boxes(boxes, max_triangles=0, counters=True)
                    same_counters(got[3], summed(lambda M, top: IO.walk_counters(s.tree, boxes_of_nodes, corners, M, boxes, top_box=top), maps, stored),
                                  COUNTERS, f"{what}, {label}: box overlap")
            finally:
                iset.close()


@pytest.mark.parametrize("name", SHAPES)
def test_triangle_intersections_and_the_collision_matrix(pkg, gpu, shapes, name):
    s = shapes(name)
    corners, positions, boxes = geometry(s)
    every = TSH.shape_triangles(s.tree, corners, boxes, 51 + len(name), small=100, own=60)
    for what, queries in layouts(every, IR.walked(every)):
        what = f"{name}, {what}"
        member = IR.intersects(queries, positions)
        GI.check_forms(GI.item_run(s.scene, queries), member, what, ks=(0, 1, 8, 64), paths=("host",))
        for label, scenes, of, maps in sets_of(s):
            iset = pkg.tracer.InstanceSet(scenes, maps)
            try:
                want = GXI.restate([positions], of, maps, queries)
                for k, counts in ((0, True), (1, True), (8, True), (8, False), (64, True)):
                    GXI.assert_answer(GXI.query(iset, queries, k, counts, "host"), want, k, counts, f"{what}, {label}: K = {k}, counts = {counts}")
                met = GXI.query(iset, queries, 0, True, "host", any_only=True)[2]
                assert np.array_equal(met, (want[2] > 0).astype(np.int32)), f"{what}, {label}: ANY"
                if len(of) == 1:
                    for any_only in (False, True):
                        w = II.walk_counters(s.tree, boxes, corners, IDENTITY, queries, any_only=any_only)
                        got = iset.intersecting_triangles(queries, max_triangles=0, counters=True, any_only=any_only)
                        same_counters(got[3], w, COUNTERS, f"{what}, {label}: intersection, ANY {any_only}")
                        plain = s.scene.intersecting_triangles(queries, max_triangles=0, counters=True, any_only=any_only)[2]
                        same_counters(plain, w, WALK, f"{what}: intersection, ANY {any_only}")
                else:   # (the ANY form of a larger set stops at a member of whichever instance its top level reaches first)
                    stored = GXO.stored_boxes(pkg, iset, len(of))
                    got = iset.intersecting_triangles(queries, max_triangles=0, counters=True)
                    same_counters(got[3], summed(lambda M, top: II.walk_counters(s.tree, boxes, corners, M, queries, top_box=top), maps, stored),
                                  COUNTERS, f"{what}, {label}: intersection")
            finally:
                iset.close()
    # The collision matrix of the shape placed once (no pair at all) and three times, the third a duplicate of the first: every
    # cell against the brute force, and the counters of the counting entry in the counts mode and in the ANY mode (a lane's
    # walks of two instances do not interact there: with the counters nothing is skipped by what a cell holds) against the sum
    # over the ordered pairs of instance_intersect_ref.walk_counters.
    for label, scenes, of, maps in sets_of(s):
        iset = pkg.tracer.InstanceSet(scenes, maps)
        try:
            n = len(of)
            brute = PR.brute(PR.memberships([positions], of, maps)[0])
            assert n == 1 or (brute[1][0, 2] > 0 and brute[1][2, 0] > 0), "an instance and its duplicate collide"
            for mode in PR.MODES:
                assert_cells(pairs_run(iset, mode, "host"), wanted(brute, mode), f"{name}, {label}, {mode}")
                assert_cells(pairs_run(iset, mode, "device"), wanted(brute, mode), f"{name}, {label}, {mode}, device")
            stored = GXO.stored_boxes(pkg, iset, n) if n > 1 else [None]   # (a set of one instance culls nothing)
            trees = [(s.tree, boxes, corners)]
            total, members = PR.walk_counters_sum(trees, [positions], of, maps, stored)
            assert np.array_equal(members, brute[1]), "the counting walk finds every member"
            ta, tb, cnt, tally = iset.collision_pairs(counters=True)
            assert np.array_equal(cnt, brute[1]) and np.array_equal(ta, PR.split_keys(brute[0])[0]) and np.array_equal(tb, PR.split_keys(brute[0])[1])
            same_counters(tally, total, PR.COUNTERS, f"{name}, {label}: collision matrix, counts")
            assert tally["samples"] == n * len(corners)
            total, _ = PR.walk_counters_sum(trees, [positions], of, maps, stored, any_only=True)
            cells, tally = pairs_any(pkg, iset)
            assert np.array_equal(cells, brute[1] > 0), f"{name}, {label}: collision matrix, ANY"
            same_counters(tally, total, PR.COUNTERS, f"{name}, {label}: collision matrix, ANY")
        finally:
            iset.close()
