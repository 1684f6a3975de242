"""Instanced triangle-distance queries on the GPU over the hand-shaped trees of tests/tree_shapes.py (a root that is a leaf,
heights that sit on the edges of the bottom-up schedule, a lopsided spine).  Per shape, one instance under the identity and under
a rotation with non-uniform scale, 512 queries of tests/intersect_shape_cases.py mapped to the world, max_dist2 a reach of five
triangle pitches (so that a query beside a seam has members in both subtrees and the walk must push the farther child and come
back to it): all 48 bytes of every record, every instance and every count at K = 8 and K = 64 and the ANY form against the
restatement on the three paths, and the counting form's node_visits, leaf_visits, triangle_tests and traversals EQUAL to
instance_clearance_ref.walk_counters, which restates the walk one query at a time over the tree's image boxes (a one-instance set
never consults its top level and lanes do not interact, so the sum over the queries is exact); under the identity also
Scene.triangle_distances' own counters."""
import numpy as np
import pytest

import clearance_ref as CR
import instance_clearance_ref as XR
import intersect_shape_cases as SH
import test_gpu_instance_point as G
import tree_shapes as T
from test_gpu_instance_clearance import PATHS, assert_answer, query, table_of
from test_gpu_instance_intersect_tree_shapes import world_queries
from test_gpu_instance_point_tree_shapes import one_map
from test_gpu_tree_shapes import shapes     # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

F = np.float32
MAP_KINDS = ("identity", "rotation_nonuniform")
QUERIES = 512
REACH = 5 * T.PITCH
COUNTERS = ("node_visits", "leaf_visits", "triangle_tests", "traversals")


@pytest.mark.parametrize("kind", MAP_KINDS)
@pytest.mark.parametrize("name", T.NAMES)
def test_one_instance_of_a_shape_under_a_map(pkg, gpu, shapes, name, kind):
    s = shapes(name)
    corners = s.corners()
    positions = corners.reshape(-1)
    node_boxes = s.tree.box
    seed = T.NAMES.index(name) * 10 + MAP_KINDS.index(kind)
    what = f"{name}, {kind}"
    M = one_map(kind, np.random.default_rng(900 + seed), positions)
    maps = M[None]
    every = SH.shape_triangles(s.tree, corners, node_boxes, 80 + seed, small=100, own=60)
    picked = np.concatenate([every[:QUERIES - 40], every[-40:]])
    assert len(picked) == QUERIES
    queries = picked if kind == "identity" else world_queries(picked, M)
    # the reach in the world: five pitches along the tree's axis (the triangles lie along x) under the map
    md = F((REACH * float(np.linalg.norm(np.asarray(M, np.float64)[:, 0]))) ** 2)
    walked = CR.walked(queries, md)
    assert (~walked).sum() >= 4
    iset = pkg.tracer.InstanceSet([s.scene], maps)
    try:
        G.assert_contained(pkg, iset, [positions], maps, what)
        table = table_of([positions], [0], maps, queries)
        want = XR.from_merged_table(table, queries, 64, md)
        cnt = want[2]
        print(what, np.bincount(np.minimum(cnt, 65)))
        assert (cnt == 0).mean() > 0.02 and (cnt > 0).mean() > 0.3, (what, np.bincount(np.minimum(cnt, 65)))
        if len(corners) > 64:
            assert (cnt > 8).mean() > 0.1 and (cnt > 64).sum() >= 1, (what, np.bincount(np.minimum(cnt, 65)))
        for path in PATHS:
            for k, counts in ((8, True), (8, False), (64, True), (64, False), (0, True)):
                assert_answer(query(iset, queries, k, counts, path, md), want, k, counts, f"{what}, K = {k}, counts = {counts}, {path}")
            met = query(iset, queries, 0, True, path, md, any_only=True)[2]
            assert np.array_equal(met, (cnt > 0).astype(np.int32)), f"{what}, ANY, {path}"
        for any_only in (False, True):
            w = XR.walk_counters(s.tree, node_boxes, corners, M, queries, md, any_only=any_only, d2s=table[2])
            assert np.array_equal(w["members"], cnt), f"{what}: the restated walk's own counts"
            assert np.array_equal(w["traversals"], walked.astype(np.int64))
            for k in ((0,) if any_only else (0, 8)):
                got = iset.triangle_distances(queries, md, max_pairs=k, counters=True, any_only=any_only)
                if any_only:
                    assert np.array_equal(got[2], (cnt > 0).astype(np.int32))
                else:
                    assert_answer(got[:3], want, k, True, f"{what}, counting form, K = {k}")
                for c in COUNTERS:
                    assert got[3][c] == int(w[c].sum()), (what, k, any_only, c, got[3], {x: int(w[x].sum()) for x in COUNTERS})
                assert got[3]["samples"] == len(queries)
            if kind == "identity":
                plain = s.scene.triangle_distances(queries, md, max_pairs=0, counters=True, any_only=any_only)[2]
                for c in ("node_visits", "leaf_visits", "triangle_tests"):
                    assert plain[c] == int(w[c].sum()), (what, any_only, c, plain)
    finally:
        iset.close()
