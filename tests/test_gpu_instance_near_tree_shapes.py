"""Instanced within-radius queries on the GPU over the hand-shaped trees of tests/tree_shapes.py (a root that is a leaf, heights
that sit on the edges of the bottom-up schedule, a lopsided spine).  Per shape, one instance under a rotation with non-uniform
scale and under the identity: every byte, instance and count at K = 8 and K = 64 against the restatement, and the counting
form's node_visits, leaf_visits, triangle_tests and traversals EQUAL to instance_near_ref.walk_counters, which restates the
counting walk one point at a time over the tree and refit_ref.node_boxes (a one-instance set never consults its top level and
lanes do not interact, so the sum over the points is exact); under the identity also Scene.triangles_within's own counters."""
import numpy as np
import pytest

import instance_near_cases as NC
import instance_near_ref as IN
import near_ref as NR
import refit_ref
import test_gpu_instance_point as G
import tree_shapes as T
from test_gpu_instance_near import assert_answer, query, restate
from test_gpu_instance_point_tree_shapes import one_map
from test_gpu_tree_shapes import shapes     # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

F = np.float32
MAP_KINDS = ("rotation_nonuniform", "identity")
POINTS = 512
COUNTERS = ("node_visits", "leaf_visits", "triangle_tests", "traversals")


@pytest.mark.parametrize("kind", MAP_KINDS)
@pytest.mark.parametrize("name", T.NAMES)
def test_one_instance_of_a_shape_under_a_map(pkg, gpu, shapes, name, kind):
    s = shapes(name)
    corners = s.corners()
    positions = corners.reshape(-1)
    boxes = refit_ref.node_boxes(s.tree, corners)
    seed = T.NAMES.index(name) * 10 + MAP_KINDS.index(kind)
    what = f"{name}, {kind}"
    M = one_map(kind, np.random.default_rng(500 + seed), positions)
    maps = M[None]
    iset = pkg.tracer.InstanceSet([s.scene], maps)
    try:
        G.assert_contained(pkg, iset, [positions], maps, what)
        pts, _, _ = NC.world_points([positions], [0], maps, POINTS, seed=seed)
        want64 = restate([positions], [0], maps, pts)
        cnt = want64[2]
        assert (cnt == 0).mean() > 0.1 and (cnt == len(corners)).mean() > 0.2, (what, np.bincount(np.minimum(cnt, 65)))
        if len(corners) > 1:
            assert ((cnt > 0) & (cnt < len(corners))).mean() > 0.04, what
        for k in (8, 64):
            for counts in (True, False):
                for path in ("host", "device", "no instance buffer"):
                    assert_answer(query(iset, pts, k, counts, path), want64, k, counts, f"{what}, K = {k}, counts = {counts}, {path}")
        w = IN.walk_counters(s.tree, boxes, corners, M, pts, device="cuda")
        assert np.array_equal(w["near"], cnt), f"{what}: the restated walk's own counts"
        assert np.array_equal(w["traversals"], NR.walked(pts).astype(np.int64))
        for k in (8, 64):
            got = iset.triangles_within(pts, max_near=k, counters=True)
            assert_answer(got[:3], want64, k, True, f"{what}, counting form, K = {k}")
            for c in COUNTERS:
                assert got[3][c] == int(w[c].sum()), (what, k, c, got[3], {x: int(w[x].sum()) for x in COUNTERS})
            assert got[3]["samples"] == len(pts)
        if kind == "identity":
            plain = s.scene.triangles_within(pts, max_near=8, counters=True)[2]
            for c in ("node_visits", "leaf_visits", "triangle_tests"):
                assert plain[c] == int(w[c].sum()), (what, c, plain)
    finally:
        iset.close()
