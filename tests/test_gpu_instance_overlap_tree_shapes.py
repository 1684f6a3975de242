"""Instanced box-overlap queries on the GPU over the hand-shaped trees of tests/tree_shapes.py (a root that is a leaf, heights
that sit on the edges of the bottom-up schedule, a lopsided spine).  Per shape, one instance under the identity and under a
rotation with non-uniform scale, 512 boxes of tests/overlap_shape_cases.py mapped to the world: every index, instance and count
at K = 0 and K = 8 and the ANY form against the restatement, and the counting form's node_visits, leaf_visits, triangle_tests and
traversals EQUAL to instance_overlap_ref.walk_counters, which restates the walk one box at a time over the tree's image boxes
(a one-instance set never consults its top level and lanes do not interact, so the sum over the boxes is exact); under the
identity also Scene.triangles_in_boxes' own counters."""
import numpy as np
import pytest

import instance_overlap_ref as IO
import overlap_ref as OR
import overlap_shape_cases as SH
import test_gpu_instance_point as G
import tree_shapes as T
from test_gpu_instance_overlap import PATHS, assert_answer, query
from test_gpu_instance_point_tree_shapes import one_map
from test_gpu_tree_shapes import shapes     # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

F = np.float32
MAP_KINDS = ("identity", "rotation_nonuniform")
BOXES = 512
COUNTERS = ("node_visits", "leaf_visits", "triangle_tests", "traversals")


def world_boxes(object_boxes, root, M):
    """the object-space boxes as world boxes: a walked box is cut to the root box widened by 1 where that leaves a box (the
    open slabs reach +-1000), then the box of its eight corners' images (computed in double, rounded to fp32); a box that is
    not walked stays as it is"""
    lo, hi = (np.array(x, np.float64) for x in OR.lo_hi(object_boxes))
    cut_lo, cut_hi = np.maximum(lo, root[:3] - 1.0), np.minimum(hi, root[3:] + 1.0)
    cut = (cut_lo <= cut_hi).all(1)
    lo[cut], hi[cut] = cut_lo[cut], cut_hi[cut]
    M = np.asarray(M, np.float64)
    ends = np.stack([lo, hi])                                                     # [2, n, 3]
    images = np.stack([np.stack([ends[(c >> a) & 1, :, a] for a in range(3)], -1) @ M[:, :3].T + M[:, 3] for c in range(8)])
    out = OR.make_boxes(images.min(0), images.max(0))
    keep = ~OR.walked(object_boxes)
    out[keep] = object_boxes[keep]
    return out


@pytest.mark.parametrize("kind", MAP_KINDS)
@pytest.mark.parametrize("name", T.NAMES)
def test_one_instance_of_a_shape_under_a_map(pkg, gpu, shapes, name, kind):
    s = shapes(name)
    corners = s.corners()
    positions = corners.reshape(-1)
    node_boxes = s.tree.box
    seed = T.NAMES.index(name) * 10 + MAP_KINDS.index(kind)
    what = f"{name}, {kind}"
    M = one_map(kind, np.random.default_rng(700 + seed), positions)
    maps = M[None]
    every = SH.shape_boxes(s.tree, corners, node_boxes, 60 + seed, small=100)
    picked = np.concatenate([every[:BOXES - 40], every[-40:]])                    # (among the last are boxes that are not walked)
    assert len(picked) == BOXES and (~OR.walked(picked)).sum() >= 10
    boxes = picked if kind == "identity" else world_boxes(picked, np.asarray(node_boxes, np.float64)[0], M)
    iset = pkg.tracer.InstanceSet([s.scene], maps)
    try:
        G.assert_contained(pkg, iset, [positions], maps, what)
        want = IO.overlap_over_instances([positions], [0], maps, boxes, 8)
        cnt = want[2]
        assert (cnt == 0).mean() > 0.05 and (cnt > 0).mean() > 0.3, (what, np.bincount(np.minimum(cnt, 65)))
        if len(corners) > 64:
            assert (cnt > 8).mean() > 0.1 and (cnt > 64).mean() > 0.04, (what, np.bincount(np.minimum(cnt, 65)))
        for path in PATHS:
            for k, counts in ((0, True), (8, True), (8, False)):
                assert_answer(query(iset, boxes, k, counts, path), want, k, counts, f"{what}, K = {k}, counts = {counts}, {path}")
            touched = query(iset, boxes, 0, True, path, any_only=True)[2]
            assert np.array_equal(touched, (cnt > 0).astype(np.int32)), f"{what}, ANY, {path}"
        for any_only in (False, True):
            w = IO.walk_counters(s.tree, node_boxes, corners, M, boxes, any_only=any_only)
            assert np.array_equal(w["touching"], cnt), f"{what}: the restated walk's own counts"
            assert np.array_equal(w["traversals"], OR.walked(boxes).astype(np.int64))
            for k in ((0,) if any_only else (0, 8)):
                got = iset.triangles_in_boxes(boxes, max_triangles=k, counters=True, any_only=any_only)
                if any_only:
                    assert np.array_equal(got[2], (cnt > 0).astype(np.int32))
                else:
                    assert_answer(got[:3], want, k, True, f"{what}, counting form, K = {k}")
                for c in COUNTERS:
                    assert got[3][c] == int(w[c].sum()), (what, k, any_only, c, got[3], {x: int(w[x].sum()) for x in COUNTERS})
                assert got[3]["samples"] == len(boxes)
            if kind == "identity":
                plain = s.scene.triangles_in_boxes(boxes, max_triangles=0, counters=True, any_only=any_only)[2]
                for c in ("node_visits", "leaf_visits", "triangle_tests"):
                    assert plain[c] == int(w[c].sum()), (what, any_only, c, plain)
    finally:
        iset.close()
