"""Box-overlap queries on the GPU over the hand-shaped trees of tests/tree_shapes.py (heights 0 to 16, siblings whose heights
differ by up to 14): every index and count against the restatement (tests/overlap_ref.py) through test_gpu_overlap's
check_every_k, and the walk's own counters -- node visits, leaf visits, triangle tests -- against overlap_ref.walk_counters over
refit_ref.node_boxes, for the counting form at K = 0 and K = 8 and for the ANY form; then the same after a refit to the twist and
collapse deformations, on the host path and on the device path on a side stream.  The boxes are overlap_shape_cases.shape_boxes:
among them the root's own box, whose walk holds one stack entry per level at once.  Nothing is tolerated: every counter is an
equality."""
import numpy as np
import pytest

import overlap_ref as OR
import overlap_shape_cases as SH
import refit_ref as R
import tree_shapes as T
from test_gpu_overlap import assert_same, check_every_k
from test_gpu_refit import deform
from test_gpu_tree_shapes import Shape, shapes   # noqa: F401  (the fixture: one resident scene per shape for this module)

pytestmark = pytest.mark.gpu

F = np.float32
BATCH = 64          # the small batch whose counters are compared box by box

# shape -> the greatest number of stack entries a walk holds (overlap_shape_cases.deepest_stack, reached by the root's own box)
# against the tree's height: every level on the perfect trees and on lopsided; on mixed_spine the four spine branches (heights
# 13 to 16) have small negative children, and the deepest column is the 12 levels of P(12) below them.
DEEPEST = {"leaf_root": (0, 0), "one_branch": (1, 1), "tail_full": (11, 11), "wide_by_one": (12, 12), "two_wide": (13, 13),
           "lopsided": (13, 13), "mixed_spine": (12, 16)}

_cases = {}


def case(s, deformation=None):
    """(vertex data, corners, node boxes, boxes, member, walk_counters of the counting form and of ANY) of a shape over its loaded or deformed vertices, once"""
    key = (s.name, deformation)
    if key not in _cases:
        vd = s.vertex_data if deformation is None else deform(s.vertex_data, deformation)
        corners = s.corners(vd)
        node_boxes = s.tree.box if deformation is None else R.node_boxes(s.tree, corners)
        seed = 50 + T.NAMES.index(s.name)
        boxes = SH.shape_boxes(s.tree, corners, node_boxes, seed, small=400 if deformation is None else 100)
        if deformation is not None:
            # the loaded shape's boxes too: where the triangles were.  After a collapse every triangle is one point, a box holds
            # all of them or none and a walk that holds them visits every node, so fewer boxes are asked.
            mine, loaded = (80, 60) if deformation == "collapse" else (500, 300)
            boxes = np.concatenate([boxes[:mine], case(s)[3][:loaded]])
        member = OR.overlaps(corners.reshape(-1), boxes)
        want = {False: OR.walk_counters(s.tree, node_boxes, corners, boxes),
                True: OR.walk_counters(s.tree, node_boxes, corners, boxes, any_only=True, member=member)}
        _cases[key] = (vd, corners, node_boxes, boxes, member, want)
    return _cases[key]


def check_counters(s, corners, boxes, member, want, what):
    """the host path's counters of the counting form (K = 0 and K = 8) and of ANY against `want` (walk_counters, counting and
    ANY): over all boxes, over one small batch, over its halves and, on the two tiny shapes, box by box"""
    n = member.sum(1).astype(np.int32)
    for rows in ([np.array([i]) for i in range(min(BATCH, len(boxes)))] if len(corners) <= 3 else []) + [np.arange(min(BATCH, len(boxes))), np.arange(len(boxes))]:
        for any_only, k in ((False, 0), (False, 8), (True, 0)):
            _, got_n, c = s.scene.triangles_in_boxes(boxes[rows], max_triangles=k, counters=True, any_only=any_only)
            assert_same(got_n, (n[rows] > 0).astype(np.int32) if any_only else n[rows], what)
            for key in OR.COUNTERS:
                assert c[key] == int(want[any_only][key][rows].sum()), (what, f"{len(rows)} boxes from {rows[0]}", "ANY" if any_only else f"K = {k}", key, c,
                                                                        {x: int(want[any_only][x][rows].sum()) for x in OR.COUNTERS})
            assert c["samples"] == len(rows)
    for rows in (np.arange(BATCH // 2), np.arange(BATCH // 2, BATCH)):
        _, _, c = s.scene.triangles_in_boxes(boxes[rows], max_triangles=0, counters=True)
        assert all(c[key] == int(want[False][key][rows].sum()) for key in OR.COUNTERS), (what, rows[0], c)


@pytest.mark.parametrize("name", T.NAMES)
def test_every_index_count_and_counter(pkg, gpu, shapes, name):
    s = shapes(name)
    _, corners, node_boxes, boxes, member, want = case(s)
    n = member.sum(1)
    triangles = len(corners)
    shares = (float((n == 0).mean()), float((n > 8).mean()), float((n > 64).mean()))
    if triangles > 64:
        assert shares[0] > 0.05 and shares[1] > 0.20 and shares[2] > 0.10, (name, shares)
    assert 900 <= len(boxes) <= 1300 and (~OR.walked(boxes)).sum() >= 30
    check_every_k(s.scene, boxes, member, name)
    check_counters(s, corners, boxes, member, want, name)
    deepest, height = int(want[False]["stack"].max()), int(T.heights(s.tree)[0])
    assert (deepest, height) == DEEPEST[name] and deepest == SH.deepest_stack(s.tree), (name, deepest, height)
    whole = np.nonzero((boxes["lo"] == node_boxes[0, :3]).all(1) & (boxes["hi"] == node_boxes[0, 3:]).all(1))[0]
    assert len(whole) == 1 and want[False]["stack"][whole[0]] == deepest and n[whole[0]] == triangles, name
    print(f"{name}: {triangles} triangles, {len(boxes)} boxes, n = 0 / > 8 / > 64: {shares[0]:.3f} / {shares[1]:.3f} / {shares[2]:.3f}, deepest stack "
          f"{deepest} of height {height}, counting walk { {k: int(want[False][k].sum()) for k in OR.COUNTERS} }, ANY { {k: int(want[True][k].sum()) for k in OR.COUNTERS} }")


@pytest.mark.parametrize("name", T.NAMES)
def test_after_a_refit(pkg, gpu, shapes, name):
    """twist on the host path, collapse on the device path on a side stream, then the other way round"""
    import torch
    s = shapes(name)
    stream = torch.cuda.Stream()
    try:
        for how, deformation in (("host", "twist"), ("device", "collapse"), ("host", "collapse"), ("device", "twist")):
            vd, corners, node_boxes, boxes, member, want = case(s, deformation)
            what = f"{name}/{how}/{deformation}"
            s.refit(vd, how, stream)
            stream.synchronize()
            assert np.array_equal(s.scene.geometry()["vertex_positions"].view(np.uint32), corners.reshape(-1).view(np.uint32)), what
            check_every_k(s.scene, boxes, member, what)
            check_counters(s, corners, boxes, member, want, what)
            n = member.sum(1)
            assert (n > 0).sum() >= 20 and (n == 0).sum() >= 20, (what, int((n > 0).sum()))
    finally:
        s.refit(s.vertex_data)
