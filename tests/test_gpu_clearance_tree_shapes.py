"""Triangle-distance queries on the GPU over the hand-shaped trees of tests/tree_shapes.py (heights 0 to 16, siblings whose
heights differ by up to 14): all 48 bytes of every record and every count against the restatement (tests/clearance_ref.py)
through test_gpu_clearance's check_forms.  The queries are intersect_shape_cases.shape_triangles, imported and not edited:
among them the whole query, whose vertex box is the root's own box (its bound is 0 at every node, so the walk that counts
enters all of them and holds one stack entry per level at once), sheets across every seam of the tree, gaps, the shape's own
triangles, far ones and unwalked ones.

max_dist2 is REACH = 1, a radius of five triangle pitches (tree_shapes.PITCH = 0.2): a query beside a seam (a triangle index
where two subtrees meet) has members in both subtrees, so the walk must push the farther child and come back to it; and +inf,
where the form that prunes drops nearly every pushed node when it is popped and the form that counts none.  The self form
runs over 130 of the shape's own triangles across the seam nearest the middle, with SKIP_SHARED.

The restatement runs on all queries for shapes of up to 5,000 triangles and on a fixed 128 (the first 128 of the shuffled set,
which starts with the whole query) for the larger ones, as the winding tests do; the GPU is asked about the same queries."""
import numpy as np
import pytest

import intersect_shape_cases as SH
import tree_shapes as T
from overlap_shape_cases import seams
from test_gpu_clearance import INF, check_forms, item_run, self_run, table
from test_gpu_tree_shapes import Shape, shapes   # noqa: F401  (the fixture: one resident scene per shape for this module)

pytestmark = pytest.mark.gpu

F = np.float32
REACH = F(1.0)
ALL_UP_TO, FIXED = 5000, 128


def case(s):
    corners = s.corners()
    queries = SH.shape_triangles(s.tree, corners, s.tree.box, 90 + T.NAMES.index(s.name))
    if len(corners) > ALL_UP_TO:
        queries = queries[:FIXED]
    return corners, table(("shape", s.name), queries, corners.reshape(-1))


@pytest.mark.parametrize("name", T.NAMES)
def test_every_record_and_count(pkg, gpu, shapes, name):
    s = shapes(name)
    corners, (queries, d2, shared) = case(s)
    pos = corners.reshape(-1)
    triangles = len(corners)
    _, n = check_forms(item_run(s.scene, queries, REACH), queries, pos, d2, shared, REACH, False, name, ks=(0, 1, 8, 9, 64))
    if triangles > 64:
        assert (n == 0).sum() >= 5 and (n > 8).mean() > 0.2 and (n > 64).sum() >= 1, (name, (n == 0).sum(), (n > 8).mean(), n.max())
        # a query beside a seam has members on both sides of it
        joints = [t for t in seams(s.tree) if 0 < t < triangles]
        member = d2 <= REACH
        assert any((member[:, t - 1] & member[:, t]).any() for t in joints), name
    check_forms(item_run(s.scene, queries, INF), queries, pos, d2, shared, INF, False, name, ks=(1, 9))
    check_forms(item_run(s.scene, queries, REACH, True), queries, pos, d2, shared, REACH, True, name + ", SKIP_SHARED", ks=(0, 8))


@pytest.mark.parametrize("name", T.NAMES)
def test_the_self_form_across_a_seam(pkg, gpu, shapes, name):
    s = shapes(name)
    corners = s.corners()
    pos = corners.reshape(-1)
    triangles = len(corners)
    joints = [t for t in seams(s.tree) if 0 < t < triangles] or [0]
    middle = min(joints, key=lambda t: abs(t - triangles // 2))
    count = min(130, triangles)
    first = int(np.clip(middle - count // 2, 0, triangles - count))
    own, d2, shared = table(("shape own", name), corners[first:first + count], pos)
    for skip in (True, False):
        _, n = check_forms(self_run(s.scene, first, count, REACH, skip), own, pos, d2, shared, REACH, skip, f"{name}, self, SKIP_SHARED {skip}",
                           ks=(0, 1, 9))
        assert skip or (n >= 1).all()
    check_forms(self_run(s.scene, first, count, INF, True), own, pos, d2, shared, INF, True, f"{name}, self, +inf", ks=(1,))
