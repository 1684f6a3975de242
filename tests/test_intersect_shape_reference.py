"""The query triangles of tests/intersect_shape_cases.py on the CPU, with the restatement (tests/intersect_ref.py) alone, on two
small hand-shaped trees: the whole query's vertex box is the root's box, its walk enters every node and holds
overlap_shape_cases.deepest_stack(tree) entries, the greatest any walk of the tree holds; a face query is entered and the one a
float short of it is not; and the mix exercises the query."""
import numpy as np
import pytest

import intersect_ref as IR
import intersect_shape_cases as SH
import tree_shapes as T
from overlap_shape_cases import deepest_stack


@pytest.mark.parametrize("name", ["one_branch", "wide_by_one"])
def test_the_whole_query_reaches_the_deepest_stack(name):
    tree, vd = T.build(name)
    corners = np.ascontiguousarray(vd[tree.triangle_vertices][:, :, :3])
    queries = SH.shape_triangles(tree, corners, tree.box, seed=90 + T.NAMES.index(name))
    assert 900 <= len(queries) <= 1300 and (~IR.walked(queries)).sum() >= 30
    lo, hi = queries[0].min(0), queries[0].max(0)
    assert (lo == tree.box[0, :3]).all() and (hi == tree.box[0, 3:]).all() and IR.walked(queries[:1]).all()
    want = IR.walk_counters(tree, tree.box, corners, queries)
    assert want["stack"].max() == deepest_stack(tree) == want["stack"][0] == int(T.heights(tree)[0]), name
    assert want["node_visits"][0] == tree.node_count and want["triangle_tests"][0] == len(corners)
    assert (want["node_visits"][~IR.walked(queries)] == 0).all()
    # a vertex box that touches the root's face enters it (the root and its two children are tested); one float short does not
    faces = IR.walk_counters(tree, tree.box, corners, np.array(SH.face_triangles(tree.box[0]), np.float32))
    assert IR.walked(np.array(SH.face_triangles(tree.box[0]), np.float32)).all() and min(faces["node_visits"][:2]) >= 3 and faces["node_visits"][2] == 1, name
    code = IR.first_axis(queries, corners.reshape(-1))
    n = (code == IR.INTERSECT).sum(1)
    if len(corners) > 64:
        shares = (float((n == 0).mean()), float((n > 8).mean()), float((n > 64).mean()))
        print(f"{name}: n = 0 / > 8 / > 64: {shares}")
        assert shares[0] > 0.05 and shares[1] > 0.20 and shares[2] > 0.05, (name, shares)
        assert n[0] == (code[0] == IR.INTERSECT).sum() > 0 and not np.isin(code[0], (0, 1, 2)).any()     # every triangle passes the whole query's stage 0
    # ANY stops at the first member: never more work than the counting walk, and less somewhere
    member = code == IR.INTERSECT
    first = IR.walk_counters(tree, tree.box, corners, queries, any_only=True, member=member)
    assert (first["triangle_tests"] <= want["triangle_tests"]).all() and (first["triangle_tests"] < want["triangle_tests"]).any()
    assert np.array_equal(first["triangle_tests"][n == 0], want["triangle_tests"][n == 0])
