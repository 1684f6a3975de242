"""Triangle-intersection queries on the GPU over the hand-shaped trees of tests/tree_shapes.py (heights 0 to 16, siblings whose
heights differ by up to 14): every index and count against the restatement (tests/intersect_ref.py) through test_gpu_intersect's
check_forms, and the walk's own counters -- node visits, leaf visits, triangle tests -- against intersect_ref.walk_counters over
refit_ref.node_boxes, for the counting form at K = 0 and K = 8 and for the ANY form, each with and without SKIP_SHARED; then the
same after a refit to the twist and collapse deformations, on the host path and on the device path on a side stream.  The
queries are intersect_shape_cases.shape_triangles: among them the whole query, whose vertex box is the root's own box and whose
walk holds one stack entry per level at once.  The walk is a copy of the box-overlap walk (own LDS column, own push and pop,
ANY's break out of the leaf loop), so it is pinned as that one is (tests/test_gpu_overlap_tree_shapes.py) and against the same
DEEPEST table.  Nothing is tolerated: every counter is an equality."""
import numpy as np
import pytest

import intersect_ref as IR
import intersect_shape_cases as SH
import refit_ref as R
import tree_shapes as T
from overlap_shape_cases import deepest_stack
from test_gpu_intersect import assert_same, check_forms, item_run
from test_gpu_overlap_tree_shapes import DEEPEST
from test_gpu_refit import deform
from test_gpu_tree_shapes import Shape, shapes   # noqa: F401  (the fixture: one resident scene per shape for this module)

pytestmark = pytest.mark.gpu

F = np.float32
BATCH = 64          # the small batch whose counters are compared as a batch, as halves and, on the tiny shapes, query by query

_cases = {}


def case(s, deformation=None):
    """(vertex data, corners, node boxes, queries, member without and with SKIP_SHARED, walk_counters keyed by (any_only, skip))
    of a shape over its loaded or deformed vertices, once"""
    key = (s.name, deformation)
    if key not in _cases:
        vd = s.vertex_data if deformation is None else deform(s.vertex_data, deformation)
        corners = s.corners(vd)
        node_boxes = s.tree.box if deformation is None else R.node_boxes(s.tree, corners)
        seed = 90 + T.NAMES.index(s.name)
        if deformation is None:
            queries = SH.shape_triangles(s.tree, corners, node_boxes, seed)
        else:
            # fewer of them, and the loaded shape's queries too: where the triangles were.  After a collapse every triangle is one
            # point, a vertex box holds all of them or none and a walk that holds them visits every node.
            mine, loaded = (30, 50) if deformation == "collapse" else (250, 150)
            queries = np.concatenate([SH.shape_triangles(s.tree, corners, node_boxes, seed, small=100, own=30)[:mine], case(s)[3][:loaded]])
        member = {skip: IR.intersects(queries, corners.reshape(-1), skip) for skip in (False, True)}
        count = IR.walk_counters(s.tree, node_boxes, corners, queries)          # (the counting walk does not look at the flag)
        want = {(False, False): count, (False, True): count}
        for skip in (False, True):
            want[(True, skip)] = IR.walk_counters(s.tree, node_boxes, corners, queries, skip, True, member[skip])
        _cases[key] = (vd, corners, node_boxes, queries, member, want)
    return _cases[key]


def check_counters(s, corners, queries, member, want, what):
    """the host path's counters of the counting form (K = 0 and K = 8) and of ANY, each with and without SKIP_SHARED, against
    `want`: over all queries, over one small batch, over its halves and, on the two tiny shapes, query by query"""
    for skip in (False, True):
        n = member[skip].sum(1).astype(np.int32)
        for rows in ([np.array([i]) for i in range(min(BATCH, len(queries)))] if len(corners) <= 3 else []) + [np.arange(min(BATCH, len(queries))), np.arange(len(queries))]:
            for any_only, k in ((False, 0), (False, 8), (True, 0)):
                _, got_n, c = s.scene.intersecting_triangles(queries[rows], max_triangles=k, counters=True, any_only=any_only, skip_shared=skip)
                assert_same(got_n, (n[rows] > 0).astype(np.int32) if any_only else n[rows], what)
                for key in IR.COUNTERS:
                    assert c[key] == int(want[(any_only, skip)][key][rows].sum()), (
                        what, f"{len(rows)} queries from {rows[0]}", "ANY" if any_only else f"K = {k}", f"SKIP_SHARED {skip}", key, c,
                        {x: int(want[(any_only, skip)][x][rows].sum()) for x in IR.COUNTERS})
                assert c["samples"] == len(rows)
        for rows in (np.arange(BATCH // 2), np.arange(BATCH // 2, BATCH)):
            _, _, c = s.scene.intersecting_triangles(queries[rows], max_triangles=0, counters=True, skip_shared=skip)
            assert all(c[key] == int(want[(False, skip)][key][rows].sum()) for key in IR.COUNTERS), (what, rows[0], c)


@pytest.mark.parametrize("name", T.NAMES)
def test_every_index_count_and_counter(pkg, gpu, shapes, name):
    s = shapes(name)
    _, corners, node_boxes, queries, member, want = case(s)
    n = member[False].sum(1)
    triangles = len(corners)
    shares = (float((n == 0).mean()), float((n > 8).mean()), float((n > 64).mean()))
    if triangles > 64:
        assert shares[0] > 0.05 and shares[1] > 0.20 and shares[2] > 0.05, (name, shares)
    assert 900 <= len(queries) <= 1300 and (~IR.walked(queries)).sum() >= 30
    check_forms(item_run(s.scene, queries), member[False], name)
    check_forms(item_run(s.scene, queries, True), member[True], name + ", SKIP_SHARED", ks=(0, 3, 8, 64))
    assert 0 < member[True].sum() < member[False].sum()
    check_counters(s, corners, queries, member, want, name)
    deepest, height = int(want[(False, False)]["stack"].max()), int(T.heights(s.tree)[0])
    assert (deepest, height) == DEEPEST[name] and deepest == deepest_stack(s.tree), (name, deepest, height)
    # the whole query: its vertex box is the root's box, it reaches the deepest stack, and it meets what the restatement says of
    # the non-degenerate triangles (every one of them passes stage 0)
    lo, hi = queries[0].min(0), queries[0].max(0)
    assert (lo == node_boxes[0, :3]).all() and (hi == node_boxes[0, 3:]).all() and want[(False, False)]["stack"][0] == deepest, name
    code = IR.first_axis(queries[:1], corners.reshape(-1))[0]
    assert not np.isin(code, (0, 1, 2)).any() and not (code == IR.DEGENERATE).any() and n[0] == (code == IR.INTERSECT).sum() and (n[0] > 0 or triangles <= 3), name
    assert want[(False, False)]["triangle_tests"][0] == triangles and want[(False, False)]["node_visits"][0] == s.tree.node_count
    print(f"{name}: {triangles} triangles, {len(queries)} queries, n = 0 / > 8 / > 64: {shares[0]:.3f} / {shares[1]:.3f} / {shares[2]:.3f}, deepest stack "
          f"{deepest} of height {height}, the whole query meets {int(n[0])}, counting walk { {k: int(want[(False, False)][k].sum()) for k in IR.COUNTERS} }, "
          f"ANY { {k: int(want[(True, False)][k].sum()) for k in IR.COUNTERS} }")


@pytest.mark.parametrize("name", T.NAMES)
def test_after_a_refit(pkg, gpu, shapes, name):
    """twist on the host path, collapse on the device path on a side stream, then the other way round"""
    import torch
    s = shapes(name)
    stream = torch.cuda.Stream()
    try:
        for how, deformation in (("host", "twist"), ("device", "collapse"), ("host", "collapse"), ("device", "twist")):
            vd, corners, node_boxes, queries, member, want = case(s, deformation)
            what = f"{name}/{how}/{deformation}"
            s.refit(vd, how, stream)
            stream.synchronize()
            assert np.array_equal(s.scene.geometry()["vertex_positions"].view(np.uint32), corners.reshape(-1).view(np.uint32)), what
            check_forms(item_run(s.scene, queries), member[False], what, ks=(0, 1, 8, 9, 64))
            check_forms(item_run(s.scene, queries, True), member[True], what + ", SKIP_SHARED", ks=(0, 8))
            check_counters(s, corners, queries, member, want, what)
            n = member[False].sum(1)
            if deformation == "collapse":
                # every scene triangle is a point: never a member, and a walked query whose vertex box holds the point still visits
                # every node and tests every triangle, each test ending in the degenerate rule
                code = IR.first_axis(queries, corners.reshape(-1))
                visits = want[(False, False)]["triangle_tests"]
                assert not member[False].any() and (code[IR.walked(queries)] <= IR.DEGENERATE).all(), what
                assert ((code == IR.DEGENERATE).all(1) & (visits == len(corners))).sum() >= 5 and (visits[~IR.walked(queries)] == 0).all(), what
            else:
                assert (n > 0).sum() >= 20 and (n == 0).sum() >= 20, (what, int((n > 0).sum()))
    finally:
        s.refit(s.vertex_data)
