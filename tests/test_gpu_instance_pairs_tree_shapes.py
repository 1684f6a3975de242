"""The instance-pair collision matrix on the GPU over the hand-shaped trees of tests/tree_shapes.py (a root that is a leaf,
heights that sit on the edges of the bottom-up schedule, a lopsided spine).  Per shape, the scene placed twice: under the
identity, and under a rotation with non-uniform scale whose translation puts the image of the shape's centre on the centre, so
that the two interpenetrate.  Both off-diagonal cells in the three modes on both paths against the brute force
(instance_pairs_ref.member_pairs: the larger shapes have 2^14 triangles, too many for a dense table on the host), and the
counting form's node_visits, leaf_visits, triangle_tests and traversals EQUAL to the sum of the two ordered pairs' restated walks
(instance_pairs_ref.pair_walk_counters) with the stored boxes as read back."""
import numpy as np
import pytest

import instance_pairs_ref as PR
import instance_point_ref as IP
import test_gpu_instance_point as G
import tree_shapes as T
from test_gpu_instance_overlap import stored_boxes
from test_gpu_instance_pairs import assert_cells, run, wanted
from test_gpu_instance_point_tree_shapes import one_map
from test_gpu_tree_shapes import shapes     # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

F = np.float32


def placed_twice(name, positions):
    """maps [2, 3, 4]: the identity, and a rotation with non-uniform scale that keeps the centroid of the shape's middle triangle
    where it is (to fp32 rounding): that triangle and its image, two triangles in different planes through one inner point,
    cross each other, and so do their neighbours along the shape"""
    M = one_map("rotation_nonuniform", np.random.default_rng(900 + T.NAMES.index(name)), positions)
    tris = np.asarray(positions, np.float64).reshape(-1, 3, 3)
    centre = tris[len(tris) // 2].mean(0)
    M[:, 3] = (centre - M[:, :3].astype(np.float64) @ centre).astype(F)
    return np.stack([np.eye(3, 4, dtype=F), M.astype(F)])


def brute_of_two(positions, maps, skip_shared=False, device="cuda"):
    """(first uint64 [2, 2], counts int64 [2, 2]) of one scene placed twice, through member_pairs"""
    merged, start = IP.merged_positions([positions], [0, 0], maps)
    world = merged.reshape(-1, 3, 3)
    w = [world[start[0]:start[1]], world[start[1]:start[2]]]
    first, counts = np.full((2, 2), PR.NONE, np.uint64), np.zeros((2, 2), np.int64)
    for a, b in ((0, 1), (1, 0)):
        first[a, b], counts[a, b] = PR.brute_of_pairs(*PR.member_pairs(w[a], w[b], skip_shared, device))
    return (first, counts), w


@pytest.mark.parametrize("name", T.NAMES)
def test_a_shape_placed_twice(pkg, gpu, shapes, name):
    s = shapes(name)
    corners = s.corners()
    positions = corners.reshape(-1)
    maps = placed_twice(name, positions)
    iset = pkg.tracer.InstanceSet([s.scene, s.scene], maps)
    try:
        G.assert_contained(pkg, iset, [positions, positions], maps, name)
        brute, world = brute_of_two(positions, maps)
        print(name, len(corners), "triangles, counts", brute[1].tolist())
        assert brute[1][0, 1] > 0 and brute[1][1, 0] > 0 and brute[1][0, 0] == brute[1][1, 1] == 0, "the two interpenetrate"
        for mode in PR.MODES:
            for path in ("host", "device"):
                assert_cells(run(iset, mode, path), wanted(brute, mode), f"{name}, {mode}, {path}")
            assert_cells(run(iset, mode, "device", upper=True), wanted((np.where([[0, 1], [0, 0]], brute[0], PR.NONE),
                                                                        np.where([[0, 1], [0, 0]], brute[1], 0)), mode), f"{name}, {mode}, UPPER")
        stored = stored_boxes(pkg, iset, 2)
        total = dict.fromkeys(PR.COUNTERS, 0)
        for a, b in ((0, 1), (1, 0)):
            w, go = PR.pair_walk_counters(s.tree, s.tree.box, world[b], maps[b], world[a], stored[b])
            for c in PR.COUNTERS:
                total[c] += w[c]
        ta, tb, cnt, tally = iset.collision_pairs(counters=True)
        assert np.array_equal(cnt, brute[1]) and np.array_equal(ta, PR.split_keys(brute[0])[0]) and np.array_equal(tb, PR.split_keys(brute[0])[1])
        for c in PR.COUNTERS:
            assert tally[c] == total[c], (name, c, tally, total)
        assert tally["samples"] == 2 * len(corners)
    finally:
        iset.close()
