"""Instanced closest-point queries on the GPU over the hand-shaped trees of tests/tree_shapes.py (a root that is a leaf, heights
that sit on the edges of the bottom-up schedule, a lopsided spine).  Per shape, one instance under a rotation with non-uniform
scale, a mirror, a shear, a signed permutation with a translation and the identity: every byte against the restatement, and the
counting form's node_visits, leaf_visits, triangle_tests and traversals EQUAL to instance_point_ref.walk_counters, which
restates instance_walk one point at a time over the tree and refit_ref.node_boxes (a one-instance set never consults its top
level and lanes do not interact, so the sum over the points is exact); under the identity also Scene.closest_points' own
counters.  Then one set of 24 instances over the seven shapes, lobed_528 and the one-triangle scene (member heights 0 to 16 in
one launch's LDS layout): bytes and containment, again after two shapes are refit ("twist", "collapse") and the set is updated
on the host; a collapsed member's triangles are one point, every pair of it ties, and its lowest triangle must win."""
import numpy as np
import pytest

import instance_point_cases as IC
import instance_point_ref as IP
import refit_ref
import test_gpu_instance_point as G
import tree_shapes as T
from test_gpu_instance_point import assert_answer, assert_contained, check_both_paths
from test_gpu_refit import deform
from test_gpu_tree_shapes import shapes     # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

F = np.float32
MAP_KINDS = ("rotation_nonuniform", "mirror", "shear", "signed_permutation_translated", "identity")
POINTS = 1024
COUNTERS = ("node_visits", "leaf_visits", "triangle_tests", "traversals")


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    for s in G._sets:
        s.close()
    G._sets.clear()
    for _, sc in G._members.values():
        sc.close()
    G._members.clear()


def one_map(kind, rng, positions):
    if kind == "signed_permutation_translated":
        lo, hi = IC.extent_of(positions)
        M = IC.map_of("signed_permutation", rng, positions, 1.5)
        M[:, 3] = np.round(rng.uniform(-1.5, 1.5, 3) * float((hi - lo).max()) * 8) / 8
        return M.astype(F)
    return IC.map_of(kind, rng, positions, 1.5).astype(F)


def restate(positions, of, maps, pts):
    pairs = len(pts) * sum(len(positions[s]) // 9 for s in of)
    return IP.closest_over_instances(positions, of, maps, pts, device="cuda" if pairs > G.NUMPY_PAIRS else None)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MAP_KINDS)
@pytest.mark.parametrize("name", T.NAMES)
def test_one_instance_of_a_shape_under_a_map(pkg, gpu, shapes, name, kind):
    s = shapes(name)
    corners = s.corners()
    positions = corners.reshape(-1)
    boxes = refit_ref.node_boxes(s.tree, corners)
    seed = T.NAMES.index(name) * 10 + MAP_KINDS.index(kind)
    what = f"{name}, {kind}"
    M = one_map(kind, np.random.default_rng(300 + seed), positions)
    maps = M[None]
    iset = pkg.tracer.InstanceSet([s.scene], maps)
    try:
        assert_contained(pkg, iset, [positions], maps, what)
        pts, _, _ = IC.world_points([positions], [0], maps, POINTS, seed=seed)
        want, want_inst = restate([positions], [0], maps, pts)
        hits = float((want["triangle"] >= 0).mean())
        assert 0.3 < hits < 0.97, (what, hits)
        check_both_paths(pkg, iset, pts, want, want_inst, what)
        got, inst, c = iset.closest_points(pts, counters=True)
        assert_answer(got, inst, want, want_inst, f"{what}, counting form")
        w = IP.walk_counters(s.tree, boxes, corners, M, pts, device="cuda")
        assert np.array_equal(w["triangle"], want["triangle"]), f"{what}: the restated walk's own answer"
        for k in COUNTERS:
            assert c[k] == int(w[k].sum()), (what, k, c, {x: int(w[x].sum()) for x in COUNTERS})
        assert c["samples"] == len(pts)
        if kind == "identity":
            _, plain = s.scene.closest_points(pts, counters=True)
            for k in ("node_visits", "leaf_visits", "triangle_tests"):
                assert plain[k] == int(w[k].sum()), (what, k, plain)
    finally:
        iset.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_a_mixed_set_of_every_shape_and_after_a_refit(pkg, gpu, shapes):
    members = [(shapes(n).corners().reshape(-1), shapes(n).scene) for n in T.NAMES] + [G.member(pkg, "lobed_528"), G.member(pkg, "one triangle")]
    heights = [int(T.heights(shapes(n).tree).max()) for n in T.NAMES]
    assert min(heights) == 0 and max(heights) >= 13, heights
    n = 24
    positions = [m[0] for m in members]
    of, maps, kinds = IC.make_set(positions, [i % len(members) for i in range(n)], seed=24, spread=1.2)
    assert set(of) == set(range(len(members))) and set(kinds) >= set(IC.MAP_KINDS)
    iset = pkg.tracer.InstanceSet([members[k][1] for k in of], maps)
    twisted, collapsed = T.NAMES.index("wide_by_one"), T.NAMES.index("mixed_spine")
    try:
        what = "24 instances of every shape"
        assert_contained(pkg, iset, [positions[k] for k in of], maps, what)
        pts, _, _ = IC.world_points(positions, of, maps, POINTS, seed=25)
        want, want_inst = restate(positions, of, maps, pts)
        check_both_paths(pkg, iset, pts, want, want_inst, what)
        assert len(set(want_inst[want_inst >= 0].tolist())) >= 12
        # two members move, and the set follows by a host update that keeps the maps
        for k, how in ((twisted, "twist"), (collapsed, "collapse")):
            s = shapes(T.NAMES[k])
            vd = deform(s.vertex_data, how)
            s.refit(vd)
            positions[k] = s.corners(vd).reshape(-1)
        point = positions[collapsed].reshape(-1, 3)
        assert (point == point[0]).all(), "a collapsed member is one point"
        iset.update()
        what = "24 instances after the refits"
        assert_contained(pkg, iset, [positions[k] for k in of], maps, what)
        pts, _, _ = IC.world_points(positions, of, maps, POINTS, seed=26)
        want2, want_inst2 = restate(positions, of, maps, pts)
        check_both_paths(pkg, iset, pts, want2, want_inst2, what)
        got, inst = iset.closest_points(pts)
        assert_answer(got, inst, want2, want_inst2, what)
        on_the_point = np.isin(inst, [i for i, k in enumerate(of) if k == collapsed])
        assert on_the_point.sum() >= 5 and (got["triangle"][on_the_point] == 0).all(), "every pair of a collapsed member ties: triangle 0"
    finally:
        iset.close()
        for k in (twisted, collapsed):
            s = shapes(T.NAMES[k])
            s.refit(s.vertex_data)
