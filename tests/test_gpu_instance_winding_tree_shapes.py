"""Instanced winding numbers on the GPU over the hand-shaped trees of tests/tree_shapes.py (a root that is a leaf, heights that
sit on the edges of the bottom-up schedule, a lopsided spine).  The members are open soups with four triangles in ten wound the
other way, so the sums are no integers and every far term counts.  Per shape, one instance under the five maps of
tests/test_gpu_instance_point_tree_shapes.py and 1,024 points, for beta 2 and the exact mode, bit for bit against the
restatement (tests/instance_winding_ref.py); the exact mode's restatement sums every triangle for every point, so on the shapes
above 5,000 triangles it is compared on the first 128 of the points (tests/test_gpu_tree_shapes.py does the same with a
quarter).  Then one set of 24 instances over the seven shapes, lobed_528 and the one-triangle scene (member heights 0 to 16 share
one launch's LDS layout), values, containing instances and winding-signed distances; and that set again after two shapes are
refit ("twist", "collapse") and the set is updated on the host, which must re-derive the members' node records."""
import math

import numpy as np
import pytest

import instance_point_cases as IC
import instance_point_ref as IP
import instance_winding_ref as IW
import tree_shapes as T
import winding_ref as WR
from helpers import single_leaf_scene
from test_gpu_instance_point_tree_shapes import MAP_KINDS, POINTS, one_map
from test_gpu_instance_sdf import assert_records
from test_gpu_instance_winding import leaf_restated, number_device, signed_device
from test_gpu_point_query import loaded, scene_path
from test_gpu_refit import deform
from test_gpu_signed_distance import assert_same_floats
from test_gpu_tree_shapes import shapes     # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

F = np.float32
EXACT_POINTS = 128      # of a shape above 5,000 triangles, in the exact mode
SET_EXACT_POINTS = 32  # of the 24-instance set, in the exact mode


def points_for(beta, triangles):
    return EXACT_POINTS if math.isinf(beta) and triangles > 5000 else POINTS


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MAP_KINDS)
@pytest.mark.parametrize("name", T.NAMES)
def test_one_instance_of_a_shape_under_a_map(pkg, gpu, shapes, name, kind):
    s = shapes(name)
    ref, _ = s.restated()
    seed = T.NAMES.index(name) * 10 + MAP_KINDS.index(kind)
    what = f"{name}, {kind}"
    maps = one_map(kind, np.random.default_rng(300 + seed), ref.positions)[None]
    iset = pkg.tracer.InstanceSet([s.scene], maps)
    try:
        pts, _, _ = IC.world_points([ref.positions], [0], maps, POINTS, seed=seed)
        W = iset.world_to_object()
        assert np.array_equal(iset.orientations(), IW.orientations(W))
        assert iset.orientations()[0] == np.sign(np.linalg.det(maps[0, :, :3].astype(np.float64))), what
        for beta in (2.0, math.inf):
            n = points_for(beta, len(s.tree.triangle_vertices))
            want, want_in = IW.winding_over_instances([ref], [0], W, pts[:n], beta)
            assert np.isnan(want).sum() > 0 and np.isfinite(want).sum() > 0.8 * n, what
            got, containing = iset.winding_number(pts[:n], beta=beta, containing=True)
            assert_same_floats(got, want, f"{what}, beta {beta}, host form")
            assert np.array_equal(containing, want_in), f"{what}, beta {beta}, host form: containing"
            got, containing = number_device(iset, pts[:n], beta)
            assert_same_floats(got, want, f"{what}, beta {beta}, device form")
            assert np.array_equal(containing, want_in), f"{what}, beta {beta}, device form: containing"
    finally:
        iset.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_a_mixed_set_of_every_shape_and_after_a_refit(pkg, gpu, shapes):
    world = pkg.World(scene_path("lobed_528"))
    tris = np.asarray(IC.TINY["one triangle"], F)
    hand = single_leaf_scene(tris)
    one = pkg.Scene(hand.desc)
    members = [shapes(n).restated()[0] for n in T.NAMES] + [WR.Restated(world), leaf_restated(hand, tris)]
    scenes = [shapes(n).scene for n in T.NAMES] + [loaded(pkg, "lobed_528")[1], one]
    heights = [int(T.heights(shapes(n).tree).max()) for n in T.NAMES]
    assert min(heights) == 0 and max(heights) >= 13, heights
    n = 24
    of, maps, kinds = IC.make_set([m.positions for m in members], [i % len(members) for i in range(n)], seed=24, spread=1.2)
    assert set(of) == set(range(len(members))) and set(kinds) >= set(IC.MAP_KINDS)
    iset = pkg.tracer.InstanceSet([scenes[k] for k in of], maps)
    twisted, collapsed = T.NAMES.index("wide_by_one"), T.NAMES.index("mixed_spine")

    def check(pts, what):
        W = iset.world_to_object()
        assert np.array_equal(iset.orientations(), IW.orientations(W)), what
        for beta, count in ((2.0, len(pts)), (math.inf, SET_EXACT_POINTS)):
            want, want_in = IW.winding_over_instances(members, of, W, pts[:count], beta)
            got, containing = iset.winding_number(pts[:count], beta=beta, containing=True)
            assert_same_floats(got, want, f"{what}, beta {beta}, host form")
            assert np.array_equal(containing, want_in), f"{what}, beta {beta}: containing"
            got, containing = number_device(iset, pts[:count], beta)
            assert_same_floats(got, want, f"{what}, beta {beta}, device form")
            assert np.array_equal(containing, want_in), f"{what}, beta {beta}, device form: containing"
        closest = IP.closest_over_instances([m.positions for m in members], of, maps, pts, device="cuda")
        signed = IW.winding_signed_over_instances(members, of, maps, W, pts, 2.0, closest=closest)[0]
        got, rec, inst = iset.winding_signed_distance(pts, closest=True)
        assert_records(rec, inst, *closest, f"{what}, winding-signed records")
        assert_same_floats(got, signed, f"{what}, winding-signed, host form")
        assert_same_floats(signed_device(iset, pts, 2.0, False, False)[0], signed, f"{what}, winding-signed, buffers omitted")
        return IW.winding_over_instances(members, of, W, pts, 2.0)

    try:
        pts, _, _ = IC.world_points([m.positions for m in members], of, maps, POINTS, seed=25)
        want, want_in = check(pts, "24 instances of every shape")
        assert len(set(want_in[want_in >= 0].tolist())) >= 3 and (np.abs(want[np.isfinite(want)]) > 0.05).sum() >= 100
        before = iset.winding_number(pts)
        # two members move, and the set follows by a host update that keeps the maps: the node records must be derived anew
        for k, how in ((twisted, "twist"), (collapsed, "collapse")):
            s = shapes(T.NAMES[k])
            vd = deform(s.vertex_data, how)
            s.refit(vd)
            members[k] = s.restated(vd)[0]
        point = members[collapsed].positions.reshape(-1, 3)
        assert (point == point[0]).all(), "a collapsed member is one point"
        iset.update()
        pts2, _, _ = IC.world_points([m.positions for m in members], of, maps, POINTS, seed=26)
        check(pts2, "24 instances after the refits")
        after = iset.winding_number(pts)
        assert (before.view(np.uint32) != after.view(np.uint32)).sum() > 20, "the refits moved something"
        assert_same_floats(after, IW.winding_over_instances(members, of, iset.world_to_object(), pts, 2.0)[0], "the first points after the refits")
    finally:
        iset.close()
        one.close()
        world.close()
        for k in (twisted, collapsed):
            s = shapes(T.NAMES[k])
            s.refit(s.vertex_data)
