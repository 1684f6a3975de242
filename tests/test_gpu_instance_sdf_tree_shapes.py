"""Instanced signed distance queries on the GPU over the hand-shaped trees of tests/tree_shapes.py (a root that is a leaf,
heights that sit on the edges of the bottom-up schedule, a lopsided spine).  The members are open soups with four triangles in
ten wound the other way; their sign data is whatever the derivation says of them (sdf_ref.derive restates it), which is the
point: the sign kernel's seeded walk and its slot lookup run on trees and sign data no closed mesh gives.  Per shape, one
instance under the five maps of tests/test_gpu_instance_point_tree_shapes.py and 1,024 points: every byte against the
restatement (tests/instance_sdf_ref.py) and against the composition with the member's cold Scene.signed_distance at
{p_o, +inf}; the counting form walks once per hit and visits no more bounds and tests no more triangles than cold
closest_points walks of the same object points.  Then that file's set of 24 instances over the seven shapes, lobed_528 and the
one-triangle scene (member heights 0 to 16 in one launch's LDS layout): bytes, again after two shapes are refit ("twist",
"collapse") and the set is updated on the host, which must re-derive the members' sign data; a collapsed member's triangles are
one point, it has no sign vector, and every value on it is the restatement's positive one."""
import numpy as np
import pytest

import instance_point_cases as IC
import instance_ref as IR
import instance_sdf_ref as IS
import sdf_ref as S
import test_gpu_instance_point as G
import tree_shapes as T
from test_gpu_instance_point_tree_shapes import MAP_KINDS, POINTS, one_map
from test_gpu_instance_sdf import assert_records, assert_values, device_form
from test_gpu_refit import deform
from test_gpu_tree_shapes import shapes     # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

F = np.float32
_sign_data = {}


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    for s in G._sets:
        s.close()
    G._sets.clear()
    for _, sc in G._members.values():
        sc.close()
    G._members.clear()
    _sign_data.clear()


def sign_data_of(name, positions):
    """sdf_ref.derive's sign data of a shape's loaded vertices, once per module"""
    if name not in _sign_data:
        _sign_data[name] = S.derive(positions)["sign_data"]
    return _sign_data[name]


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MAP_KINDS)
@pytest.mark.parametrize("name", T.NAMES)
def test_one_instance_of_a_shape_under_a_map(pkg, gpu, shapes, name, kind):
    s = shapes(name)
    positions = s.corners().reshape(-1)
    seed = T.NAMES.index(name) * 10 + MAP_KINDS.index(kind)
    what = f"{name}, {kind}"
    M = one_map(kind, np.random.default_rng(300 + seed), positions)
    maps = M[None]
    iset = pkg.tracer.InstanceSet([s.scene], maps)
    try:
        assert not iset.closed()
        pts, _, _ = IC.world_points([positions], [0], maps, POINTS, seed=seed)
        W = iset.world_to_object()
        want, want_rec, want_inst = IS.signed_over_instances([positions], [0], maps, W, pts, device="cuda",
                                                             sign_data=[sign_data_of(name, positions)])
        hit = want_inst >= 0
        assert 0.3 < hit.mean() < 0.97, (what, hit.mean())
        assert (want[hit] < 0).sum() >= 30 and (want[hit] > 0).sum() >= 30, (what, (want < 0).sum(), (want > 0).sum())
        got, rec, inst = iset.signed_distance(pts, closest=True)
        assert_records(rec, inst, want_rec, want_inst, f"{what}, host form")
        assert_values(got, want, f"{what}, host form")
        got, rec, inst = device_form(iset, pts)
        assert_records(rec, inst, want_rec, want_inst, f"{what}, device form")
        assert_values(got, want, f"{what}, device form")
        # the composition: the member's cold signed distance at {p_o, +inf}
        with np.errstate(all="ignore"):
            p_o = IR.object_vectors(W[0], pts["p"][hit], True)
            d = np.sqrt(want_rec["dist2"][hit])
        assert np.isfinite(p_o).all()
        cold = pkg.tracer.make_points(p_o)
        sigma = s.scene.signed_distance(cold)
        composed = want.copy()
        composed[hit] = np.where((sigma < 0) & (want_rec["dist2"][hit] > 0), -d, d)
        assert_values(got, composed, f"{what}: the composition")
        # the counters: one sign walk per hit, within cold walks of the same object points
        got, rec, inst, c = iset.signed_distance(pts, closest=True, counters=True)
        assert_records(rec, inst, want_rec, want_inst, f"{what}, counting form")
        assert_values(got, want, f"{what}, counting form")
        _, cc = s.scene.closest_points(cold, counters=True)
        hits = int(hit.sum())
        assert c["traversals"] == hits and c["samples"] == len(pts), (what, c)
        assert hits <= c["node_visits"] <= cc["node_visits"] and hits <= c["triangle_tests"] <= cc["triangle_tests"], (what, c, cc)
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

    def check(pts, what):
        want, want_rec, want_inst = IS.signed_over_instances(positions, of, maps, iset.world_to_object(), pts, device="cuda")
        got, rec, inst = iset.signed_distance(pts, closest=True)
        assert_records(rec, inst, want_rec, want_inst, f"{what}, host form")
        assert_values(got, want, f"{what}, host form")
        got, rec, inst = device_form(iset, pts)
        assert_records(rec, inst, want_rec, want_inst, f"{what}, device form")
        assert_values(got, want, f"{what}, device form")
        got, _, _ = device_form(iset, pts, records=False, instances=False)
        assert_values(got, want, f"{what}, buffers omitted")
        return want, want_inst

    try:
        pts, _, _ = IC.world_points(positions, of, maps, POINTS, seed=25)
        want, want_inst = check(pts, "24 instances of every shape")
        assert len(set(want_inst[want_inst >= 0].tolist())) >= 12 and (want < 0).sum() >= 30 and (want > 0).sum() >= 30
        before = iset.signed_distance(pts)
        # two members move, and the set follows by a host update that keeps the maps: the sign data must be derived anew
        for k, how in ((twisted, "twist"), (collapsed, "collapse")):
            s = shapes(T.NAMES[k])
            vd = deform(s.vertex_data, how)
            s.refit(vd)
            positions[k] = s.corners(vd).reshape(-1)
        point = positions[collapsed].reshape(-1, 3)
        assert (point == point[0]).all(), "a collapsed member is one point"
        assert not S.derive(positions[collapsed])["sign_data"].any(), "and has no sign vector"
        iset.update()
        pts2, _, _ = IC.world_points(positions, of, maps, POINTS, seed=26)
        want2, want_inst2 = check(pts2, "24 instances after the refits")
        on_the_point = np.isin(want_inst2, [i for i, k in enumerate(of) if k == collapsed])
        on_the_twisted = np.isin(want_inst2, [i for i, k in enumerate(of) if k == twisted])
        assert on_the_point.sum() >= 5 and (want2[on_the_point] >= 0).all(), "no value on a collapsed member is negative"
        assert on_the_twisted.sum() >= 5
        after = iset.signed_distance(pts)
        assert (before.view(np.uint32) != after.view(np.uint32)).sum() > 20, "the refits moved something"
        assert_values(after, IS.signed_over_instances(positions, of, maps, iset.world_to_object(), pts, device="cuda")[0],
                      "the first points after the refits")
    finally:
        iset.close()
        for k in (twisted, collapsed):
            s = shapes(T.NAMES[k])
            s.refit(s.vertex_data)
