"""Instanced signed distance queries on the GPU where the sign can go wrong (the cases of tests/instance_sdf_cases.py, pinned on
the CPU by tests/test_instance_sdf_cases_reference.py), byte for byte against the restatement (tests/instance_sdf_ref.py):

  - the hollow member, a box with a spike-shaped cavity, under the eight kinds of map and an exact duplicate: both signs at every
    one of the seven pseudonormal slots and points that only the right slot signs right, on the host form, the device form and
    the counting form, and against the composition of closest_points, world_to_object and the member's Scene.signed_distance at
    {p_o, +inf} (the seed's claim).  A failure names the wrong variant of instance_sdf_ref.WRONG_VARIANTS that reproduces the
    GPU's values, if one does.  The member is one leaf that keeps hollow()'s triangle order, which the pinned figures are of (a
    vertex's ties go to its lowest triangle, so another order gives other slots); the same mesh as a built tree of several
    leaves is compared too.
  - the peel loop: 72 one-leaf members on a grid and waves of 64 distinct instances in descending order and in a permutation, a
    wave whose only hit is lane 63, one whose only hit is lane 0, an all-miss wave and a partial last wave.
  - more than 256 scene slots: 260 distinct one-leaf tetrahedra, neighbours and slots 256 apart wound opposite ways, so that a
    sign-data pointer from another slot flips the sign (store_sign_slots' second launch)."""
import numpy as np
import pytest

import instance_ref as IR
import instance_sdf_cases as C
import instance_sdf_ref as IS
import point_query_ref as R
import sdf_ref as S
from helpers import single_leaf_scene
from test_gpu_instance_sdf import assert_records, assert_values, device_form, same_floats

pytestmark = pytest.mark.gpu

F = np.float32
_open = []
_hands = []      # the hand-built descriptors' arrays live as long as the module


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    for thing in reversed(_open):      # the sets before their member scenes
        thing.close()
    _open.clear()
    _hands.clear()


def keep(thing):
    _open.append(thing)
    return thing


def leaf_scene(pkg, positions):
    """a resident one-leaf scene of the triangles, in their order"""
    hand = single_leaf_scene(np.asarray(positions, F).reshape(-1, 3, 3))
    _hands.append(hand)
    return keep(pkg.Scene(hand.desc))


# the hollow member -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["one leaf, hollow()'s order", "a built tree"])
def hollow(request, pkg, gpu, tmp_path_factory):
    """the set, the points and the restatement's intermediate results with the set's own W, once"""
    _, of, maps, kinds = C.hollow_set()
    if request.param == "a built tree":
        path = str(tmp_path_factory.mktemp("instance_sdf_edges") / "hollow.trisrc")
        pkg.scenes.write_trisrc(path, *C.hollow())
        world = keep(pkg.World(path))
        positions = np.asarray(world.arrays()["vertex_positions"], F).reshape(-1).copy()
        scene = keep(pkg.Scene(world.flatten()))
        assert sorted(map(bytes, positions.reshape(-1, 9))) == sorted(map(bytes, S.corners_of(*C.hollow()).reshape(-1, 9)))
    else:
        positions = S.corners_of(*C.hollow())
        scene = leaf_scene(pkg, positions)
    assert scene.surface_info()["closed"] == 1
    s = keep(pkg.tracer.InstanceSet([scene] * len(of), maps))
    assert s.closed()
    pts, _ = C.hollow_points()
    W = s.world_to_object()
    parts = IS.signed_parts([positions], of, maps, W, pts)
    want, want_rec, want_inst = IS.signed_over_instances([positions], of, maps, W, pts, device="cuda")
    assert np.array_equal(R.as_bits(want_rec), R.as_bits(parts["records"])) and np.array_equal(want_inst, parts["instances"])
    assert same_floats(IS.values_of(parts), want).all()
    pinned = request.param != "a built tree"
    if pinned:   # the CPU test's conditions, with the set's own W
        figures, changed = C.slot_figures(parts), C.changed_by(parts)
        print(figures, changed)
        assert min(figures["negative"]) >= 5 and min(figures["positive"]) >= 5 and min(figures["decided"][1:]) >= 15 and min(changed.values()) >= 15
    return dict(s=s, scene=scene, positions=positions, of=of, maps=maps, pts=pts, W=W, parts=parts, want=want, want_rec=want_rec,
                want_inst=want_inst, what=request.param)


def assert_hollow_values(h, got, what):
    bad = np.nonzero(~same_floats(got, h["want"]))[0]
    if len(bad):
        named = C.reproduced_by(h["parts"], got)
        slots = IS.object_slots(h["parts"])[1][bad]
        raise AssertionError(
            f"{h['what']}, {what}: {len(bad)} of {len(got)} values differ, first {bad[:5]}: got {np.asarray(got)[bad[:5]]} want {h['want'][bad[:5]]}; "
            f"by slot {dict(zip(C.SLOTS, np.bincount(slots, minlength=7).tolist()))}; "
            + (f"these are the values of the wrong variant {named}" if named else "no named wrong variant gives these values"))


def test_the_hollow_member_on_every_form(hollow):
    h = hollow
    s, pts = h["s"], h["pts"]
    got, rec, inst = s.signed_distance(pts, closest=True)
    assert_records(rec, inst, h["want_rec"], h["want_inst"], "host form")
    assert_hollow_values(h, got, "host form")
    got, rec, inst = device_form(s, pts)
    assert_records(rec, inst, h["want_rec"], h["want_inst"], "device form")
    assert_hollow_values(h, got, "device form")
    got, _, _ = device_form(s, pts, records=False, instances=False)
    assert_hollow_values(h, got, "device form, buffers omitted")
    got, rec, inst, c = s.signed_distance(pts, closest=True, counters=True)
    assert_records(rec, inst, h["want_rec"], h["want_inst"], "counting form")
    assert_hollow_values(h, got, "counting form")
    assert c["traversals"] == len(pts) == int((h["want_inst"] >= 0).sum()) and c["samples"] == len(pts)


def test_the_hollow_member_is_the_composition_of_the_public_calls(pkg, hollow):
    """closest_points for the magnitude, world_to_object for the object point, the member's Scene.signed_distance at {p_o, +inf}
    for the sign: the seeded walk must return the +inf walk's record"""
    h = hollow
    s, pts = h["s"], h["pts"]
    rec, inst = s.closest_points(pts)
    W = s.world_to_object()
    with np.errstate(all="ignore"):
        d = np.sqrt(rec["dist2"])
    want = np.where(inst >= 0, d, F(np.nan)).astype(F)
    for i in sorted(set(inst[inst >= 0].tolist())):
        at = np.nonzero(inst == i)[0]
        with np.errstate(all="ignore"):
            p_o = IR.object_vectors(W[i], pts["p"][at], True)
        sigma = h["scene"].signed_distance(pkg.tracer.make_points(p_o))
        with np.errstate(invalid="ignore"):
            want[at] = np.where((sigma < 0) & (rec["dist2"][at] > 0), -d[at], d[at])
    got, got_rec, got_inst = s.signed_distance(pts, closest=True)
    assert_records(got_rec, got_inst, rec, inst, "the closest part is closest_points")
    assert_values(got, want, f"{h['what']}: the composition")
    assert_hollow_values(h, want, "the composition against the restatement")


# the peel shapes -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def peel(pkg, gpu):
    positions, of, maps = C.peel_set()
    scenes = [leaf_scene(pkg, p) for p in positions]
    s = keep(pkg.tracer.InstanceSet([scenes[k] for k in of], maps))
    pts, wanted = C.peel_points()
    want, want_rec, want_inst = IS.signed_over_instances(positions, of, maps, s.world_to_object(), pts)
    C.assert_peel_shapes(want_inst, wanted)
    return dict(s=s, of=of, pts=pts, want=want, want_rec=want_rec, want_inst=want_inst)


def test_the_peel_waves(peel):
    m = peel
    got, rec, inst = device_form(m["s"], m["pts"])
    assert_records(rec, inst, m["want_rec"], m["want_inst"], "the peel waves, device form")
    assert_values(got, m["want"], "the peel waves, device form")
    for w, name in enumerate(C.PEEL_WAVES):
        lanes = slice(64 * w, 64 * w + 64)
        assert_values(got[lanes], m["want"][lanes], f"wave {w} ({name})")
    got, rec, inst = device_form(m["s"], m["pts"], records=False, instances=False)
    assert rec is None and inst is None
    assert_values(got, m["want"], "the peel waves, buffers omitted")
    got, rec, inst = m["s"].signed_distance(m["pts"], closest=True)
    assert_records(rec, inst, m["want_rec"], m["want_inst"], "the peel waves, host form")
    assert_values(got, m["want"], "the peel waves, host form")


def test_the_peel_waves_count_one_walk_per_hit(peel):
    m = peel
    got, c = m["s"].signed_distance(m["pts"], counters=True)
    assert_values(got, m["want"], "the peel waves, counting form")
    hits = int((m["want_inst"] >= 0).sum())
    assert c["traversals"] == hits == 157 and c["samples"] == len(m["pts"])
    assert c["leaf_visits"] == hits and c["node_visits"] == hits, "every member is one leaf: the root and nothing else"
    assert c["triangle_tests"] == sum(4 if m["of"][i] % 2 == 0 else 12 for i in m["want_inst"][m["want_inst"] >= 0])


# more than 256 scene slots ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(pkg, gpu):
    positions, of, maps, pts = C.many_scene_set()
    scenes = [leaf_scene(pkg, p) for p in positions]
    s = keep(pkg.tracer.InstanceSet(scenes, maps))
    return dict(s=s, positions=positions, of=of, maps=maps, pts=pts)


def test_more_than_256_scene_slots(many):
    """every slot's sign-data pointer is its own scene's: the table's second launch writes slots 256 to 259"""
    m = many
    s, pts = m["s"], m["pts"]
    want, want_rec, want_inst = IS.signed_over_instances(m["positions"], m["of"], m["maps"], s.world_to_object(), pts)
    C.assert_many_scene_shapes(want, want_inst)
    for lo, hi in ((0, 256), (256, C.MANY_SCENES)):
        part = want[2 * lo:2 * hi:2]       # the inside points of these slots
        assert (part < 0).any() and (part > 0).any(), (lo, hi)
    got, rec, inst = device_form(s, pts)
    assert_records(rec, inst, want_rec, want_inst, "260 scenes, device form")
    bad = np.nonzero(~same_floats(got, want))[0]
    assert len(bad) == 0, f"260 scenes: the values of slots {sorted(set((bad // 2).tolist()))[:12]} differ: got {got[bad[:6]]} want {want[bad[:6]]}"
    got, rec, inst = s.signed_distance(pts, closest=True)
    assert_records(rec, inst, want_rec, want_inst, "260 scenes, host form")
    assert_values(got, want, "260 scenes, host form")
    # a second query of the same set: the table is staged anew for every query
    got, _, _ = device_form(s, pts[::-1].copy(), records=False, instances=False)
    assert_values(got, want[::-1], "260 scenes, the points reversed, buffers omitted")
