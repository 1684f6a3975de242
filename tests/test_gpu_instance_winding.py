"""Instanced winding numbers on the GPU (include/shader_ray_instance_winding.h) against the restatement
(tests/instance_winding_ref.py), bit for bit (a NaN is any NaN): the mixed-wave set of tests/test_gpu_instance_sdf.py (scenes of
three heights, maps of every kind, an exact duplicate, points of every kind) for beta 2, 0.5 and the exact mode on the host
form, the device form and torch tensors, and against the composition a caller would write from the public calls; the
winding-signed distance with its record and instance buffers kept and omitted, and a count that takes two scratch chunks; point
counts 1, 63, 64 and 65; one identity instance against Scene.winding_number; overflowing and non-finite points; a device refit,
a device update that turns a rotation into a mirror and the query on one side stream, the same by a host update, and a first
derivation on a side stream followed by a default-stream query; 260 distinct one-leaf members, so that the per-slot pointer
table takes two launches; the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import instance_point_cases as IC
import instance_point_ref as IP
import instance_ref as IR
import instance_winding_ref as IW
import point_query_ref as R
import refit_ref
import sdf_ref as S
import winding_ref as WR
from helpers import single_leaf_scene
from test_gpu_instance_sdf import assert_records, dev_points, host_records
from test_gpu_point_query import loaded, make_points, scene_path
from test_gpu_signed_distance import assert_same_floats, moved_lobed

pytestmark = pytest.mark.gpu

F = np.float32
EYE = IC.EYE
BETAS = (2.0, 0.5, math.inf)
_members = {}
_sets = []


def leaf_restated(hand, tris):
    """winding_ref.Restated of a hand-made scene of one leaf: its one node's box is the scene's"""
    t = len(tris)
    tree = refit_ref.TreeArrays(np.array([-1], np.int32), np.array([-1], np.int32), np.array([-1], np.int32),
                                np.concatenate([hand.keep["bmin"][0], hand.keep["bmax"][0]]).astype(F)[None], np.zeros((1, 3), F),
                                np.array([0], np.int32), np.array([t], np.int32), np.arange(3 * t, dtype=np.int32).reshape(t, 3))
    return WR.Restated.of_tree(tree, np.asarray(tris, F).reshape(-1), tree.box)


def member(pkg, tmp_path_factory, name):
    """(winding_ref.Restated, resident scene) of a named member: the cube as a scene file of its own, the 11-triangle leaf as
    a hand-shaped tree, lobed_528 as the other tests load it.  The scene's node records are the restatement's."""
    if name not in _members:
        if name == "lobed_528":
            _, sc = loaded(pkg, name)
            world = pkg.World(scene_path(name))
            _members[name] = (WR.Restated(world), sc, world, False)
        elif name == "cube":
            path = str(tmp_path_factory.mktemp("instance_winding") / "cube.trisrc")
            pkg.scenes.write_trisrc(path, *S.cube())
            world = pkg.World(path)
            _members[name] = (WR.Restated(world), pkg.Scene(world.flatten()), world, True)
        else:
            tris = np.asarray(IC.TINY[name], F)
            hand = single_leaf_scene(tris)
            _members[name] = (leaf_restated(hand, tris), pkg.Scene(hand.desc), hand, True)
        ref, sc = _members[name][:2]
        assert_same_floats(sc.winding_data(), ref.records, f"{name}: node records")
    return _members[name][0], _members[name][1]


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    for s in _sets:
        s.close()
    _sets.clear()
    for ref, sc, keep, own in _members.values():
        if own:
            sc.close()
    _members.clear()


def number_device(s, pts, beta, containing=True, stream=None):
    """winding_number_into on the current torch stream (or `stream`): (values, containing or None) as numpy"""
    import torch
    n = len(pts)
    d_pts = dev_points(pts)
    d_out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    d_in = torch.full((n,), -7, dtype=torch.int32, device="cuda") if containing else None
    st = stream or torch.cuda.current_stream()
    s.winding_number_into(d_pts.data_ptr(), n, d_out.data_ptr(), d_in.data_ptr() if containing else 0, beta, st.cuda_stream)
    st.synchronize()
    return d_out.cpu().numpy(), d_in.cpu().numpy() if containing else None


def signed_device(s, pts, beta, records=True, instances=True, stream=None):
    """winding_signed_distance_into: (values, records or None, instances or None) as numpy"""
    import torch
    n = len(pts)
    d_pts = dev_points(pts)
    d_out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    d_rec = torch.full((n, 8), -7, dtype=torch.int32, device="cuda") if records else None
    d_inst = torch.full((n,), -7, dtype=torch.int32, device="cuda") if instances else None
    st = stream or torch.cuda.current_stream()
    s.winding_signed_distance_into(d_pts.data_ptr(), n, d_out.data_ptr(), d_rec.data_ptr() if records else 0,
                                   d_inst.data_ptr() if instances else 0, beta, st.cuda_stream)
    st.synchronize()
    return d_out.cpu().numpy(), host_records(d_rec) if records else None, d_inst.cpu().numpy() if instances else None


# the mixed-wave set ----------------------------------------------------------------------------------------------------------
NAMES = ["cube", "11-triangle leaf", "lobed_528"]
KINDS = list(IC.MAP_KINDS[:4]) + ["identity"] + list(IC.MAP_KINDS[4:])       # instance 4 becomes the duplicate of instance 1


@pytest.fixture(scope="module")
def mixed(pkg, gpu, tmp_path_factory):
    """the set, its 333 points and the restatement's answers, computed once"""
    members = [member(pkg, tmp_path_factory, n)[0] for n in NAMES]
    positions = [m.positions for m in members]
    of, maps, kinds = IC.make_set(positions, [i % 3 for i in range(9)], seed=26, spread=1.2, kinds=KINDS)
    assert set(kinds) == set(IC.MAP_KINDS) | {"duplicate of 1"} and of[4] == of[1]
    s = pkg.tracer.InstanceSet([member(pkg, tmp_path_factory, NAMES[k])[1] for k in of], maps)
    _sets.append(s)
    pts, kind, radius = IC.world_points(positions, of, maps, 333, seed=27)
    W = s.world_to_object()
    want = {beta: IW.winding_over_instances(members, of, W, pts, beta) for beta in BETAS}
    closest = IP.closest_over_instances(positions, of, maps, pts)
    signed = {beta: IW.winding_signed_over_instances(members, of, maps, W, pts, beta, closest=closest)[0] for beta in BETAS}
    return dict(s=s, members=members, positions=positions, of=of, maps=maps, pts=pts, W=W, want=want, closest=closest, signed=signed)


def test_the_mixed_set_is_mixed(mixed):
    """what the other tests rest on: the orientations, both signs of the sum, overlaps, NaN for the non-finite points, every
    instance containing some point, and waves whose adjacent lanes are nearest different instances"""
    m = mixed
    s = m["s"]
    assert np.array_equal(s.orientations(), IW.orientations(m["W"])) and (s.orientations() == -1).sum() >= 1
    w, containing = m["want"][math.inf]
    finite = np.isfinite(m["pts"]["p"]).all(1)
    assert np.array_equal(np.isnan(w), ~finite) and (~finite).sum() > 10
    assert (w > 0.5).sum() > 20 and (np.abs(w) < 0.5).sum() > 50 and (containing >= 0).sum() > 20 and (containing[~finite] == -1).all()
    inst = m["closest"][1]
    for first in range(0, 320, 64):
        lanes = inst[first:first + 64]
        held = lanes[lanes >= 0]
        assert len(set(held.tolist())) >= 4 and (held[1:] != held[:-1]).mean() > 0.5
    signed = m["signed"][2.0]
    assert (signed < 0).sum() > 5 and (signed > 0).sum() > 50 and np.isnan(signed).sum() > 30


@pytest.mark.parametrize("beta", BETAS)
def test_every_form_equals_the_restatement(mixed, beta):
    import torch
    m = mixed
    s, pts = m["s"], m["pts"]
    want, want_in = m["want"][beta]
    got, containing = s.winding_number(pts, beta=beta, containing=True)
    assert got.dtype == F and containing.dtype == np.int32
    assert_same_floats(got, want, f"beta {beta}, host form")
    assert np.array_equal(containing, want_in), f"beta {beta}, host form: containing"
    assert_same_floats(s.winding_number(pts, beta=beta), want, f"beta {beta}, host form without containing")
    got, containing = number_device(s, pts, beta)
    assert_same_floats(got, want, f"beta {beta}, device form")
    assert np.array_equal(containing, want_in), f"beta {beta}, device form: containing"
    assert_same_floats(number_device(s, pts, beta, containing=False)[0], want, f"beta {beta}, device form without containing")
    t_out, t_in = s.winding_number(dev_points(pts), beta=beta, containing=True)
    assert t_out.dtype == torch.float32 and tuple(t_out.shape) == (333,) and t_in.dtype == torch.int32 and t_out.is_cuda
    torch.cuda.current_stream().synchronize()
    assert_same_floats(t_out.cpu().numpy(), want, f"beta {beta}, tensors")
    assert np.array_equal(t_in.cpu().numpy(), want_in), f"beta {beta}, tensors: containing"
    p3 = torch.from_numpy(np.ascontiguousarray(pts["p"])).cuda()
    only = s.winding_number(p3, beta=beta)
    torch.cuda.current_stream().synchronize()
    assert_same_floats(only.cpu().numpy(), want, f"beta {beta}, [n, 3] tensor")
    for count in (1, 63, 64, 65):
        assert_same_floats(s.winding_number(pts[:count], beta=beta), want[:count], f"beta {beta}, host form, {count} points")
        got, containing = number_device(s, pts[:count], beta)
        assert_same_floats(got, want[:count], f"beta {beta}, device form, {count} points")
        assert np.array_equal(containing, want_in[:count])


@pytest.mark.parametrize("beta", BETAS)
def test_it_is_the_composition_of_the_public_calls(pkg, tmp_path_factory, mixed, beta):
    """world_to_object for the object point, the member's Scene.winding_number for the term, the orientation for its sign, and
    an fp32 accumulation in instance order"""
    m = mixed
    s, pts = m["s"], m["pts"]
    W, orient = s.world_to_object(), s.orientations()
    p = np.ascontiguousarray(pts["p"])
    live = np.isfinite(p).all(1)
    acc = np.zeros(int(live.sum()), F)
    first = np.full(int(live.sum()), -1, np.int32)
    for i in range(len(W)):
        with np.errstate(all="ignore"):
            p_o = IR.object_vectors(W[i], p[live], True)
        w_i = member(pkg, tmp_path_factory, NAMES[m["of"][i]])[1].winding_number(pkg.tracer.make_points(p_o), beta=beta)
        t = -w_i if orient[i] < 0 else w_i
        with np.errstate(all="ignore"):
            acc = (acc + t).astype(F)
            first = np.where((first < 0) & (t > F(0.5)), np.int32(i), first).astype(np.int32)
    want = np.full(len(p), np.nan, F)
    want_in = np.full(len(p), -1, np.int32)
    want[live], want_in[live] = acc, first
    got, containing = s.winding_number(pts, beta=beta, containing=True)
    assert_same_floats(got, want, f"beta {beta}: the composition")
    assert np.array_equal(containing, want_in)


@pytest.mark.parametrize("beta", BETAS)
def test_winding_signed_values_and_records(mixed, beta):
    import torch
    m = mixed
    s, pts = m["s"], m["pts"]
    want = m["signed"][beta]
    rec0, inst0 = s.closest_points(pts)
    assert_records(rec0, inst0, *m["closest"], "closest_points is the restatement")
    got, rec, inst = s.winding_signed_distance(pts, beta=beta, closest=True)
    assert got.dtype == F and rec.dtype == R.CLOSEST_DTYPE and inst.dtype == np.int32
    assert_records(rec, inst, rec0, inst0, f"beta {beta}, host form")
    assert_same_floats(got, want, f"beta {beta}, host form")
    assert_same_floats(s.winding_signed_distance(pts, beta=beta), want, f"beta {beta}, host form without records")
    for records, instances in ((True, True), (False, True), (True, False), (False, False)):
        got, rec, inst = signed_device(s, pts, beta, records, instances)
        what = f"beta {beta}, records {'kept' if records else 'omitted'}, instances {'kept' if instances else 'omitted'}"
        assert_same_floats(got, want, what)
        if records:
            assert np.array_equal(R.as_bits(rec), R.as_bits(rec0)), what
        if instances:
            assert np.array_equal(inst, inst0), what
    t_out, t_rec, t_inst = s.winding_signed_distance(dev_points(pts), beta=beta, closest=True)
    torch.cuda.current_stream().synchronize()
    assert_records(host_records(t_rec), t_inst.cpu().numpy(), rec0, inst0, f"beta {beta}, tensors")
    assert_same_floats(t_out.cpu().numpy(), want, f"beta {beta}, tensors")
    for count in (1, 63, 64, 65):
        assert_same_floats(signed_device(s, pts[:count], beta, False, False)[0], want[:count], f"beta {beta}, {count} points")


def test_a_count_split_over_two_scratch_chunks(pkg, gpu, tmp_path_factory):
    """2^22 + 1000 points with neither buffer kept on a one-leaf set: the records' scratch holds 2^22 points, so the query
    runs as two chunks.  Far points with radius 0 are misses (NaN); the second chunk's points and real points scattered over
    the first are restated."""
    import torch
    ref, leaf = member(pkg, tmp_path_factory, "11-triangle leaf")
    of, maps, _ = IC.make_set([ref.positions], [0, 0], seed=41, spread=1.0, kinds=["shear", "mirror"])
    s = pkg.tracer.InstanceSet([leaf, leaf], maps)
    _sets.append(s)
    n = (1 << 22) + 1000
    real, _, _ = IC.world_points([ref.positions], of, maps, 1000 + 2048, seed=42)
    tail, spread = real[:1000], real[1000:]
    far = np.zeros(1, R.POINT_DTYPE)
    far["p"] = (1e6, -2e6, 3e6)
    far["max_dist2"] = 0.0
    d_pts = dev_points(far).repeat(n, 1)
    d_pts[n - 1000:] = dev_points(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 1000, 2048, replace=False)).cuda()
    d_pts[sample] = dev_points(spread)
    d_out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    s.winding_signed_distance_into(d_pts.data_ptr(), n, d_out.data_ptr(), 0, 0, 2.0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    W = s.world_to_object()
    want = IW.winding_signed_over_instances([ref], of, maps, W, tail)[0]
    assert np.isfinite(want).sum() > 300
    assert_same_floats(d_out[n - 1000:].cpu().numpy(), want, "the second chunk's points")
    assert_same_floats(d_out[sample].cpu().numpy(), IW.winding_signed_over_instances([ref], of, maps, W, spread)[0], "points of the first chunk")
    rest = torch.ones(n - 1000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    assert bool(torch.isnan(d_out[: n - 1000][rest]).all())


# one identity instance -------------------------------------------------------------------------------------------------------
def test_one_identity_instance_is_the_winding_query(pkg, gpu):
    arrays, sc = loaded(pkg, "lobed_528")
    s = pkg.tracer.InstanceSet([sc], EYE[None])
    _sets.append(s)
    assert np.array_equal(s.orientations(), [1.0])
    pts = make_points(arrays, 3000, seed=5)
    for beta in BETAS:
        want = sc.winding_number(pts, beta=beta)
        assert np.isnan(want).sum() > 0 and (want > 0.5).sum() > 50
        got, containing = s.winding_number(pts, beta=beta, containing=True)
        assert_same_floats(got, want, f"identity, beta {beta}, host form")
        assert np.array_equal(containing, np.where(want > F(0.5), 0, -1))
        assert_same_floats(number_device(s, pts, beta)[0], want, f"identity, beta {beta}, device form")
    want, want_rec = sc.winding_signed_distance(pts, closest=True)
    got, rec, inst = s.winding_signed_distance(pts, closest=True)
    assert_records(rec, inst, want_rec, np.where(want_rec["triangle"] >= 0, 0, -1), "identity, winding-signed records")
    assert_same_floats(got, want, "identity, winding-signed, host form")
    assert_same_floats(signed_device(s, pts, 2.0)[0], want, "identity, winding-signed, device form")


# overflowing and non-finite points -------------------------------------------------------------------------------------------
def test_overflowing_and_non_finite_points(pkg, gpu, tmp_path_factory):
    """The cube grown by 2^20 and the cube squeezed to 2^-70 along x: a world point at x = 2^60 has a finite object point in the
    first and none in the second, whose term is NaN, and so is the sum; its signed value is +sqrtf(dist2)."""
    ref, cube = member(pkg, tmp_path_factory, "cube")
    squeezed = EYE.copy()
    squeezed[0, 0] = F(2.0 ** -70)
    maps = np.stack([(EYE * F(2.0 ** 20)).astype(F), squeezed])
    s = pkg.tracer.InstanceSet([cube, cube], maps)
    _sets.append(s)
    W = s.world_to_object()
    assert W[1, 0, 0] == F(2.0 ** 70) and W[0, 0, 0] == F(2.0 ** -20)
    p = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [2.0 ** 60, 0.5, 0.5], [-2.0 ** 62, 0.25, 2.0]], F)
    pts = pkg.tracer.make_points(p)
    for beta in (2.0, math.inf):
        want, want_in = IW.winding_over_instances([ref], [0, 0], W, pts, beta)
        assert np.isnan(want).all() and (want_in == -1).all()
        for got, containing in (s.winding_number(pts, beta=beta, containing=True), number_device(s, pts, beta)):
            assert_same_floats(got, want, f"overflow, beta {beta}")
            assert np.array_equal(containing, want_in)
        want, want_rec, want_inst = IW.winding_signed_over_instances([ref], [0, 0], maps, W, pts, beta)
        assert np.isnan(want[:3]).all() and (want[3:] > 0).all()
        for got, rec, inst in (s.winding_signed_distance(pts, beta=beta, closest=True), signed_device(s, pts, beta)):
            assert_records(rec, inst, want_rec, want_inst, f"overflow, beta {beta}")
            assert_same_floats(got, want, f"overflow, winding-signed, beta {beta}")
    # each instance alone, where the other's overflow does not hide it
    alone = pkg.tracer.InstanceSet([cube], maps[:1])
    _sets.append(alone)
    q = pkg.tracer.make_points(np.array([[2.0 ** 19, 2.0 ** 19, 2.0 ** 19], [2.0 ** 60, 0.5, 0.5], [-3.0, 0.5, 0.5]], F))
    want, want_in = IW.winding_over_instances([ref], [0], alone.world_to_object(), q, 2.0)
    assert want[0] > 0.9 and np.isfinite(want).all() and np.array_equal(want_in, [0, -1, -1])
    got, containing = alone.winding_number(q, containing=True)
    assert_same_floats(got, want, "the grown cube alone")
    assert np.array_equal(containing, want_in)


# stream order ----------------------------------------------------------------------------------------------------------------
def lobed_moved(world):
    """(the lobed sphere's corners moved, the restatement of the refit scene)"""
    pos = moved_lobed(np.asarray(world.arrays()["vertex_positions"], F).reshape(-1, 3))
    tree = refit_ref.TreeArrays.of(world.export_tree())
    return pos, WR.Restated(world, positions=pos, boxes=refit_ref.node_boxes(tree, pos))


def test_refit_update_and_query_on_one_side_stream_then_a_host_update(pkg, gpu, tmp_path_factory):
    """A device refit of a member, a device update that turns instance 0's rotation into a mirror and the two queries,
    enqueued on one side stream with nothing between them: the queries see the new geometry, node records re-derived from it,
    the new W and its orientation (a stale orientation would flip instance 0's terms, stale records would move them).  Then
    the old maps again by a host update."""
    import torch
    world = pkg.World(scene_path("lobed_528"))
    own = pkg.Scene(world.flatten())            # a scene of its own: it is refit below
    cube_ref, cube = member(pkg, tmp_path_factory, "cube")
    before = WR.Restated(world)
    pos, after = lobed_moved(world)
    of = [0, 1, 0]
    rng = np.random.default_rng(90)
    positions = [after.positions, cube_ref.positions]
    maps0 = np.stack([IC.map_of(k, rng, positions[of[i]], 0.8) for i, k in enumerate(("rotation_uniform", "shear", "translation"))]).astype(F)
    maps1 = maps0.copy()
    maps1[0] = IC.map_of("mirror", rng, positions[0], 0.8).astype(F)
    s = pkg.tracer.InstanceSet([own if k == 0 else cube for k in of], maps0)
    try:
        pts, _, _ = IC.world_points(positions, of, maps1, 1500, seed=91)
        first = s.winding_number(pts)            # (derives the records of the old geometry)
        assert_same_floats(first, IW.winding_over_instances([before, cube_ref], of, s.world_to_object(), pts)[0], "before the refit")
        assert np.array_equal(s.orientations(), [1.0, 1.0, 1.0])
        n = len(pts)
        d_moved, d_maps, d_pts = torch.from_numpy(pos).cuda(), torch.from_numpy(maps1).cuda(), dev_points(pts)
        d_out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        d_in = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        d_signed = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            own.refit(d_moved, stream_ptr=side.cuda_stream)
            s.update_into(d_maps.data_ptr(), side.cuda_stream)
            s.winding_number_into(d_pts.data_ptr(), n, d_out.data_ptr(), d_in.data_ptr(), 2.0, side.cuda_stream)
            s.winding_signed_distance_into(d_pts.data_ptr(), n, d_signed.data_ptr(), 0, 0, 2.0, side.cuda_stream)
        side.synchronize()
        assert s.update_status() == -1
        assert np.array_equal(s.orientations(), [-1.0, 1.0, 1.0])
        members = [after, cube_ref]
        W = s.world_to_object()
        want, want_in = IW.winding_over_instances(members, of, W, pts)
        assert_same_floats(d_out.cpu().numpy(), want, "one side stream")
        assert np.array_equal(d_in.cpu().numpy(), want_in), "one side stream: containing"
        assert_same_floats(d_signed.cpu().numpy(), IW.winding_signed_over_instances(members, of, maps1, W, pts)[0], "one side stream, winding-signed")
        assert (~(np.isnan(first) | (first.view(np.uint32) == want.view(np.uint32)))).sum() > 300, "the refit and the update moved something"
        stale = IW.winding_over_instances(members, of, W, pts, signs=[1.0, 1.0, 1.0])[0]
        assert (np.abs(stale - want) > 0.5).sum() > 20, "a stale orientation would have flipped values"
        # the old maps again, by a host update
        s.update(maps0)
        assert np.array_equal(s.orientations(), [1.0, 1.0, 1.0])
        want, want_in = IW.winding_over_instances(members, of, s.world_to_object(), pts)
        got, containing = s.winding_number(pts, containing=True)
        assert_same_floats(got, want, "after the host update")
        assert np.array_equal(containing, want_in)
        assert_same_floats(number_device(s, pts, 2.0)[0], want, "after the host update, device form")
    finally:
        s.close()
        own.close()
        world.close()


def test_records_first_derived_on_a_side_stream_then_a_default_stream_query(pkg, gpu):
    """The first winding query of a set over a fresh scene runs on a side stream, so the member's node records are derived
    there; with no synchronisation a query on the default stream must wait for it on the device."""
    import torch
    world = pkg.World(scene_path("lobed_528"))
    fresh = pkg.Scene(world.flatten())
    ref = WR.Restated(world)
    _, maps, _ = IC.make_set([ref.positions], [0, 0, 0], seed=95, spread=0.8, kinds=["shear", "mirror", "rotation_nonuniform"])
    s = pkg.tracer.InstanceSet([fresh] * 3, maps)
    try:
        pts, _, _ = IC.world_points([ref.positions], [0, 0, 0], maps, 1500, seed=96)
        d_pts = dev_points(pts)
        d_side = torch.full((len(pts),), -7.0, dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            s.winding_number_into(d_pts.data_ptr(), len(pts), d_side.data_ptr(), 0, 2.0, side.cuda_stream)
        d_main = s.winding_number(d_pts)
        want = IW.winding_over_instances([ref], [0, 0, 0], s.world_to_object(), pts)[0]
        torch.cuda.current_stream().synchronize()
        assert_same_floats(d_main.cpu().numpy(), want, "default stream after a side-stream derivation")
        side.synchronize()
        assert_same_floats(d_side.cpu().numpy(), want, "the side stream's own query")
        assert (want > 0.5).sum() > 30 and (want < -0.5).sum() > 5
    finally:
        s.close()
        fresh.close()
        world.close()


# the pointer table's second launch -------------------------------------------------------------------------------------------
def test_260_distinct_members_take_two_table_launches(pkg, gpu):
    """260 one-leaf tetrahedra, each a scene of its own, 5 apart along x and of different sizes, slot j wound inward when
    (j + (j >> 8)) & 1.  A point inside tetrahedron j gets +-1 from it and about 0 from the others.  With the node records
    of a neighbouring slot, or of slot j - 256, tetrahedron j is far from its own inside points and adds about 0, so a
    wrong table entry changes the sum."""
    pos, tri = S.tetrahedron()
    scenes, members, hands, inside = [], [], [], []
    count = 260
    try:
        for j in range(count):
            v = (pos * F(0.8 + 0.4 * (j % 7) / 6) + F([5.0 * j, 0.25 * (j % 3), 0])).astype(F)
            t = tri[:, ::-1] if (j + (j >> 8)) & 1 else tri
            tris = v[t]
            hand = single_leaf_scene(tris)
            hands.append(hand)
            scenes.append(pkg.Scene(hand.desc))
            members.append(leaf_restated(hand, tris))
            inside.append(v.mean(0))
        s = pkg.tracer.InstanceSet(scenes, np.tile(EYE, (count, 1, 1)))
        try:
            p = np.concatenate([np.array(inside, F), np.array(inside, F) + F([0, 5, 0])]).astype(F)
            pts = pkg.tracer.make_points(p)
            of = list(range(count))
            want, want_in = IW.winding_over_instances(members, of, s.world_to_object(), pts, 2.0)
            sign = np.array([-1.0 if (j + (j >> 8)) & 1 else 1.0 for j in range(count)])
            assert np.abs(want[:count] - sign).max() < 0.05 and np.abs(want[count:]).max() < 0.05
            assert np.array_equal(want_in[:count], np.where(sign > 0, np.arange(count), -1)) and (want_in[count:] == -1).all()
            # what a wrong table entry would give: slot j's walk with the records of slot j + 1 or j - 256
            for wrong, moved in ((lambda j: j + 1 if j + 1 < count else j - 1, slice(0, count)), (lambda j: j - 256 if j >= 256 else j, slice(256, count))):
                mixed_up = []
                for j in range(count):
                    m = leaf_restated(hands[j], members[j].positions.reshape(-1, 3, 3))
                    m.records = members[wrong(j)].records
                    mixed_up.append(m)
                other = IW.winding_over_instances(mixed_up, of, s.world_to_object(), pts, 2.0)[0]
                assert (np.abs(other[:count] - want[:count])[moved] > 0.5).all()
            got, containing = s.winding_number(pts, containing=True)
            assert_same_floats(got, want, "260 members, host form")
            assert np.array_equal(containing, want_in)
            got, containing = number_device(s, pts, 2.0)
            assert_same_floats(got, want, "260 members, device form")
            assert np.array_equal(containing, want_in)
            assert_same_floats(signed_device(s, pts, 2.0, False, False)[0],
                               IW.winding_signed_over_instances(members, of, np.tile(EYE, (count, 1, 1)), s.world_to_object(), pts, 2.0)[0],
                               "260 members, winding-signed")
        finally:
            s.close()
    finally:
        for sc in scenes:
            sc.close()


# refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops(pkg, gpu, mixed):
    """count 0 is a no-op; the binding refuses a tensor of the wrong shape; a NaN or negative beta and misaligned device
    buffers are argument errors"""
    import torch
    s = mixed["s"]
    assert len(s.winding_number(np.zeros((0, 3), F))) == 0 and len(s.winding_signed_distance(np.zeros((0, 3), F))) == 0
    with pytest.raises(ValueError):
        s.winding_number(torch.zeros((4, 5), device="cuda"))
    for beta in (math.nan, -1.0):
        with pytest.raises(pkg._native.ShrayError):
            s.winding_number(mixed["pts"], beta=beta)
        with pytest.raises(pkg._native.ShrayError):
            s.winding_signed_distance(mixed["pts"], beta=beta)
    lib = pkg._native.load_instance_winding()
    d = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    num, sgn, V = lib.shray_winding_number_instances_device, lib.shray_winding_signed_distance_instances_device, C.c_void_p
    base = d.data_ptr()
    assert num(s._handle, V(base + 4), 1, 2.0, V(base + 128), V(base + 96), None) == -1
    assert num(s._handle, V(base), 1, 2.0, V(base + 130), V(base + 96), None) == -1
    assert num(s._handle, V(base), 1, 2.0, V(base + 128), V(base + 98), None) == -1
    assert num(s._handle, V(base), 1, 2.0, V(base + 132), V(base + 100), None) == 0
    assert sgn(s._handle, V(base), 1, 2.0, V(base + 128), V(base + 40), V(base + 96), None) == -1
    assert sgn(s._handle, V(base), 1, 2.0, V(base + 128), V(base + 32), V(base + 98), None) == -1
    assert sgn(s._handle, V(base), 1, 2.0, V(base + 132), V(base + 32), V(base + 100), None) == 0
    assert sgn(s._handle, V(base), 0, 2.0, V(base + 128), None, None, None) == 0
    torch.cuda.synchronize()
