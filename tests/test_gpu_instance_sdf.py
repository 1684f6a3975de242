"""Instanced signed distance queries on the GPU (include/shader_ray_instance_sdf.h) against the restatement
(tests/instance_sdf_ref.py), byte for byte: one set whose waves mix instances, scenes of three heights, maps of every kind, an
exact duplicate, and points of every kind and radius class, on the host form, the device form and torch tensors, and against
the composition of the public calls; the device form with its record and instance buffers omitted, and a count that takes two
scratch chunks; one identity instance against Scene.signed_distance; an object point that overflows; a refit, a device update
and the query on one side stream, and a first derivation on a side stream followed by a default-stream query; the seed's work
against cold walks; the refusals."""
import ctypes as C

import numpy as np
import pytest

import instance_point_cases as IC
import instance_ref as IR
import instance_sdf_ref as IS
import point_query_ref as R
import sdf_ref as S
from helpers import single_leaf_scene
from test_gpu_point_query import BAD_TREE, loaded, make_points, scene_path

pytestmark = pytest.mark.gpu

F = np.float32
EYE = IC.EYE
_members = {}
_sets = []


def member(pkg, tmp_path_factory, name):
    """(vertex_positions, resident scene) of a named member: the cube as a scene file of its own, the 11-triangle leaf as a
    hand-shaped tree, lobed_528 as the other tests load it"""
    if name == "lobed_528":
        arrays, sc = loaded(pkg, name)
        return np.asarray(arrays["vertex_positions"], F).reshape(-1), sc
    if name not in _members:
        if name == "cube":
            path = str(tmp_path_factory.mktemp("instance_sdf") / "cube.trisrc")
            pkg.scenes.write_trisrc(path, *S.cube())
            world = pkg.World(path)
            _members[name] = (np.asarray(world.arrays()["vertex_positions"], F).reshape(-1).copy(), pkg.Scene(world.flatten()), world)
        else:
            tris = np.asarray(IC.TINY[name], F)
            hand = single_leaf_scene(tris)
            _members[name] = (tris.reshape(-1), pkg.Scene(hand.desc), hand)
    return _members[name][0], _members[name][1]


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    for s in _sets:
        s.close()
    _sets.clear()
    for entry in _members.values():
        entry[1].close()
    _members.clear()


def same_floats(got, want):
    g, w = np.ascontiguousarray(got, F).reshape(-1), np.ascontiguousarray(want, F).reshape(-1)
    return g.view(np.uint32) == w.view(np.uint32)


def assert_values(got, want, what):
    bad = np.nonzero(~same_floats(got, want))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} values differ, first {bad[:5]}: got {np.asarray(got)[bad[:5]]} want {want[bad[:5]]}"


def assert_records(got, got_inst, want, want_inst, what):
    bad = np.nonzero((R.as_bits(got) != R.as_bits(want)).any(1) | (np.asarray(got_inst) != want_inst))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} records differ, first {bad[:5]}: got {got[bad[:3]]} want {want[bad[:3]]}"


def dev_points(pts):
    import torch
    return torch.from_numpy(np.ascontiguousarray(pts).view(F).reshape(-1, 4).copy()).cuda()


def host_records(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1)


def device_form(s, pts, records=True, instances=True, stream=None):
    """signed_distance_into on the current torch stream (or `stream`): (values, records or None, instances or None) as numpy"""
    import torch
    n = len(pts)
    d_pts = dev_points(pts)
    d_out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    d_rec = torch.full((n, 8), -7, dtype=torch.int32, device="cuda") if records else None
    d_inst = torch.full((n,), -7, dtype=torch.int32, device="cuda") if instances else None
    st = stream or torch.cuda.current_stream()
    s.signed_distance_into(d_pts.data_ptr(), n, d_out.data_ptr(), d_rec.data_ptr() if records else 0, d_inst.data_ptr() if instances else 0,
                           st.cuda_stream)
    st.synchronize()
    return d_out.cpu().numpy(), host_records(d_rec) if records else None, d_inst.cpu().numpy() if instances else None


# the mixed-wave set ----------------------------------------------------------------------------------------------------------
NAMES = ["cube", "11-triangle leaf", "lobed_528"]
KINDS = list(IC.MAP_KINDS[:4]) + ["identity"] + list(IC.MAP_KINDS[4:])       # instance 4 becomes the duplicate of instance 1


@pytest.fixture(scope="module")
def mixed(pkg, gpu, tmp_path_factory):
    """the set, its 333 points and the restatement's answer, computed once"""
    positions = [member(pkg, tmp_path_factory, n)[0] for n in NAMES]
    of, maps, kinds = IC.make_set(positions, [i % 3 for i in range(9)], seed=26, spread=1.2, kinds=KINDS)
    assert set(kinds) == set(IC.MAP_KINDS) | {"duplicate of 1"} and of[4] == of[1] and np.array_equal(maps[4].view(np.uint32), maps[1].view(np.uint32))
    s = pkg.tracer.InstanceSet([member(pkg, tmp_path_factory, NAMES[k])[1] for k in of], maps)
    _sets.append(s)
    pts, kind, radius = IC.world_points(positions, of, maps, 333, seed=27)
    W = s.world_to_object()
    want, want_rec, want_inst = IS.signed_over_instances(positions, of, maps, W, pts)
    return dict(s=s, positions=positions, of=of, maps=maps, pts=pts, kind=kind, radius=radius, W=W, want=want, want_rec=want_rec,
                want_inst=want_inst)


def test_the_mixed_set_is_mixed(mixed):
    """what the other tests rest on: every kind of point and radius, misses, both signs, and waves whose adjacent lanes hold
    different instances and different scenes"""
    m = mixed
    IC.assert_mixed(m["pts"], m["kind"], m["radius"], m["want_rec"], "the mixed set")
    want, inst = m["want"], m["want_inst"]
    assert np.isnan(want).sum() > 30 and (want < 0).sum() > 15 and (want > 0).sum() > 50 and (want == 0).sum() > 5
    assert np.array_equal(np.isnan(want), inst < 0)
    for first in range(0, 320, 64):      # the five full waves
        lanes = inst[first:first + 64]
        held = lanes[lanes >= 0]
        assert len(set(held.tolist())) >= 4 and len({m["of"][i] for i in held.tolist()}) == 3, (first, sorted(set(held.tolist())))
        assert (held[1:] != held[:-1]).mean() > 0.5, "adjacent lanes hold different instances"
    assert (inst == 1).sum() > 5 and (inst == 4).sum() == 0, "an exact duplicate never wins against the lower index"


def test_host_form_equals_the_restatement(mixed):
    m = mixed
    got, rec, inst = m["s"].signed_distance(m["pts"], closest=True)
    assert got.dtype == F and rec.dtype == R.CLOSEST_DTYPE and inst.dtype == np.int32
    assert_records(rec, inst, m["want_rec"], m["want_inst"], "host form")
    assert_values(got, m["want"], "host form")
    assert_values(m["s"].signed_distance(m["pts"]), m["want"], "host form without records")
    for count in (1, 63, 64, 65):
        assert_values(m["s"].signed_distance(m["pts"][:count]), m["want"][:count], f"host form, {count} points")


def test_device_form_and_tensors_equal_the_restatement(mixed):
    import torch
    m = mixed
    got, rec, inst = device_form(m["s"], m["pts"])
    assert_records(rec, inst, m["want_rec"], m["want_inst"], "device form")
    assert_values(got, m["want"], "device form")
    t_out, t_rec, t_inst = m["s"].signed_distance(dev_points(m["pts"]), closest=True)
    assert t_out.dtype == torch.float32 and tuple(t_out.shape) == (333,) and t_rec.dtype == torch.int32 and tuple(t_rec.shape) == (333, 8)
    assert t_inst.dtype == torch.int32 and t_out.is_cuda
    torch.cuda.current_stream().synchronize()
    assert_records(host_records(t_rec), t_inst.cpu().numpy(), m["want_rec"], m["want_inst"], "tensors")
    assert_values(t_out.cpu().numpy(), m["want"], "tensors")
    only = m["s"].signed_distance(dev_points(m["pts"]))
    torch.cuda.current_stream().synchronize()
    assert_values(only.cpu().numpy(), m["want"], "tensors without records")
    # [n, 3] points with one radius for all
    p3 = torch.from_numpy(np.ascontiguousarray(m["pts"]["p"])).cuda()
    both = m["s"].signed_distance(p3, max_dist2=0.01)
    torch.cuda.current_stream().synchronize()
    pts = m["pts"].copy()
    pts["max_dist2"] = 0.01
    assert_values(both.cpu().numpy(), IS.signed_over_instances(m["positions"], m["of"], m["maps"], m["W"], pts)[0], "one radius for all")


def test_it_is_the_composition_of_the_public_calls(pkg, tmp_path_factory, mixed):
    """closest_points for the magnitude, world_to_object for the object point, the member's Scene.signed_distance for the sign"""
    m = mixed
    s, pts = m["s"], m["pts"]
    rec, inst = s.closest_points(pts)
    W = s.world_to_object()
    with np.errstate(all="ignore"):
        d = np.sqrt(rec["dist2"])
    want = np.where(inst >= 0, d, F(np.nan)).astype(F)
    for i in sorted(set(inst[inst >= 0].tolist())):
        at = np.nonzero(inst == i)[0]
        with np.errstate(all="ignore"):
            p_o = IR.object_vectors(W[i], pts["p"][at], True)
        sigma = member(pkg, tmp_path_factory, NAMES[m["of"][i]])[1].signed_distance(pkg.tracer.make_points(p_o))
        with np.errstate(invalid="ignore"):
            want[at] = np.where((sigma < 0) & (rec["dist2"][at] > 0), -d[at], d[at])
    got, got_rec, got_inst = s.signed_distance(pts, closest=True)
    assert_records(got_rec, got_inst, rec, inst, "the closest part is closest_points")
    assert_values(got, want, "the composition")


def test_omitted_buffers_give_the_same_values(mixed):
    m = mixed
    for records, instances in ((False, True), (True, False), (False, False)):
        got, rec, inst = device_form(m["s"], m["pts"], records, instances)
        what = f"records {'kept' if records else 'omitted'}, instances {'kept' if instances else 'omitted'}"
        assert_values(got, m["want"], what)
        if records:
            assert np.array_equal(R.as_bits(rec), R.as_bits(m["want_rec"])), what
        if instances:
            assert np.array_equal(inst, m["want_inst"]), what


def test_the_seed_keeps_the_sign_walks_below_cold_walks(pkg, tmp_path_factory, mixed):
    """The counters are the sign walks': one walk per hit, and no more bounds or triangle tests than cold walks (+inf radius) of
    the same object points on their member scenes."""
    m = mixed
    s, pts = m["s"], m["pts"]
    got, rec, inst, c = s.signed_distance(pts, closest=True, counters=True)
    assert_records(rec, inst, m["want_rec"], m["want_inst"], "counting form")
    assert_values(got, m["want"], "counting form")
    only, c2 = s.signed_distance(pts, counters=True)
    assert_values(only, m["want"], "counting form without records")
    assert c2 == c
    hits = int((inst >= 0).sum())
    assert c["traversals"] == hits and c["samples"] == len(pts) and c["shaded_hits"] == c["env_lookups"] == c["bad_hits"] == 0
    cold = {"node_visits": 0, "triangle_tests": 0, "leaf_visits": 0}
    for k, name in enumerate(NAMES):
        parts = []
        for i in [i for i in range(len(m["of"])) if m["of"][i] == k]:
            with np.errstate(all="ignore"):
                parts.append(IR.object_vectors(m["W"][i], pts["p"][inst == i], True))
        p_o = np.concatenate(parts)
        _, cc = member(pkg, tmp_path_factory, name)[1].closest_points(pkg.tracer.make_points(p_o), counters=True)
        for key in cold:
            cold[key] += cc[key]
    print(f"sign walks: {c['node_visits']} bounds, {c['triangle_tests']} triangle tests, {c['leaf_visits']} leaves for {hits} hits; "
          f"cold walks: {cold['node_visits']}, {cold['triangle_tests']}, {cold['leaf_visits']}")
    assert c["triangle_tests"] <= cold["triangle_tests"] and c["node_visits"] <= cold["node_visits"], (c, cold)
    assert c["triangle_tests"] >= hits and c["node_visits"] >= hits


def test_a_count_split_over_two_scratch_chunks(pkg, gpu, tmp_path_factory):
    """2^22 + 1000 points with neither buffer kept: stage 1's scratch holds 2^22 points, so the query runs as two chunks.  Far
    points with radius 0 are misses (NaN); the second chunk's points and real points scattered over the first are restated."""
    import torch
    positions, cube = member(pkg, tmp_path_factory, "cube")
    of, maps, _ = IC.make_set([positions], [0, 0], seed=41, spread=1.0, kinds=["shear", "mirror"])
    s = pkg.tracer.InstanceSet([cube, cube], maps)
    _sets.append(s)
    n = (1 << 22) + 1000
    real, _, _ = IC.world_points([positions], of, maps, 1000 + 2048, seed=42)
    tail, spread = real[:1000], real[1000:]
    far = np.zeros(1, R.POINT_DTYPE)
    far["p"] = (1e6, -2e6, 3e6)
    far["max_dist2"] = 0.0
    d_pts = dev_points(far).repeat(n, 1)
    d_pts[n - 1000:] = dev_points(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 1000, 2048, replace=False)).cuda()
    d_pts[sample] = dev_points(spread)
    d_out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    s.signed_distance_into(d_pts.data_ptr(), n, d_out.data_ptr(), 0, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    W = s.world_to_object()
    want = IS.signed_over_instances([positions], of, maps, W, tail)[0]
    assert (want < 0).sum() > 20 and (want > 0).sum() > 20
    assert_values(d_out[n - 1000:].cpu().numpy(), want, "the second chunk's points")
    assert_values(d_out[sample].cpu().numpy(), IS.signed_over_instances([positions], of, maps, W, spread)[0], "points of the first chunk")
    rest = torch.ones(n - 1000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    assert bool(torch.isnan(d_out[: n - 1000][rest]).all())


# one identity instance -------------------------------------------------------------------------------------------------------
def test_one_identity_instance_is_the_signed_distance_query(pkg, gpu):
    arrays, sc = loaded(pkg, "lobed_528")
    s = pkg.tracer.InstanceSet([sc], EYE[None])
    _sets.append(s)
    assert s.closed() and sc.surface_info()["closed"] == 1
    pts = make_points(arrays, 3000, seed=5)
    want, want_rec = sc.signed_distance(pts, closest=True)
    assert np.isnan(want).sum() > 50 and (want < 0).sum() > 50
    got, rec, inst = s.signed_distance(pts, closest=True)
    assert_records(rec, inst, want_rec, np.where(want_rec["triangle"] >= 0, 0, -1), "identity, host form")
    assert_values(got, want, "identity, host form")
    got, rec, inst = device_form(s, pts)
    assert_records(rec, inst, want_rec, np.where(want_rec["triangle"] >= 0, 0, -1), "identity, device form")
    assert_values(got, want, "identity, device form")


def test_closed_reports_an_open_member(pkg, gpu, tmp_path_factory):
    _, leaf = member(pkg, tmp_path_factory, "11-triangle leaf")
    _, cube = member(pkg, tmp_path_factory, "cube")
    both = pkg.tracer.InstanceSet([cube, leaf], np.stack([EYE, EYE]))
    only = pkg.tracer.InstanceSet([cube, cube], np.stack([EYE, EYE]))
    try:
        assert not both.closed() and only.closed()
    finally:
        both.close()
        only.close()


# an object point that overflows ----------------------------------------------------------------------------------------------
def test_an_object_point_that_overflows_is_outside(pkg, gpu, tmp_path_factory):
    """The cube squeezed to 2^-70 along x: W scales x by 2^70, and a world point at x = 2^60 has no finite object point.  Its
    object sign is NaN and its value +sqrtf(dist2)."""
    positions, cube = member(pkg, tmp_path_factory, "cube")
    M = EYE.copy()
    M[0, 0] = F(2.0 ** -70)
    s = pkg.tracer.InstanceSet([cube], M[None])
    _sets.append(s)
    W = s.world_to_object()
    assert W[0, 0, 0] == F(2.0 ** 70)
    p = np.array([[2.0 ** 60, 0.5, 0.5], [-2.0 ** 62, 0.25, 2.0], [2.0 ** 59, -3.0, 0.5], [0.5, 0.5, 1.5], [0.0, 0.5, 0.5], [-1.0, 0.5, 0.5]], F)
    pts = pkg.tracer.make_points(p)
    with np.errstate(all="ignore"):
        assert not np.isfinite(IR.object_vectors(W[0], p[:3], True)).all(1).any() and np.isfinite(IR.object_vectors(W[0], p[3:], True)).all()
    want, want_rec, want_inst = IS.signed_over_instances([positions], [0], M[None], W, pts)
    for got, rec, inst in (s.signed_distance(pts, closest=True), device_form(s, pts)):
        assert_records(rec, inst, want_rec, want_inst, "overflow")
        assert_values(got, want, "overflow")
        assert (inst == 0).all() and np.isfinite(rec["dist2"]).all() and (rec["dist2"][:3] > 2.0 ** 100).all()
        assert_values(got[:3], np.sqrt(rec["dist2"][:3]), "the overflowed points")


# stream order ----------------------------------------------------------------------------------------------------------------
def test_refit_update_and_query_on_one_side_stream(pkg, gpu, tmp_path_factory):
    """A device refit of a member, a device update with new maps and the query, enqueued on one side stream with nothing
    between them: the query sees the new geometry, sign data re-derived from it, and the new W."""
    import torch
    world = pkg.World(scene_path("lobed_528"))
    own = pkg.Scene(world.flatten())            # a scene of its own: it is refit below
    cube_positions, cube = member(pkg, tmp_path_factory, "cube")
    before = np.asarray(world.arrays()["vertex_positions"], F).reshape(-1)
    of = [0, 1, 0, 1, 0]
    kinds = ["rotation_nonuniform", "shear", "mirror", "translation", "rotation_uniform"]
    maps = [IC.make_set([before, cube_positions], of, seed=90 + k, spread=0.8, kinds=kinds[k:] + kinds[:k])[1] for k in range(2)]
    s = pkg.tracer.InstanceSet([own if k == 0 else cube for k in of], maps[0])
    try:
        moved = (before.reshape(-1, 3) * np.array([1.3, 0.8, 1.1], F) + F(0.2)).astype(F)
        positions = [moved.reshape(-1), cube_positions]
        pts, _, _ = IC.world_points(positions, of, maps[1], 1500, seed=91)
        first = s.signed_distance(pts)           # (derives the sign data of the old geometry)
        d_moved, d_maps, d_pts = torch.from_numpy(moved).cuda(), torch.from_numpy(maps[1]).cuda(), dev_points(pts)
        d_out = torch.full((len(pts),), -7.0, dtype=torch.float32, device="cuda")
        d_rec = torch.full((len(pts), 8), -7, dtype=torch.int32, device="cuda")
        d_inst = torch.full((len(pts),), -7, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            own.refit(d_moved, stream_ptr=side.cuda_stream)
            s.update_into(d_maps.data_ptr(), side.cuda_stream)
            s.signed_distance_into(d_pts.data_ptr(), len(pts), d_out.data_ptr(), d_rec.data_ptr(), d_inst.data_ptr(), side.cuda_stream)
        side.synchronize()
        assert s.update_status() == -1
        want, want_rec, want_inst = IS.signed_over_instances(positions, of, maps[1], s.world_to_object(), pts)
        assert_records(host_records(d_rec), d_inst.cpu().numpy(), want_rec, want_inst, "one side stream")
        assert_values(d_out.cpu().numpy(), want, "one side stream")
        assert (~same_floats(first, want)).sum() > 300, "the refit and the update moved something"
        assert (want < 0).sum() > 30 and set(want_inst[want_inst >= 0].tolist()) == set(range(5))
    finally:
        s.close()
        own.close()
        world.close()


def test_sign_data_first_derived_on_a_side_stream_then_a_default_stream_query(pkg, gpu, tmp_path_factory):
    """The first signed query of a set over a fresh scene runs on a side stream, so the member's sign data is derived there;
    with no synchronisation a query on the default stream must wait for it on the device."""
    import torch
    world = pkg.World(scene_path("lobed_528"))
    fresh = pkg.Scene(world.flatten())
    positions = np.asarray(world.arrays()["vertex_positions"], F).reshape(-1)
    _, maps, _ = IC.make_set([positions], [0, 0, 0], seed=95, spread=0.8, kinds=["shear", "mirror", "rotation_nonuniform"])
    s = pkg.tracer.InstanceSet([fresh] * 3, maps)
    try:
        pts, _, _ = IC.world_points([positions], [0, 0, 0], maps, 1500, seed=96)
        d_pts = dev_points(pts)
        d_side = torch.full((len(pts),), -7.0, dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            s.signed_distance_into(d_pts.data_ptr(), len(pts), d_side.data_ptr(), 0, 0, side.cuda_stream)
        d_main = s.signed_distance(d_pts)
        want = IS.signed_over_instances([positions], [0, 0, 0], maps, s.world_to_object(), pts)[0]
        torch.cuda.current_stream().synchronize()
        assert_values(d_main.cpu().numpy(), want, "default stream after a side-stream derivation")
        side.synchronize()
        assert_values(d_side.cpu().numpy(), want, "the side stream's own query")
        assert (want < 0).sum() > 30
    finally:
        s.close()
        fresh.close()
        world.close()


# refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops(pkg, gpu, mixed):
    """A member without a packed tree is refused when the set is created, and scene creation keeps no packed tree for a tree
    deeper than SHRAY_POINT_MAX_HEIGHT (a 150-level comb), so the height refusal is not reachable from here;
    count 0 is a no-op; the binding refuses a tensor of the wrong shape and counters on the device path; misaligned device
    buffers are argument errors."""
    import torch
    import test_oracle_kat as kat
    _, sc = loaded(pkg, "lobed_528")
    comb = pkg.Scene(kat.comb_scene(150).desc)
    try:
        with pytest.raises(pkg._native.ShrayError) as err:
            pkg.tracer.InstanceSet([sc, comb], np.stack([EYE, EYE]))
        assert err.value.code == BAD_TREE
    finally:
        comb.close()
    s = mixed["s"]
    assert len(s.signed_distance(np.zeros((0, 3), F))) == 0
    with pytest.raises(ValueError):
        s.signed_distance(torch.zeros((4, 5), device="cuda"))
    with pytest.raises(ValueError):
        s.signed_distance(torch.zeros((4, 4), device="cuda"), counters=True)
    lib = pkg._native.load_instance_sdf()
    d = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    call, V = lib.shray_signed_distance_instances_device, C.c_void_p
    base = d.data_ptr()
    assert call(s._handle, V(base + 4), 1, V(base + 128), V(base + 32), V(base + 96), None) == -1
    assert call(s._handle, V(base), 1, V(base + 130), V(base + 32), V(base + 96), None) == -1
    assert call(s._handle, V(base), 1, V(base + 128), V(base + 40), V(base + 96), None) == -1
    assert call(s._handle, V(base), 1, V(base + 128), V(base + 32), V(base + 98), None) == -1
    assert call(s._handle, V(base), 1, V(base + 132), V(base + 32), V(base + 100), None) == 0
    assert call(s._handle, V(base), 0, V(base + 128), None, None, None) == 0
    torch.cuda.synchronize()
