"""Instanced closest-point queries on the GPU (include/shader_ray_instance_point.h) against the restatement
(tests/instance_point_ref.py): every byte of every record and every instance index, on the host and the device path, for sets
of 1, 2, 17 and 301 instances over the small scenes and the hand-shaped trees, with maps of every kind and points of every kind
mixed in one wave; one identity instance against Scene.closest_points (bytes and counters); the cull on a grid of copies; the
containment of every mapped corner in its instance's stored top-level box, for every set built here; a refit, a device update
and the query on one stream, and a host update followed by the query; a count split over two launches; the refusals."""
import ctypes as C

import numpy as np
import pytest

import instance_point_cases as IC
import instance_point_ref as IP
import point_query_ref as R
from helpers import single_leaf_scene
from test_gpu_instances import BAD_TREE, scene
from test_gpu_ray_query import loaded
from test_oracle_kat import chain_scene

pytestmark = pytest.mark.gpu

F = np.float32
EYE = IC.EYE
COUNTS = (1, 63, 64, 65, 3000)
NUMPY_PAIRS = 2 * 10 ** 7
_members = {}
_sets = []


def member(pkg, name):
    """(vertex_positions, resident scene) of a named member: the small scene files, or a hand-shaped tree of its own"""
    if name in ("small_trisrc", "lobed_528", "bunny"):
        arrays, sc = scene(pkg, name)
        return np.asarray(arrays.positions, F).reshape(-1), sc
    if name not in _members:
        if name == "two-leaf tree":
            from test_gpu_uniform_leaf import two_leaf_scene
            hand = two_leaf_scene()
            positions = hand.keep["pos"][:24].reshape(-1).copy()
        else:
            tris = np.asarray(IC.TINY[name], F)
            hand, positions = single_leaf_scene(tris), tris.reshape(-1)
        _members[name] = (np.asarray(positions, F), pkg.Scene(hand.desc))
    return _members[name]


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    for s in _sets:
        s.close()
    _sets.clear()
    for _, sc in _members.values():
        sc.close()
    _members.clear()


def assert_contained(pkg, s, positions_of_instance, maps, what):
    """Every fp32 world corner of every instance lies inside that instance's stored top-level box (the nodes as the next query
    reads them): what the top-level cull's exactness rests on."""
    N = pkg._native.load_instance()
    count = C.c_int32()
    assert N.shrayi_instance_set_arrays(s._handle, None, None, C.byref(count)) == 0
    nodes = np.zeros((count.value, 8), np.uint32)
    assert N.shrayi_instance_set_arrays(s._handle, nodes.ctypes.data_as(C.c_void_p), None, None) == 0
    leaves = nodes[(nodes[:, 7] & 0x80000000) != 0]
    assert len(leaves) == len(maps)
    boxes = leaves.view(F)
    seen = set()
    for row, link in zip(boxes, leaves[:, 7]):
        i = int(link & 0x7fffffff)
        seen.add(i)
        w = IP.map_corners(maps[i], positions_of_instance[i])
        assert (w >= row[0:3]).all() and (w <= row[4:7]).all(), f"{what}: instance {i}: a mapped corner outside the stored box {row}"
    assert seen == set(range(len(maps)))


def build(pkg, names, maps, what, keep=True):
    """an InstanceSet over the named members, checked for containment"""
    s = pkg.tracer.InstanceSet([member(pkg, n)[1] for n in names], maps)
    if keep:
        _sets.append(s)
    assert_contained(pkg, s, [member(pkg, n)[0] for n in names], maps, what)
    return s


def restate(pkg, names, maps, pts):
    distinct = sorted(set(names))
    positions = [member(pkg, n)[0] for n in distinct]
    of = [distinct.index(n) for n in names]
    pairs = len(pts) * sum(len(positions[s]) // 9 for s in of)
    return IP.closest_over_instances(positions, of, maps, pts, device="cuda" if pairs > NUMPY_PAIRS else None)


def dev_points(pts):
    import torch
    return torch.from_numpy(np.ascontiguousarray(pts).view(F).reshape(-1, 4).copy()).cuda()


def host_records(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1)


def assert_answer(got, got_inst, want, want_inst, what):
    g, w = R.as_bits(got), R.as_bits(want)
    bad = np.nonzero((g != w).any(1) | (np.asarray(got_inst) != want_inst))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(g)} points differ, first {bad[:5]}: got {got[bad[:3]]} / {got_inst[bad[:3]]} "
                           f"want {want[bad[:3]]} / {want_inst[bad[:3]]}")


def check_both_paths(pkg, s, pts, want, want_inst, what):
    import torch
    for count in [c for c in COUNTS if c <= len(pts)]:
        got, inst = s.closest_points(pts[:count])
        assert got.dtype == R.CLOSEST_DTYPE and inst.dtype == np.int32
        assert_answer(got, inst, want[:count], want_inst[:count], f"{what}, {count} points, host path")
        d_out, d_inst = s.closest_points(dev_points(pts[:count]))
        assert d_out.dtype == torch.int32 and tuple(d_out.shape) == (count, 8) and d_inst.dtype == torch.int32 and d_inst.is_cuda
        torch.cuda.current_stream().synchronize()
        assert_answer(host_records(d_out), d_inst.cpu().numpy(), want[:count], want_inst[:count], f"{what}, {count} points, device path")


SCENES = ["small_trisrc", "lobed_528", "one triangle", "11-triangle leaf", "two-leaf tree"]


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_one_identity_instance_is_the_closest_point_query(pkg, gpu, name):
    """Scene.closest_points' bytes with instance 0 on every hit, and its three counters: the root of a one-instance set is not
    tested, and an identity map's image boxes are the boxes."""
    positions, sc = member(pkg, name)
    s = build(pkg, [name], EYE[None], name)
    pts, kind, radius = IC.world_points([positions], [0], EYE[None], 3000, seed=len(name))
    want = sc.closest_points(pts)
    assert np.array_equal(R.as_bits(want), R.as_bits(R.closest(positions, pts))), "the plain query is the restatement"
    IC.assert_mixed(pts, kind, radius, want, name)
    check_both_paths(pkg, s, pts, want, np.where(want["triangle"] >= 0, 0, -1).astype(np.int32), f"{name}, identity")
    _, wc = sc.closest_points(pts, counters=True)
    got, inst, gc = s.closest_points(pts, counters=True)
    assert_answer(got, inst, want, np.where(want["triangle"] >= 0, 0, -1), f"{name}, counting form")
    for k in ("node_visits", "leaf_visits", "triangle_tests", "samples"):
        assert gc[k] == wc[k], (name, k, gc, wc)
    walked = np.isfinite(pts["p"]).all(1) & (pts["max_dist2"] >= 0)
    assert gc["traversals"] == int(walked.sum()) and gc["shaded_hits"] == gc["env_lookups"] == gc["bad_hits"] == 0


# 2 ---------------------------------------------------------------------------------------------------------------------------
SETS = {
    "two scenes of different heights": (["lobed_528", "small_trisrc"], ["rotation_nonuniform", "mirror"], 0.25),
    "17 instances": (["lobed_528", "small_trisrc", "two-leaf tree", "lobed_528", "lobed_528", "11-triangle leaf"], None, 1.2),
    "301 tiny instances": (["one triangle", "11-triangle leaf", "two-leaf tree"], None, 4.0),
}
SIZES = {"two scenes of different heights": 2, "17 instances": 17, "301 tiny instances": 301}


def the_set(pkg, which):
    cycle, kinds, spread = SETS[which]
    n = SIZES[which]
    names = [cycle[i % len(cycle)] for i in range(n)]
    distinct = sorted(set(names))
    of, maps, kinds = IC.make_set([member(pkg, d)[0] for d in distinct], [distinct.index(x) for x in names], seed=n, spread=spread, kinds=kinds)
    names = [distinct[k] for k in of]
    return names, maps, kinds


@pytest.mark.parametrize("which", sorted(SETS))
def test_sets_equal_the_restatement(pkg, gpu, which):
    names, maps, kinds = the_set(pkg, which)
    if len(names) >= 17:
        assert set(kinds) >= set(IC.MAP_KINDS) | {"duplicate of 1"}, kinds
        assert np.array_equal(maps[4].view(np.uint32), maps[1].view(np.uint32)) and names[4] == names[1]
    s = build(pkg, names, maps, which)
    distinct = sorted(set(names))
    pts, kind, radius = IC.world_points([member(pkg, d)[0] for d in distinct], [distinct.index(x) for x in names], maps, 3000, seed=len(names) + 7)
    want, want_inst = restate(pkg, names, maps, pts)
    IC.assert_mixed(pts, kind, radius, want, which)
    if which == "17 instances":     # the larger brute force went through torch: a part of it against numpy
        part, part_inst = IP.closest_over_instances([member(pkg, d)[0] for d in distinct], [distinct.index(x) for x in names], maps, pts[:150])
        assert_answer(part, part_inst, want[:150], want_inst[:150], "the torch restatement against numpy")
    check_both_paths(pkg, s, pts, want, want_inst, which)
    hit = want_inst >= 0
    assert len(set(want_inst[hit].tolist())) >= min(len(names), 12), "the answers come from many instances"
    if len(names) >= 5:
        assert (want_inst == 1).sum() > 5 and (want_inst == 4).sum() == 0, "an exact duplicate never wins against the lower index"
    got, inst, c = s.closest_points(pts, counters=True)
    assert_answer(got, inst, want, want_inst, f"{which}, counting form")
    walked = int((np.isfinite(pts["p"]).all(1) & (pts["max_dist2"] >= 0)).sum())
    assert c["samples"] == len(pts) and int(hit.sum()) <= c["traversals"] <= walked * len(names)
    assert c["node_visits"] >= c["traversals"] and c["triangle_tests"] >= int(hit.sum()) and c["leaf_visits"] > 0


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_the_cull_on_a_grid_of_copies(pkg, gpu):
    """8 x 8 copies of lobed_528, each rotated, 1.6 world sizes apart, and points near their surfaces: the records are the
    restatement's, and the walks test under half of points x instances x triangles (a condition on the cull, not a timing)."""
    positions, _ = member(pkg, "lobed_528")
    rng = np.random.default_rng(88)
    lo, hi = IC.extent_of(positions)
    size = float((hi - lo).max())
    maps = np.zeros((64, 3, 4))
    for i in range(64):
        A = IC.rotation(rng) / size
        maps[i, :, :3] = A
        maps[i, :, 3] = np.array([(i % 8) * 1.6, (i // 8) * 1.6, 0.0]) - A @ ((lo + hi) / 2)
    maps = maps.astype(F)
    names = ["lobed_528"] * 64
    s = build(pkg, names, maps, "the grid")
    n = 1024
    tris = positions.reshape(-1, 3, 3).astype(np.float64)
    i, t = rng.integers(0, 64, n), rng.integers(0, len(tris), n)
    on = tris[t].mean(1)
    world = np.einsum("nrc,nc->nr", maps[i, :, :3].astype(np.float64), on) + maps[i, :, 3] + rng.normal(size=(n, 3)) * 0.01
    pts = pkg.tracer.make_points(world.astype(F))
    want, want_inst = restate(pkg, names, maps, pts)
    got, inst, c = s.closest_points(pts, counters=True)
    assert_answer(got, inst, want, want_inst, "the grid")
    assert (want["triangle"] >= 0).all() and (want_inst == i).mean() > 0.9
    brute = n * 64 * len(tris)
    print(f"the grid: {c['triangle_tests'] / n:.1f} triangle tests, {c['node_visits'] / n:.1f} bounds and {c['traversals'] / n:.2f} walks "
          f"a point; the brute force is {brute // n} tests a point")
    assert c["triangle_tests"] < brute / 2, (c, brute)


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_refit_update_and_query_on_one_stream_and_after_a_host_update(pkg, gpu):
    """A device refit of a member, a device update with moved maps and the query, enqueued on one side stream with nothing
    between them; then a host update with other maps followed by the query on both paths.  Each against the restatement of
    the state the query must see."""
    import torch
    world, _, _ = loaded(pkg, "lobed_528")
    own = pkg.Scene(world.flatten())            # a scene of its own: it is refit below
    small_positions, small = member(pkg, "small_trisrc")
    before = np.asarray(own.geometry()["vertex_positions"], F).reshape(-1)
    names = ["lobed_528", "small_trisrc", "lobed_528", "lobed_528", "small_trisrc"]
    members = [own if x == "lobed_528" else small for x in names]
    of = [0 if x == "lobed_528" else 1 for x in names]
    kinds = ["rotation_nonuniform", "shear", "mirror", "translation", "rotation_uniform"]
    maps = [IC.make_set([before, small_positions], of, seed=70 + k, spread=0.8, kinds=kinds[k:] + kinds[:k])[1] for k in range(3)]
    s = pkg.tracer.InstanceSet(members, maps[0])
    try:
        assert_contained(pkg, s, [before if x == "lobed_528" else small_positions for x in names], maps[0], "before the updates")
        moved = (before.reshape(-1, 3) * F(1.3) + F(0.2)).astype(F)
        pts, _, _ = IC.world_points([moved.reshape(-1), small_positions], of, maps[1], 3000, seed=71)
        first, first_inst = s.closest_points(pts)
        d_moved, d_maps, d_pts = torch.from_numpy(moved).cuda(), torch.from_numpy(maps[1]).cuda(), dev_points(pts)
        d_out = torch.full((len(pts), 8), -7, dtype=torch.int32, device="cuda")
        d_inst = torch.full((len(pts),), -7, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            own.refit(d_moved, stream_ptr=side.cuda_stream)
            s.update_into(d_maps.data_ptr(), side.cuda_stream)
            s.closest_points_into(d_pts.data_ptr(), len(pts), d_out.data_ptr(), d_inst.data_ptr(), side.cuda_stream)
        side.synchronize()
        assert s.update_status() == -1
        want, want_inst = IP.closest_over_instances([moved.reshape(-1), small_positions], of, maps[1], pts)
        assert (R.as_bits(first) != R.as_bits(want)).any(1).sum() > 500, "the refit and the update moved something"
        assert_answer(host_records(d_out), d_inst.cpu().numpy(), want, want_inst, "one stream")
        assert_contained(pkg, s, [moved.reshape(-1) if x == "lobed_528" else small_positions for x in names], maps[1], "after the device update")
        # the device path without an instance buffer writes the same records
        d_only = torch.full((len(pts), 8), -7, dtype=torch.int32, device="cuda")
        s.closest_points_into(d_pts.data_ptr(), len(pts), d_only.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().synchronize()
        assert torch.equal(d_only, d_out)
        # a host update: the device copy of the maps is behind it until the next query stages them on its stream
        s.update(maps[2])
        want, want_inst = IP.closest_over_instances([moved.reshape(-1), small_positions], of, maps[2], pts)
        d_out2, d_inst2 = s.closest_points(d_pts)
        torch.cuda.current_stream().synchronize()
        assert_answer(host_records(d_out2), d_inst2.cpu().numpy(), want, want_inst, "after a host update, device path")
        got, inst = s.closest_points(pts)
        assert_answer(got, inst, want, want_inst, "after a host update, host path")
        assert (R.as_bits(host_records(d_out)) != R.as_bits(want)).any(1).sum() > 500, "the host update moved something"
        assert_contained(pkg, s, [moved.reshape(-1) if x == "lobed_528" else small_positions for x in names], maps[2], "after the host update")
    finally:
        s.close()
        own.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_a_count_split_over_two_launches(pkg, gpu):
    """2^24 + 3000 points (one launch holds 2^24) on the one-triangle scene placed twice: far points with radius 0 are misses;
    the last launch's points and real points scattered over the first launch are restated."""
    import torch
    positions, _ = member(pkg, "one triangle")
    names = ["one triangle", "one triangle"]
    _, maps, _ = IC.make_set([positions], [0, 0], seed=5, spread=1.0, kinds=["rotation_nonuniform", "mirror"])
    s = build(pkg, names, maps, "one triangle, twice")
    n = (1 << 24) + 3000
    real, _, _ = IC.world_points([positions], [0, 0], maps, 3000 + 4096, seed=33)
    tail, spread = real[:3000], real[3000:]
    far = np.zeros(1, R.POINT_DTYPE)
    far["p"] = (1e6, -2e6, 3e6)
    far["max_dist2"] = 0.0
    d_pts = dev_points(far).repeat(n, 1)
    d_pts[n - 3000:] = dev_points(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, 4096, replace=False)).cuda()
    d_pts[sample] = dev_points(spread)
    d_out = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    d_inst = torch.empty(n, dtype=torch.int32, device="cuda")
    s.closest_points_into(d_pts.data_ptr(), n, d_out.data_ptr(), d_inst.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    want, want_inst = restate(pkg, names, maps, tail)
    assert (want_inst == 0).sum() > 100 and (want_inst == 1).sum() > 100
    assert_answer(host_records(d_out[n - 3000:]), d_inst[n - 3000:].cpu().numpy(), want, want_inst, "the last launch's points")
    want, want_inst = restate(pkg, names, maps, spread)
    assert_answer(host_records(d_out[sample]), d_inst[sample].cpu().numpy(), want, want_inst, "points of the first launch")
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    far_want, far_inst = restate(pkg, names, maps, far)
    assert far_want["triangle"][0] == -1 and far_inst[0] == -1
    far_record = torch.from_numpy(R.as_bits(far_want).view(np.int32).copy()).cuda()
    assert bool((d_out[: n - 3000][rest] == far_record).all()) and bool((d_inst[: n - 3000][rest] == -1).all())


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops(pkg, gpu):
    import torch
    positions, sc = member(pkg, "lobed_528")
    chain = pkg.Scene(chain_scene(5).desc)        # no packed tree: refused when the set is created, so no query ever meets one
    try:
        with pytest.raises(pkg._native.ShrayError) as err:
            pkg.tracer.InstanceSet([sc, chain], np.concatenate([EYE[None], EYE[None]]))
        assert err.value.code == BAD_TREE
    finally:
        chain.close()
    s = build(pkg, ["lobed_528"], EYE[None], "refusals")
    got, inst = s.closest_points(np.zeros((0, 3), F))
    assert len(got) == 0 and len(inst) == 0
    with pytest.raises(ValueError):
        s.closest_points(torch.zeros((4, 5), device="cuda"))
    with pytest.raises(ValueError):
        s.closest_points(torch.zeros((4, 4), device="cuda"), counters=True)
    lib = pkg._native.load_instance_point()
    d = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
    call, V = lib.shray_closest_points_instances_device, C.c_void_p
    assert call(s._handle, V(d.data_ptr() + 4), 1, V(d.data_ptr() + 32), None, None) == -1
    assert call(s._handle, V(d.data_ptr()), 1, V(d.data_ptr() + 40), None, None) == -1
    assert call(s._handle, V(d.data_ptr()), 1, V(d.data_ptr() + 32), V(d.data_ptr() + 98), None) == -1
    assert call(s._handle, V(d.data_ptr()), 1, V(d.data_ptr() + 32), V(d.data_ptr() + 100), None) == 0
    assert call(s._handle, V(d.data_ptr()), 0, V(d.data_ptr() + 32), None, None) == 0
    torch.cuda.synchronize()
