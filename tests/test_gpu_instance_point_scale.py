"""Instanced closest-point queries on the GPU at the cells of tests/instance_point_scale_cases.py (world, scene and cancelling
scales, far translations, ill-conditioned maps, negative zeros, the two cells where every dist2 is 0), every byte of every
record and instance index against the restatement on the host and the device path with 1, 63, 64, 65 and all points; the
containment of the mapped corners in the stored top-level boxes wherever the corners are normal or 0, and for every set the
property the top-level cull needs (no stored box's bound above a dist2 of its instance); the top-level nodes and the four
counters under a cancelling scale; a device update from the k = 0 maps to the k = 40 maps and a host update back; a count
split over two launches at an outside cell.  tests/test_instance_point_scale_reference.py pins the cells on the CPU.

Scenes.  A ("scene", k) or ("subnormal", k) cell loads its scenes under GEOMETRY_SCALE = 2^k (ray_scale_cases.load_scaled) and
restates on that world's own arrays: the build's triangle order and boxes are that scale's.  A ("cancel", a) cell does not: a
scene loaded at 2^a is another tree (at 2^-40 every node box is box3d::add's absolute 1e-5 pad) and its root box is not 2^a
times the unscaled one, so neither the stored top-level boxes nor the counters could be the a = 0 set's.  Its scenes are the
unscaled scenes' own trees with every vertex and every node box multiplied by 2^a (refit_ref.tree_desc, flattened and created
like the hand-shaped trees), and its twin is the a = 0 set made the same way; then every product keeps its bits, and with
them place_box's doubles, every image box and every counter."""
import ctypes as C

import numpy as np
import pytest

import instance_point_cases as IC
import instance_point_ref as IP
import instance_point_scale_cases as SC
import point_query_ref as R
import point_scale_cases as PC
import ray_scale_cases as X
import refit_ref
import test_gpu_instance_point as G
from test_gpu_instance_point import assert_answer, assert_contained, build, check_both_paths, dev_points, host_records

pytestmark = pytest.mark.gpu

F = np.float32
TINY = F(2.0 ** -126)
_scenes = {}
_sets = []
_memo = {}


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    for s in _sets + G._sets:
        s.close()
    _sets.clear()
    G._sets.clear()
    for _, scene, world in _scenes.values():
        scene.close()
        if world is not None:
            world.close()
    _scenes.clear()
    for _, sc in G._members.values():
        sc.close()
    G._members.clear()
    _memo.clear()


def loaded(pkg, name, k):
    """(positions, resident scene) of the scene loaded under GEOMETRY_SCALE = 2^k, once per module"""
    if (name, k, "loaded") not in _scenes:
        world = X.load_scaled(pkg, name, k)
        positions = np.asarray(world.arrays()["vertex_positions"], F).reshape(-1).copy()
        want = PC.scaled_positions(pkg, name, k)
        assert np.array_equal(X.triangle_rows(positions), X.triangle_rows(want)), (name, k)
        _scenes[(name, k, "loaded")] = (positions, pkg.Scene(world.flatten()), world)
    return _scenes[(name, k, "loaded")][:2]


def scaled_tree(pkg, name, a):
    """(positions, resident scene) of the unscaled scene's own tree with every vertex and node box times 2^a, once per module"""
    if (name, a, "tree") not in _scenes:
        world = pkg.World(X.scene_path(name))
        try:
            desc = world.export_tree()
            tree = refit_ref.TreeArrays.of(desc)
            vd = np.ctypeslib.as_array(desc.vertex_data, shape=(desc.vertex_count * 9,)).reshape(-1, 9).copy()
        finally:
            world.close()
        S = F(2.0 ** a)
        vd[:, :3] *= S
        boxes = tree.box * S
        assert np.isfinite(boxes).all() and ((boxes != 0) == (tree.box != 0)).all()
        flat = pkg.tracer.DeviceFlat(refit_ref.tree_desc(tree, boxes, vd))
        scene = pkg.Scene(flat.download(), pkg.scenes.environment_constant())
        flat.close()
        positions = np.ascontiguousarray(vd[tree.triangle_vertices][:, :, :3]).reshape(-1)
        assert np.array_equal(np.asarray(scene.geometry()["vertex_positions"], F).reshape(-1).view(np.uint32), positions.view(np.uint32))
        _scenes[(name, a, "tree")] = (positions, scene, None)
    return _scenes[(name, a, "tree")][:2]


def members_of(pkg, c, trees=False):
    """the two member scenes of a cell: [(positions, scene)] in instance_point_scale_cases.SCENES' order"""
    get = scaled_tree if trees or c.key[0] == "cancel" else loaded
    return [get(pkg, name, c.scene_exp) for name in SC.SCENES]


def read_nodes(pkg, s):
    """the set's top-level nodes as the next query reads them: uint32 [n, 8] (lo xyz, k, hi xyz, link)"""
    N = pkg._native.load_instance()
    count = C.c_int32()
    assert N.shrayi_instance_set_arrays(s._handle, None, None, C.byref(count)) == 0
    nodes = np.zeros((count.value, 8), np.uint32)
    assert N.shrayi_instance_set_arrays(s._handle, nodes.ctypes.data_as(C.c_void_p), None, None) == 0
    return nodes


def restate(members, of, maps, pts):
    return IP.closest_over_instances([m[0] for m in members], of, maps, pts, device="cuda")


def normal_or_zero(members, of, maps):
    return all(((np.abs(w) >= TINY) | (w == 0)).all() for w in (IP.map_corners(maps[i], members[s][0]) for i, s in enumerate(of)))


def assert_no_stored_bound_above_a_dist2(pkg, s, members, of, maps, pts, what):
    """What the top-level cull needs, from the nodes as read back: for every walked point and every instance, box_bound of the
    instance's stored box is not above the restated dist2 of any pair of that instance (the least of them is checked)."""
    nodes = read_nodes(pkg, s)
    leaves = nodes[(nodes[:, 7] & 0x80000000) != 0]
    assert len(leaves) == len(maps)
    go = SC.walked(pts)
    every = pts[go].copy()
    every["max_dist2"] = np.inf
    p = np.ascontiguousarray(every["p"])
    for row in leaves:
        i = int(row[7] & 0x7fffffff)
        box = row.view(F)
        least = R.closest_torch(IP.map_corners(maps[i], members[of[i]][0]).reshape(-1), every)
        assert (least["triangle"] >= 0).all()
        lb = IP.bound(p, box[0:3], box[4:7])
        bad = np.nonzero(lb > least["dist2"])[0]
        assert len(bad) == 0, f"{what}: instance {i}: the stored box {box} bounds {lb[bad[:3]]} above dist2 {least['dist2'][bad[:3]]}"


def make_set(pkg, members, of, maps, pts, what):
    """an InstanceSet over the members, kept until the module ends, with the containment asserted where it is claimed and the
    cull's own property everywhere"""
    s = pkg.tracer.InstanceSet([members[k][1] for k in of], maps)
    _sets.append(s)
    check_the_boxes(pkg, s, members, of, maps, pts, what)
    return s


def check_the_boxes(pkg, s, members, of, maps, pts, what):
    if normal_or_zero(members, of, maps):
        assert_contained(pkg, s, [members[k][0] for k in of], maps, what)
    assert_no_stored_bound_above_a_dist2(pkg, s, members, of, maps, pts, what)


def check_every_count(pkg, s, pts, want, want_inst, what):
    """both paths with 1, 63, 64 and 65 points (check_both_paths) and with all of them"""
    import torch
    assert len(pts) < G.COUNTS[-1]
    check_both_paths(pkg, s, pts, want, want_inst, what)
    got, inst = s.closest_points(pts)
    assert_answer(got, inst, want, want_inst, f"{what}, all points, host path")
    d_out, d_inst = s.closest_points(dev_points(pts))
    torch.cuda.current_stream().synchronize()
    assert_answer(host_records(d_out), d_inst.cpu().numpy(), want, want_inst, f"{what}, all points, device path")


def cell_run(pkg, key):
    """(cell, members, set, restated records, restated instances) of a cell, once per module"""
    if key not in _memo:
        c = SC.cell(pkg, key)
        members = members_of(pkg, c)
        s = make_set(pkg, members, c.of, c.maps, c.points, str(c))
        _memo[key] = (c, members, s) + restate(members, c.of, c.maps, c.points)
    return _memo[key]


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SC.CELLS, ids=lambda k: f"{k[0]} {k[1]}")
def test_a_cell_equals_the_restatement(pkg, gpu, key):
    c, members, s, want, want_inst = cell_run(pkg, key)
    part, part_inst = IP.closest_over_instances([m[0] for m in members], c.of, c.maps, c.points[:96])
    assert_answer(part, part_inst, want[:96], want_inst[:96], f"{c}: the torch restatement against numpy")
    if key not in SC.ALL_ZERO:
        IC.assert_mixed(c.points, c.kind, c.radius, want, str(c))
    check_every_count(pkg, s, c.points, want, want_inst, str(c))
    got, inst, counters = s.closest_points(c.points, counters=True)
    assert_answer(got, inst, want, want_inst, f"{c}, counting form")
    go = SC.walked(c.points)
    assert counters["samples"] == len(go) and counters["traversals"] <= int(go.sum()) * len(c.of)
    if key in SC.ALL_ZERO:
        # every dist2 is 0: (instance 0, triangle 0) on every walked point, and nothing is culled where a bound of 0 meets a best
        # of 0: every walked point walks every instance and tests every triangle of the set
        assert (got["triangle"][go] == 0).all() and (inst[go] == 0).all() and (got["dist2"][go] == 0).all()
        assert (got["triangle"][~go] == -1).all() and (inst[~go] == -1).all()
        triangles = sum(len(members[k][0]) // 9 for k in c.of)
        assert counters["triangle_tests"] == int(go.sum()) * triangles, (counters, int(go.sum()), triangles)
        assert counters["traversals"] == int(go.sum()) * len(c.of), counters
    twin = SC.expected_cell(key)
    if twin and key[0] == "negzero":
        _, _, _, t_want, t_inst = cell_run(pkg, twin)
        assert_answer(got, inst, t_want, t_inst, f"{c} against {twin}")


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", SC.CANCEL_EXPONENTS)
def test_a_cancelling_scale_keeps_every_bit(pkg, gpu, a):
    """The scenes at 2^a under linear parts x 2^-a, against the a = 0 set made the same way: the records, the instance indices,
    the top-level nodes as read back and the counting form's four counters are equal, bit for bit."""
    c, members, s, want, want_inst = cell_run(pkg, ("cancel", a))
    if ("cancel", 0) not in _memo:
        c0 = SC.cell(pkg, ("world", 0))
        members0 = members_of(pkg, c0, trees=True)
        s0 = make_set(pkg, members0, c0.of, c0.maps, c0.points, "the a = 0 twin")
        _memo[("cancel", 0)] = (c0, members0, s0) + restate(members0, c0.of, c0.maps, c0.points)
    c0, members0, s0, want0, want_inst0 = _memo[("cancel", 0)]
    assert_answer(want, want_inst, want0, want_inst0, f"{c}: the restatement against a = 0's")
    got, inst, counters = s.closest_points(c.points, counters=True)
    got0, inst0, counters0 = s0.closest_points(c0.points, counters=True)
    assert_answer(got, inst, got0, inst0, f"{c} against the a = 0 set")
    nodes, nodes0 = read_nodes(pkg, s), read_nodes(pkg, s0)
    assert np.array_equal(nodes, nodes0), f"{c}: {(nodes != nodes0).any(1).sum()} of {len(nodes)} top-level nodes differ from a = 0's"
    for k in ("node_visits", "leaf_visits", "triangle_tests", "traversals"):
        assert counters[k] == counters0[k] > 0, (c, k, counters, counters0)


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_a_device_update_across_magnitudes_and_a_host_update_back(pkg, gpu):
    """One set goes from the k = 0 maps to the k = 40 maps by update_into on a side stream with the query behind it on that
    stream, and back by the host update: each state against its restatement, the boxes checked after each."""
    import torch
    c0, c40 = SC.cell(pkg, ("world", 0)), SC.cell(pkg, ("world", 40))
    members = members_of(pkg, c0)
    s = make_set(pkg, members, c0.of, c0.maps, c0.points, "before the updates")
    n = len(c40.points)
    d_maps, d_pts = torch.from_numpy(c40.maps).cuda(), dev_points(c40.points)
    d_out = torch.full((n, 8), -7, dtype=torch.int32, device="cuda")
    d_inst = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.update_into(d_maps.data_ptr(), side.cuda_stream)
        s.closest_points_into(d_pts.data_ptr(), n, d_out.data_ptr(), d_inst.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert s.update_status() == -1
    want, want_inst = restate(members, c40.of, c40.maps, c40.points)
    assert_answer(host_records(d_out), d_inst.cpu().numpy(), want, want_inst, "after the device update to 2^40")
    check_the_boxes(pkg, s, members, c40.of, c40.maps, c40.points, "after the device update to 2^40")
    s.update(c0.maps)
    want0, want_inst0 = restate(members, c0.of, c0.maps, c0.points)
    assert (R.as_bits(want0) != R.as_bits(want)).any(1).sum() > 500
    check_every_count(pkg, s, c0.points, want0, want_inst0, "after the host update back to 2^0")
    check_the_boxes(pkg, s, members, c0.of, c0.maps, c0.points, "after the host update back to 2^0")


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_a_count_split_over_two_launches_at_an_outside_cell(pkg, gpu):
    """2^24 + 3000 points (one launch holds 2^24) on the one-triangle scene placed twice under maps x 2^-40, an outside cell:
    far points with radius 0 are misses; the last launch's points and real points scattered over the first launch are restated."""
    import torch
    k = -40
    assert SC.flag(k) == SC.OUTSIDE
    positions, _ = G.member(pkg, "one triangle")
    names = ["one triangle", "one triangle"]
    _, maps, _ = IC.make_set([positions], [0, 0], seed=5, spread=1.0, kinds=["rotation_nonuniform", "mirror"])
    real, _, _ = IC.world_points([positions], [0, 0], maps, 3000 + 4096, seed=33)
    maps = maps * F(2.0 ** k)
    real = PC.scaled_points(real, k)
    s = build(pkg, names, maps, "one triangle, twice, at 2^-40")
    n = (1 << 24) + 3000
    tail, spread = real[:3000], real[3000:]
    far = np.zeros(1, R.POINT_DTYPE)
    far["p"] = (1e6, -2e6, 3e6)
    far["max_dist2"] = 0.0
    far = PC.scaled_points(far, k)
    d_pts = dev_points(far).repeat(n, 1)
    d_pts[n - 3000:] = dev_points(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, 4096, replace=False)).cuda()
    d_pts[sample] = dev_points(spread)
    d_out = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    d_inst = torch.empty(n, dtype=torch.int32, device="cuda")
    s.closest_points_into(d_pts.data_ptr(), n, d_out.data_ptr(), d_inst.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    want, want_inst = IP.closest_over_instances([positions], [0, 0], maps, tail)
    assert (want_inst == 0).sum() > 100 and (want_inst == 1).sum() > 100
    assert_answer(host_records(d_out[n - 3000:]), d_inst[n - 3000:].cpu().numpy(), want, want_inst, "the last launch's points")
    want, want_inst = IP.closest_over_instances([positions], [0, 0], maps, spread)
    assert_answer(host_records(d_out[sample]), d_inst[sample].cpu().numpy(), want, want_inst, "points of the first launch")
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    far_want, far_inst = IP.closest_over_instances([positions], [0, 0], maps, far)
    assert far_want["triangle"][0] == -1 and far_inst[0] == -1
    far_record = torch.from_numpy(R.as_bits(far_want).view(np.int32).copy()).cuda()
    assert bool((d_out[: n - 3000][rest] == far_record).all()) and bool((d_inst[: n - 3000][rest] == -1).all())
