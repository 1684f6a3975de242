"""Instanced box-overlap queries on the GPU (include/shader_ray_instance_overlap.h) against the restatement
(tests/instance_overlap_ref.py): every triangle index, every instance index and every count, on the host path, the device path
and the device path without an instance buffer (the scratch path above K = 8), for K in {0, 1, 2, 3, 4, 5, 8, 9, 64} with and
without counts and for SHRAY_OVERLAP_ANY, with 1, 63, 64, 65 and 1,536 boxes.  One identity instance against
Scene.triangles_in_boxes (indices, counts and its three counters); the nine-instance set of tests/instance_overlap_cases.py, two
scenes of different heights and 301 instances of the tiny scenes; the counters of the nine-instance set against
instance_overlap_ref.walk_counters with the stored boxes as read back; a refit, a device update and the query on one stream, and
a host update followed by the query; surface_voxels against the merged scene's; a count split over two launches; the refusals."""
import ctypes as C

import numpy as np
import pytest

import instance_overlap_cases as XC
import instance_overlap_ref as IO
import instance_point_cases as IC
import instance_point_ref as IP
import overlap_cases as OC
import overlap_ref as OR
import refit_ref
import test_gpu_instance_point as G
from test_gpu_instance_point import build, member
from test_gpu_ray_query import loaded

pytestmark = pytest.mark.gpu

F = np.float32
EYE = IC.EYE
KS = (0, 1, 2, 3, 4, 5, 8, 9, 64)
SMALL_COUNTS = (1, 63, 64, 65)
PATHS = ("host", "device", "no instance buffer")
COUNTERS = ("node_visits", "leaf_visits", "triangle_tests", "traversals")
_answers = {}


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    _answers.clear()
    for s in G._sets:
        s.close()
    G._sets.clear()
    for _, sc in G._members.values():
        sc.close()
    G._members.clear()


def dev_boxes(boxes):
    import torch
    return torch.from_numpy(np.ascontiguousarray(boxes).view(F).reshape(-1, 8).copy()).cuda()


def restate(positions, of, maps, boxes, k=64):
    member_, first = IO.membership(positions, of, maps, boxes)
    return IO.from_membership(member_, first, k)


def query(s, boxes, k, counts, path, any_only=False):
    """(triangles [n, k], instances [n, k], counts [n]) as numpy, None for what is not returned.  Paths: the blocking host form;
    the device form through triangles_in_boxes on the current torch stream; the device form without an instance buffer."""
    import torch
    n = len(boxes)
    if path == "host":
        tri, inst, cnt = s.triangles_in_boxes(boxes, max_triangles=k, counts=counts, any_only=any_only)
        assert (tri is None) == (k == 0) and (inst is None) == (k == 0) and (cnt is None) == (not counts)
        if k:
            assert tri.dtype == np.int32 and tri.shape == (n, k) and inst.dtype == np.int32 and inst.shape == (n, k)
        return tri, inst, cnt
    if path == "device":
        tri, inst, cnt = s.triangles_in_boxes(dev_boxes(boxes), max_triangles=k, counts=counts, any_only=any_only)
        torch.cuda.current_stream().synchronize()
        assert (tri is None) == (k == 0) and (inst is None) == (k == 0) and (cnt is None) == (not counts)
        if k:
            assert tri.dtype == torch.int32 and tuple(tri.shape) == (n, k) and tuple(inst.shape) == (n, k) and inst.is_cuda
        return (tri.cpu().numpy() if k else None), (inst.cpu().numpy() if k else None), (cnt.cpu().numpy() if counts else None)
    assert path == "no instance buffer"
    d_boxes = dev_boxes(boxes)
    out = torch.full((n, max(k, 1)), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    s.triangles_in_boxes_into(d_boxes.data_ptr(), n, out.data_ptr() if k else 0, 0, cnt.data_ptr() if counts else 0, k, any_only,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    return (out.cpu().numpy() if k else None), None, (cnt.cpu().numpy() if counts else None)


def assert_answer(got, want64, k, counts, what):
    tri, inst, cnt = got
    w_tri, w_inst, w_cnt = want64
    if k:
        bad = np.nonzero((tri != w_tri[:len(tri), :k]).any(1))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {len(tri)} boxes differ, first {bad[:5]}: got {tri[bad[:3]]} want {w_tri[bad[:3], :k]}"
        if inst is not None:
            assert np.array_equal(inst, w_inst[:len(inst), :k]), (what, np.nonzero((inst != w_inst[:len(inst), :k]).any(1))[0][:5])
    else:
        assert tri is None and inst is None, what
    if counts:
        assert cnt.dtype == np.int32 and np.array_equal(cnt, w_cnt[:len(cnt)]), (what, np.nonzero(cnt != w_cnt[:len(cnt)])[0][:5])
    else:
        assert cnt is None, what


def check_every_form(s, boxes, want64, what):
    """every K with and without counts and the ANY form on the three paths at all the boxes, the two short forms, and the small
    counts (where the last wave is partial, full, and one lane over) at the Ks on either side of the register slots' edge;
    K = 0 without counts is refused by the binding"""
    import torch
    touched = (want64[2] > 0).astype(np.int32)
    for k in KS:
        for counts in (True, False):
            if k == 0 and not counts:
                with pytest.raises(ValueError):
                    s.triangles_in_boxes(boxes, max_triangles=0, counts=False)
                continue
            for path in PATHS:
                assert_answer(query(s, boxes, k, counts, path), want64, k, counts, f"{what}, K = {k}, counts = {counts}, {path}")
    for path in PATHS:
        got = query(s, boxes, 0, True, path, any_only=True)
        assert got[0] is None and got[1] is None and got[2].dtype == np.int32 and np.array_equal(got[2], touched), f"{what}, ANY, {path}"
    assert np.array_equal(s.box_counts(boxes), want64[2]) and np.array_equal(s.boxes_touched(boxes), touched != 0), what
    on_device = s.boxes_touched(dev_boxes(boxes))
    assert on_device.dtype == torch.bool and np.array_equal(on_device.cpu().numpy(), touched != 0), what
    for count in SMALL_COUNTS:
        for k, counts in ((1, False), (8, True), (9, False), (64, True)):
            for path in PATHS:
                assert_answer(query(s, boxes[:count], k, counts, path), want64, k, counts,
                              f"{what}, {count} boxes, K = {k}, counts = {counts}, {path}")


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_trisrc", "lobed_528", "one triangle", "11-triangle leaf"])
def test_one_identity_instance_is_the_box_overlap_query(pkg, gpu, name):
    """Scene.triangles_in_boxes' indices and counts with instance 0 on every held slot, and its three counters: the root of a
    one-instance set is not tested, and an identity map's image boxes are the boxes."""
    positions, sc = member(pkg, name)
    s = build(pkg, [name], EYE[None], name)
    boxes = OC.make_boxes({"vertex_positions": positions}, XC.NINE_BOXES, seed=len(name))
    tri, cnt = sc.triangles_in_boxes(boxes, max_triangles=64)
    want, want_cnt = OR.overlap(positions, boxes, 64)
    assert np.array_equal(tri, want) and np.array_equal(cnt, want_cnt), "the plain query is the restatement"
    assert (cnt == 0).mean() > 0.1 and (cnt > 0).mean() > 0.3
    want64 = (tri, np.where(tri >= 0, 0, -1).astype(np.int32), cnt)
    check_every_form(s, boxes, want64, f"{name}, identity")
    walked = int(OR.walked(boxes).sum())
    for k, counts, any_only in ((8, True, False), (0, True, False), (64, False, False), (0, True, True)):
        plain = sc.triangles_in_boxes(boxes, max_triangles=k, counts=counts, counters=True, any_only=any_only)[-1]
        got = s.triangles_in_boxes(boxes, max_triangles=k, counts=counts, counters=True, any_only=any_only)
        if any_only:
            assert np.array_equal(got[2], (cnt > 0).astype(np.int32))
        else:
            assert_answer(got[:3], want64, k, counts, f"{name}, counting form, K = {k}")
        tally = got[3]
        for c in ("node_visits", "leaf_visits", "triangle_tests", "samples"):
            assert tally[c] == plain[c], (name, k, any_only, c, tally, plain)
        assert tally["traversals"] == walked and tally["shaded_hits"] == tally["env_lookups"] == tally["bad_hits"] == 0


# 2 ---------------------------------------------------------------------------------------------------------------------------
def nine(pkg):
    """(names, distinct positions, scene of every instance, maps, the set, boxes, the restatement at K = 64, first-axis codes)"""
    if "nine" not in _answers:
        positions, of, maps, kinds, names = XC.nine_instances(lambda name: member(pkg, name)[0])
        assert kinds[4] == "duplicate of 1" and names[4] == names[1] and np.array_equal(maps[4].view(np.uint32), maps[1].view(np.uint32))
        s = build(pkg, names, maps, "nine instances")
        boxes = XC.world_boxes(positions, of, maps)
        merged, first = IP.merged_positions(positions, of, maps)
        code = OR.first_axis(merged, boxes)
        _answers["nine"] = (names, positions, of, maps, s, boxes, IO.from_membership(code == OR.OVERLAP, first, 64), code)
    return _answers["nine"]


def test_the_nine_instance_set(pkg, gpu):
    names, positions, of, maps, s, boxes, want64, code = nine(pkg)
    print(XC.assert_mixed(boxes, want64[1], want64[2], code, "nine instances"))
    check_every_form(s, boxes, want64, "nine instances")
    inst = want64[1]
    assert ((inst == 1).sum(1) >= (inst == 4).sum(1)).all() and (inst == 4).sum() > 100, "the duplicate sorts behind its original"


def stored_boxes(pkg, s, n):
    """the boxes the set's top level stores for its instances, from the nodes as the next query reads them"""
    N = pkg._native.load_instance()
    count = C.c_int32()
    assert N.shrayi_instance_set_arrays(s._handle, None, None, C.byref(count)) == 0
    nodes = np.zeros((count.value, 8), np.uint32)
    assert N.shrayi_instance_set_arrays(s._handle, nodes.ctypes.data_as(C.c_void_p), None, None) == 0
    stored = {int(row[7] & 0x7fffffff): (row.view(F)[0:3].copy(), row.view(F)[4:7].copy()) for row in nodes if row[7] & 0x80000000}
    assert sorted(stored) == list(range(n))
    return stored


def test_the_counters_of_the_nine_instance_set(pkg, gpu):
    """node_visits, leaf_visits, triangle_tests and traversals of the counting form, equal to the sum over the instances of
    instance_overlap_ref.walk_counters on the member's own tree, with the box the set's top level stores for the instance: a
    lane walks an instance exactly when no guarded axis separates that box from its query box (the boxes above it hold it)."""
    names, positions, of, maps, s, boxes, want64, _ = nine(pkg)
    boxes = boxes[:512]
    stored = stored_boxes(pkg, s, 9)
    world = loaded(pkg, "lobed_528")[0]
    desc = world.export_tree()
    lobed_tree = refit_ref.TreeArrays.of(desc)
    vd = np.ctypeslib.as_array(desc.vertex_data, shape=(desc.vertex_count * 9,)).reshape(-1, 9)
    lobed_corners = np.ascontiguousarray(vd[lobed_tree.triangle_vertices][:, :, :3])
    assert np.array_equal(lobed_corners.reshape(-1).view(np.uint32), positions[0].view(np.uint32)), "the scene's triangles are in the tree's order"
    i32 = lambda *v: np.array(v, np.int32)
    trees = {}
    for name, p in zip(("lobed_528", "one triangle", "11-triangle leaf"), positions):
        corners = p.reshape(-1, 3, 3)
        if name == "lobed_528":
            trees[name] = (lobed_tree, lobed_tree.box, corners)
        else:
            v = corners.reshape(-1, 3)
            box = np.concatenate([v.min(0) - 1e-5, v.max(0) + 1e-5]).astype(F)[None]        # helpers.single_leaf_scene's
            trees[name] = (refit_ref.TreeArrays(i32(-1), i32(-1), i32(-1), None, None, i32(0), i32(len(corners)), None), box, corners)
    total = dict.fromkeys(COUNTERS, 0)
    touching = np.zeros(len(boxes), np.int64)
    for i, name in enumerate(names):
        tree, node_boxes, corners = trees[name]
        w = IO.walk_counters(tree, node_boxes, corners, maps[i], boxes, top_box=stored[i])
        assert (w["touching"][w["traversals"] == 0] == 0).all(), "no pair is behind a culled instance"
        for c in COUNTERS:
            total[c] += int(w[c].sum())
        touching += w["touching"]
    assert np.array_equal(touching * OR.walked(boxes), want64[2][:len(boxes)]), "the counting walk finds every member"
    walked = int(OR.walked(boxes).sum())
    assert walked < total["traversals"] < 9 * walked, "the top level culls some instances and not all"
    for k, counts in ((8, True), (64, False), (0, True)):
        got = s.triangles_in_boxes(boxes, max_triangles=k, counts=counts, counters=True)
        assert_answer(got[:3], want64, k, counts, f"nine instances, counting form, K = {k}")
        for c in COUNTERS:
            assert got[3][c] == total[c], (k, c, got[3], total)
        assert got[3]["samples"] == len(boxes)


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["two scenes of different heights", "301 tiny instances"])
def test_sets_equal_the_restatement(pkg, gpu, which):
    names, maps, kinds = G.the_set(pkg, which)
    s = build(pkg, names, maps, which)
    distinct = sorted(set(names))
    positions, of = [member(pkg, d)[0] for d in distinct], [distinct.index(x) for x in names]
    boxes = XC.world_boxes(positions, of, maps, XC.NINE_BOXES, seed=len(names) + 7)
    want64 = restate(positions, of, maps, boxes)
    cnt, inst = want64[2], want64[1]
    assert (cnt == 0).mean() > 0.05 and ((cnt > 0) & (cnt <= 64)).mean() > 0.04 and (cnt > 64).mean() > 0.04, (which, np.bincount(np.minimum(cnt, 65)))
    assert len(set(inst[inst >= 0].tolist())) >= min(len(names), 12), "the held pairs come from many instances"
    check_every_form(s, boxes, want64, which)


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_refit_update_and_query_on_one_stream_and_after_a_host_update(pkg, gpu):
    """A device refit of a member, a device update with moved maps and the query, enqueued on one side stream with nothing
    between them; then a host update with other maps followed by the query on all paths.  Each against the restatement of the
    state the query must see."""
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
    K = 8
    try:
        moved = (before.reshape(-1, 3) * F(1.3) + F(0.2)).astype(F)
        now = [moved.reshape(-1), small_positions]
        boxes = XC.world_boxes(now, of, maps[1], XC.NINE_BOXES, seed=71)
        first = query(s, boxes, K, True, "host")
        d_moved, d_maps, d_boxes = torch.from_numpy(moved).cuda(), torch.from_numpy(maps[1]).cuda(), dev_boxes(boxes)
        d_out = torch.full((len(boxes), K), -7, dtype=torch.int32, device="cuda")
        d_inst = torch.full((len(boxes), K), -7, dtype=torch.int32, device="cuda")
        d_cnt = torch.full((len(boxes),), -7, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            own.refit(d_moved, stream_ptr=side.cuda_stream)
            s.update_into(d_maps.data_ptr(), side.cuda_stream)
            s.triangles_in_boxes_into(d_boxes.data_ptr(), len(boxes), d_out.data_ptr(), d_inst.data_ptr(), d_cnt.data_ptr(), K, False,
                                      side.cuda_stream)
        side.synchronize()
        assert s.update_status() == -1
        want = restate(now, of, maps[1], boxes)
        assert (first[0] != want[0][:, :K]).any(1).sum() > 300, "the refit and the update moved something"
        assert_answer((d_out.cpu().numpy(), d_inst.cpu().numpy(), d_cnt.cpu().numpy()), want, K, True, "one stream")
        # a host update: the device copy of the maps is behind it until the next query stages them on its stream
        s.update(maps[2])
        want2 = restate(now, of, maps[2], boxes)
        assert (want2[0] != want[0]).any(1).sum() > 300, "the host update moved something"
        for path in PATHS:
            assert_answer(query(s, boxes, K, True, path), want2, K, True, f"after a host update, {path}")
            assert_answer(query(s, boxes, 9, False, path), want2, 9, False, f"after a host update, K = 9, {path}")
    finally:
        s.close()
        own.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_surface_voxels_are_the_merged_scene_s(pkg, gpu, tmp_path):
    """The 16 x 16 x 16 occupancy grid of three placed copies of lobed_528, numpy and torch, equal to Scene.surface_voxels of
    the merged scene (the mapped corners written to a file and loaded as a scene of its own) and to the restatement."""
    import torch
    positions, _ = member(pkg, "lobed_528")
    names = ["lobed_528"] * 3
    _, maps, _ = IC.make_set([positions], [0, 0, 0], seed=81, spread=0.7, kinds=["rotation_nonuniform", "mirror", "shear"])
    s = build(pkg, names, maps, "three copies")
    merged, _ = IP.merged_positions([positions], [0, 0, 0], maps)
    path = tmp_path / "merged.obj"
    v = merged.reshape(-1, 3)
    path.write_text("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v) + "".join(f"f {3 * t + 1} {3 * t + 2} {3 * t + 3}\n" for t in range(len(v) // 3)))
    world = pkg.World(str(path))
    scene = pkg.Scene(world.flatten())
    try:
        loaded_back = np.asarray(scene.geometry()["vertex_positions"], F).reshape(-1, 9)
        assert set(map(bytes, loaded_back)) == set(map(bytes, merged.reshape(-1, 9))), "the merged scene holds the mapped corners' bits"
        lo, hi = v.min(0), v.max(0)
        dims = (16, 16, 16)
        origin = (lo - F(0.01)).astype(F)
        cell = ((hi - lo + F(0.02)) / F(16)).astype(F)
        want = scene.surface_voxels(origin, cell, dims)
        assert 0.05 < want.mean() < 0.95, want.mean()
        assert np.array_equal(want, OR.overlaps(merged, pkg.tracer.voxel_boxes(origin, cell, dims)).any(1).reshape(dims))
        grid = s.surface_voxels(origin, cell, dims)
        assert grid.dtype == np.bool_ and grid.shape == dims and np.array_equal(grid, want)
        grid = s.surface_voxels(origin, cell, dims, device="cuda")
        assert grid.dtype == torch.bool and grid.is_cuda and tuple(grid.shape) == dims and np.array_equal(grid.cpu().numpy(), want)
    finally:
        scene.close()
        world.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_a_count_split_over_two_launches(pkg, gpu):
    """2^24 + 3000 boxes (one launch holds 2^24) on the one-triangle scene placed twice, K = 2: far boxes touch nothing; the
    last launch's boxes and real boxes scattered over the first launch are restated.  Slot box * K of the last boxes lies
    beyond 2^25 indices: indexed in 64 bits."""
    import torch
    positions, _ = member(pkg, "one triangle")
    names = ["one triangle", "one triangle"]
    _, maps, _ = IC.make_set([positions], [0, 0], seed=5, spread=0.3, kinds=["rotation_nonuniform", "mirror"])
    s = build(pkg, names, maps, "one triangle, twice")
    n, K = (1 << 24) + 3000, 2
    real = XC.world_boxes([positions], [0, 0], maps, 3000 + 4096, seed=33)
    tail, spread = real[:3000], real[3000:]
    far = OR.make_boxes([[1e6, -2e6, 3e6]], [[1e6 + 1, -2e6 + 1, 3e6 + 1]])
    d_boxes = dev_boxes(far).repeat(n, 1)
    d_boxes[n - 3000:] = dev_boxes(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, 4096, replace=False)).cuda()
    d_boxes[sample] = dev_boxes(spread)
    d_out = torch.empty((n, K), dtype=torch.int32, device="cuda")
    d_inst = torch.empty((n, K), dtype=torch.int32, device="cuda")
    d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    s.triangles_in_boxes_into(d_boxes.data_ptr(), n, d_out.data_ptr(), d_inst.data_ptr(), d_cnt.data_ptr(), K, False,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    want = restate([positions], [0, 0], maps, tail, K)
    assert (want[2] == 2).sum() > 30 and (want[2] == 1).sum() > 30 and (want[2] == 0).sum() > 100, np.bincount(want[2])
    assert_answer((d_out[n - 3000:].cpu().numpy(), d_inst[n - 3000:].cpu().numpy(), d_cnt[n - 3000:].cpu().numpy()), want, K, True,
                  "the last launch's boxes")
    want = restate([positions], [0, 0], maps, spread, K)
    assert_answer((d_out[sample].cpu().numpy(), d_inst[sample].cpu().numpy(), d_cnt[sample].cpu().numpy()), want, K, True,
                  "boxes of the first launch")
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    assert restate([positions], [0, 0], maps, far, K)[2][0] == 0
    assert bool((d_out[: n - 3000][rest] == -1).all()) and bool((d_inst[: n - 3000][rest] == -1).all())
    assert bool((d_cnt[: n - 3000][rest] == 0).all())


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops(pkg, gpu):
    import torch
    s = build(pkg, ["lobed_528"], EYE[None], "refusals")
    tri, inst, cnt = s.triangles_in_boxes(np.zeros((0, 6), F))
    assert tri.shape == (0, 8) and inst.shape == (0, 8) and len(cnt) == 0
    assert len(s.box_counts(np.zeros((0, 8), F))) == 0
    everything = np.array([[-1e3] * 3 + [1e3] * 3] * 4, F)
    assert np.array_equal(s.box_counts(everything), np.full(4, 528, np.int32))
    assert torch.equal(s.box_counts(torch.from_numpy(everything).cuda()).cpu(), torch.full((4,), 528, dtype=torch.int32))
    assert s.boxes_touched(everything).all()
    with pytest.raises(ValueError):
        s.triangles_in_boxes(torch.zeros((4, 5), device="cuda"))
    with pytest.raises(ValueError):
        s.triangles_in_boxes(torch.zeros((4, 6), device="cuda"), counters=True)
    with pytest.raises(ValueError):
        s.triangles_in_boxes(everything, max_triangles=0, counts=False)
    for k in (-1, 65):
        with pytest.raises(pkg._native.ShrayError) as err:
            s.triangles_in_boxes(everything, max_triangles=k)
        assert err.value.code == -1
    with pytest.raises(pkg._native.ShrayError):
        s.triangles_in_boxes(everything, max_triangles=8, any_only=True)
    lib = pkg._native.load_instance_overlap()
    d = torch.zeros((64, 8), dtype=torch.int32, device="cuda")
    call, V = lib.shray_overlap_triangles_instances_device, C.c_void_p
    op = pkg.tracer._set_overlap_params(1)
    base = d.data_ptr()
    assert call(s._handle, C.byref(op), V(base + 4), 1, V(base + 32), None, None, None) == -1
    assert call(s._handle, C.byref(op), V(base), 1, V(base + 34), None, None, None) == -1
    assert call(s._handle, C.byref(op), V(base), 1, V(base + 32), V(base + 98), None, None) == -1
    assert call(s._handle, C.byref(op), V(base), 1, V(base + 32), None, V(base + 98), None) == -1
    assert call(s._handle, C.byref(op), V(base), 1, None, None, V(base + 100), None) == -1          # K = 1 without indices
    assert call(s._handle, C.byref(op), V(base), 1, V(base + 36), V(base + 100), V(base + 104), None) == 0
    assert call(s._handle, C.byref(op), V(base), 0, V(base + 32), None, None, None) == 0
    torch.cuda.synchronize()
