"""Instanced within-radius queries on the GPU (include/shader_ray_instance_near.h) against the restatement
(tests/instance_near_ref.py): every byte of every record, every instance index and every count, on the host and the device
path, for K in {0, 1, 2, 3, 8, 9, 64} with counts, without counts and without an instance buffer (the scratch path above
K = 8), with 1, 63, 64, 65 and 1,536 points.  One identity instance against Scene.triangles_within (bytes, counts and its three
counters); K = 1 without counts against InstanceSet.closest_points; the nine-instance set of tests/instance_near_cases.py, two
scenes of different heights and 301 instances of the tiny scenes; the counters of the nine-instance set against
instance_near_ref.walk_counters; a refit, a device update and the query on one stream, and a host update followed by the
query; a count split over two launches; the refusals."""
import ctypes as C

import numpy as np
import pytest

import instance_near_cases as NC
import instance_near_ref as IN
import instance_point_cases as IC
import near_ref as NR
import point_query_ref as R
import refit_ref
import test_gpu_instance_point as G
from test_gpu_instance_point import build, dev_points, member
from test_gpu_ray_query import loaded

pytestmark = pytest.mark.gpu

F = np.float32
EYE = IC.EYE
KS = (0, 1, 2, 3, 8, 9, 64)
SMALL_COUNTS = (1, 63, 64, 65)
POINTS = 1536
NUMPY_PAIRS = 10 ** 6
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


def restate(positions, of, maps, pts, k=64):
    pairs = len(pts) * sum(len(positions[s]) // 9 for s in of)
    return IN.near_over_instances(positions, of, maps, pts, k, device="cuda" if pairs > NUMPY_PAIRS else None)


def records(t, k):
    return np.ascontiguousarray(t.cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1, k)


def query(s, pts, k, counts, path):
    """(records [n, k], instances [n, k], counts [n]) as numpy, None for what is not returned.  Paths: the blocking host form;
    the device form through triangles_within on the current torch stream; the device form without an instance buffer."""
    import torch
    n = len(pts)
    if path == "host":
        rec, inst, cnt = s.triangles_within(pts, max_near=k, counts=counts)
        assert (rec is None) == (k == 0) and (inst is None) == (k == 0) and (cnt is None) == (not counts)
        if k:
            assert rec.dtype == R.CLOSEST_DTYPE and rec.shape == (n, k) and inst.dtype == np.int32 and inst.shape == (n, k)
        return rec, inst, cnt
    if path == "device":
        rec, inst, cnt = s.triangles_within(dev_points(pts), max_near=k, counts=counts)
        torch.cuda.current_stream().synchronize()
        assert (rec is None) == (k == 0) and (inst is None) == (k == 0) and (cnt is None) == (not counts)
        if k:
            assert rec.dtype == torch.int32 and tuple(rec.shape) == (n, k, 8) and tuple(inst.shape) == (n, k) and inst.is_cuda
        return (records(rec, k) if k else None), (inst.cpu().numpy() if k else None), (cnt.cpu().numpy() if counts else None)
    assert path == "no instance buffer"
    d_pts = dev_points(pts)
    out = torch.full((n, max(k, 1), 8), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    s.triangles_within_into(d_pts.data_ptr(), n, out.data_ptr() if k else 0, 0, cnt.data_ptr() if counts else 0, k,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    return (records(out, k) if k else None), None, (cnt.cpu().numpy() if counts else None)


def assert_answer(got, want64, k, counts, what):
    rec, inst, cnt = got
    w_rec, w_inst, w_cnt = want64
    if k:
        g, w = NR.as_bits(rec), NR.as_bits(w_rec[:len(rec), :k])
        bad = np.nonzero((g != w).any(1))[0]
        assert len(bad) == 0, (f"{what}: {len(bad)} of {len(g)} records differ, first (flat index) {bad[:5]}: got {rec.reshape(-1)[bad[:3]]} "
                               f"want {w_rec[:len(rec), :k].reshape(-1)[bad[:3]]}")
        if inst is not None:
            assert np.array_equal(inst, w_inst[:len(inst), :k]), (what, np.nonzero((inst != w_inst[:len(inst), :k]).any(1))[0][:5])
    else:
        assert rec is None and inst is None, what
    if counts:
        assert cnt.dtype == np.int32 and np.array_equal(cnt, w_cnt[:len(cnt)]), (what, np.nonzero(cnt != w_cnt[:len(cnt)])[0][:5])
    else:
        assert cnt is None, what


def check_every_form(s, pts, want64, what):
    """every K with and without counts on the three paths at all the points, and the small counts (where the last wave is
    partial, full, and one lane over) at the Ks on either side of the register slots' edge; K = 0 without counts is refused by
    the binding"""
    for k in KS:
        for counts in (True, False):
            if k == 0 and not counts:
                with pytest.raises(ValueError):
                    s.triangles_within(pts, max_near=0, counts=False)
                continue
            for path in ("host", "device", "no instance buffer"):
                assert_answer(query(s, pts, k, counts, path), want64, k, counts, f"{what}, K = {k}, counts = {counts}, {path}")
    for count in SMALL_COUNTS:
        for k, counts in ((1, False), (8, True), (9, False), (64, True)):
            for path in ("host", "device", "no instance buffer"):
                assert_answer(query(s, pts[:count], k, counts, path), want64, k, counts,
                              f"{what}, {count} points, K = {k}, counts = {counts}, {path}")


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_trisrc", "lobed_528", "one triangle", "11-triangle leaf"])
def test_one_identity_instance_is_the_within_radius_query(pkg, gpu, name):
    """Scene.triangles_within's bytes and counts with instance 0 on every held record, and its three counters: the root of a
    one-instance set is not tested, and an identity map's image boxes are the boxes."""
    positions, sc = member(pkg, name)
    s = build(pkg, [name], EYE[None], name)
    pts, _, _ = NC.world_points([positions], [0], EYE[None], POINTS, seed=len(name))
    rec, cnt = sc.triangles_within(pts, max_near=64)
    want, want_cnt = NR.near(positions, pts, 64)
    assert np.array_equal(NR.as_bits(rec), NR.as_bits(want)) and np.array_equal(cnt, want_cnt), "the plain query is the restatement"
    assert (cnt == 0).mean() > 0.1 and (cnt > 0).mean() > 0.3
    want64 = (rec, np.where(rec["triangle"] >= 0, 0, -1).astype(np.int32), cnt)
    check_every_form(s, pts, want64, f"{name}, identity")
    walked = int(NR.walked(pts).sum())
    for k, counts in ((8, True), (0, True), (64, False)):
        _, _, plain = sc.triangles_within(pts, max_near=k, counts=counts, counters=True)[-3:]
        got = s.triangles_within(pts, max_near=k, counts=counts, counters=True)
        assert_answer(got[:3], want64, k, counts, f"{name}, counting form, K = {k}")
        tally = got[3]
        for c in ("node_visits", "leaf_visits", "triangle_tests", "samples"):
            assert tally[c] == plain[c], (name, k, c, tally, plain)
        assert tally["traversals"] == walked and tally["shaded_hits"] == tally["env_lookups"] == tally["bad_hits"] == 0


# 2 ---------------------------------------------------------------------------------------------------------------------------
def nine(pkg):
    """(names, distinct positions, scene of every instance, maps, the set, points, radius classes, the restatement at K = 64)"""
    if "nine" not in _answers:
        positions, of, maps, kinds, names = NC.nine_instances(lambda name: member(pkg, name)[0])
        assert kinds[4] == "duplicate of 1" and names[4] == names[1] and np.array_equal(maps[4].view(np.uint32), maps[1].view(np.uint32))
        s = build(pkg, names, maps, "nine instances")
        pts, _, radius = NC.world_points(positions, of, maps, NC.NINE_POINTS, NC.NINE_POINT_SEED)
        _answers["nine"] = (names, positions, of, maps, s, pts, radius, restate(positions, of, maps, pts))
    return _answers["nine"]


def test_the_nine_instance_set(pkg, gpu):
    names, positions, of, maps, s, pts, radius, want64 = nine(pkg)
    print(NC.assert_mixed(pts, radius, *want64, "nine instances"))
    part = IN.near_over_instances(positions, of, maps, pts[:48], 64)       # the brute force went through torch: a part against numpy
    assert_answer(part, want64, 64, True, "the torch restatement against numpy")
    check_every_form(s, pts, want64, "nine instances")
    inst = want64[1]
    assert ((inst == 1).sum(1) >= (inst == 4).sum(1)).all() and (inst == 4).sum() > 100, "the duplicate sorts behind its original"


def test_k_1_without_counts_is_the_instanced_closest_point(pkg, gpu):
    import torch
    _, _, _, _, s, pts, _, _ = nine(pkg)
    want, want_inst = s.closest_points(pts)
    assert 0.1 < (want_inst < 0).mean() < 0.9
    for path in ("host", "device"):
        rec, inst, _ = query(s, pts, 1, False, path)
        assert np.array_equal(NR.as_bits(rec[:, 0]), NR.as_bits(want)) and np.array_equal(inst[:, 0], want_inst), path
    torch.cuda.synchronize()


def test_the_counters_of_the_nine_instance_set(pkg, gpu):
    """node_visits, leaf_visits, triangle_tests and traversals of the counting form, equal to the sum over the instances of
    instance_near_ref.walk_counters on the member's own tree, with the box the set's top level stores for the instance: a lane
    walks an instance exactly when the bound of that box is not above its max_dist2 (the boxes above it hold it)."""
    names, positions, of, maps, s, pts, _, want64 = nine(pkg)
    pts = pts[:512]
    N = pkg._native.load_instance()
    count = C.c_int32()
    assert N.shrayi_instance_set_arrays(s._handle, None, None, C.byref(count)) == 0
    nodes = np.zeros((count.value, 8), np.uint32)
    assert N.shrayi_instance_set_arrays(s._handle, nodes.ctypes.data_as(C.c_void_p), None, None) == 0
    stored = {int(row[7] & 0x7fffffff): (row.view(F)[0:3], row.view(F)[4:7]) for row in nodes if row[7] & 0x80000000}
    assert sorted(stored) == list(range(9))
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
    near = np.zeros(len(pts), np.int64)
    for i, name in enumerate(names):
        tree, boxes, corners = trees[name]
        w = IN.walk_counters(tree, boxes, corners, maps[i], pts, top_box=stored[i], device="cuda")
        for c in COUNTERS:
            total[c] += int(w[c].sum())
        near += w["near"]
    assert np.array_equal(near, want64[2][:len(pts)]), "the counting walk finds every member"
    walked = int(NR.walked(pts).sum())
    assert walked < total["traversals"] < 9 * walked, "the top level culls some instances and not all"
    for k, counts in ((8, True), (64, False), (0, True)):
        got = s.triangles_within(pts, max_near=k, counts=counts, counters=True)
        assert_answer(got[:3], want64, k, counts, f"nine instances, counting form, K = {k}")
        for c in COUNTERS:
            assert got[3][c] == total[c], (k, c, got[3], total)
        assert got[3]["samples"] == len(pts)


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["two scenes of different heights", "301 tiny instances"])
def test_sets_equal_the_restatement(pkg, gpu, which):
    names, maps, kinds = G.the_set(pkg, which)
    s = build(pkg, names, maps, which)
    distinct = sorted(set(names))
    positions, of = [member(pkg, d)[0] for d in distinct], [distinct.index(x) for x in names]
    pts, _, _ = NC.world_points(positions, of, maps, POINTS, seed=len(names) + 7)
    want64 = restate(positions, of, maps, pts)
    part = IN.near_over_instances(positions, of, maps, pts[:48], 64)
    assert_answer(part, want64, 64, True, "the torch restatement against numpy")
    cnt, inst = want64[2], want64[1]
    assert (cnt == 0).mean() > 0.1 and ((cnt > 0) & (cnt <= 64)).mean() > 0.04 and (cnt > 64).mean() > 0.2, which
    assert len(set(inst[inst >= 0].tolist())) >= min(len(names), 12), "the records come from many instances"
    check_every_form(s, pts, want64, which)


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
    K = 8
    try:
        moved = (before.reshape(-1, 3) * F(1.3) + F(0.2)).astype(F)
        now = [moved.reshape(-1), small_positions]
        pts, _, _ = NC.world_points(now, of, maps[1], POINTS, seed=71)
        first = query(s, pts, K, True, "host")
        d_moved, d_maps, d_pts = torch.from_numpy(moved).cuda(), torch.from_numpy(maps[1]).cuda(), dev_points(pts)
        d_out = torch.full((len(pts), K, 8), -7, dtype=torch.int32, device="cuda")
        d_inst = torch.full((len(pts), K), -7, dtype=torch.int32, device="cuda")
        d_cnt = torch.full((len(pts),), -7, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            own.refit(d_moved, stream_ptr=side.cuda_stream)
            s.update_into(d_maps.data_ptr(), side.cuda_stream)
            s.triangles_within_into(d_pts.data_ptr(), len(pts), d_out.data_ptr(), d_inst.data_ptr(), d_cnt.data_ptr(), K, side.cuda_stream)
        side.synchronize()
        assert s.update_status() == -1
        want = restate(now, of, maps[1], pts)
        assert (NR.as_bits(first[0]) != NR.as_bits(want[0][:, :K])).any(1).sum() > 500, "the refit and the update moved something"
        assert_answer((records(d_out, K), d_inst.cpu().numpy(), d_cnt.cpu().numpy()), want, K, True, "one stream")
        # a host update: the device copy of the maps is behind it until the next query stages them on its stream
        s.update(maps[2])
        want2 = restate(now, of, maps[2], pts)
        assert (NR.as_bits(want2[0]) != NR.as_bits(want[0])).any(1).sum() > 500, "the host update moved something"
        for path in ("device", "host", "no instance buffer"):
            assert_answer(query(s, pts, K, True, path), want2, K, True, f"after a host update, {path}")
            assert_answer(query(s, pts, 9, False, path), want2, 9, False, f"after a host update, K = 9, {path}")
    finally:
        s.close()
        own.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_a_count_split_over_two_launches(pkg, gpu):
    """2^24 + 3000 points (one launch holds 2^24) on the one-triangle scene placed twice, K = 2: far points with radius 0 are
    misses; the last launch's points and real points scattered over the first launch are restated.  Slot point * K of the last
    points lies beyond 2^25 records, byte offset beyond 2^30: indexed in 64 bits."""
    import torch
    positions, _ = member(pkg, "one triangle")
    names = ["one triangle", "one triangle"]
    _, maps, _ = IC.make_set([positions], [0, 0], seed=5, spread=1.0, kinds=["rotation_nonuniform", "mirror"])
    s = build(pkg, names, maps, "one triangle, twice")
    n, K = (1 << 24) + 3000, 2
    real, _, _ = NC.world_points([positions], [0, 0], maps, 3000 + 4096, seed=33)
    tail, spread = real[:3000], real[3000:]
    far = np.zeros(1, R.POINT_DTYPE)
    far["p"] = (1e6, -2e6, 3e6)
    far["max_dist2"] = 0.0
    d_pts = dev_points(far).repeat(n, 1)
    d_pts[n - 3000:] = dev_points(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, 4096, replace=False)).cuda()
    d_pts[sample] = dev_points(spread)
    d_out = torch.empty((n, K, 8), dtype=torch.int32, device="cuda")
    d_inst = torch.empty((n, K), dtype=torch.int32, device="cuda")
    d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    s.triangles_within_into(d_pts.data_ptr(), n, d_out.data_ptr(), d_inst.data_ptr(), d_cnt.data_ptr(), K, torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    want = restate([positions], [0, 0], maps, tail, K)
    assert (want[2] == 2).sum() > 100 and (want[2] == 0).sum() > 100
    assert_answer((records(d_out[n - 3000:], K), d_inst[n - 3000:].cpu().numpy(), d_cnt[n - 3000:].cpu().numpy()), want, K, True,
                  "the last launch's points")
    want = restate([positions], [0, 0], maps, spread, K)
    assert_answer((records(d_out[sample], K), d_inst[sample].cpu().numpy(), d_cnt[sample].cpu().numpy()), want, K, True,
                  "points of the first launch")
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    far_want = restate([positions], [0, 0], maps, far, K)
    assert (far_want[0]["triangle"] == -1).all() and (far_want[1] == -1).all() and far_want[2][0] == 0
    far_record = torch.from_numpy(NR.as_bits(far_want[0]).view(np.int32).copy()).cuda()
    assert bool((d_out[: n - 3000][rest] == far_record).all()) and bool((d_inst[: n - 3000][rest] == -1).all())
    assert bool((d_cnt[: n - 3000][rest] == 0).all())


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops(pkg, gpu):
    import torch
    s = build(pkg, ["lobed_528"], EYE[None], "refusals")
    rec, inst, cnt = s.triangles_within(np.zeros((0, 3), F))
    assert rec.shape == (0, 8) and inst.shape == (0, 8) and len(cnt) == 0
    assert len(s.near_counts(np.zeros((0, 4), F))) == 0
    pts = np.zeros((4, 4), F)
    pts[:, 3] = np.inf
    assert np.array_equal(s.near_counts(pts), np.full(4, 528, np.int32))
    assert torch.equal(s.near_counts(torch.from_numpy(pts).cuda()).cpu(), torch.full((4,), 528, dtype=torch.int32))
    with pytest.raises(ValueError):
        s.triangles_within(torch.zeros((4, 5), device="cuda"))
    with pytest.raises(ValueError):
        s.triangles_within(torch.zeros((4, 4), device="cuda"), counters=True)
    with pytest.raises(ValueError):
        s.triangles_within(pts, max_near=0, counts=False)
    for k in (-1, 65):
        with pytest.raises(pkg._native.ShrayError) as err:
            s.triangles_within(pts, max_near=k)
        assert err.value.code == -1
    lib = pkg._native.load_instance_near()
    d = torch.zeros((64, 8), dtype=torch.int32, device="cuda")
    call, V = lib.shray_near_triangles_instances_device, C.c_void_p
    np_ = pkg.tracer.near_params(1)
    base = d.data_ptr()
    assert call(s._handle, C.byref(np_), V(base + 4), 1, V(base + 32), None, None, None) == -1
    assert call(s._handle, C.byref(np_), V(base), 1, V(base + 40), None, None, None) == -1
    assert call(s._handle, C.byref(np_), V(base), 1, V(base + 32), V(base + 98), None, None) == -1
    assert call(s._handle, C.byref(np_), V(base), 1, V(base + 32), None, V(base + 98), None) == -1
    assert call(s._handle, C.byref(np_), V(base), 1, None, None, V(base + 100), None) == -1          # K = 1 without records
    assert call(s._handle, C.byref(np_), V(base), 1, V(base + 32), V(base + 100), V(base + 104), None) == 0
    assert call(s._handle, C.byref(np_), V(base), 0, V(base + 32), None, None, None) == 0
    torch.cuda.synchronize()
