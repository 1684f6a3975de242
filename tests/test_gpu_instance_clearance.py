"""Instanced triangle-distance queries on the GPU (include/shader_ray_instance_clearance.h) against the restatement
(tests/instance_clearance_ref.py): all 48 bytes of every record, every instance index and every count, on the host path, the
device path and the device path without an instance buffer (the scratch path above K = 8), for K in {0, 1, 2, 4, 8, 9, 64} with
and without counts, max_dist2 in {0, (4 %)^2, +inf, -1, NaN}, SHRAY_CLEARANCE_SKIP_SHARED and SHRAY_CLEARANCE_ANY, with 1, 63, 64,
65 and 600 queries.  One identity instance against Scene.triangle_distances (bytes, counts and its three counters) and, in the
instance form, against Scene.self_clearance; the nine-instance set of tests/instance_clearance_cases.py in the item form and,
for every instance, in the instance form with and without SHRAY_CLEARANCE_SKIP_OWN_INSTANCE; instances_within and
instance_distance against the brute force; two scenes of different heights and 301 instances of the tiny scenes; the counters
of the nine-instance set against instance_clearance_ref.walk_counters with the stored boxes as read back; a refit, a device
update and both device forms on one stream, and a host update followed by the queries; a count split over two launches; the
refusals.

The restatement's pair table of a set's query set is computed once, on the GPU through point_query_ref.TorchOps (each fp32
operation in float64, rounded: exact), and shared by every case of that set; it is never written to."""
import ctypes as C

import numpy as np
import pytest

import clearance_ref as CR
import instance_clearance_cases as XC
import instance_clearance_ref as XR
import instance_point_cases as IC
import instance_point_ref as IP
import intersect_ref as IR
import point_query_ref as PQ
import refit_ref
import test_gpu_instance_point as G
from test_gpu_instance_overlap import stored_boxes
from test_gpu_instance_point import build, member
from test_gpu_ray_query import loaded

pytestmark = pytest.mark.gpu

F = np.float32
EYE = IC.EYE
INF = F(np.inf)
KS = (0, 1, 2, 4, 8, 9, 64)
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


def ops():
    return PQ.TorchOps("cuda")


def dev_triangles(queries):
    import torch
    return torch.from_numpy(IR.make_triangles(queries).view(F).reshape(-1, 12).copy()).cuda()


def table_of(positions, of, maps, queries):
    return XR.merged_table(positions, of, maps, queries, ops(), pairs=1 << 22)


def bits(records):
    """a PAIR_DISTANCE_DTYPE array [n, k] or an int32 [n, k, 12] array as uint32 [n, k * 12]"""
    r = np.ascontiguousarray(records)
    return r.view(np.uint32).reshape(len(r), -1) if len(r) else np.zeros((0, 0), np.uint32)


def query(s, queries, k, counts, path, md=INF, any_only=False, skip_shared=False):
    """(records, instances [n, k], counts [n]) as numpy, None for what is not returned.  Paths: the blocking host form; the
    device form through triangle_distances on the current torch stream; the device form without an instance buffer."""
    import torch
    n = len(queries)
    if path == "host":
        rec, inst, cnt = s.triangle_distances(queries, md, max_pairs=k, counts=counts, any_only=any_only, skip_shared=skip_shared)
        assert (rec is None) == (k == 0) and (inst is None) == (k == 0) and (cnt is None) == (not counts)
        if k:
            assert rec.dtype == CR.PAIR_DISTANCE_DTYPE and rec.shape == (n, k) and inst.dtype == np.int32 and inst.shape == (n, k)
        return rec, inst, cnt
    if path == "device":
        rec, inst, cnt = s.triangle_distances(dev_triangles(queries), md, max_pairs=k, counts=counts, any_only=any_only,
                                              skip_shared=skip_shared)
        torch.cuda.current_stream().synchronize()
        assert (rec is None) == (k == 0) and (inst is None) == (k == 0) and (cnt is None) == (not counts)
        if k:
            assert rec.dtype == torch.int32 and tuple(rec.shape) == (n, k, 12) and tuple(inst.shape) == (n, k) and inst.is_cuda
        return (rec.cpu().numpy() if k else None), (inst.cpu().numpy() if k else None), (cnt.cpu().numpy() if counts else None)
    assert path == "no instance buffer"
    d = dev_triangles(queries)
    out = torch.full((n, max(k, 1), 12), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    s.triangle_distances_into(d.data_ptr(), n, out.data_ptr() if k else 0, 0, cnt.data_ptr() if counts else 0, md, k, any_only, skip_shared,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    return (out.cpu().numpy() if k else None), None, (cnt.cpu().numpy() if counts else None)


def own_query(s, q, k, counts, path, md=INF, any_only=False, skip_shared=False, skip_own=True, first=0, count=None):
    """the instance form on the same three paths"""
    import torch
    if path == "host":
        return s.instance_clearance(q, md, max_pairs=k, counts=counts, any_only=any_only, skip_shared=skip_shared, skip_own=skip_own,
                                    first=first, count=count)
    if path == "device":
        got = s.instance_clearance(q, md, max_pairs=k, counts=counts, any_only=any_only, skip_shared=skip_shared, skip_own=skip_own,
                                   first=first, count=count, device=True)
        torch.cuda.current_stream().synchronize()
        assert all(g is None or (g.is_cuda and g.dtype == torch.int32) for g in got)
        return tuple(None if g is None else g.cpu().numpy() for g in got)
    n = s.triangle_count(q) - first if count is None else count
    out = torch.full((max(n, 1), max(k, 1), 12), -7, dtype=torch.int32, device="cuda")      # (an empty tensor has no pointer)
    cnt = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    s.instance_clearance_into(q, first, n, out.data_ptr() if k else 0, 0, cnt.data_ptr() if counts else 0, md, k, any_only, skip_shared,
                              skip_own, torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    assert bool((out[n:] == -7).all()) and bool((cnt[n:] == -7).all()), "nothing is written past the range"
    return (out[:n].cpu().numpy() if k else None), None, (cnt[:n].cpu().numpy() if counts else None)


def assert_answer(got, want64, k, counts, what):
    rec, inst, cnt = got
    w_rec, w_inst, w_cnt = want64
    if k:
        g, w = bits(rec), bits(w_rec[:len(rec), :k])
        assert g.shape == w.shape, (what, g.shape, w.shape)
        bad = np.nonzero((g != w).any(1))[0]
        if len(bad):
            r = rec if rec.dtype == CR.PAIR_DISTANCE_DTYPE else np.ascontiguousarray(rec).view(CR.PAIR_DISTANCE_DTYPE).reshape(len(rec), -1)
            raise AssertionError(f"{what}: {len(bad)} of {len(g)} queries differ, first {bad[:5]}: got {r[bad[0]][:3]} want {w_rec[bad[0]][:3]}")
        if inst is not None:
            assert np.array_equal(inst, w_inst[:len(inst), :k]), (what, np.nonzero((inst != w_inst[:len(inst), :k]).any(1))[0][:5])
    else:
        assert rec is None and inst is None, what
    if counts:
        assert cnt.dtype == np.int32 and np.array_equal(cnt, w_cnt[:len(cnt)]), (what, np.nonzero(cnt != w_cnt[:len(cnt)])[0][:5])
    else:
        assert cnt is None, what


def check_every_form(s, queries, table, md, what, ks=KS, paths=PATHS, skip_shared=False, small=False):
    """every K with and without counts and the ANY form on the paths at all the queries; with `small` also the small counts
    (where the last wave is partial, full, and one lane over) at the Ks on either side of the register slots' edge"""
    want = XR.from_merged_table(table, queries, 64, md, skip_shared)
    met = (want[2] > 0).astype(np.int32)
    for k in ks:
        for counts in (True, False):
            if k == 0 and not counts:
                continue
            for path in paths:
                assert_answer(query(s, queries, k, counts, path, md, skip_shared=skip_shared), want, k, counts,
                              f"{what}, max_dist2 = {md}, K = {k}, counts = {counts}, SKIP_SHARED = {skip_shared}, {path}")
    for path in paths:
        got = query(s, queries, 0, True, path, md, any_only=True, skip_shared=skip_shared)
        assert got[0] is None and got[1] is None and got[2].dtype == np.int32 and np.array_equal(got[2], met), f"{what}, ANY, {path}"
    if small:
        for count in SMALL_COUNTS:
            for k, counts in ((1, False), (8, True), (9, False), (64, True)):
                for path in paths:
                    assert_answer(query(s, queries[:count], k, counts, path, md), want, k, counts,
                                  f"{what}, {count} queries, K = {k}, counts = {counts}, {path}")
    return want


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_trisrc", "lobed_528", "one triangle", "11-triangle leaf"])
def test_one_identity_instance_is_the_triangle_distance_query(pkg, gpu, name):
    """Consequence 1: Scene.triangle_distances' bytes and counts with instance 0 on every held slot, and its three counters, the
    ANY form's too.  Consequence 7: the instance form without SKIP_OWN_INSTANCE is Scene.self_clearance."""
    import torch
    positions, sc = member(pkg, name)
    s = build(pkg, [name], EYE[None], name)
    queries = XC.world_queries([positions], [0], EYE[None], 300, seed=len(name))
    mid = XC.mid_value([positions], [0], EYE[None])
    table = table_of([positions], [0], EYE[None], queries)
    for skip_shared in (False, True):
        for md in (mid, INF):
            rec, cnt = sc.triangle_distances(queries, md, max_pairs=64, skip_shared=skip_shared)
            want = XR.from_merged_table(table, queries, 64, md, skip_shared)
            assert np.array_equal(bits(rec), bits(want[0])) and np.array_equal(cnt, want[2]), "the plain query is the restatement"
            assert np.array_equal(want[1], np.where(rec["triangle"] >= 0, 0, -1))
    check_every_form(s, queries, table, mid, f"{name}, identity", small=True)
    check_every_form(s, queries, table, mid, f"{name}, identity", ks=(0, 2, 9), skip_shared=True)
    check_every_form(s, queries, table, INF, f"{name}, identity", ks=(1, 8, 64))
    want = XR.from_merged_table(table, queries, 64, mid)
    walked = int(CR.walked(queries, mid).sum())
    for k, counts, any_only, skip_shared in ((8, True, False, False), (0, True, False, True), (64, False, False, False), (0, True, True, False),
                                             (0, True, True, True)):
        plain = sc.triangle_distances(queries, mid, max_pairs=k, counts=counts, counters=True, any_only=any_only, skip_shared=skip_shared)[-1]
        got = s.triangle_distances(queries, mid, max_pairs=k, counts=counts, counters=True, any_only=any_only, skip_shared=skip_shared)
        if not any_only and not skip_shared:
            assert_answer(got[:3], want, k, counts, f"{name}, counting form, K = {k}")
        tally = got[3]
        for c in ("node_visits", "leaf_visits", "triangle_tests", "samples"):
            assert tally[c] == plain[c], (name, k, any_only, c, tally, plain)
        assert tally["traversals"] == walked and tally["shaded_hits"] == tally["env_lookups"] == tally["bad_hits"] == 0
    # the instance form against the self form
    triangles = len(positions) // 9
    assert s.triangle_count(0) == triangles == sc.triangle_count()
    for skip_shared in (False, True):
        for k, counts, md in ((8, True, mid), (64, False, INF), (0, True, mid), (9, True, mid)):
            self_rec, self_cnt = sc.self_clearance(md, max_pairs=k, counts=counts, skip_shared=skip_shared)
            w_inst = None if self_rec is None else np.where(self_rec["triangle"] >= 0, 0, -1).astype(np.int32)
            for path in PATHS:
                got = own_query(s, 0, k, counts, path, md, skip_shared=skip_shared, skip_own=False)
                assert_answer(got, (self_rec, w_inst, self_cnt), k, counts, f"{name}, instance form against self form, K = {k}, {path}")
        met = sc.self_clearance(mid, max_pairs=0, any_only=True, skip_shared=skip_shared)[1]
        assert np.array_equal(own_query(s, 0, 0, True, "host", mid, any_only=True, skip_shared=skip_shared, skip_own=False)[2], met)
    with_flag = s.instance_clearance(0, max_pairs=8)
    assert (with_flag[0]["triangle"] == -1).all() and (with_flag[1] == -1).all() and (with_flag[2] == 0).all(), "one instance: nothing but its own"
    assert not s.instances_within(INF).any()
    if triangles > 3:
        lo, n = triangles - 3, 3
        sub = sc.self_clearance(mid, max_pairs=8, skip_shared=False, first=lo, count=n)
        got = s.instance_clearance(0, mid, max_pairs=8, skip_own=False, first=lo, count=n)
        assert np.array_equal(bits(got[0]), bits(sub[0])) and np.array_equal(got[2], sub[1]), "a sub-range with the last triangle"
    torch.cuda.synchronize()


# 2 ---------------------------------------------------------------------------------------------------------------------------
def nine(pkg):
    """(names, distinct positions, scene of every instance, maps, the set, queries, max_dist2, the pair table)"""
    if "nine" not in _answers:
        positions, of, maps, kinds, names = XC.nine_instances(lambda name: member(pkg, name)[0])
        assert kinds[4] == "duplicate of 1" and names[4] == names[1] and np.array_equal(maps[4].view(np.uint32), maps[1].view(np.uint32))
        s = build(pkg, names, maps, "nine instances")
        queries = XC.world_queries(positions, of, maps)
        _answers["nine"] = (names, positions, of, maps, s, queries, XC.mid_value(positions, of, maps), table_of(positions, of, maps, queries))
    return _answers["nine"]


def test_the_nine_instance_set(pkg, gpu):
    names, positions, of, maps, s, queries, mid, table = nine(pkg)
    want = check_every_form(s, queries, table, mid, "nine instances", small=True)
    print(XC.assert_mixed(queries, mid, *want, "nine instances"))
    inst = want[1]
    assert ((inst == 1).sum(1) >= (inst == 4).sum(1)).all() and (inst == 4).sum() > 100, "the duplicate sorts behind its original"
    shared = check_every_form(s, queries, table, mid, "nine instances", ks=(0, 2, 8, 64), skip_shared=True)
    assert 0 < shared[2].sum() < want[2].sum(), "SKIP_SHARED removes members"
    assert np.array_equal(s.clearance_counts(queries, mid), want[2])
    assert np.array_equal(s.within_tolerance(queries, mid, skip_shared=True), shared[2] > 0)
    on_device = s.within_tolerance(dev_triangles(queries), mid)
    assert np.array_equal(on_device.cpu().numpy(), want[2] > 0)


@pytest.mark.parametrize("md", ["0", "+inf", "-1", "NaN"])
def test_the_other_tolerances_on_the_nine_instance_set(pkg, gpu, md):
    names, positions, of, maps, s, queries, mid, table = nine(pkg)
    value = {"0": F(0), "+inf": INF, "-1": F(-1), "NaN": F(np.nan)}[md]
    want = check_every_form(s, queries, table, value, "nine instances", ks=(0, 1, 8, 9, 64) if md in ("0", "+inf") else (0, 1, 9))
    total = sum(len(positions[k]) // 9 for k in of)
    if md == "+inf":
        assert set(np.unique(want[2]).tolist()) == {0, total}
    elif md == "0":
        assert 0.1 < (want[2] > 0).mean() < 0.7
        assert (want[0]["dist2"][want[1] >= 0] == 0).all()
    else:
        assert not want[2].any() and (want[1] == -1).all()
        assert np.array_equal(want[0]["dist2"].view(np.uint32), np.full((len(queries), 64), value, F).view(np.uint32))


@pytest.mark.parametrize("q", range(9))
def test_the_instance_form_on_the_nine_instance_set(pkg, gpu, q):
    """Consequence 6 for every instance: the instance form equals the item form fed with instance q's rows of the merged scene;
    with SKIP_OWN_INSTANCE the pairs of instance q are gone and n is less by their number.  Sub-ranges, the last triangle
    among them."""
    names, positions, of, maps, s, _, mid, _ = nine(pkg)
    triangles = s.triangle_count(q)
    assert triangles == len(positions[of[q]]) // 9
    rows = XR.own_queries(positions, of, maps, q)
    table = table_of(positions, of, maps, rows)
    item = query(s, rows, 64, True, "host", mid)
    for skip_own in (False, True):
        want = XR.from_merged_table(table, rows, 64, mid, without=q if skip_own else None)
        if not skip_own:
            assert_answer(item, want, 64, True, f"instance {q}: the item form on its own rows")
            assert (want[2] >= 1).all()
            plain = want
        else:
            assert not (want[1] == q).any()
            own_pairs = (table[2][:, table[1][q]:table[1][q + 1]] <= mid).sum(1)
            assert np.array_equal(want[2], plain[2] - own_pairs)
        for path in PATHS:
            for k, counts in ((64, True), (8, False), (9, False), (0, True), (4, True), (1, False)):
                assert_answer(own_query(s, q, k, counts, path, mid, skip_own=skip_own), want, k, counts,
                              f"instance {q}, SKIP_OWN_INSTANCE = {skip_own}, K = {k}, counts = {counts}, {path}")
            got = own_query(s, q, 0, True, path, mid, any_only=True, skip_own=skip_own)
            assert np.array_equal(got[2], (want[2] > 0).astype(np.int32)), f"instance {q}, ANY, {path}"
    shared = XR.from_merged_table(table, rows, 64, mid, True, q)
    assert_answer(own_query(s, q, 64, True, "device", mid, skip_shared=True), shared, 64, True, f"instance {q}, SKIP_SHARED on world corners")
    nearest = XR.from_merged_table(table, rows, 2, INF, without=q)
    for path in PATHS:
        assert_answer(own_query(s, q, 2, False, path), nearest, 2, False, f"instance {q}, the nearest other instance, {path}")
    want = XR.from_merged_table(table, rows, 64, mid, without=q)
    for first, count in ((triangles - 1, 1), (triangles // 3, min(70, triangles - triangles // 3)), (0, 0), (triangles, 0)):
        part = tuple(w[first:first + count] for w in want)
        for path in PATHS:
            assert_answer(own_query(s, q, 8, True, path, mid, first=first, count=count), part, 8, True, f"instance {q}, [{first}, +{count}), {path}")
    records, inst, n, least = s.instance_distance(q)
    assert_answer((records, inst, n), XR.from_merged_table(table, rows, 1, INF, without=q), 1, True, f"instance_distance({q})")
    others = np.delete(table[2], np.s_[table[1][q]:table[1][q + 1]], axis=1)
    assert least == float(others.min())


def test_instances_within(pkg, gpu):
    names, positions, of, maps, s, _, mid, _ = nine(pkg)
    tables = [table_of(positions, of, maps, XR.own_queries(positions, of, maps, q)) for q in range(9)]
    for md in (F(0), mid, mid * F(100), INF):
        got = s.instances_within(md)
        want = XR.within(positions, of, maps, md, tables=tables)
        assert got.dtype == np.bool_ and got.tolist() == want.tolist(), (md, got, want)
    assert s.instances_within(F(0))[1] and s.instances_within(F(0))[4], "the duplicates touch each other"
    assert s.instances_within(INF).all()


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["two scenes of different heights", "301 tiny instances"])
def test_sets_equal_the_restatement(pkg, gpu, which):
    names, maps, kinds = G.the_set(pkg, which)
    s = build(pkg, names, maps, which)
    distinct = sorted(set(names))
    positions, of = [member(pkg, d)[0] for d in distinct], [distinct.index(x) for x in names]
    queries = XC.world_queries(positions, of, maps, 384, seed=len(names) + 7)
    mid = XC.mid_value(positions, of, maps)
    table = table_of(positions, of, maps, queries)
    want = check_every_form(s, queries, table, mid, which, ks=(0, 1, 8, 9, 64))
    cnt, inst = want[2], want[1]
    print(which, np.bincount(np.minimum(cnt, 65)))
    assert (cnt == 0).mean() > 0.05 and (cnt > 0).mean() > 0.2, (which, np.bincount(np.minimum(cnt, 65)))
    check_every_form(s, queries, table, INF, which, ks=(1, 9))
    nearest = XR.from_merged_table(table, queries, 64, INF)[1]
    assert len(set(nearest[nearest >= 0].tolist())) >= min(len(names), 12), "the held pairs come from many instances"
    for q in (0, len(names) - 1, len(names) // 2):
        rows = XR.own_queries(positions, of, maps, q)
        own_table = table_of(positions, of, maps, rows)
        want = XR.from_merged_table(own_table, rows, 64, mid, without=q)
        for path in PATHS:
            assert_answer(own_query(s, q, 64, True, path, mid), want, 64, True, f"{which}, instance {q}, {path}")
            assert_answer(own_query(s, q, 8, False, path, mid), want, 8, False, f"{which}, instance {q}, pruned, {path}")


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_the_counters_of_the_nine_instance_set(pkg, gpu):
    """node_visits, leaf_visits, triangle_tests and traversals of the counting form, equal to the sum over the instances of
    instance_clearance_ref.walk_counters on the member's own tree, with the box the set's top level stores for the instance: a
    lane walks an instance exactly when the bound of that box is not above max_dist2 (the boxes above it hold it, so their
    bounds are no larger).  On the same boxes, the bound is never above any pair's restated dist2."""
    names, positions, of, maps, s, queries, mid, table = nine(pkg)
    queries = queries[:384]
    table = (table[0], table[1], table[2][:384], table[3][:384])
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
    for md, skip_shared in ((mid, False), (mid, True), (INF, False)):
        want = XR.from_merged_table(table, queries, 64, md, skip_shared)
        walked = CR.walked(queries, md)
        total = dict.fromkeys(COUNTERS, 0)
        members = np.zeros(len(queries), np.int64)
        for i, name in enumerate(names):
            tree, node_boxes, corners = trees[name]
            d2s = table[2][:, table[1][i]:table[1][i + 1]]
            w = XR.walk_counters(tree, node_boxes, corners, maps[i], queries, md, top_box=stored[i], skip_shared=skip_shared, d2s=d2s)
            assert (w["members"][w["traversals"] == 0] == 0).all(), "no pair is behind a culled instance"
            with np.errstate(invalid="ignore"):
                assert (w["top_bound"][walked] <= w["least"][walked]).all(), "the stored box's bound is under every pair's dist2"
            for c in COUNTERS:
                total[c] += int(w[c].sum())
            members += w["members"]
        assert np.array_equal(members, want[2]), "the counting walk finds every member"
        if md == mid:
            assert int(walked.sum()) < total["traversals"] < 9 * int(walked.sum()), "the top level culls some instances and not all"
        for k, counts in ((8, True), (64, False), (0, True)):
            got = s.triangle_distances(queries, md, max_pairs=k, counts=counts, counters=True, skip_shared=skip_shared)
            assert_answer(got[:3], want, k, counts, f"nine instances, counting form, K = {k}")
            for c in COUNTERS:
                assert got[3][c] == total[c], (md, skip_shared, k, c, got[3], total)
            assert got[3]["samples"] == len(queries)


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_refit_update_and_query_on_one_stream_and_after_a_host_update(pkg, gpu):
    """A device refit of a member, a device update with moved maps and both device forms, enqueued on one side stream with
    nothing between them; then a host update with other maps followed by the queries on all paths.  Each against the
    restatement of the state the query must see: the instance form's queries are the moved mesh under the new map."""
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
    K, Q = 8, 0
    try:
        moved = (before.reshape(-1, 3) * F(1.3) + F(0.2)).astype(F)
        now = [moved.reshape(-1), small_positions]
        queries = XC.world_queries(now, of, maps[1], 384, seed=71)
        mid = XC.mid_value(now, of, maps[1])
        first = query(s, queries, K, True, "host", mid)
        first_own = own_query(s, Q, K, True, "host", mid)
        triangles = s.triangle_count(Q)
        d_moved, d_maps, d_q = torch.from_numpy(moved).cuda(), torch.from_numpy(maps[1]).cuda(), dev_triangles(queries)
        new = lambda n, *shape: torch.full((n, *shape), -7, dtype=torch.int32, device="cuda")
        d_out, d_inst, d_cnt = new(len(queries), K, 12), new(len(queries), K), new(len(queries))
        o_out, o_inst, o_cnt = new(triangles, K, 12), new(triangles, K), new(triangles)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            own.refit(d_moved, stream_ptr=side.cuda_stream)
            s.update_into(d_maps.data_ptr(), side.cuda_stream)
            s.triangle_distances_into(d_q.data_ptr(), len(queries), d_out.data_ptr(), d_inst.data_ptr(), d_cnt.data_ptr(), mid, K,
                                      stream_ptr=side.cuda_stream)
            s.instance_clearance_into(Q, 0, triangles, o_out.data_ptr(), o_inst.data_ptr(), o_cnt.data_ptr(), mid, K,
                                      stream_ptr=side.cuda_stream)
        side.synchronize()
        assert s.update_status() == -1
        want = XR.from_merged_table(table_of(now, of, maps[1], queries), queries, 64, mid)
        assert (bits(first[0]) != bits(want[0][:, :K])).any(1).sum() > 100, "the refit and the update moved something"
        assert_answer((d_out.cpu().numpy(), d_inst.cpu().numpy(), d_cnt.cpu().numpy()), want, K, True, "one stream")
        rows = XR.own_queries(now, of, maps[1], Q)
        want_own = XR.from_merged_table(table_of(now, of, maps[1], rows), rows, 64, mid, without=Q)
        assert (first_own[2] != want_own[2]).sum() > 50 and (want_own[2] > 0).sum() > 20, "the instance form sees the moved mesh"
        assert_answer((o_out.cpu().numpy(), o_inst.cpu().numpy(), o_cnt.cpu().numpy()), want_own, K, True, "one stream, the instance form")
        # a host update: the device copy of the maps is behind it until the next query stages them on its stream
        s.update(maps[2])
        want2 = XR.from_merged_table(table_of(now, of, maps[2], queries), queries, 64, mid)
        assert (bits(want2[0]) != bits(want[0])).any(1).sum() > 100, "the host update moved something"
        rows2 = XR.own_queries(now, of, maps[2], Q)
        want2_own = XR.from_merged_table(table_of(now, of, maps[2], rows2), rows2, 64, mid, without=Q)
        for path in PATHS:
            assert_answer(query(s, queries, K, True, path, mid), want2, K, True, f"after a host update, {path}")
            assert_answer(query(s, queries, 9, False, path, mid), want2, 9, False, f"after a host update, K = 9, {path}")
            assert_answer(own_query(s, Q, K, True, path, mid), want2_own, K, True, f"after a host update, the instance form, {path}")
            assert_answer(own_query(s, Q, 9, False, path, mid), want2_own, 9, False, f"after a host update, the instance form, K = 9, {path}")
    finally:
        s.close()
        own.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_a_count_split_over_two_launches(pkg, gpu):
    """2^24 + 3000 queries (one launch holds 2^24), counts only, on the one-triangle scene placed twice: a tile of 4,096
    distinct queries repeated on the device (2^24 is a whole number of tiles, so the second launch starts on a tile's first
    query), the counts compared there with the restatement's tile.  The launch split, not a workload."""
    import torch
    positions, _ = member(pkg, "one triangle")
    names = ["one triangle", "one triangle"]
    _, maps, _ = IC.make_set([positions], [0, 0], seed=5, spread=0.3, kinds=["rotation_nonuniform", "mirror"])
    s = build(pkg, names, maps, "one triangle, twice")
    n, TILE = (1 << 24) + 3000, 4096
    tile = XC.world_queries([positions], [0, 0], maps, TILE, seed=33)
    mid = XC.mid_value([positions], [0, 0], maps) * F(25)
    want = XR.from_merged_table(table_of([positions], [0, 0], maps, tile), tile, 0, mid)[2]
    assert (want == 2).sum() > 100 and (want == 1).sum() > 100 and (want == 0).sum() > 100, np.bincount(want)
    repeats = (n + TILE - 1) // TILE
    d = dev_triangles(tile).repeat(repeats, 1)[:n].contiguous()
    d_cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    s.triangle_distances_into(d.data_ptr(), n, 0, 0, d_cnt.data_ptr(), mid, 0, stream_ptr=torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    del d
    w = torch.from_numpy(want).cuda()
    whole = (n // TILE) * TILE
    assert bool((d_cnt[:whole].reshape(n // TILE, TILE) == w[None]).all()), "every whole tile"
    assert torch.equal(d_cnt[whole:], w[:n - whole]), "the last launch's tail"


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops(pkg, gpu):
    import torch
    s = build(pkg, ["lobed_528", "one triangle"], np.stack([EYE, EYE]), "refusals")
    rec, inst, cnt = s.triangle_distances(np.zeros((0, 9), F))
    assert rec.shape == (0, 1) and rec.dtype == CR.PAIR_DISTANCE_DTYPE and inst.shape == (0, 1) and len(cnt) == 0
    assert len(s.clearance_counts(np.zeros((0, 12), F), 1.0)) == 0
    with pytest.raises(ValueError):
        s.triangle_distances(torch.zeros((4, 5), device="cuda"))
    with pytest.raises(ValueError):
        s.triangle_distances(torch.zeros((4, 9), device="cuda"), counters=True)
    with pytest.raises(ValueError):
        s.triangle_distances(np.zeros((4, 9), F), max_pairs=0, counts=False)
    with pytest.raises(ValueError):
        s.instance_clearance(0, max_pairs=0, counts=False)
    with pytest.raises(ValueError):
        s.instance_distance(0, max_pairs=0)
    for k in (-1, 65):
        with pytest.raises(pkg._native.ShrayError) as err:
            s.triangle_distances(np.zeros((4, 9), F), max_pairs=k)
        assert err.value.code == -1
    with pytest.raises(pkg._native.ShrayError):
        s.triangle_distances(np.zeros((4, 9), F), max_pairs=8, any_only=True)
    # the instance form's own refusals: an instance outside the set, then a range beyond its scene's triangles
    error = lambda: pkg._native.load_hip().shray_last_error().decode()
    for instance in (-1, 2):
        with pytest.raises(pkg._native.ShrayError) as err:
            s.instance_clearance(instance)
        assert err.value.code == -1 and "is not among the set's 2" in str(err.value)
    for first, count in ((0, 529), (528, 1), (529, 0), (100, 1 << 40)):
        for device in (False, True):
            with pytest.raises(pkg._native.ShrayError) as err:
                s.instance_clearance(0, first=first, count=count, device=device)
            assert err.value.code == -1 and "are not all among the 528" in str(err.value)
    with pytest.raises(pkg._native.ShrayError) as err:
        s.instance_clearance(1, first=1, count=1)
    assert "are not all among the 1 of instance 1" in str(err.value)
    with pytest.raises(pkg._native.ShrayError) as err:
        s.instance_clearance(0, first=-1, count=1)
    assert "negative first triangle" in str(err.value)
    assert len(s.instance_clearance(0, first=528, count=0)[2]) == 0, "an empty range at the end is a no-op"
    lib = pkg._native.load_instance_clearance()
    d = torch.zeros((64, 12), dtype=torch.int32, device="cuda")
    call, own, V = lib.shray_clearance_triangles_instances_device, lib.shray_clearance_instance_device, C.c_void_p
    op = pkg.tracer._set_clearance_params(1)
    base = d.data_ptr()
    assert call(s._handle, C.byref(op), V(base + 4), 1, V(base + 48), None, None, None) == -1
    assert call(s._handle, C.byref(op), V(base), 1, V(base + 52), None, None, None) == -1           # the records: 16 bytes
    assert call(s._handle, C.byref(op), V(base), 1, V(base + 48), V(base + 98), None, None) == -1
    assert call(s._handle, C.byref(op), V(base), 1, V(base + 48), None, V(base + 98), None) == -1
    assert call(s._handle, C.byref(op), V(base), 1, None, None, V(base + 100), None) == -1          # K = 1 without records
    assert call(s._handle, C.byref(op), V(base), 1, V(base + 48), V(base + 100), V(base + 104), None) == 0
    assert call(s._handle, C.byref(op), V(base), 0, V(base + 48), None, None, None) == 0
    # the order: the instance before the count, the alignment before the range
    assert own(s._handle, C.byref(op), 7, 0, -1, V(base), None, None, None) == -1 and "is not among the set's 2" in error()
    assert own(s._handle, C.byref(op), 0, 0, -1, V(base), None, None, None) == -1 and "negative triangle count" in error()
    assert own(s._handle, C.byref(op), 0, 0, 600, V(base + 4), None, None, None) == -1 and "aligned" in error()
    assert own(s._handle, C.byref(op), 0, 0, 600, V(base), None, None, None) == -1 and "are not all among" in error()
    assert own(s._handle, C.byref(op), 0, 520, 8, V(base), V(base + 1024), V(base + 2048), None) == 0
    flagged = pkg.tracer._set_clearance_params(1, skip_own=True)
    assert call(s._handle, C.byref(flagged), V(base), 1, V(base + 48), None, None, None) == -1 and "flags 0x4" in error()
    torch.cuda.synchronize()
