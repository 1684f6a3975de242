"""Triangle-distance queries on the GPU (include/shader_ray_clearance.h) against the restatement (tests/clearance_ref.py): all
48 bytes of every record and every count, for the mixed kinds of query of tests/clearance_cases.py (near, far, crossing, own
triangles, points, segments, NaN/inf), K in {0, 1, 2, 4, 8, 9, 64} (the boundary between register and memory slots, and
queries with more members than K), max_dist2 in {0, a mid value, +inf, -1, NaN}, with and without counts (the form that counts
every member and the form that prunes agree on the records), on the host, device (torch stream) and counters paths; ANY
against n > 0; 1, 63, 65 and 130 queries; the self form with and without SKIP_SHARED and with first > 0; a refit on the same
stream followed by both forms; a DeviceWorld; one case on the bunny-class scene; and the refusals that need a scene.

The restatement's pair table of a scene's query set is computed once, on the GPU through point_query_ref.TorchOps (each fp32
operation in float64, rounded: exact), and shared by every case of that scene; it is never written to.  No case is skipped
or tolerated."""
import ctypes as C

import numpy as np
import pytest

import clearance_cases as CC
import clearance_ref as CR
import intersect_cases as IC
import point_query_ref as PQ
from test_gpu_intersect import device_triangles, loaded, on_host
from test_oracle_kat import chain_scene

pytestmark = pytest.mark.gpu

F = np.float32
BAD_TREE, INVALID = -6, -1
KS = (0, 1, 2, 4, 8, 9, 64)
INF = F(np.inf)

_tables = {}


def table(key, queries, pos):
    """(queries, dist2 [n, T], shared [n, T]) of a query set over a scene's positions, once per key"""
    if key not in _tables:
        d2, _ = CR.pair_table(PQ.TorchOps("cuda"), queries, pos, pairs=1 << 22)
        d2.setflags(write=False)
        _tables[key] = (queries, d2, CR.shared_table(queries, pos))
    return _tables[key]


def scene_queries(name, pos, n):
    return table((name, n), CC.make_queries(pos, n, seed=n + len(name)), pos)


def mid_value(pos):
    """a max_dist2 that near queries reach with a handful of triangles and far ones with none: (4 % of the extent)^2"""
    return F((0.04 * IC.scene_extent(pos)) ** 2)


def bits(records):
    """a PAIR_DISTANCE_DTYPE array or an int32 [n, k, 12] tensor as uint32 [n, k * 12]"""
    r = on_host(records)
    return np.ascontiguousarray(r).view(np.uint32).reshape(len(r), -1)


def assert_records(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero((g != w).any(1))[0]
    if len(bad):
        r = on_host(got)
        r = r if r.dtype == CR.PAIR_DISTANCE_DTYPE else np.ascontiguousarray(r).view(CR.PAIR_DISTANCE_DTYPE).reshape(len(r), -1)
        raise AssertionError(f"{what}: {len(bad)} of {len(g)} queries differ, first {bad[:5]}: got {r[bad[0]][:3]} want {want[bad[0]][:3]}")


def assert_counts(got, want, what):
    got = on_host(got)
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} counts differ, first {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"


def check_forms(run, queries, pos, d2, shared, md, skip, what, ks=KS, paths=("host", "device")):
    """run(path, k, counts, any_only) -> (records, counts) for every K with and without counts on the given paths, and the ANY
    form: all 48 bytes of every record, every count"""
    import torch
    want64, want_n = CR.from_table(queries, pos, d2, shared, 64, md, skip)
    for k in ks:
        for counts in (True, False):
            if k == 0 and not counts:
                continue
            for path in paths:
                got, n = run(path, k, counts, False)
                torch.cuda.current_stream().synchronize()
                tag = f"{what}, max_dist2 = {md}, K = {k}, counts = {counts}, {path} path"
                assert (got is None) == (k == 0) and (n is None) == (not counts), tag
                if path == "device":
                    assert all(x is None or (x.is_cuda and x.dtype == torch.int32) for x in (got, n)), tag
                if k:
                    assert_records(got, want64[:, :k], tag)   # (the restatement's records for K are its first K of 64)
                if counts:
                    assert_counts(n, want_n, tag)
    for path in paths:
        got, n = run(path, 0, True, True)
        torch.cuda.current_stream().synchronize()
        assert got is None
        assert_counts(n, (want_n > 0).astype(np.int32), f"{what}, max_dist2 = {md}, ANY, {path} path")
    return want64, want_n


def item_run(scene, queries, md, skip=False):
    d9, d12 = device_triangles(queries, False), device_triangles(queries, True)

    def run(path, k, counts, any_only):
        q = queries if path == "host" else d12 if k % 2 else d9
        return scene.triangle_distances(q, md, max_pairs=k, counts=counts, any_only=any_only, skip_shared=skip)
    return run


def self_run(scene, first, count, md, skip):
    def run(path, k, counts, any_only):
        return scene.self_clearance(md, max_pairs=k, skip_shared=skip, first=first, count=count, counts=counts, any_only=any_only,
                                    device=path == "device")
    return run


@pytest.mark.parametrize("name", ["lobed_528", "small_trisrc"])
def test_small_scenes_exact(pkg, gpu, name):
    pos, scene = loaded(pkg, name)
    queries, d2, shared = scene_queries(name, pos, 600)
    kind = CC.kinds(600, 600 + len(name))
    assert all((kind == i).sum() >= 20 for i in range(len(CC.KINDS)))
    mid = mid_value(pos)
    want64, n = check_forms(item_run(scene, queries, mid), queries, pos, d2, shared, mid, False, name)
    assert (n == 0).mean() > 0.1 and (n > 8).mean() > 0.2 and (n > 64).mean() > 0.01, ((n == 0).mean(), (n > 8).mean(), (n > 64).mean())
    feature = want64["feature"][want64["triangle"] >= 0]
    assert (np.bincount(feature, minlength=16) > 0).all(), np.bincount(feature, minlength=16)   # every feature and the stage win somewhere
    _, n = check_forms(item_run(scene, queries, INF), queries, pos, d2, shared, INF, False, name)
    assert set(np.unique(n).tolist()) == {0, len(pos) // 9}
    _, n = check_forms(item_run(scene, queries, F(0)), queries, pos, d2, shared, F(0), False, name, ks=(0, 1, 8, 9))
    assert 0.1 < (n > 0).mean() < 0.6
    for bad in (F(-1), F(np.nan)):
        _, n = check_forms(item_run(scene, queries, bad), queries, pos, d2, shared, bad, False, name, ks=(0, 1, 9))
        assert not n.any()
    _, n_skip = check_forms(item_run(scene, queries, mid, True), queries, pos, d2, shared, mid, True, name + ", SKIP_SHARED", ks=(0, 2, 8, 64))
    assert 0 < n_skip.sum() < CR.from_table(queries, pos, d2, shared, 0, mid)[1].sum()


def test_counters_form_agrees_and_the_short_forms(pkg, gpu):
    import torch
    pos, scene = loaded(pkg, "lobed_528")
    queries, d2, shared = scene_queries("lobed_528", pos, 600)
    mid = mid_value(pos)
    want64, want_n = CR.from_table(queries, pos, d2, shared, 64, mid)
    for k in (0, 1, 8, 9):
        got, n, c = scene.triangle_distances(queries, mid, max_pairs=k, counters=True)
        if k:
            assert_records(got, want64[:, :k], f"counters form, K = {k}")
        assert_counts(n, want_n, f"counters form, K = {k}")
        walked = int(CR.walked(queries, mid).sum())
        assert c["samples"] == len(queries) and c["triangle_tests"] >= int(want_n.sum()) and c["node_visits"] >= walked, c
        assert c["triangle_tests"] < walked * len(pos) // 9 // 4, c   # the walk culls: far fewer pairs than brute force
    _, n, c = scene.triangle_distances(queries, mid, max_pairs=0, counters=True, any_only=True)
    assert_counts(n, (want_n > 0).astype(np.int32), "counters form, ANY")
    assert_counts(scene.clearance_counts(queries, mid), want_n, "clearance_counts")
    skipped = CR.from_table(queries, pos, d2, shared, 0, mid, True)[1]
    assert_counts(scene.clearance_counts(queries, mid, skip_shared=True), skipped, "clearance_counts, SKIP_SHARED")
    assert np.array_equal(scene.within_tolerance(queries, mid), want_n > 0)
    hit = scene.within_tolerance(device_triangles(queries), mid, skip_shared=True)
    assert hit.dtype == torch.bool and np.array_equal(hit.cpu().numpy(), skipped > 0)
    with pytest.raises(ValueError):
        scene.triangle_distances(queries, mid, max_pairs=0, counts=False)
    with pytest.raises(ValueError):
        scene.triangle_distances(device_triangles(queries), mid, counters=True)


@pytest.mark.parametrize("count", [1, 63, 65, 130])
def test_query_counts(pkg, gpu, count):
    pos, scene = loaded(pkg, "lobed_528")
    queries, d2, shared = scene_queries("lobed_528", pos, 600)
    rows = np.arange(count) + 7
    mid = mid_value(pos)
    assert CR.from_table(queries[rows], pos, d2[rows], shared[rows], 0, mid)[1].any() or count == 1
    check_forms(item_run(scene, queries[rows], mid), queries[rows], pos, d2[rows], shared[rows], mid, False, f"{count} queries", ks=(0, 1, 8, 9))


def test_the_self_form(pkg, gpu):
    pos, scene = loaded(pkg, "lobed_528")
    tris = pos.reshape(-1, 3, 3)
    T = len(tris)
    queries, d2, shared = table(("lobed_528", "own"), tris, pos)
    mid = mid_value(pos)
    for first, count, ks in ((0, T, KS), (5, 64, (0, 1, 9)), (T - 3, 3, (0, 2)), (130, 65, (0, 8))):
        rows = slice(first, first + count)
        for skip in (False, True):
            _, n = check_forms(self_run(scene, first, count, mid, skip), queries[rows], pos, d2[rows], shared[rows], mid, skip,
                               f"self [{first}, {first + count}), SKIP_SHARED {skip}", ks=ks)
            assert (n > 0).all() if not skip else n.sum() > 0
    want, want_n = CR.from_table(queries, pos, d2, shared, 1, INF, True)
    got, n = scene.self_clearance()   # max_dist2 = +inf, K = 1, SKIP_SHARED: the nearest triangle that is no neighbour
    assert_records(got, want, "self_clearance()")
    assert_counts(n, want_n, "self_clearance()")
    assert (got["dist2"] > 0).all() and (got["triangle"][:, 0] != np.arange(T)).all()
    # the item form fed the same triangles answers the same
    a, an = scene.self_clearance(mid, max_pairs=9, skip_shared=False)
    b, bn = scene.triangle_distances(tris, mid, max_pairs=9)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(an, bn)
    out, cnt = scene.self_clearance(first=7, count=0)
    assert out.shape == (0, 1) and cnt.shape == (0,)
    for first, count in ((0, T + 1), (T, 1), (T + 1, 0), (2 ** 40, 2 ** 40)):
        for device in (False, True):
            with pytest.raises(pkg._native.ShrayError) as err:
                scene.self_clearance(first=first, count=count, device=device)
            assert err.value.code == INVALID, (first, count)


def test_a_refit_on_the_same_stream_then_both_forms(pkg, gpu):
    """A device refit and the queries enqueued behind it on one side stream: the item form and the self form see the moved mesh
    (restated on the new corners)."""
    import torch
    world = pkg.World(IC.scene_path("lobed_528"))
    scene = pkg.Scene(world.flatten())
    try:
        pos = np.asarray(world.arrays()["vertex_positions"], F).reshape(-1, 3)
        rng = np.random.default_rng(4)
        moved = (pos * F(1.3) + rng.normal(size=pos.shape).astype(F) * F(0.01) + F(0.5)).astype(F)
        new_pos = moved.reshape(-1)
        T = len(new_pos) // 9
        queries, d2, shared = table(("moved", 300), CC.make_queries(new_pos, 300, seed=19), new_pos)
        own, own_d2, own_shared = table(("moved", "own"), new_pos.reshape(-1, 3, 3), new_pos)
        mid = mid_value(new_pos)
        stale = CR.from_table(queries, pos.reshape(-1), CR.pair_table(PQ.TorchOps("cuda"), queries, pos.reshape(-1), pairs=1 << 22)[0],
                              None, 1, mid)[0]
        d_moved, d_q = torch.from_numpy(moved).cuda(), device_triangles(queries)
        forms = [(8, True), (1, False), (64, True), (0, True)]
        first, count = 40, T - 100
        new = lambda rows, k: torch.full((rows, max(k, 1), 12), -7, dtype=torch.int32, device="cuda")
        item_out, self_out = [new(len(queries), k) for k, _ in forms], [new(count, k) for k, _ in forms]
        item_cnt = [torch.full((len(queries),), -7, dtype=torch.int32, device="cuda") for _ in forms]
        self_cnt = [torch.full((count,), -7, dtype=torch.int32, device="cuda") for _ in forms]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            scene.refit(d_moved, stream_ptr=side.cuda_stream)
            for i, (k, counts) in enumerate(forms):
                scene.triangle_distances_into(d_q.data_ptr(), len(queries), item_out[i].data_ptr() if k else 0,
                                              item_cnt[i].data_ptr() if counts else 0, mid, max_pairs=k, stream_ptr=side.cuda_stream)
                scene.self_clearance_into(first, count, self_out[i].data_ptr() if k else 0, self_cnt[i].data_ptr() if counts else 0, mid,
                                          max_pairs=k, skip_shared=True, stream_ptr=side.cuda_stream)
        side.synchronize()
        assert np.array_equal(scene.geometry()["vertex_positions"].view(np.uint32), new_pos.view(np.uint32))
        want64, want_n = CR.from_table(queries, new_pos, d2, shared, 64, mid)
        rows = slice(first, first + count)
        self64, self_n = CR.from_table(own[rows], new_pos, own_d2[rows], own_shared[rows], 64, mid, True)
        assert not np.array_equal(bits(want64[:, :1]), bits(stale))   # the moved mesh answers differently
        for i, (k, counts) in enumerate(forms):
            what = f"after the refit, K = {k}, counts = {counts}"
            for out, cnt, w64, wn in ((item_out[i], item_cnt[i], want64, want_n), (self_out[i], self_cnt[i], self64, self_n)):
                if k:
                    assert_records(out[:, :k], w64[:, :k], what)
                else:
                    assert bool((out == -7).all())   # not touched
                if counts:
                    assert_counts(cnt, wn, what)
                else:
                    assert bool((cnt == -7).all())
    finally:
        scene.close()
        world.close()


def test_device_world_and_distance_to(pkg, gpu):
    pos, scene = loaded(pkg, "lobed_528")
    queries, d2, shared = scene_queries("lobed_528", pos, 600)
    mid = mid_value(pos)
    dw = pkg.tracer.DeviceWorld(IC.scene_path("lobed_528"))
    try:
        flat = np.asarray(dw.flat_arrays()["vertex_positions"], F)
        assert np.array_equal(flat.view(np.uint32), pos.view(np.uint32))
        check_forms(item_run(dw.scene, queries, mid), queries, pos, d2, shared, mid, False, "DeviceWorld", ks=(0, 1, 8, 9, 64))
        # mesh against mesh: the device-built scene refit to a moved copy is the query set of the host-built one
        moved = IC.moved_copy(pos, seed=8, shift=0.2).reshape(-1, 3)
        dw.scene.refit(moved)
        theirs, t_d2, t_shared = table(("lobed_528", "moved copy"), moved.reshape(-1, 3, 3), pos)
        want, want_n = CR.from_table(theirs, pos, t_d2, t_shared, 2, INF)
        got, n, least = scene.distance_to(dw.scene, max_pairs=2)
        assert_records(got, want, "distance_to")
        assert_counts(n, want_n, "distance_to")
        assert least == float(t_d2.min())
        got, n, least = scene.distance_to(dw.scene, max_dist2=F(1e-12))
        assert least == (0.0 if (t_d2 == 0).any() else float("inf")) and int(n.sum()) == int((t_d2 <= F(1e-12)).sum())
        with pytest.raises(ValueError):
            scene.distance_to(dw.scene, max_pairs=0)
    finally:
        dw.close()


def test_the_bunny_class_scene(pkg, gpu):
    """256 queries on the benchmark-sized scene: the restatement's pair table through TorchOps on the GPU."""
    pos, scene = loaded(pkg, "bunny")
    queries, d2, shared = scene_queries("bunny", pos, 256)
    mid = mid_value(pos)
    _, n = check_forms(item_run(scene, queries, mid), queries, pos, d2, shared, mid, False, "bunny", ks=(0, 1, 8, 9), paths=("device",))
    assert (n > 64).any() and (n == 0).any()
    check_forms(item_run(scene, queries, INF), queries, pos, d2, shared, INF, False, "bunny", ks=(1, 9), paths=("device",))


def test_refusals_and_no_ops(pkg, gpu):
    """A scene without a packed tree is refused with SHRAY_ERR_BAD_TREE (before anything is launched); count 0 is a no-op; a
    GPU tensor of the wrong shape and "nothing asked for" are refused by the binding; a misaligned device pointer by the
    library."""
    import torch
    hand = chain_scene(5)
    scene = pkg.Scene(hand.desc)
    try:
        for kwargs in ({}, {"max_pairs": 0}, {"counts": False}, {"counters": True}, {"max_pairs": 0, "any_only": True}, {"skip_shared": True}):
            with pytest.raises(pkg._native.ShrayError) as err:
                scene.triangle_distances(np.ones((4, 9), F).cumsum(1), **kwargs)
            assert err.value.code == BAD_TREE
        for device in (False, True):
            with pytest.raises(pkg._native.ShrayError) as err:
                scene.self_clearance(first=0, count=1, device=device)
            assert err.value.code == BAD_TREE
    finally:
        scene.close()
    pos, good = loaded(pkg, "lobed_528")
    out, n = good.triangle_distances(np.zeros((0, 9), F))
    assert out.shape == (0, 1) and out.dtype == CR.PAIR_DISTANCE_DTYPE and n.shape == (0,)
    with pytest.raises(ValueError):
        good.triangle_distances(torch.zeros((4, 8), device="cuda"))
    with pytest.raises(ValueError):
        good.triangle_distances(np.zeros((4, 8), F))
    with pytest.raises(ValueError):
        good.self_clearance(max_pairs=0, counts=False)
    with pytest.raises(pkg._native.ShrayError):
        good.triangle_distances(np.zeros((4, 9), F), max_pairs=65)
    with pytest.raises(pkg._native.ShrayError):
        good.triangle_distances(np.zeros((4, 9), F), max_pairs=8, any_only=True)
    lib = pkg._native.load_clearance()
    d = torch.zeros((64, 12), dtype=torch.int32, device="cuda")
    op = pkg.tracer.clearance_params(1)
    assert lib.shray_clearance_triangles_device(good._handle, C.byref(op), C.c_void_p(d.data_ptr() + 4), 1, C.c_void_p(d.data_ptr() + 96), None, None) == -1
    assert lib.shray_clearance_triangles_device(good._handle, C.byref(op), C.c_void_p(d.data_ptr()), 1, C.c_void_p(d.data_ptr() + 104), None, None) == -1
    assert lib.shray_clearance_self_device(good._handle, C.byref(op), 0, 1, C.c_void_p(d.data_ptr() + 100), None, None) == -1
