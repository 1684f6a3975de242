"""Triangle-intersection queries on the GPU (include/shader_ray_intersect.h) against the restatement (tests/intersect_ref.py):
every index and every count, for the mixed kinds of query of tests/intersect_cases.py, K in {0, 1, 2, 3, 4, 5, 8, 9, 64} with and
without counts, on the host and device (torch stream) paths; ANY and SKIP_SHARED alone and together; the tiny trees; a flat
integer lattice, the one scene whose pairs are exactly coplanar, also against the exact truth; degenerate scene triangles; the
self form over sub-ranges, against the item form and after a refit on the same stream that folds the mesh through itself;
one scene against a moved copy of itself; the counters; a count split over launches; and the refusals.  No case is skipped or
tolerated."""
import ctypes as C

import numpy as np
import pytest

import intersect_cases as IC
import intersect_ref as IR
from helpers import single_leaf_scene
from test_oracle_kat import chain_scene

pytestmark = pytest.mark.gpu

F = np.float32
BAD_TREE, INVALID = -6, -1
KS = (0, 1, 2, 3, 4, 5, 8, 9, 64)

_cache = {}


def loaded(pkg, name):
    """(vertex positions, resident host-built scene), once per scene file"""
    if name not in _cache:
        world = pkg.World(IC.scene_path(name))
        pos = np.asarray(world.arrays()["vertex_positions"], F).copy()
        _cache[name] = (world, pos, pkg.Scene(world.flatten()))
    return _cache[name][1], _cache[name][2]


def device_triangles(queries, padded=True):
    """a [n, 12] (the shray_triangle layout) or [n, 9] float32 tensor of query corners [n, 3, 3]"""
    import torch
    q = np.ascontiguousarray(queries, F).reshape(-1, 9)
    if padded:
        q = IR.make_triangles(q).view(F).reshape(-1, 12)
    return torch.from_numpy(q.copy()).cuda()


def assert_same(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} queries differ, first {bad[:5]}: got {got[bad[:3]]} want {want[bad[:3]]}"


def on_host(x):
    return x if x is None or isinstance(x, np.ndarray) else x.cpu().numpy()


def check_forms(run, member, what, ks=KS, paths=("host", "device")):
    """run(path, k, counts, any_only) -> (indices, counts) for every K with and without counts on the given paths, and the ANY
    form: all indices, all counts"""
    import torch
    want64, want_n = IR.from_set(member, 64)
    for k in ks:
        for counts in (True, False):
            if k == 0 and not counts:
                continue
            for path in paths:
                got, n = run(path, k, counts, False)
                torch.cuda.current_stream().synchronize()
                tag = f"{what}, K = {k}, counts = {counts}, {path} path"
                assert (got is None) == (k == 0) and (n is None) == (not counts), tag
                if path == "device":
                    assert all(x is None or (x.is_cuda and x.dtype == torch.int32) for x in (got, n)), tag
                if k:
                    assert_same(on_host(got), want64[:, :k], tag)   # (the restatement's indices for K are its first K of 64)
                if counts:
                    assert_same(on_host(n), want_n, tag)
    for path in paths:
        got, n = run(path, 0, True, True)
        torch.cuda.current_stream().synchronize()
        assert got is None
        assert_same(on_host(n), (want_n > 0).astype(np.int32), f"{what}, ANY, {path} path")


def item_run(scene, queries, skip_shared=False):
    d9, d12 = device_triangles(queries, False), device_triangles(queries, True)

    def run(path, k, counts, any_only):
        q = queries if path == "host" else d12 if k % 2 else d9
        return scene.intersecting_triangles(q, max_triangles=k, counts=counts, any_only=any_only, skip_shared=skip_shared)
    return run


def check_short_forms(scene, queries, member, skipped, what):
    import torch
    n, n_skip = member.sum(1).astype(np.int32), skipped.sum(1).astype(np.int32)
    assert_same(scene.intersection_counts(queries), n, what)
    assert_same(scene.intersection_counts(queries, skip_shared=True), n_skip, what)
    assert np.array_equal(scene.triangles_intersected(queries), n > 0), what
    assert np.array_equal(scene.triangles_intersected(IR.make_triangles(queries), skip_shared=True), n_skip > 0), what
    hit = scene.triangles_intersected(device_triangles(queries), skip_shared=True)
    assert hit.dtype == torch.bool and np.array_equal(hit.cpu().numpy(), n_skip > 0), what
    with pytest.raises(ValueError):
        scene.intersecting_triangles(queries, max_triangles=0, counts=False)


def codes(name, pos, n):
    """(queries, first_axis codes without and with SKIP_SHARED) of a file scene's query set, once"""
    key = ("codes", name, n)
    if key not in _cache:
        queries = IC.make_queries({"vertex_positions": pos}, n, seed=n + len(name))
        _cache[key] = (queries, IR.first_axis(queries, pos), IR.first_axis(queries, pos, True))
    return _cache[key]


SCENES = [("small_trisrc", 1200), ("lobed_528", 3000)]


@pytest.mark.parametrize("name, n", SCENES)
def test_small_scenes_exact(pkg, gpu, name, n):
    pos, scene = loaded(pkg, name)
    queries, code, code_skip = codes(name, pos, n)
    IC.assert_interesting(code, name)
    member, skipped = code == IR.INTERSECT, code_skip == IR.INTERSECT
    assert 0 < skipped.sum() < member.sum() - 1000 and (code_skip == IR.SHARED).sum() >= member.sum() - skipped.sum()
    check_forms(item_run(scene, queries), member, name)
    check_forms(item_run(scene, queries, True), skipped, name + ", SKIP_SHARED", ks=(0, 3, 8, 64))
    check_short_forms(scene, queries, member, skipped, name)


def flat_scene(pkg, tmp_path_factory):
    """the flat lattice written as an .obj, loaded and built like any scene: (positions in the tree's order, scene)"""
    if "flat" not in _cache:
        tris = IC.flat_lattice()
        path = str(tmp_path_factory.mktemp("intersect") / "flat_lattice.obj")
        pkg.scenes.write_obj(path, tris.reshape(-1, 3).astype(np.float64), np.arange(3 * len(tris)).reshape(-1, 3))
        world = pkg.World(path)
        pos = np.asarray(world.arrays()["vertex_positions"], F).copy()
        assert len(pos) == tris.size and (pos == np.round(pos)).all()
        assert sorted(map(tuple, pos.reshape(-1, 9).tolist())) == sorted(map(tuple, tris.reshape(-1, 9).tolist()))
        _cache["flat"] = (world, pos, pkg.Scene(world.flatten()))
    return _cache["flat"][1], _cache["flat"][2]


def flat_codes(pos):
    if "flat codes" not in _cache:
        queries = IC.flat_queries(3000, seed=41)
        _cache["flat codes"] = (queries, IR.first_axis(queries, pos), IR.first_axis(queries, pos, True))
    return _cache["flat codes"]


def test_flat_lattice_reaches_the_in_plane_axes(pkg, gpu, tmp_path_factory):
    """Exactly coplanar pairs: the integer grid in z = 0 and the sheet in x = 5 under integer queries, half of them in z = 0.
    Every operation is exact here, so the restatement is also held against the exact clip."""
    pos, scene = flat_scene(pkg, tmp_path_factory)
    queries, code, code_skip = flat_codes(pos)
    c = IC.coverage(code, "flat lattice")
    assert min(c["per_axis"][11:]) >= 1 and c["n == 0"] > 0.05 and c["n > 8"] > 0.20 and c["later"] > 0.10, c
    member, skipped = code == IR.INTERSECT, code_skip == IR.INTERSECT
    tris = pos.reshape(-1, 3, 3)
    rows = np.nonzero(IR.walked(queries))[0][:100]
    past0 = code[rows] > 2
    truth = np.array([[IC.exact_intersects(queries[r], tris[t]) if past0[i, t] or member[r, t] else False for t in range(len(tris))]
                      for i, r in enumerate(rows)])
    assert np.array_equal(truth, member[rows]) and truth.sum() > 300
    assert (code == IR.UNWALKED).all(1).sum() > 20
    check_forms(item_run(scene, queries), member, "flat lattice")
    check_forms(item_run(scene, queries, True), skipped, "flat lattice, SKIP_SHARED", ks=(0, 4, 9))
    # its own triangles: the grid's neighbours touch along edges and corners, the two sheets cross
    own, own_skip = IR.intersects(tris, pos), IR.intersects(tris, pos, True)
    assert own_skip.any() and own_skip.sum() < own.sum() / 4
    check_forms(self_run(scene, 0, len(tris), False), own, "flat lattice, self")
    check_forms(self_run(scene, 0, len(tris), True), own_skip, "flat lattice, self, SKIP_SHARED", ks=(0, 2, 8))
    assert scene.is_self_intersecting()


def test_every_axis_separates_first_somewhere(pkg, gpu, tmp_path_factory):
    """Over the suite's query sets, on the restatement alone: each of the 17 axes is the first to separate some pair (the
    general-position scenes never reach the last six: the flat lattice does)."""
    total = np.zeros(IR.AXES, np.int64)
    for name, n in SCENES:
        pos, _ = loaded(pkg, name)
        total += np.bincount(codes(name, pos, n)[1].ravel().astype(np.int64) + 1, minlength=IR.UNWALKED + 2)[IR.AXIS0 + 1:IR.UNWALKED + 1]
    general = total.copy()
    pos, _ = flat_scene(pkg, tmp_path_factory)
    total += np.bincount(flat_codes(pos)[1].ravel().astype(np.int64) + 1, minlength=IR.UNWALKED + 2)[IR.AXIS0 + 1:IR.UNWALKED + 1]
    print("first separating axis, general position:", dict(zip(IR.AXIS_NAMES, general.tolist())), "with the flat lattice:", total.tolist())
    assert (total >= 1).all(), total


def tiny_scenes():
    one = [[[0.25, 0.5, 1.0], [2.0, 0.75, 1.5], [1.0, 3.0, -0.5]]]
    eleven = [[[-5, -5, -float(k)], [5, -5, -float(k)], [0, 5, -float(k)]] for k in range(10)] + [[[-5, -5, 1.0], [5, -5, 1.0], [0, 5, 1.0]]]
    # a point and a segment among valid triangles: neither is ever a member, as a query neither is walked
    mixed = eleven[:3] + [[[0, 0, -1.5]] * 3] + eleven[3:6] + [[[-1, 0, -9.5], [1, 0, 1.5], [1, 0, 1.5]]] + eleven[6:]
    return {"one triangle": one, "11-triangle leaf": eleven, "a point and a segment in the leaf": mixed}


def leaf_tree(tris):
    """a single_leaf_scene as tree arrays for walk_counters, with the node box that scene stores"""
    import refit_ref
    i32 = lambda *x: np.array(x, np.int32)
    pts = tris.reshape(-1, 3)
    box = np.concatenate([pts.min(0) - 1e-5, pts.max(0) + 1e-5]).astype(F)[None]
    return refit_ref.TreeArrays(i32(-1), i32(-1), i32(-1), None, None, i32(0), i32(len(tris)), None), box


def check_counters(scene, tree, node_boxes, tris, queries, what):
    """the host path's three counters of the counting form (K = 0, K = 8), of ANY and of both with SKIP_SHARED against
    walk_counters: over all queries, and query by query over the first 24"""
    for skip in (False, True):
        member = IR.intersects(queries, tris.reshape(-1), skip)
        want = {any_only: IR.walk_counters(tree, node_boxes, tris, queries, skip, any_only, member) for any_only in (False, True)}
        for rows in [np.array([i]) for i in range(min(24, len(queries)))] + [np.arange(len(queries))]:
            for any_only, k in ((False, 0), (False, 8), (True, 0)):
                _, n, c = scene.intersecting_triangles(queries[rows], max_triangles=k, counters=True, any_only=any_only, skip_shared=skip)
                assert_same(n, np.minimum(member[rows].sum(1), 1 if any_only else 1 << 30).astype(np.int32), what)
                assert c["samples"] == len(rows)
                for key in IR.COUNTERS:
                    assert c[key] == int(want[any_only][key][rows].sum()), (what, skip, any_only, k, key, rows[:3], c)


def check_query_counts(pkg, desc, tris, name, tree=None, node_boxes=None):
    scene = pkg.Scene(desc)
    try:
        for count in (1, 63, 64, 65):
            queries = IC.make_queries({"vertex_positions": tris.reshape(-1)}, count, seed=count)
            queries[0] = tris[0]
            member = IR.intersects(queries, tris.reshape(-1))
            assert member.any()
            check_forms(item_run(scene, queries), member, f"{name}, {count} queries")
        own = IR.intersects(tris, tris.reshape(-1))
        check_forms(self_run(scene, 0, len(tris), False), own, f"{name}, self")
        if tree is not None:
            check_counters(scene, tree, node_boxes, tris, queries, name)
    finally:
        scene.close()


@pytest.mark.parametrize("name", list(tiny_scenes()))
def test_tiny_trees(pkg, gpu, name):
    """A root that is a leaf (height 0): one triangle, a leaf of 11, and that leaf with a point triangle and a segment triangle
    among the valid ones (never members, though the segment pierces the others); 1, 63, 64 and 65 queries, the self form, and
    the walk's counters."""
    tris = np.asarray(tiny_scenes()[name], F)
    if name.startswith("a point"):
        inside = IR.first_axis(tris, tris.reshape(-1))
        assert (inside[[3, 7]] == IR.UNWALKED).all() and not (inside[:, [3, 7]] == IR.INTERSECT).any()
        assert (inside[:, 7] == IR.DEGENERATE).sum() == 11   # the segment passes stage 0 with every valid triangle
    tree, box = leaf_tree(tris)
    check_query_counts(pkg, single_leaf_scene(tris).desc, tris, name, tree, box)


def test_two_leaves_under_one_branch(pkg, gpu):
    """Height 1, the smallest tree whose walk pushes: test_gpu_uniform_leaf's branch with a leaf of 3 and a leaf of 5 triangles
    whose boxes share a band about x = 0: queries there enter both leaves, others one, others none."""
    from test_gpu_uniform_leaf import two_leaf_scene
    from test_overlap_reference import two_leaf_tree
    hand = two_leaf_scene()
    tris = hand.keep["pos"][:24].reshape(-1, 3, 3).copy()
    tree, node_boxes, corners = two_leaf_tree()
    assert np.array_equal(corners, tris)
    q = np.asarray([[(0, -4.9, -1.9), (0.05, -4.9, 0.9), (-0.05, -4.8, 0.9)], [(-5, -4.5, -1.9), (-4.5, -4.5, 0.9), (-4.5, -4.4, 0.9)],
                    [(4, -4.5, -1.9), (4.5, -4.5, 0.9), (4.5, -4.4, 0.9)], [(7, 0, 0), (8, 0, 0), (7, 1, 0)]], F)
    member = IR.intersects(q, tris.reshape(-1))
    assert member.sum(1).tolist() == [8, 3, 5, 0]   # both leaves, the left one, the right one, neither
    scene = pkg.Scene(hand.desc)
    try:
        check_forms(item_run(scene, q), member, "two leaves, the band")
        _, _, c = scene.intersecting_triangles(q[:1], max_triangles=8, counters=True)
        assert c["node_visits"] == 3 and c["leaf_visits"] == 2 and c["triangle_tests"] == 8, c   # one was pushed
        queries = np.concatenate([q, IC.make_queries({"vertex_positions": tris.reshape(-1)}, 60, seed=2), tris])
        check_counters(scene, tree, node_boxes, tris, queries, "two leaves")
    finally:
        scene.close()
    check_query_counts(pkg, hand.desc, tris, "two leaves")


def self_run(scene, first, count, skip_shared):
    def run(path, k, counts, any_only):
        return scene.self_intersections(max_triangles=k, counts=counts, any_only=any_only, skip_shared=skip_shared, first=first,
                                        count=count, device=path == "device")
    return run


def folded(pos):
    """lobed_528's corners with every vertex right of the centre pushed 1.2 half-widths to the left: the right cap passes
    through the left side of the mesh"""
    p = pos.reshape(-1, 3).copy()
    centre, half = (p[:, 0].max() + p[:, 0].min()) / 2, (p[:, 0].max() - p[:, 0].min()) / 2
    p[p[:, 0] > centre, 0] -= F(1.2) * half
    return p


def test_self_intersections_over_sub_ranges_and_against_the_item_form(pkg, gpu):
    pos, scene = loaded(pkg, "lobed_528")
    tris = pos.reshape(-1, 3, 3)
    T = len(tris)
    assert scene.triangle_count() == T == 528
    own, own_skip = IR.intersects(tris, pos), IR.intersects(tris, pos, True)
    n = own.sum(1)
    assert own[np.arange(T), np.arange(T)].all() and 4 <= n.min() and 9 < n.max() < 64 and not own_skip.any()
    for first, count in ((0, T), (5, 64), (T - 3, 3), (130, 65)):
        rows = slice(first, first + count)
        check_forms(self_run(scene, first, count, False), own[rows], f"self [{first}, {first + count})", ks=KS if count == T else (0, 5, 9))
        check_forms(self_run(scene, first, count, True), own_skip[rows], f"self [{first}, {first + count}), SKIP_SHARED", ks=(0, 8))
    # the item form fed the same triangles answers the same
    for skip in (False, True):
        for k in (5, 64):
            a, an = scene.self_intersections(max_triangles=k, skip_shared=skip)
            b, bn = scene.intersecting_triangles(tris, max_triangles=k, skip_shared=skip)
            assert np.array_equal(a, b) and np.array_equal(an, bn)
    out, cnt = scene.self_intersections(first=7, count=0)
    assert out.shape == (0, 8) and cnt.shape == (0,)
    out, cnt = scene.self_intersections(first=T)            # the empty range at the end
    assert out.shape == (0, 8) and cnt.shape == (0,)
    assert scene.is_self_intersecting() is False
    lib = pkg._native.load_intersect()
    op = pkg.tracer.intersect_params(0)
    counts = np.zeros(T + 8, np.int32)
    for first, count in ((0, T + 1), (T, 1), (T + 1, 0), (1, T), (2 ** 40, 2 ** 40)):
        for device in (False, True):
            with pytest.raises(pkg._native.ShrayError) as err:
                scene.self_intersections(first=first, count=count, device=device)
            assert err.value.code == INVALID, (first, count)
    assert lib.shray_intersect_self(scene._handle, C.byref(op), T - 1, 1, None, counts.ctypes.data_as(C.c_void_p)) == 0 and counts[0] == n[T - 1]


def test_a_refit_on_the_same_stream_folds_the_mesh_through_itself(pkg, gpu):
    """A device refit and the self queries enqueued behind it on one side stream: they see the folded mesh (restated on the new
    corners), which does intersect itself; is_self_intersecting turns true."""
    import torch
    world = pkg.World(IC.scene_path("lobed_528"))
    scene = pkg.Scene(world.flatten())
    try:
        pos = np.asarray(world.arrays()["vertex_positions"], F)
        moved = folded(pos)
        T = len(moved) // 3
        tris = moved.reshape(-1, 3, 3)
        member, stale = IR.intersects(tris, moved.reshape(-1), True), IR.intersects(pos.reshape(-1, 3, 3), pos, True)
        n = member.sum(1)
        assert not stale.any() and (n > 0).mean() > 0.1 and n.max() > 8, ((n > 0).mean(), n.max())
        assert scene.is_self_intersecting() is False
        d_moved = torch.from_numpy(moved).cuda()
        forms = [(8, True, False), (3, False, False), (64, True, False), (0, True, False), (0, True, True)]
        first, count = 40, T - 100
        d_out = [torch.full((count, max(k, 1)), -7, dtype=torch.int32, device="cuda") for k, _, _ in forms]
        d_cnt = [torch.full((count,), -7, dtype=torch.int32, device="cuda") for _ in forms]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            scene.refit(d_moved, stream_ptr=side.cuda_stream)
            for (k, counts, any_only), out, cnt in zip(forms, d_out, d_cnt):
                scene.self_intersections_into(first, count, out.data_ptr() if k else 0, cnt.data_ptr() if counts else 0, max_triangles=k,
                                              any_only=any_only, stream_ptr=side.cuda_stream)
            whole = scene.self_intersections(max_triangles=9, device=True)   # (the current torch stream is the side stream)
        side.synchronize()
        assert np.array_equal(scene.geometry()["vertex_positions"].view(np.uint32), moved.reshape(-1).view(np.uint32))
        want64, want_n = IR.from_set(member, 64)
        rows = slice(first, first + count)
        for (k, counts, any_only), out, cnt in zip(forms, d_out, d_cnt):
            what = f"after the fold, K = {k}, counts = {counts}, any = {any_only}"
            if k:
                assert_same(out.cpu().numpy(), want64[rows, :k], what)
            else:
                assert bool((out == -7).all())   # not touched
            if counts:
                assert_same(cnt.cpu().numpy(), (want_n[rows] > 0).astype(np.int32) if any_only else want_n[rows], what)
            else:
                assert bool((cnt == -7).all())
        assert_same(whole[0].cpu().numpy(), want64[:, :9], "the whole folded mesh")
        assert_same(whole[1].cpu().numpy(), want_n, "the whole folded mesh")
        assert scene.is_self_intersecting() is True
        check_forms(self_run(scene, 0, T, True), member, "the folded mesh, self, SKIP_SHARED")
        check_forms(item_run(scene, tris, True), member, "the folded mesh, the item form", ks=(0, 8))
    finally:
        scene.close()
        world.close()


def test_intersections_with_a_moved_copy(pkg, gpu):
    """Mesh against mesh: a second resident scene of the same file, refit to a rotated and shifted copy, is the query set."""
    pos, scene = loaded(pkg, "lobed_528")
    world = pkg.World(IC.scene_path("lobed_528"))
    other = pkg.Scene(world.flatten())
    try:
        moved = IC.moved_copy(pos, seed=8).reshape(-1, 3)
        other.refit(moved)
        theirs = np.asarray(other.geometry()["vertex_positions"], F)
        assert np.array_equal(theirs.view(np.uint32), moved.reshape(-1).view(np.uint32))
        member = IR.intersects(moved.reshape(-1, 3, 3), pos)
        n = member.sum(1)
        assert 0.05 < (n > 0).mean() < 0.95, (n > 0).mean()
        for k in (0, 8, 64):
            got, cnt = scene.intersections_with(other, max_triangles=k)
            want, want_n = IR.from_set(member, k)
            assert (got is None) if k == 0 else np.array_equal(got, want)
            assert_same(cnt, want_n, f"intersections_with, K = {k}")
        assert np.array_equal(scene.intersections_with(other, max_triangles=0, any_only=True)[1], (n > 0).astype(np.int32))
        # the other way round is another query: the copy's tree, this scene's triangles
        back = IR.intersects(pos.reshape(-1, 3, 3), moved.reshape(-1))
        assert_same(other.intersections_with(scene, max_triangles=0)[1], back.sum(1).astype(np.int32), "the copy against the scene")
    finally:
        other.close()
        world.close()


def test_a_count_split_over_launches(pkg, gpu):
    """2^24 + 3000 queries (one launch holds 2^24) with K = 0 on the 11-triangle leaf: far queries have n = 0; the last launch's
    queries and real queries scattered over the first launch are restated."""
    import torch
    tris = np.asarray(tiny_scenes()["11-triangle leaf"], F)
    scene = pkg.Scene(single_leaf_scene(tris).desc)
    try:
        n = (1 << 24) + 3000
        real = IC.make_queries({"vertex_positions": tris.reshape(-1)}, 3000 + 4096, seed=33)
        tail, spread = real[:3000], real[3000:]
        far = np.asarray([[(1e6, -2e6, 3e6), (1.5e6, -2e6, 3e6), (1e6, -1e6, 4e6)]], F)
        assert IR.walked(far).all() and not IR.intersects(far, tris.reshape(-1)).any()
        d = device_triangles(far).repeat(n, 1)
        d[n - 3000:] = device_triangles(tail)
        sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, 4096, replace=False)).cuda()
        d[sample] = device_triangles(spread)
        d_cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        scene.intersecting_triangles_into(d.data_ptr(), n, 0, d_cnt.data_ptr(), max_triangles=0,
                                          stream_ptr=torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().synchronize()
        want_n = IR.intersect(tail, tris.reshape(-1), 0)[1]
        assert (want_n > 0).mean() > 0.3
        assert_same(d_cnt[n - 3000:].cpu().numpy(), want_n, "the last launch's counts")
        assert_same(d_cnt[sample].cpu().numpy(), IR.intersect(spread, tris.reshape(-1), 0)[1], "counts of the first launch")
        rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
        rest[sample] = False
        assert bool((d_cnt[: n - 3000][rest] == 0).all())
    finally:
        scene.close()


def test_refusals_and_no_ops(pkg, gpu):
    """A scene without a packed tree is refused with SHRAY_ERR_BAD_TREE (before anything is launched); count 0 is a no-op; a
    GPU tensor of the wrong shape and "nothing asked for" are refused by the binding; a misaligned device pointer by the
    library."""
    import torch
    hand = chain_scene(5)
    scene = pkg.Scene(hand.desc)
    try:
        for kwargs in ({}, {"max_triangles": 0}, {"counts": False}, {"counters": True}, {"max_triangles": 0, "any_only": True},
                       {"skip_shared": True}):
            with pytest.raises(pkg._native.ShrayError) as err:
                scene.intersecting_triangles(np.ones((4, 9), F).cumsum(1), **kwargs)
            assert err.value.code == BAD_TREE
        for device in (False, True):
            with pytest.raises(pkg._native.ShrayError) as err:
                scene.self_intersections(first=0, count=1, device=device)
            assert err.value.code == BAD_TREE
        with pytest.raises(pkg._native.ShrayError) as err:
            scene.is_self_intersecting()
        assert err.value.code == BAD_TREE
    finally:
        scene.close()
    pos, good = loaded(pkg, "lobed_528")
    out, n = good.intersecting_triangles(np.zeros((0, 9), F))
    assert out.shape == (0, 8) and out.dtype == np.int32 and n.shape == (0,)
    with pytest.raises(ValueError):
        good.intersecting_triangles(torch.zeros((4, 8), device="cuda"))
    with pytest.raises(ValueError):
        good.intersecting_triangles(torch.zeros((4, 9), device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        good.intersecting_triangles(np.zeros((4, 8), F))
    with pytest.raises(ValueError):
        good.intersecting_triangles(np.zeros((4, 9), F), max_triangles=0, counts=False)
    with pytest.raises(ValueError):
        good.self_intersections(max_triangles=0, counts=False)
    with pytest.raises(ValueError):
        good.intersecting_triangles(device_triangles(pos.reshape(-1, 9)[:4]), counters=True)
    with pytest.raises(pkg._native.ShrayError):
        good.intersecting_triangles(np.zeros((4, 9), F), max_triangles=65)
    with pytest.raises(pkg._native.ShrayError):
        good.intersecting_triangles(np.zeros((4, 9), F), max_triangles=8, any_only=True)
    with pytest.raises(pkg._native.ShrayError):
        good.self_intersections(max_triangles=8, any_only=True)
    lib = pkg._native.load_intersect()
    d = torch.zeros((4, 12), dtype=torch.int32, device="cuda")
    op = pkg.tracer.intersect_params(1)
    assert lib.shray_intersect_triangles_device(good._handle, C.byref(op), C.c_void_p(d.data_ptr() + 4), 1, C.c_void_p(d.data_ptr() + 96), None, None) == -1
    assert lib.shray_intersect_triangles_device(good._handle, C.byref(op), C.c_void_p(d.data_ptr()), 1, C.c_void_p(d.data_ptr() + 98), None, None) == -1
    assert lib.shray_intersect_self_device(good._handle, C.byref(op), 0, 1, C.c_void_p(d.data_ptr() + 98), None, None) == -1
