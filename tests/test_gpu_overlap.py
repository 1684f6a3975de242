"""Box-overlap queries on the GPU (include/shader_ray_overlap.h) against the restatement (tests/overlap_ref.py): every index and
every count, for the mixed kinds of box of tests/overlap_cases.py, K in {0, 1, 2, 3, 4, 5, 8, 9, 64} with and without counts, on
the host and device (torch stream) paths; the tiny trees; the ANY form, box_counts and boxes_touched; surface_voxels; the
counters; DeviceWorld; after a device refit on the same stream; a count split over launches; and the refusals.  No case is
skipped or tolerated."""
import ctypes as C

import numpy as np
import pytest

import overlap_cases as OC
import overlap_ref as OR
from helpers import single_leaf_scene
from test_oracle_kat import chain_scene

pytestmark = pytest.mark.gpu

F = np.float32
BAD_TREE = -6
KS = (0, 1, 2, 3, 4, 5, 8, 9, 64)

_cache = {}


def loaded(pkg, name):
    """(flattened arrays, resident host-built scene), once per scene file"""
    if name not in _cache:
        world = pkg.World(OC.scene_path(name))
        arrays = world.arrays()
        _cache[name] = (world, arrays, pkg.Scene(world.flatten()))
    return _cache[name][1], _cache[name][2]


def device_boxes(boxes):
    import torch
    return torch.from_numpy(np.ascontiguousarray(boxes).view(F).reshape(-1, 8).copy()).cuda()


def device_query(scene, boxes, k, counts):
    """the device path on the current torch stream, from a [n, 8] float32 tensor"""
    import torch
    out, cnt = scene.triangles_in_boxes(device_boxes(boxes), max_triangles=k, counts=counts)
    torch.cuda.current_stream().synchronize()
    if k == 0:
        assert out is None
    else:
        assert out.dtype == torch.int32 and out.shape == (len(boxes), k) and out.is_cuda
    if counts:
        assert cnt.dtype == torch.int32 and cnt.shape == (len(boxes),) and cnt.is_cuda
    else:
        assert cnt is None
    return (out.cpu().numpy() if k else None), (cnt.cpu().numpy() if counts else None)


def assert_same(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} boxes differ, first {bad[:5]}: got {got[bad[:3]]} want {want[bad[:3]]}"


def check_every_k(scene, boxes, member, what, paths=("host", "device")):
    """every K, with and without counts, on the given paths: all indices, all counts; K = 0 without counts is refused by the
    binding"""
    want64, want_n = OR.from_set(member, 64)
    for k in KS:
        for counts in (True, False):
            if k == 0 and not counts:
                with pytest.raises(ValueError):
                    scene.triangles_in_boxes(boxes, max_triangles=0, counts=False)
                continue
            for path in paths:
                if path == "host":
                    got, n = scene.triangles_in_boxes(boxes, max_triangles=k, counts=counts)
                else:
                    got, n = device_query(scene, boxes, k, counts)
                tag = f"{what}, K = {k}, counts = {counts}, {path} path"
                if k:
                    assert_same(got, want64[:, :k], tag)   # (the restatement's indices for K are its first K of 64: test_overlap_reference)
                else:
                    assert got is None, tag
                if counts:
                    assert_same(n, want_n, tag)
                else:
                    assert n is None, tag
    # the ANY form, and the two short forms
    assert np.array_equal(scene.boxes_touched(boxes), want_n > 0), what
    assert_same(scene.box_counts(boxes), want_n, what)
    import torch
    touched = scene.boxes_touched(device_boxes(boxes))
    assert touched.dtype == torch.bool and np.array_equal(touched.cpu().numpy(), want_n > 0), what


@pytest.mark.parametrize("name, n", [("small_trisrc", 6000), ("lobed_528", 6000), ("quads_mixed", 2000), ("quads_nonormals", 4000)])
def test_small_scenes_exact(pkg, gpu, name, n):
    arrays, scene = loaded(pkg, name)
    boxes = OC.make_boxes(arrays, n, seed=n + len(name))
    code = OR.first_axis(arrays["vertex_positions"], boxes)
    OC.assert_interesting(code, name)
    check_every_k(scene, boxes, code == OR.OVERLAP, name)


def tiny_scenes():
    one = [[[0.25, 0.5, 1.0], [2.0, 0.75, 1.5], [1.0, 3.0, -0.5]]]
    eleven = [[[-5, -5, -float(k)], [5, -5, -float(k)], [0, 5, -float(k)]] for k in range(10)] + [[[-5, -5, 1.0], [5, -5, 1.0], [0, 5, 1.0]]]
    return {"one triangle": one, "11-triangle leaf": eleven}


def check_box_counts(pkg, desc, tris, name):
    scene = pkg.Scene(desc)
    try:
        arrays = {"vertex_positions": tris.reshape(-1)}
        for count in (1, 63, 64, 65):
            boxes = OC.make_boxes(arrays, count, seed=count)
            member = OR.overlaps(tris.reshape(-1), boxes)
            assert member.any()
            check_every_k(scene, boxes, member, f"{name}, {count} boxes")
    finally:
        scene.close()


@pytest.mark.parametrize("name", ["one triangle", "11-triangle leaf"])
def test_tiny_trees(pkg, gpu, name):
    """A root that is a leaf (height 0): one triangle, and a leaf of 11; 1, 63, 64 and 65 boxes.  test_oracle_kat.chain_scene
    itself cannot be queried: its links are a chain and not a canonical tree, so it has no packed tree and is the scene
    test_refusals_and_no_ops expects SHRAY_ERR_BAD_TREE from.  The 11 triangles (more than K = 8 and 9, fewer than 64) are
    therefore one leaf of helpers.single_leaf_scene, the builder chain_scene's leaves come from."""
    tris = np.asarray(tiny_scenes()[name], F)
    check_box_counts(pkg, single_leaf_scene(tris).desc, tris, name)


def test_two_leaves_under_one_branch(pkg, gpu):
    """Height 1, the smallest tree whose walk pushes: test_gpu_uniform_leaf's branch with a leaf of 3 and a leaf of 5 triangles
    whose boxes share a band about x = 0, so boxes there enter both leaves, others one, others none."""
    from test_gpu_uniform_leaf import two_leaf_scene
    hand = two_leaf_scene()
    tris = hand.keep["pos"][:24].reshape(-1, 3, 3).copy()
    arrays = {"vertex_positions": tris.reshape(-1)}
    band = OR.make_boxes([(-0.1, -5.0, -2.0), (-6.0, -4.0, -2.0), (0.5, -4.0, -2.0), (7.0, 0.0, 0.0)],
                         [(0.1, -4.75, 1.0), (-4.0, -3.0, 1.0), (4.0, -3.0, 1.0), (8.0, 1.0, 1.0)])
    n = OR.overlap(tris.reshape(-1), band, 8)[1]
    assert n.tolist() == [8, 3, 5, 0]   # both leaves, the left one, the right one, neither
    scene = pkg.Scene(hand.desc)
    try:
        check_every_k(scene, band, OR.overlaps(tris.reshape(-1), band), "two leaves, the band")
        _, _, c = scene.triangles_in_boxes(band[:1], max_triangles=8, counters=True)
        assert c["leaf_visits"] == 2 and c["triangle_tests"] == 8, c   # one box walked both leaves: one was pushed
    finally:
        scene.close()
    check_box_counts(pkg, hand.desc, tris, "two leaves")


def test_bunny_counters_and_any(pkg, gpu):
    """The bunny-class mesh, 4,096 boxes at K = 64 with counters: the walk tests far fewer triangles than the brute force."""
    arrays, scene = loaded(pkg, "bunny")
    pos = arrays["vertex_positions"]
    boxes = OC.make_boxes(arrays, 4096, seed=7)
    member = OR.overlaps(pos, boxes)
    want64, want_n = OR.from_set(member, 64)
    got, n, c = scene.triangles_in_boxes(boxes, max_triangles=64, counters=True)
    assert_same(got, want64, "bunny, K = 64")
    assert_same(n, want_n, "bunny, counts")
    print("bunny counters", c, "sum n", int(want_n.sum()))
    assert c["samples"] == len(boxes) and c["node_visits"] > 0 and c["leaf_visits"] > 0
    assert int(want_n.sum()) <= c["triangle_tests"] < len(boxes) * (len(pos) // 9)
    assert c["shaded_hits"] == c["env_lookups"] == c["traversals"] == c["bad_hits"] == 0
    _, any_n = scene.triangles_in_boxes(boxes, max_triangles=0, any_only=True)
    assert_same(any_n, (want_n > 0).astype(np.int32), "bunny, ANY")
    assert np.array_equal(scene.boxes_touched(boxes), want_n > 0)
    assert_same(scene.box_counts(boxes), want_n, "bunny, box_counts")
    got8, n8 = device_query(scene, boxes, 8, True)
    assert_same(got8, want64[:, :8], "bunny, K = 8, device path")
    assert_same(n8, want_n, "bunny, counts, device path")
    with pytest.raises(ValueError):
        scene.triangles_in_boxes(device_boxes(boxes[:4]), counters=True)


def test_surface_voxels(pkg, gpu):
    """lobed_528 at 16 x 16 x 16, numpy and torch: the restatement over the same boxes, whose bounds are compared as bits"""
    import torch
    arrays, scene = loaded(pkg, "lobed_528")
    verts = np.asarray(arrays["vertex_positions"], F).reshape(-1, 3)
    lo, hi = verts.min(0), verts.max(0)
    dims = (16, 16, 16)
    origin = (lo - F(0.01)).astype(F)
    cell = ((hi - lo + F(0.02)) / F(16)).astype(F)
    planes = [origin[a] + np.arange(17, dtype=F) * cell[a] for a in range(3)]
    i, j, k = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    want = OR.make_boxes(np.stack([planes[0][i], planes[1][j], planes[2][k]], -1).reshape(-1, 3),
                         np.stack([planes[0][i + 1], planes[1][j + 1], planes[2][k + 1]], -1).reshape(-1, 3))
    host = pkg.tracer.voxel_boxes(origin, cell, dims)
    dev = pkg.tracer.voxel_boxes(origin, cell, dims, device="cuda")
    for got in (host.view(F).reshape(-1, 8), dev.cpu().numpy()):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32).reshape(-1, 8))
    occupied = OR.overlaps(arrays["vertex_positions"], want).any(1).reshape(dims)
    assert 0.05 < occupied.mean() < 0.95, occupied.mean()
    grid = scene.surface_voxels(origin, cell, dims)
    assert grid.dtype == np.bool_ and grid.shape == dims and np.array_equal(grid, occupied)
    grid = scene.surface_voxels(origin, cell, dims, device="cuda")
    assert grid.dtype == torch.bool and grid.is_cuda and tuple(grid.shape) == dims and np.array_equal(grid.cpu().numpy(), occupied)


def test_device_world_matches_host_scene(pkg, gpu):
    arrays, scene = loaded(pkg, "lobed_528")
    dw = pkg.tracer.DeviceWorld(OC.scene_path("lobed_528"))
    try:
        flat = dw.flat_arrays()
        assert np.array_equal(np.asarray(flat["vertex_positions"], F).view(np.uint32),
                              np.asarray(arrays["vertex_positions"], F).view(np.uint32))
        boxes = OC.make_boxes(arrays, 3000, seed=21)
        member = OR.overlaps(flat["vertex_positions"], boxes)
        check_every_k(dw, boxes, member, "DeviceWorld")
        got, n = scene.triangles_in_boxes(boxes, max_triangles=9)
        want, want_n = OR.from_set(member, 9)
        assert_same(got, want, "host Scene")
        assert_same(n, want_n, "host Scene")
    finally:
        dw.close()


def test_triangles_in_boxes_into_on_a_stream_after_a_device_refit(pkg, gpu):
    """A refit and the queries enqueued on one side stream: they see the refit geometry (restated on the new corners)."""
    import torch
    world = pkg.World(OC.scene_path("lobed_528"))
    scene = pkg.Scene(world.flatten())
    try:
        pos = np.asarray(world.arrays()["vertex_positions"], F).reshape(-1, 3)
        rng = np.random.default_rng(4)
        moved = (pos * F(1.3) + rng.normal(size=pos.shape).astype(F) * F(0.01) + F(0.5)).astype(F)
        boxes = OC.make_boxes({"vertex_positions": moved.reshape(-1)}, 4000, seed=9)
        d_moved = torch.from_numpy(moved).cuda()
        d_boxes = device_boxes(boxes)
        forms = [(8, True, False), (8, False, False), (64, False, False), (0, True, False), (0, True, True)]
        d_out = [torch.full((len(boxes), max(k, 1)), -7, dtype=torch.int32, device="cuda") for k, _, _ in forms]
        d_cnt = [torch.full((len(boxes),), -7, dtype=torch.int32, device="cuda") for _ in forms]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            scene.refit(d_moved, stream_ptr=side.cuda_stream)
            for (k, counts, any_only), out, cnt in zip(forms, d_out, d_cnt):
                scene.triangles_in_boxes_into(d_boxes.data_ptr(), len(boxes), out.data_ptr() if k else 0, cnt.data_ptr() if counts else 0,
                                              max_triangles=k, any_only=any_only, stream_ptr=side.cuda_stream)
        side.synchronize()
        now = scene.geometry()["vertex_positions"]
        assert np.array_equal(now.view(np.uint32), moved.reshape(-1).view(np.uint32))
        member = OR.overlaps(moved.reshape(-1), boxes)
        stale = OR.overlaps(pos.reshape(-1), boxes)
        assert (member != stale).any(1).mean() > 0.3   # the old geometry would answer otherwise
        want64, want_n = OR.from_set(member, 64)
        for (k, counts, any_only), out, cnt in zip(forms, d_out, d_cnt):
            what = f"after the device refit, K = {k}, counts = {counts}, any = {any_only}"
            if k:
                assert_same(out.cpu().numpy(), want64[:, :k], what)
            else:
                assert bool((out == -7).all())   # not touched
            if counts:
                assert_same(cnt.cpu().numpy(), (want_n > 0).astype(np.int32) if any_only else want_n, what)
            else:
                assert bool((cnt == -7).all())
    finally:
        scene.close()
        world.close()


def test_a_count_split_over_launches(pkg, gpu):
    """2^24 + 3000 boxes (one launch holds 2^24) at K = 1 with counts: far boxes have n = 0 and index -1; the last launch's
    boxes and real boxes scattered over the first launch are restated."""
    import torch
    arrays, scene = loaded(pkg, "small_trisrc")
    n = (1 << 24) + 3000
    real = OC.make_boxes(arrays, 3000 + 4096, seed=33)
    tail, spread = real[:3000], real[3000:]
    far = OR.make_boxes([(1e6, -2e6, 3e6)], [(1.5e6, -1e6, 4e6)])
    pos = arrays["vertex_positions"]
    assert OR.walked(far).all() and not OR.overlaps(pos, far).any()
    d_boxes = device_boxes(far).repeat(n, 1)
    d_boxes[n - 3000:] = device_boxes(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, 4096, replace=False)).cuda()
    d_boxes[sample] = device_boxes(spread)
    d_out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    scene.triangles_in_boxes_into(d_boxes.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr(), max_triangles=1,
                                  stream_ptr=torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    want, want_n = OR.overlap(pos, tail, 1)
    assert (want_n > 0).mean() > 0.3
    assert_same(d_out[n - 3000:].cpu().numpy().reshape(-1, 1), want, "the last launch's boxes")
    assert_same(d_cnt[n - 3000:].cpu().numpy(), want_n, "the last launch's counts")
    want, want_n = OR.overlap(pos, spread, 1)
    assert_same(d_out[sample].cpu().numpy().reshape(-1, 1), want, "boxes of the first launch")
    assert_same(d_cnt[sample].cpu().numpy(), want_n, "counts of the first launch")
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    assert bool((d_out[: n - 3000][rest] == -1).all())
    assert bool((d_cnt[: n - 3000][rest] == 0).all())


def test_refusals_and_no_ops(pkg, gpu):
    """A scene without a packed tree is refused with SHRAY_ERR_BAD_TREE (before anything is launched); count 0 is a no-op; a
    GPU tensor of the wrong shape and "nothing asked for" are refused by the binding; a misaligned device pointer by the
    library."""
    import torch
    hand = chain_scene(5)
    scene = pkg.Scene(hand.desc)
    try:
        for kwargs in ({}, {"max_triangles": 0}, {"counts": False}, {"counters": True}, {"max_triangles": 0, "any_only": True}):
            with pytest.raises(pkg._native.ShrayError) as err:
                scene.triangles_in_boxes(np.zeros((4, 6), F), **kwargs)
            assert err.value.code == BAD_TREE
    finally:
        scene.close()
    arrays, good = loaded(pkg, "lobed_528")
    out, n = good.triangles_in_boxes(np.zeros((0, 6), F))
    assert out.shape == (0, 8) and out.dtype == np.int32 and n.shape == (0,)
    with pytest.raises(ValueError):
        good.triangles_in_boxes(torch.zeros((4, 5), device="cuda"))
    with pytest.raises(ValueError):
        good.triangles_in_boxes(np.zeros((4, 5), F))
    with pytest.raises(ValueError):
        good.triangles_in_boxes(np.zeros((4, 6), F), max_triangles=0, counts=False)
    with pytest.raises(pkg._native.ShrayError):
        good.triangles_in_boxes(np.zeros((4, 6), F), max_triangles=65)
    with pytest.raises(pkg._native.ShrayError):
        good.triangles_in_boxes(np.zeros((4, 6), F), max_triangles=8, any_only=True)
    lib = pkg._native.load_overlap()
    d = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
    op = pkg.tracer.overlap_params(1)
    assert lib.shray_overlap_triangles_device(good._handle, C.byref(op), C.c_void_p(d.data_ptr() + 4), 1, C.c_void_p(d.data_ptr() + 64), None, None) == -1
    assert lib.shray_overlap_triangles_device(good._handle, C.byref(op), C.c_void_p(d.data_ptr()), 1, C.c_void_p(d.data_ptr() + 66), None, None) == -1
