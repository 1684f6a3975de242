"""Within-radius queries on the GPU (include/shader_ray_near.h) against the restatement (tests/near_ref.py): every byte of every
record and every count, for the closest-point tests' kinds of point and radius mix plus radii of 5 to 20 % of the extent
(tests/near_cases.py), K in {0, 1, 2, 3, 4, 5, 8, 9, 64} with and without counts; the pruned form against the counting form and,
at K = 1, against Scene.closest_points byte for byte; the host and device (torch stream) paths; host-built scenes and
DeviceWorld; after a device refit on the same stream; the counters; a count split over launches; and the refusals.  No case is
skipped or tolerated."""
import ctypes as C

import numpy as np
import pytest

import near_ref as NR
import point_query_ref as R
from near_cases import make_points, scene_extent, scene_path
from test_oracle_kat import chain_scene

pytestmark = pytest.mark.gpu

F = np.float32
BAD_TREE = -6
KS = (0, 1, 2, 3, 4, 5, 8, 9, 64)

_cache = {}


def loaded(pkg, name):
    """(flattened arrays, resident host-built scene), once per scene file"""
    if name not in _cache:
        world = pkg.World(scene_path(name))
        arrays = world.arrays()
        _cache[name] = (world, arrays, pkg.Scene(world.flatten()))
    return _cache[name][1], _cache[name][2]


def assert_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = NR.as_bits(got), NR.as_bits(want)
    bad = np.nonzero((g != w).any(1))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(g)} records differ, first (flat index) {bad[:5]}: "
                           f"got {got.reshape(-1)[bad[:3]]} want {want.reshape(-1)[bad[:3]]}")


def device_points(points):
    import torch
    return torch.from_numpy(np.ascontiguousarray(points).view(F).reshape(-1, 4).copy()).cuda()


def records(t, k):
    return np.ascontiguousarray(t.cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1, k)


def device_query(scene, points, k, counts):
    """the device path on the current torch stream, from a [n, 4] float32 tensor"""
    import torch
    out, cnt = scene.triangles_within(device_points(points), max_near=k, counts=counts)
    torch.cuda.current_stream().synchronize()
    if k == 0:
        assert out is None
    else:
        assert out.dtype == torch.int32 and out.shape == (len(points), k, 8) and out.is_cuda
    if counts:
        assert cnt.dtype == torch.int32 and cnt.shape == (len(points),) and cnt.is_cuda
    else:
        assert cnt is None
    return (records(out, k) if k else None), (cnt.cpu().numpy() if counts else None)


def check_every_k(scene, pts, want64, want_n, what, paths=("host", "device")):
    """every K, with and without counts, on the given paths: all bytes of all records, all counts; K = 0 without counts is
    refused by the binding"""
    for k in KS:
        for counts in (True, False):
            if k == 0 and not counts:
                with pytest.raises(ValueError):
                    scene.triangles_within(pts, max_near=0, counts=False)
                continue
            for path in paths:
                if path == "host":
                    got, n = scene.triangles_within(pts, max_near=k, counts=counts)
                else:
                    got, n = device_query(scene, pts, k, counts)
                tag = f"{what}, K = {k}, counts = {counts}, {path} path"
                if k:
                    assert_bits(got, want64[:, :k], tag)   # (the restatement's records for K are its first K of 64: test_near_reference)
                else:
                    assert got is None, tag
                if counts:
                    assert n.dtype == np.int32 and np.array_equal(n, want_n), tag
                else:
                    assert n is None, tag


def assert_interesting(positions, pts, want_n, what):
    """The case that matters cannot vanish.  A third of the points have radius +inf and are walked, so n is the whole scene
    for over 30 %; the unwalked points and the far ones with finite radii give n = 0 for over 5 %.  In a scene of more than 64
    triangles, over 10 % of the points have more triangles within a FINITE radius than the register slots hold (a quarter get
    5 to 20 % of the extent, most of them near the surface), and over 30 % more than any K."""
    triangles = len(positions) // 9
    finite = np.isfinite(pts["max_dist2"])
    print(f"{what}: {triangles} triangles, n > 8 at a finite radius {((want_n > 8) & finite).mean():.3f}, n > 8 {(want_n > 8).mean():.3f}, "
          f"n > 64 {(want_n > 64).mean():.3f}, n == 0 {(want_n == 0).mean():.3f}, max n {want_n.max()}")
    assert (want_n > 8).mean() > 0.30 and (want_n == 0).mean() > 0.05, what
    if triangles > 64:
        assert ((want_n > 8) & finite).mean() > 0.10 and (want_n > 64).mean() > 0.30, what


@pytest.mark.parametrize("name, n", [("small_trisrc", 6000), ("lobed_528", 6000), ("quads_mixed", 2000), ("quads_nonormals", 4000)])
def test_small_scenes_bit_exact(pkg, gpu, name, n):
    arrays, scene = loaded(pkg, name)
    pts = make_points(arrays, n, seed=n + len(name))
    want64, want_n = NR.near(arrays["vertex_positions"], pts, 64)
    assert_interesting(arrays["vertex_positions"], pts, want_n, name)
    check_every_k(scene, pts, want64, want_n, name)
    # K = 1 without counts is the closest-point query's record, all 32 bytes, misses included
    got1, _ = scene.triangles_within(pts, max_near=1, counts=False)
    assert_bits(got1[:, 0], scene.closest_points(pts), f"{name}, K = 1 against closest_points")


def test_bunny_bit_exact_and_counters(pkg, gpu):
    """The bunny-class mesh against the torch restatement (itself checked against numpy on a subset); the counters are those
    of the walk that prunes only by max_dist2: identical for every K and across runs, triangle_tests >= sum(n)."""
    arrays, scene = loaded(pkg, "bunny")
    pts = make_points(arrays, 2000, seed=7)
    pos = arrays["vertex_positions"]
    want64, want_n = NR.near_torch(pos, pts, 64)
    sub64, sub_n = NR.near(pos, pts[:60], 64)
    assert_bits(want64[:60], sub64, "torch restatement against numpy")
    assert np.array_equal(want_n[:60], sub_n)
    assert_interesting(pos, pts, want_n, "bunny")
    check_every_k(scene, pts, want64, want_n, "bunny")
    got1, _ = scene.triangles_within(pts, max_near=1, counts=False)
    assert_bits(got1[:, 0], scene.closest_points(pts), "bunny, K = 1 against closest_points")

    tallies = []
    for k, counts in ((8, True), (8, False), (0, True), (64, True), (8, True)):
        got, n, c = scene.triangles_within(pts, max_near=k, counts=counts, counters=True)
        if k:
            assert_bits(got, want64[:, :k], f"bunny, counters form, K = {k}")
        if counts:
            assert np.array_equal(n, want_n)
        tallies.append(c)
    assert all(c == tallies[0] for c in tallies), tallies
    c = tallies[0]
    assert c["samples"] == len(pts) and c["triangle_tests"] >= int(want_n.sum()) and c["leaf_visits"] > 0 and c["node_visits"] > 0
    assert c["shaded_hits"] == c["env_lookups"] == c["traversals"] == c["bad_hits"] == 0
    with pytest.raises(ValueError):
        scene.triangles_within(device_points(pts[:4]), counters=True)
    # a small radius tests far fewer triangles than the brute force: a mean below 1 % of the scene's
    small = pts.copy()
    small["max_dist2"] = F((scene_extent(pos) / 100) ** 2)
    _, n, c = scene.triangles_within(small, max_near=0, counters=True)
    assert c["triangle_tests"] >= int(n.sum()) and c["triangle_tests"] / len(small) < len(pos) / 9 / 100, c
    assert np.array_equal(scene.near_counts(small), n)


def test_device_world_matches_host_scene(pkg, gpu):
    arrays, scene = loaded(pkg, "lobed_528")
    dw = pkg.tracer.DeviceWorld(scene_path("lobed_528"))
    try:
        flat = dw.flat_arrays()
        assert np.array_equal(np.asarray(flat["vertex_positions"], F).view(np.uint32),
                              np.asarray(arrays["vertex_positions"], F).view(np.uint32))
        pts = make_points(arrays, 4000, seed=21)
        want64, want_n = NR.near(flat["vertex_positions"], pts, 64)
        check_every_k(dw, pts, want64, want_n, "DeviceWorld")
        assert np.array_equal(dw.near_counts(pts), want_n)
        got, n = scene.triangles_within(pts, max_near=9)
        assert_bits(got, want64[:, :9], "host Scene")
        assert np.array_equal(n, want_n)
    finally:
        dw.close()


def test_triangles_within_into_on_a_stream_after_a_device_refit(pkg, gpu):
    """A refit and the queries enqueued on one side stream: they see the refit geometry (restated on the new corners)."""
    import torch
    world = pkg.World(scene_path("lobed_528"))
    scene = pkg.Scene(world.flatten())
    try:
        pos = np.asarray(world.arrays()["vertex_positions"], F).reshape(-1, 3)
        rng = np.random.default_rng(4)
        moved = (pos * F(1.3) + rng.normal(size=pos.shape).astype(F) * F(0.01) + F(0.5)).astype(F)
        pts = make_points({"vertex_positions": moved.reshape(-1), "group_boxmin": world.arrays()["group_boxmin"],
                           "group_boxmax": world.arrays()["group_boxmax"]}, 4000, seed=9)
        d_moved = torch.from_numpy(moved).cuda()
        d_pts = device_points(pts)
        forms = [(8, True), (8, False), (64, False), (0, True)]
        d_out = [torch.full((len(pts), max(k, 1), 8), -7, dtype=torch.int32, device="cuda") for k, _ in forms]
        d_cnt = [torch.full((len(pts),), -7, dtype=torch.int32, device="cuda") for _ in forms]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            scene.refit(d_moved, stream_ptr=side.cuda_stream)
            for (k, counts), out, cnt in zip(forms, d_out, d_cnt):
                scene.triangles_within_into(d_pts.data_ptr(), len(pts), out.data_ptr() if k else 0, cnt.data_ptr() if counts else 0,
                                            max_near=k, stream_ptr=side.cuda_stream)
        side.synchronize()
        now = scene.geometry()["vertex_positions"]
        assert np.array_equal(now.view(np.uint32), moved.reshape(-1).view(np.uint32))
        want64, want_n = NR.near(moved.reshape(-1), pts, 64)
        assert (want_n > 8).mean() > 0.4
        for (k, counts), out, cnt in zip(forms, d_out, d_cnt):
            if k:
                assert_bits(records(out, k), want64[:, :k], f"after the device refit, K = {k}, counts = {counts}")
            else:
                assert bool((out == -7).all())   # not touched
            assert np.array_equal(cnt.cpu().numpy(), want_n) if counts else bool((cnt == -7).all())
    finally:
        scene.close()
        world.close()


def test_a_count_split_over_launches(pkg, gpu):
    """2^24 + 3000 points (one launch holds 2^24) at K = 1 with counts: far points with radius 0 are misses with n = 0; the
    last launch's points and real points scattered over the first launch are restated."""
    import torch
    arrays, scene = loaded(pkg, "small_trisrc")
    n = (1 << 24) + 3000
    real = make_points(arrays, 3000 + 4096, seed=33)
    tail, spread = real[:3000], real[3000:]
    far = np.zeros(1, R.POINT_DTYPE)
    far["p"] = (1e6, -2e6, 3e6)
    far["max_dist2"] = 0.0
    d_pts = device_points(far).repeat(n, 1)
    d_pts[n - 3000:] = device_points(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, 4096, replace=False)).cuda()
    d_pts[sample] = device_points(spread)
    d_out = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    scene.triangles_within_into(d_pts.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr(), max_near=1,
                                stream_ptr=torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    pos = arrays["vertex_positions"]
    want, want_n = NR.near(pos, tail, 1)
    assert_bits(records(d_out[n - 3000:], 1), want, "the last launch's points")
    assert np.array_equal(d_cnt[n - 3000:].cpu().numpy(), want_n)
    want, want_n = NR.near(pos, spread, 1)
    assert_bits(records(d_out[sample], 1), want, "points of the first launch")
    assert np.array_equal(d_cnt[sample].cpu().numpy(), want_n)
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    far_want, far_n = NR.near(pos, far, 1)
    far_record = torch.from_numpy(NR.as_bits(far_want).view(np.int32).copy()).cuda()
    assert far_record[0, 6] == -1 and far_n[0] == 0
    assert bool((d_out[: n - 3000][rest] == far_record).all())
    assert bool((d_cnt[: n - 3000][rest] == 0).all())


def test_refusals_and_no_ops(pkg, gpu):
    """A scene without a packed tree is refused with SHRAY_ERR_BAD_TREE (before anything is launched); count 0 is a no-op; a
    GPU tensor of the wrong shape and "nothing asked for" are refused by the binding; a misaligned device pointer by the
    library."""
    import torch
    hand = chain_scene(5)
    scene = pkg.Scene(hand.desc)
    try:
        for kwargs in ({}, {"max_near": 0}, {"counts": False}, {"counters": True}):
            with pytest.raises(pkg._native.ShrayError) as err:
                scene.triangles_within(np.zeros((4, 3), F), **kwargs)
            assert err.value.code == BAD_TREE
    finally:
        scene.close()
    arrays, good = loaded(pkg, "lobed_528")
    rec, n = good.triangles_within(np.zeros((0, 3), F))
    assert rec.shape == (0, 8) and rec.dtype == R.CLOSEST_DTYPE and n.shape == (0,)
    with pytest.raises(ValueError):
        good.triangles_within(torch.zeros((4, 5), device="cuda"))
    with pytest.raises(ValueError):
        good.triangles_within(np.zeros((4, 3), F), max_near=0, counts=False)
    with pytest.raises(pkg._native.ShrayError):
        good.triangles_within(np.zeros((4, 3), F), max_near=65)
    lib = pkg._native.load_near()
    d = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    np_ = pkg.tracer.near_params(1)
    assert lib.shray_near_triangles_device(good._handle, C.byref(np_), C.c_void_p(d.data_ptr() + 4), 1, C.c_void_p(d.data_ptr()), None, None) == -1
