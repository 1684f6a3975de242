"""Closest-point queries on the GPU (include/shader_ray_point.h) against the restatement (tests/point_query_ref.py): all 32 bytes
of every record bit for bit, for points on the surface, near it, inside the mesh, on node box faces, at vertices, far away and
duplicated, with mixed radii and non-finite inputs; the host and device (torch stream) paths; host-built scenes and
DeviceWorld; after a device refit on the same stream; the counters; a count split over launches; and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import point_query_ref as R
from test_oracle_kat import chain_scene

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAD_TREE = -6


def scene_path(name):
    return {"small_trisrc": helpers.small_trisrc, "bunny": helpers.bunny_trisrc,
            "lobed_528": lambda: os.path.join(GOLDEN, "lobed_528.trisrc"),
            "quads_mixed": lambda: os.path.join(GOLDEN, "quads_mixed.obj"),
            "quads_nonormals": lambda: os.path.join(GOLDEN, "quads_nonormals.obj")}[name]()


_cache = {}


def loaded(pkg, name):
    """(flattened arrays, resident host-built scene), once per scene file"""
    if name not in _cache:
        world = pkg.World(scene_path(name))
        arrays = world.arrays()
        _cache[name] = (world, arrays, pkg.Scene(world.flatten()))
    return _cache[name][1], _cache[name][2]


def make_points(arrays, n, seed):
    """POINT_DTYPE points of every kind the header cares about (module doc), with radii +inf (most), finite, 0, negative, NaN."""
    rng = np.random.default_rng(seed)
    tris = np.asarray(arrays["vertex_positions"], F).reshape(-1, 3, 3)
    verts = tris.reshape(-1, 3)
    lo, hi = verts.min(0), verts.max(0)
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    extent = float(np.linalg.norm(hi - lo))
    kind = rng.integers(0, 7, n)
    p = np.zeros((n, 3), F)
    t = rng.integers(0, len(tris), n)
    b = rng.random((n, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    v = tris[t].astype(np.float64)
    on = (v[:, 0] + b[:, :1] * (v[:, 1] - v[:, 0]) + b[:, 1:] * (v[:, 2] - v[:, 0]))
    p[:] = on.astype(F)                                                                      # 0: on the surface
    near = kind == 1
    p[near] = (on[near] + rng.normal(size=(near.sum(), 3)) * extent / 100 / 1.7).astype(F)   # 1: near it
    inside = kind == 2
    p[inside] = (centre + (rng.random((inside.sum(), 3)) * 2 - 1) * 0.3 * half).astype(F)  # 2: inside the mesh
    face = np.nonzero(kind == 3)[0]                                                         # 3: on a node box face
    bmin = np.asarray(arrays["group_boxmin"], F).reshape(-1, 3)
    bmax = np.asarray(arrays["group_boxmax"], F).reshape(-1, 3)
    node = rng.integers(0, len(bmin), len(face))
    f = (bmin[node] + (bmax[node] - bmin[node]) * rng.random((len(face), 3))).astype(F)
    axis = rng.integers(0, 3, len(face))
    f[np.arange(len(face)), axis] = np.where(rng.random(len(face)) < 0.5, bmin[node, axis], bmax[node, axis])
    corner = rng.random(len(face)) < 0.2
    f[corner] = np.where(rng.random((corner.sum(), 3)) < 0.5, bmin[node[corner]], bmax[node[corner]])
    p[face] = f
    at = kind == 4
    p[at] = verts[rng.integers(0, len(verts), at.sum())]                                    # 4: exactly at vertices
    far = kind == 5
    p[far] = (centre + rng.normal(size=(far.sum(), 3)) * 100 * extent).astype(F)            # 5: far away
    dup = np.nonzero(kind == 6)[0]                                                          # 6: duplicates of others
    p[dup] = p[rng.integers(0, n, len(dup))]
    md = np.full(n, np.inf, F)
    r = rng.random(n)
    sel = (r >= 0.6) & (r < 0.85)
    md[sel] = (rng.random(sel.sum()) * extent / 20) ** 2
    md[(r >= 0.85) & (r < 0.88)] = 0.0
    md[(r >= 0.88) & (r < 0.90)] = -1.0
    md[(r >= 0.90) & (r < 0.92)] = np.nan
    bad = np.nonzero((r >= 0.92) & (r < 0.94))[0]
    p[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(bad))
    out = np.zeros(n, R.POINT_DTYPE)
    out["p"], out["max_dist2"] = p, md
    return out


def assert_bits(got, want, what):
    g, w = R.as_bits(got), R.as_bits(want)
    bad = np.nonzero((g != w).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(g)} records differ, first {bad[:5]}: got {got[bad[:3]]} want {want[bad[:3]]}"


def device_query(pkg, scene, points):
    """the device path on the current torch stream, from a [n, 4] float32 tensor"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(points).view(F).reshape(-1, 4).copy()).cuda()
    out = scene.closest_points(t)
    assert out.dtype == torch.int32 and out.shape == (len(points), 8) and out.is_cuda
    torch.cuda.current_stream().synchronize()
    return np.ascontiguousarray(out.cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1)


@pytest.mark.parametrize("name, n", [("small_trisrc", 20000), ("lobed_528", 20000), ("quads_mixed", 3000),
                                     ("quads_nonormals", 12000)])
def test_small_scenes_bit_exact(pkg, gpu, name, n):
    arrays, scene = loaded(pkg, name)
    pts = make_points(arrays, n, seed=n + len(name))
    want = R.closest(arrays["vertex_positions"], pts)
    assert (want["triangle"] >= 0).sum() > n // 2
    assert_bits(scene.closest_points(pts), want, f"{name}, host path")
    assert_bits(device_query(pkg, scene, pts), want, f"{name}, device path")


def test_bunny_bit_exact_and_counters(pkg, gpu):
    """A few thousand points on the bunny-class mesh against the torch restatement (itself checked against numpy on a subset);
    the counters: identical across runs, triangle_tests >= hits, and near-surface points test far fewer triangles than the
    brute force (asserted: a mean below 1 % of the scene's triangles)."""
    arrays, scene = loaded(pkg, "bunny")
    pts = make_points(arrays, 4000, seed=7)
    want = R.closest_torch(arrays["vertex_positions"], pts, device="cuda")
    assert_bits(want[:120], R.closest(arrays["vertex_positions"], pts[:120]), "torch restatement against numpy")
    got, c1 = scene.closest_points(pts, counters=True)
    assert_bits(got, want, "bunny, host path")
    assert_bits(device_query(pkg, scene, pts), want, "bunny, device path")
    _, c2 = scene.closest_points(pts, counters=True)
    assert c1 == c2
    hits = int((want["triangle"] >= 0).sum())
    assert c1["samples"] == len(pts) and c1["triangle_tests"] >= hits and c1["leaf_visits"] > 0 and c1["node_visits"] > 0
    assert c1["shaded_hits"] == c1["env_lookups"] == c1["traversals"] == c1["bad_hits"] == 0

    tris = np.asarray(arrays["vertex_positions"], F).reshape(-1, 3, 3)
    rng = np.random.default_rng(8)
    t = rng.integers(0, len(tris), 2048)
    extent = float(np.linalg.norm(tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)))
    near = (tris[t].mean(1) + rng.normal(size=(2048, 3)) * extent / 100 / 1.7).astype(F)
    got, c = scene.closest_points(pkg.tracer.make_points(near), counters=True)
    assert (got["triangle"] >= 0).all()
    mean_tests = c["triangle_tests"] / len(near)
    assert mean_tests < len(tris) / 100, (mean_tests, c)


def test_device_world_matches_host_scene(pkg, gpu):
    arrays, scene = loaded(pkg, "lobed_528")
    dw = pkg.tracer.DeviceWorld(scene_path("lobed_528"))
    try:
        flat = dw.flat_arrays()
        assert np.array_equal(np.asarray(flat["vertex_positions"], F).view(np.uint32),
                              np.asarray(arrays["vertex_positions"], F).view(np.uint32))
        pts = make_points(arrays, 8000, seed=21)
        want = R.closest(flat["vertex_positions"], pts)
        assert_bits(dw.closest_points(pts), want, "DeviceWorld, host path")
        assert_bits(device_query(pkg, dw, pts), want, "DeviceWorld, device path")
        assert_bits(scene.closest_points(pts), want, "host Scene")
    finally:
        dw.close()


def test_closest_points_into_on_a_stream_after_a_device_refit(pkg, gpu):
    """A refit and a query enqueued on one side stream: the query sees the refit geometry (restated on the new corners)."""
    import torch
    world = pkg.World(scene_path("lobed_528"))
    scene = pkg.Scene(world.flatten())
    try:
        pos = np.asarray(world.arrays()["vertex_positions"], F).reshape(-1, 3)
        rng = np.random.default_rng(4)
        moved = (pos * F(1.3) + rng.normal(size=pos.shape).astype(F) * F(0.01) + F(0.5)).astype(F)
        pts = make_points({"vertex_positions": moved.reshape(-1), "group_boxmin": world.arrays()["group_boxmin"],
                           "group_boxmax": world.arrays()["group_boxmax"]}, 6000, seed=9)
        d_moved = torch.from_numpy(moved).cuda()
        d_pts = torch.from_numpy(np.ascontiguousarray(pts).view(F).reshape(-1, 4).copy()).cuda()
        d_out = torch.full((len(pts), 8), -7, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            scene.refit(d_moved, stream_ptr=side.cuda_stream)
            scene.closest_points_into(d_pts.data_ptr(), len(pts), d_out.data_ptr(), side.cuda_stream)
        side.synchronize()
        got = np.ascontiguousarray(d_out.cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1)
        now = scene.geometry()["vertex_positions"]
        assert np.array_equal(now.view(np.uint32), moved.reshape(-1).view(np.uint32))
        assert_bits(got, R.closest(moved.reshape(-1), pts), "after the device refit")
    finally:
        scene.close()
        world.close()


def test_a_count_split_over_launches(pkg, gpu):
    """2^24 + 3000 points (one launch holds 2^24): far points with radius 0 are misses; the last launch's points and real
    points scattered over the first launch are restated."""
    import torch
    arrays, scene = loaded(pkg, "small_trisrc")
    n = (1 << 24) + 3000
    real = make_points(arrays, 3000 + 4096, seed=33)
    tail, spread = real[:3000], real[3000:]
    far = np.zeros(1, R.POINT_DTYPE)
    far["p"] = (1e6, -2e6, 3e6)
    far["max_dist2"] = 0.0

    def dev(p):
        return torch.from_numpy(np.ascontiguousarray(p).view(F).reshape(-1, 4).copy()).cuda()

    d_pts = dev(far).repeat(n, 1)
    d_pts[n - 3000:] = dev(tail)
    sample = torch.from_numpy(np.random.default_rng(1).choice(n - 3000, 4096, replace=False)).cuda()
    d_pts[sample] = dev(spread)
    d_out = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    scene.closest_points_into(d_pts.data_ptr(), n, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()

    def records(t):
        return np.ascontiguousarray(t.cpu().numpy()).view(R.CLOSEST_DTYPE).reshape(-1)

    assert_bits(records(d_out[n - 3000:]), R.closest(arrays["vertex_positions"], tail), "the last launch's points")
    assert_bits(records(d_out[sample]), R.closest(arrays["vertex_positions"], spread), "points of the first launch")
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    far_record = torch.from_numpy(R.as_bits(R.closest(arrays["vertex_positions"], far)).view(np.int32).copy()).cuda()
    assert far_record[0, 6] == -1
    assert bool((d_out[: n - 3000][rest] == far_record).all())


def test_refusals_and_no_ops(pkg, gpu):
    """A scene without a packed tree is refused with SHRAY_ERR_BAD_TREE (before anything is launched); count 0 is a no-op; a
    GPU tensor of the wrong shape is refused by the binding."""
    import torch
    hand = chain_scene(5)
    scene = pkg.Scene(hand.desc)
    try:
        with pytest.raises(pkg._native.ShrayError) as err:
            scene.closest_points(np.zeros((4, 3), F))
        assert err.value.code == BAD_TREE
    finally:
        scene.close()
    arrays, good = loaded(pkg, "lobed_528")
    assert len(good.closest_points(np.zeros((0, 3), F))) == 0
    with pytest.raises(ValueError):
        good.closest_points(torch.zeros((4, 5), device="cuda"))
    with pytest.raises(ValueError):
        good.closest_points(torch.zeros((4, 4), device="cuda"), counters=True)
    lib = pkg._native.load_point()
    d = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    assert lib.shray_closest_points_device(good._handle, C.c_void_p(d.data_ptr() + 4), 1, C.c_void_p(d.data_ptr()), None) == -1
