"""Ray queries on the GPU (include/shader_ray_query.h) against the CPU restatement (tests/ray_query_ref.py): t, u, v as bits
and the triangle of every ray, for kernel id 0 (packed stack traversal) and kernel id 1 (literal threaded traversal); the
work counters; the iteration cap; the any-hit contract; primary hits against the oracle; the device-built scene; device
buffers and argument errors."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import ray_query_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_RAYS = (1 << 17) - 3
KERNELS = [0, 1]
SCENES = ["small_trisrc", "lobed_528", "bunny"]


def scene_path(name):
    return {"small_trisrc": helpers.small_trisrc, "bunny": helpers.bunny_trisrc,
            "lobed_528": lambda: os.path.join(GOLDEN, "lobed_528.trisrc")}[name]()


_cache = {}


def loaded(pkg, name, resident=True):
    """(world, scene arrays, resident scene), once per scene file (resident=False: no scene on the device yet)"""
    if name not in _cache:
        world = pkg.World(scene_path(name))
        _cache[name] = [world, R.SceneArrays(world.arrays()), None]
    entry = _cache[name]
    if resident and entry[2] is None:
        entry[2] = pkg.Scene(entry[0].flatten())
    return tuple(entry)


def random_rays(arrays: R.SceneArrays, n: int, seed: int):
    """Origins in twice the scene's box, inside the mesh and on it; uniform directions, 10 % axis-aligned with +-0.0
    components; mixed tmax (1e7, +inf, random, 0, negative, NaN)."""
    rng = np.random.default_rng(seed)
    pts = arrays.positions.reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    kind = rng.integers(0, 3, n)
    o = (centre + (rng.random((n, 3)) * 2 - 1) * 2 * half).astype(F)                    # twice the box
    inside = kind == 1
    o[inside] = (centre + (rng.random((inside.sum(), 3)) * 2 - 1) * 0.3 * half).astype(F)
    on = kind == 2
    tri = rng.integers(0, len(arrays.positions), on.sum())
    b = rng.random((on.sum(), 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    v = arrays.positions[tri].astype(np.float64)
    o[on] = (v[:, 0] + b[:, :1] * (v[:, 1] - v[:, 0]) + b[:, 1:] * (v[:, 2] - v[:, 0])).astype(F)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    axis = rng.random(n) < 0.1
    k = np.nonzero(axis)[0]
    zeros = np.where(rng.random((len(k), 3)) < 0.5, F(0.0), F(-0.0)).astype(F)
    zeros[np.arange(len(k)), rng.integers(0, 3, len(k))] = np.where(rng.random(len(k)) < 0.5, F(1), F(-1))
    d[k] = zeros
    extent = float(np.linalg.norm(hi - lo))
    tmax = np.full(n, F(1e7))
    r = rng.random(n)
    tmax[r < 0.15] = np.inf
    sel = (r >= 0.15) & (r < 0.5)
    tmax[sel] = (rng.random(sel.sum()) * extent).astype(F)
    tmax[(r >= 0.5) & (r < 0.53)] = 0.0
    tmax[(r >= 0.53) & (r < 0.56)] = -1.5
    tmax[(r >= 0.56) & (r < 0.59)] = np.nan
    return o, d, tmax


def ray_buffer(pkg, o, d, tmax):
    return pkg.tracer.make_rays(o, d, tmax)


def assert_same_hits(got, want, what, skip_cap_uv=True):
    assert got.shape == want.shape
    tri_bad = got["triangle"] != want["triangle"]
    bits = lambda a, f: np.ascontiguousarray(a[f]).view(np.uint32)
    t_bad = bits(got, "t") != bits(want, "t")
    uv_bad = (bits(got, "u") != bits(want, "u")) | (bits(got, "v") != bits(want, "v"))
    if skip_cap_uv:   # a bad hit's u, v are not part of the contract (the timed form may stop its walk at another turn)
        uv_bad &= want["triangle"] != R.HIT_CAP
    bad = np.nonzero(tri_bad | t_bad | uv_bad)[0]
    assert not len(bad), f"{what}: {len(bad)} of {len(got)} rays differ; first: " + "; ".join(
        f"#{i} got {got[i]} want {want[i]}" for i in bad[:5])


_refs = {}


def reference(pkg, name, max_bvh_iterations=400):
    key = (name, max_bvh_iterations)
    if key not in _refs:
        _, arrays, _ = loaded(pkg, name, resident=False)
        o, d, tmax = random_rays(arrays, N_RAYS, seed=SCENES.index(name) + 17)
        hits, counts = R.trace(arrays, o, d, tmax, max_bvh_iterations=max_bvh_iterations)
        _refs[key] = (o, d, tmax, hits, counts)
    return _refs[key]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", SCENES)
def test_closest_hits_and_counters_equal_the_restatement(pkg, gpu, name, kernel):
    _, arrays, scene = loaded(pkg, name)
    scene.set_kernel(kernel)
    o, d, tmax, want, want_counts = reference(pkg, name)
    rays = ray_buffer(pkg, o, d, tmax)
    got = scene.trace_rays(rays)
    assert_same_hits(got, want, f"{name}, kernel {kernel}")
    assert (want["triangle"] >= 0).sum() > N_RAYS // 20 and (want["triangle"] == -1).sum() > N_RAYS // 20
    counted, counters = scene.trace_rays(rays, counters=True)
    assert_same_hits(counted, want, f"{name}, kernel {kernel}, counting instance")
    for k in R.COUNTER_NAMES:
        assert counters[k] == want_counts[k], (k, counters, want_counts)
    assert counters["samples"] == N_RAYS


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["lobed_528", "bunny"])
def test_iteration_cap(pkg, gpu, name, kernel):
    _, arrays, scene = loaded(pkg, name)
    scene.set_kernel(kernel)
    o, d, tmax, want, want_counts = reference(pkg, name, max_bvh_iterations=8)
    assert want_counts["bad_hits"] > 100
    got, counters = scene.trace_rays(ray_buffer(pkg, o, d, tmax), max_bvh_iterations=8, counters=True)
    assert counters["bad_hits"] == want_counts["bad_hits"]
    plain = scene.trace_rays(ray_buffer(pkg, o, d, tmax), max_bvh_iterations=8)
    for hits in (got, plain):
        assert np.array_equal(hits["triangle"] == R.HIT_CAP, want["triangle"] == R.HIT_CAP)
        assert_same_hits(hits, want, f"{name}, kernel {kernel}, cap 8")


def own_test(arrays: R.SceneArrays, o, d, tri):
    """triangle_intersect's distance and barycentrics of triangle `tri` for each ray, without its range tests"""
    v0, v1, v2 = (arrays.positions[tri, m].T for m in range(3))
    e0 = tuple(v1[a] - v0[a] for a in range(3))
    e1 = tuple(v0[a] - v2[a] for a in range(3))
    D = tuple(d[:, a] for a in range(3))
    M = R._cross(e1, D)
    with np.errstate(all="ignore"):
        inv_det = F(1) / R._dot(e0, M)
        T = tuple(o[:, a] - v0[a] for a in range(3))
        Q = R._cross(T, e0)
        return -R._dot(e1, Q) * inv_det, R._dot(T, M) * inv_det, R._dot(D, Q) * inv_det


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", SCENES)
def test_any_hit_contract(pkg, gpu, name, kernel):
    _, arrays, scene = loaded(pkg, name)
    scene.set_kernel(kernel)
    o, d, tmax, closest, _ = reference(pkg, name)
    anyh = scene.trace_rays(ray_buffer(pkg, o, d, tmax), any_hit=True)
    assert np.array_equal(anyh["triangle"] == R.HIT_MISS, closest["triangle"] == R.HIT_MISS)
    k = np.nonzero(anyh["triangle"] >= 0)[0]
    assert (anyh["t"][k] < tmax[k]).all()
    t, u, v = own_test(arrays, o[k], d[k], anyh["triangle"][k])
    for field, mine in (("t", t), ("u", u), ("v", v)):
        assert np.array_equal(anyh[field][k].view(np.uint32), mine.astype(F).view(np.uint32)), field


def first_orbit_view(pkg, world, width, height):
    import bench
    return bench.orbit_params(pkg, world, width, height)[0]


@pytest.mark.parametrize("kernel", KERNELS)
def test_primary_hits_full_hd_equal_the_oracle(pkg, gpu, oracle_mod, kernel):
    world, _, scene = loaded(pkg, "bunny")
    scene.set_kernel(kernel)
    W, H = 1920, 1080
    params = first_orbit_view(pkg, world, W, H)
    hits = scene.primary_hits(params, W, H)
    assert hits.shape == (H, W)
    key = ("oracle_first", W, H)
    if key not in _refs:
        p = params.copy()
        p.bounce_count = 1
        p.diffuse_color[:] = [0.0, 0.0, 0.0]
        _refs[key] = oracle_mod.render_with_paths(world.flatten(), pkg.scenes.environment_constant(), p, W, H, threads=16)[3]
    first = _refs[key]
    tri = np.where(hits["triangle"] == R.HIT_CAP, -1, hits["triangle"])
    bad = np.argwhere(tri != first)
    assert not len(bad), f"{len(bad)} pixels differ from the oracle's first triangle; first {bad[:5].tolist()}"
    assert (tri >= 0).sum() > W * H // 20


@pytest.mark.parametrize("kernel", KERNELS)
def test_primary_hits_equal_the_restatement(pkg, gpu, oracle_mod, kernel):
    world, arrays, scene = loaded(pkg, "bunny")
    scene.set_kernel(kernel)
    W = H = 256
    params = first_orbit_view(pkg, world, W, H)
    o, d = R.camera_rays(oracle_mod, params, W, H)
    want, _ = R.trace(arrays, o, d, F(1e7), max_bvh_iterations=params.max_bvh_iterations, max_leaf_tests=params.max_leaf_tests)
    assert_same_hits(scene.primary_hits(params, W, H).reshape(-1), want, f"primary hits, kernel {kernel}")


def test_device_world_equals_host_scene(pkg, gpu):
    path = helpers.bunny_trisrc()
    dw = pkg.tracer.DeviceWorld(path)
    try:
        _, arrays, scene = loaded(pkg, "bunny")
        scene.set_kernel(0)
        o, d, tmax, _, _ = reference(pkg, "bunny")
        rays = ray_buffer(pkg, o, d, tmax)
        a, b = dw.trace_rays(rays), scene.trace_rays(rays)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        params = dw.frame_params(320, 240)
        assert np.array_equal(dw.primary_hits(params, 320, 240).view(np.uint32), scene.primary_hits(params, 320, 240).view(np.uint32))
    finally:
        dw.close()


def test_device_buffers_on_the_torch_stream(pkg, gpu):
    import torch
    _, arrays, scene = loaded(pkg, "bunny")
    scene.set_kernel(0)
    o, d, tmax, _, _ = reference(pkg, "bunny")
    rays = ray_buffer(pkg, o, d, tmax)
    want = scene.trace_rays(rays)
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    d_hits = torch.empty((len(rays), 4), dtype=torch.int32, device="cuda")
    scene.trace_rays_into(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got = d_hits.cpu().numpy().view(pkg.tracer.HIT_DTYPE).reshape(-1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_count_beyond_one_launch(pkg, gpu):
    import torch
    _, arrays, scene = loaded(pkg, "bunny")
    scene.set_kernel(0)
    n = (1 << 24) + 5
    g = torch.Generator(device="cuda").manual_seed(5)
    pts = torch.from_numpy(arrays.positions.reshape(-1, 3)).cuda()
    lo, hi = pts.min(0).values, pts.max(0).values
    d_rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    d_rays[:, 0:3] = lo + (hi - lo) * (torch.rand((n, 3), generator=g, device="cuda") * 2 - 0.5)
    d_rays[:, 3] = 1e7
    dirs = torch.randn((n, 3), generator=g, device="cuda")
    d_rays[:, 4:7] = dirs / dirs.norm(dim=1, keepdim=True)
    d_rays[:, 7] = 0
    d_hits = torch.full((n, 4), 7, dtype=torch.int32, device="cuda")
    scene.trace_rays_into(d_rays.data_ptr(), n, d_hits.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    sample = np.random.default_rng(11).choice(n, 4096, replace=False)
    sample = np.concatenate([sample, np.arange(n - 5, n)])   # the second launch's rays
    rays = d_rays[torch.from_numpy(sample).cuda()].cpu().numpy()
    got = d_hits[torch.from_numpy(sample).cuda()].cpu().numpy().view(pkg.tracer.HIT_DTYPE).reshape(-1)
    want, _ = R.trace(arrays, rays[:, 0:3], rays[:, 4:7], rays[:, 3])
    assert_same_hits(got, want, "2^24 + 5 rays, sampled")
    assert (got["triangle"] >= 0).any()


def test_argument_errors(pkg, gpu):
    import torch
    N = pkg._native
    lib = N.load_query()
    _, _, scene = loaded(pkg, "small_trisrc")
    h = scene._handle
    qp = pkg.tracer.query_params()
    d_rays = torch.zeros((64, 8), dtype=torch.float32, device="cuda")
    d_hits = torch.zeros((64 + 1, 4), dtype=torch.int32, device="cuda")
    rp, hp, st = C.c_void_p(d_rays.data_ptr()), C.c_void_p(d_hits.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    E = -1   # SHRAY_ERR_INVALID_ARGUMENT
    assert lib.shray_trace_rays_device(h, C.byref(qp), rp, 0, hp, st) == 0
    assert lib.shray_trace_rays_device(h, C.byref(qp), rp, -1, hp, st) == E
    assert lib.shray_trace_rays_device(None, C.byref(qp), rp, 4, hp, st) == E
    assert lib.shray_trace_rays_device(h, None, rp, 4, hp, st) == E
    assert lib.shray_trace_rays_device(h, C.byref(qp), None, 4, hp, st) == E
    assert lib.shray_trace_rays_device(h, C.byref(qp), rp, 4, None, st) == E
    assert lib.shray_trace_rays_device(h, C.byref(qp), C.c_void_p(d_rays.data_ptr() + 4), 4, hp, st) == E
    assert lib.shray_trace_rays_device(h, C.byref(qp), rp, 4, C.c_void_p(d_hits.data_ptr() + 8), st) == E
    assert N.load_hip().shray_last_error()
    bad = pkg.tracer.query_params()
    bad.struct_size = 12
    assert lib.shray_trace_rays_device(h, C.byref(bad), rp, 4, hp, st) == E
    rays = np.zeros(4, pkg.tracer.RAY_DTYPE)
    hits = np.zeros(4, pkg.tracer.HIT_DTYPE)
    assert lib.shray_trace_rays(h, C.byref(bad), rays.ctypes.data_as(C.c_void_p), 4, hits.ctypes.data_as(C.c_void_p)) == E
    assert lib.shray_trace_rays(h, C.byref(qp), rays.ctypes.data_as(C.c_void_p), -3, hits.ctypes.data_as(C.c_void_p)) == E
    assert lib.shray_trace_rays(h, C.byref(qp), None, 4, hits.ctypes.data_as(C.c_void_p)) == E
    assert lib.shray_trace_rays(h, C.byref(qp), rays.ctypes.data_as(C.c_void_p), 4, None) == E
    assert lib.shray_trace_rays(h, C.byref(qp), rays.ctypes.data_as(C.c_void_p), 0, hits.ctypes.data_as(C.c_void_p)) == 0
    c = N.Counters()
    assert lib.shray_trace_rays_counters(h, C.byref(qp), rays.ctypes.data_as(C.c_void_p), 4, None, None) == E
    assert lib.shray_trace_rays_counters(h, C.byref(qp), rays.ctypes.data_as(C.c_void_p), -1, None, C.byref(c)) == E
    params = N.FrameParams()
    N.load_hip().shray_frame_params_init(C.byref(params))
    assert lib.shray_primary_hits_device(h, C.byref(params), 8, 8, C.c_void_p(d_hits.data_ptr() + 4), st) == E
    assert lib.shray_primary_hits_device(h, None, 8, 8, hp, st) == E
    assert lib.shray_primary_hits_device(h, C.byref(params), 0, 8, hp, st) == E
    params.struct_size = 4
    assert lib.shray_primary_hits_device(h, C.byref(params), 8, 8, hp, st) == E
