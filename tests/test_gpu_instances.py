"""Instanced ray queries on the GPU (include/shader_ray_instance.h): one identity instance is the plain query bit for bit
(hits and counters); rigid permutations and flips are the plain query on the transformed rays; sets of 2 to 4096 instances
equal the composition of per-instance queries on rays moved by the set's own W (t, u, v, triangle and instance as bits);
the any-hit contract and the cap; updates and refits; the device form on a torch stream; argument errors."""
import ctypes as C

import numpy as np
import pytest

import instance_ref as I
import ray_query_ref as R
from test_gpu_ray_query import loaded, random_rays
from test_oracle_kat import chain_scene

pytestmark = pytest.mark.gpu

F = np.float32
SCENES = ["small_trisrc", "lobed_528", "bunny"]
INVALID, BAD_TREE = -1, -6


def scene(pkg, name):
    _, arrays, sc = loaded(pkg, name)
    sc.set_kernel(0)   # (the plain query's kernel id 0 is the walk every instance runs)
    return arrays, sc


def bits(a, f):
    return np.ascontiguousarray(a[f]).view(np.uint32)


def mismatches(got, want, got_inst=None, want_inst=None, cap_uv=False):
    bad = (got["triangle"] != want["triangle"]) | (bits(got, "t") != bits(want, "t"))
    uv = (bits(got, "u") != bits(want, "u")) | (bits(got, "v") != bits(want, "v"))
    bad |= uv if cap_uv else uv & (want["triangle"] != R.HIT_CAP)
    if got_inst is not None:
        bad |= got_inst != want_inst
    return np.nonzero(bad)[0]


def assert_same(got, want, what, got_inst=None, want_inst=None):
    bad = mismatches(got, want, got_inst, want_inst)
    assert not len(bad), f"{what}: {len(bad)} of {len(got)} rays differ; first: " + "; ".join(
        f"#{i} got {got[i]} / {None if got_inst is None else got_inst[i]} want {want[i]} / "
        f"{None if want_inst is None else want_inst[i]}" for i in bad[:5])


def counters_of(c):
    return {k: c[k] for k in R.COUNTER_NAMES}


# 1, 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_one_identity_instance_is_the_plain_query(pkg, gpu, name):
    arrays, sc = scene(pkg, name)
    o, d, tmax = random_rays(arrays, (1 << 15) + 7, seed=SCENES.index(name) + 101)
    rays = pkg.tracer.make_rays(o, d, tmax)
    s = pkg.tracer.InstanceSet([sc], np.eye(3, 4, dtype=F)[None])
    assert np.array_equal(s.world_to_object()[0], np.eye(3, 4, dtype=F))
    for any_hit in (False, True):
        want = sc.trace_rays(rays, any_hit=any_hit)
        got, inst = s.trace_rays(rays, any_hit=any_hit)
        assert_same(got, want, f"{name}, any_hit {any_hit}")
        assert np.array_equal(inst, np.where(want["triangle"] >= 0, 0, -1))
    want, wc = sc.trace_rays(rays, counters=True)
    got, inst, gc = s.trace_rays(rays, counters=True)
    assert_same(got, want, f"{name}, counting")
    assert counters_of(gc) == counters_of(wc)
    s.close()


RIGID = {
    "translation": [[1, 0, 0, 0.75], [0, 1, 0, -2.0], [0, 0, 1, 0.5]],
    "permutation": [[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]],
    "flip": [[-1, 0, 0, 0.25], [0, 1, 0, 0], [0, 0, -1, 3.0]],
    "permuted_flip": [[0, 0, -1, 0], [-1, 0, 0, 1.0], [0, 1, 0, 0]],
}


@pytest.mark.parametrize("kind", sorted(RIGID))
def test_rigid_maps_are_the_plain_query_on_moved_rays(pkg, gpu, kind):
    arrays, sc = scene(pkg, "lobed_528")
    M = np.asarray(RIGID[kind], F)
    s = pkg.tracer.InstanceSet([sc], M[None])
    W = s.world_to_object()[0]
    o, d, tmax = random_rays(arrays, 1 << 14, seed=5)
    # world rays whose object rays are the random ones (up to rounding): then the query sees the moved rays
    wo, wd = I.object_vectors(M, o, True), I.object_vectors(M, d, False)   # (the same rule keeps signed zeros through M)
    Po, Do = I.object_rays(W, wo, wd)
    assert np.array_equal(np.signbit(Do), np.signbit(d)), "a rigid map keeps the direction's signed zeros"
    for any_hit in (False, True):
        want = sc.trace_rays(pkg.tracer.make_rays(Po, Do, tmax), any_hit=any_hit)
        got, inst = s.trace_rays(pkg.tracer.make_rays(wo, wd, tmax), any_hit=any_hit)
        assert_same(got, want, f"{kind}, any_hit {any_hit}")
    want, wc = sc.trace_rays(pkg.tracer.make_rays(Po, Do, tmax), counters=True)
    got, _, gc = s.trace_rays(pkg.tracer.make_rays(wo, wd, tmax), counters=True)
    assert counters_of(gc) == counters_of(wc)
    s.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def object_box(arrays):
    p = arrays.positions.reshape(-1, 3)
    return p.min(0).astype(np.float64), p.max(0).astype(np.float64)


def random_set(pkg, names, n, seed, spread=2.0):
    """n instances over the named scenes: rotations, non-uniform scales, mirrors, overlaps, exact duplicates, one far away"""
    rng = np.random.default_rng(seed)
    pick = [names[i % len(names)] for i in range(n)]
    M = np.zeros((n, 3, 4))
    for i in range(n):
        lo, hi = object_box(scene(pkg, pick[i])[0])
        size = float((hi - lo).max())
        A = rotation(rng) @ np.diag(rng.uniform(0.5, 1.8, 3))
        if rng.random() < 0.25:
            A = A @ np.diag([-1.0, 1.0, 1.0])
        M[i, :, :3] = A
        M[i, :, 3] = rng.uniform(-spread, spread, 3) * size * (n ** (1 / 3)) * 0.5
    if n >= 3:
        pick[2], M[2] = pick[0], M[0]                              # an exact duplicate: ties everywhere
    if n >= 4:
        M[3, :, 3] = [1e5, -2e5, 3e4]                              # far away
    return pick, M.astype(F)


def world_boxes(pkg, pick, M):
    out = []
    for name, m in zip(pick, M.astype(np.float64)):
        lo, hi = object_box(scene(pkg, name)[0])
        c = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        w = c @ m[:, :3].T + m[:, 3]
        out.append((w.min(0), w.max(0), c, w))
    return out


def world_rays(pkg, pick, M, n, seed):
    """random rays through the set's region, rays aimed at world-box corners and edges (grazing), rays from inside instances"""
    rng = np.random.default_rng(seed)
    boxes = world_boxes(pkg, pick, M)
    near = [b for b in boxes if np.abs(b[0]).max() < 5e4] or boxes
    lo = np.min([b[0] for b in near], 0)
    hi = np.max([b[1] for b in near], 0)
    kind = rng.integers(0, 4, n)
    o = lo + (hi - lo) * (rng.random((n, 3)) * 1.4 - 0.2)
    d = rng.normal(size=(n, 3))
    k = np.nonzero(kind == 1)[0]                                   # at a corner of a world box
    for j in k:
        b = boxes[rng.integers(len(boxes))]
        d[j] = b[3][rng.integers(8)] - o[j]
    k = np.nonzero(kind == 2)[0]                                   # at a point of an edge of a world box
    for j in k:
        b = boxes[rng.integers(len(boxes))]
        a, c = b[3][rng.integers(8)], b[3][rng.integers(8)]
        d[j] = a + rng.random() * (c - a) - o[j]
    k = np.nonzero(kind == 3)[0]                                   # from inside an instance's box
    for j in k:
        b = boxes[rng.integers(len(boxes))]
        o[j] = b[0] + (b[1] - b[0]) * rng.random(3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    axis = rng.random(n) < 0.05
    d[axis] = np.eye(3)[rng.integers(0, 3, axis.sum())] * rng.choice([-1, 1], (axis.sum(), 1))
    tmax = np.full(n, F(1e7))
    tmax[rng.random(n) < 0.1] = np.inf
    r = rng.random(n)
    tmax[r < 0.2] = (rng.random((r < 0.2).sum()) * float((hi - lo).max())).astype(F)
    tmax[r > 0.98] = 0.0
    return o.astype(F), d.astype(F), tmax


def composition(pkg, s, pick, o, d, tmax, **kw):
    """per-instance Scene.trace_rays on rays moved by the set's own W, composed; one query per scene for all its instances"""
    W = s.world_to_object()
    n = len(o)
    per = [None] * len(pick)
    for name in sorted(set(pick)):
        ids = [i for i, p in enumerate(pick) if p == name]
        rays = np.concatenate([pkg.tracer.make_rays(*I.object_rays(W[i], o, d), tmax) for i in ids])
        h = scene(pkg, name)[1].trace_rays(rays, **kw)
        for j, i in enumerate(ids):
            per[i] = h[j * n:(j + 1) * n]
    return I.compose(per, tmax)


def same_t_other_triangle(pkg, pick, got, gi, want, wi, j):
    """the one admissible disagreement: another triangle of the same instance at the same t"""
    return gi[j] == wi[j] and gi[j] >= 0 and bits(got, "t")[j] == bits(want, "t")[j] and got["triangle"][j] != want["triangle"][j]


@pytest.mark.parametrize("n,names", [(2, ["lobed_528", "small_trisrc"]), (17, ["lobed_528", "small_trisrc", "bunny"]),
                                     (301, ["small_trisrc", "lobed_528"])])
def test_sets_equal_the_composition(pkg, gpu, n, names):
    pick, M = random_set(pkg, names, n, seed=n)
    s = pkg.tracer.InstanceSet([scene(pkg, p)[1] for p in pick], M)
    o, d, tmax = world_rays(pkg, pick, M, 1 << 13, seed=n + 1)
    want, wi = composition(pkg, s, pick, o, d, tmax, max_bvh_iterations=0)
    got, gi = s.trace_rays(pkg.tracer.make_rays(o, d, tmax), max_bvh_iterations=0)
    bad = mismatches(got, want, gi, wi, cap_uv=True)
    ties = [j for j in bad if same_t_other_triangle(pkg, pick, got, gi, want, wi, j)]
    assert len(ties) == len(bad), "rays differ: " + "; ".join(f"#{j} got {got[j]} / {gi[j]} want {want[j]} / {wi[j]}"
                                                              for j in bad if j not in ties)[:2000]
    assert len(ties) <= len(o) // 1000
    assert (wi >= 0).sum() > len(o) // 10
    if n >= 3:
        assert not np.any(gi == 2), "the duplicate of instance 0 never wins its ties"
    s.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_any_hit_and_the_cap(pkg, gpu):
    pick, M = random_set(pkg, ["lobed_528", "small_trisrc"], 17, seed=4)
    s = pkg.tracer.InstanceSet([scene(pkg, p)[1] for p in pick], M)
    o, d, tmax = world_rays(pkg, pick, M, 1 << 13, seed=41)
    rays = pkg.tracer.make_rays(o, d, tmax)
    closest, ci = s.trace_rays(rays)
    assert not np.any(closest["triangle"] == R.HIT_CAP), "the default cap produces no cap results here"
    uncapped, ui = s.trace_rays(rays, max_bvh_iterations=0)
    assert_same(closest, uncapped, "default cap against no cap", ci, ui)
    anyh, ai = s.trace_rays(rays, any_hit=True)
    assert np.array_equal(anyh["triangle"] == R.HIT_MISS, closest["triangle"] == R.HIT_MISS)
    assert np.array_equal(ai >= 0, anyh["triangle"] >= 0)
    # (t, u, v, triangle) of an any-hit ray are its instance walk's own: the plain any-hit query of that instance's ray
    W = s.world_to_object()
    for i in np.unique(ai[ai >= 0]):
        k = np.nonzero(ai == i)[0]
        want = scene(pkg, pick[i])[1].trace_rays(pkg.tracer.make_rays(*I.object_rays(W[i], o[k], d[k]), tmax[k]), any_hit=True)
        assert_same(anyh[k], want, f"any hit, instance {i}")
    capped, pi = s.trace_rays(rays, max_bvh_iterations=6)
    cap = capped["triangle"] == R.HIT_CAP
    assert cap.sum() > 0
    assert np.all(pi[cap] == -1) and np.all(capped["t"][cap] == -1)
    assert_same(capped[~cap], uncapped[~cap], "capped rays that did not reach the cap", pi[~cap], ui[~cap])
    s.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_update_refit_and_failed_update(pkg, gpu):
    world, arrays, _ = loaded(pkg, "lobed_528")
    own = pkg.Scene(world.flatten())           # a scene of its own: it is refit below
    other = scene(pkg, "small_trisrc")[1]
    pick, M = random_set(pkg, ["lobed_528", "small_trisrc"], 9, seed=9)
    members = [own if p == "lobed_528" else other for p in pick]
    s = pkg.tracer.InstanceSet(members, M)
    o, d, tmax = world_rays(pkg, pick, M, 1 << 12, seed=91)
    rays = pkg.tracer.make_rays(o, d, tmax)
    _, M2 = random_set(pkg, ["lobed_528", "small_trisrc"], 9, seed=10)
    s.update(M2)
    fresh = pkg.tracer.InstanceSet(members, M2)
    assert np.array_equal(s.world_to_object(), fresh.world_to_object())
    a, ai = s.trace_rays(rays)
    b, bi = fresh.trace_rays(rays)
    assert_same(a, b, "updated against fresh", ai, bi)
    fresh.close()
    # a failed update (a singular map) leaves the set as it was
    bad = M2.copy()
    bad[4, :, :3] = 0
    with pytest.raises(pkg._native.ShrayError) as err:
        s.update(bad)
    assert err.value.code == INVALID
    c, ci = s.trace_rays(rays)
    assert_same(c, a, "after a failed update", ci, ai)
    # refit a member (grow it and move it), then update: the composition over the refit scene
    corners = own.geometry()["vertex_positions"].reshape(-1, 3)
    own.refit(np.ascontiguousarray(corners * F(1.25) + F(0.1)))
    s.update()
    want, wi = composition_with(pkg, s, members, o, d, tmax)
    got, gi = s.trace_rays(rays, max_bvh_iterations=0)
    bad = mismatches(got, want, gi, wi, cap_uv=True)
    assert not len(bad), f"{len(bad)} rays differ after refit + update; first {[(got[j], gi[j], want[j], wi[j]) for j in bad[:3]]}"
    s.close()
    own.close()


def composition_with(pkg, s, members, o, d, tmax):
    W = s.world_to_object()
    per = [m.trace_rays(pkg.tracer.make_rays(*I.object_rays(W[i], o, d), tmax), max_bvh_iterations=0) for i, m in enumerate(members)]
    return I.compose(per, tmax)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_device_form_on_a_torch_stream(pkg, gpu):
    import torch
    pick, M = random_set(pkg, ["lobed_528", "small_trisrc"], 5, seed=6)
    s = pkg.tracer.InstanceSet([scene(pkg, p)[1] for p in pick], M)
    n = (1 << 24) + 5
    o, d, tmax = world_rays(pkg, pick, M, 1 << 12, seed=61)
    base = torch.from_numpy(np.ascontiguousarray(pkg.tracer.make_rays(o, d, tmax)).view(np.float32).reshape(-1, 8))
    reps = (n + len(base) - 1) // len(base)
    d_rays = base.cuda().repeat(reps, 1)[:n].contiguous()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_hits = torch.full((n, 4), 7, dtype=torch.int32, device="cuda")
        d_inst = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        s.trace_rays_into(d_rays.data_ptr(), n, d_hits.data_ptr(), d_inst.data_ptr(), stream.cuda_stream)
        d_hits2 = torch.full((n, 4), 7, dtype=torch.int32, device="cuda")
        s.trace_rays_into(d_rays.data_ptr(), n, d_hits2.data_ptr(), 0, stream.cuda_stream)
    stream.synchronize()
    want, wi = s.trace_rays(pkg.tracer.make_rays(o, d, tmax))
    hits = d_hits.cpu().numpy().view(R.HIT_DTYPE).reshape(-1)
    inst = d_inst.cpu().numpy()
    idx = np.arange(n) % len(base)
    for part in (slice(0, 1 << 13), slice((1 << 24) - (1 << 12), n)):
        assert_same(hits[part], want[idx[part]], f"device form {part}", inst[part], wi[idx[part]])
    assert torch.equal(d_hits, d_hits2)
    # trace_rays takes a GPU tensor on the set's device (the device path); one on another device is refused
    got, gi = s.trace_rays(base.cuda())
    assert_same(got, want, "GPU tensor through trace_rays", gi, wi)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            s.trace_rays(base.to(torch.device("cuda", 1 - s.device if s.device < 2 else 0)))
    s.close()


def test_device_world_members_outlive_the_callers_references(pkg, gpu):
    """A DeviceWorld passed to a set and dropped by the caller stays alive with the set (closing it would destroy its scene)."""
    import gc
    path = scene_path_of("lobed_528")
    arrays = scene(pkg, "lobed_528")[0]
    M = np.stack([np.eye(3, 4), np.hstack([np.diag([-1.0, 1.0, 1.0]), [[0.5], [0.0], [0.25]]])]).astype(F)
    s = pkg.tracer.InstanceSet([pkg.tracer.DeviceWorld(path), pkg.tracer.DeviceWorld(path)], M)
    gc.collect()
    o, d, tmax = random_rays(arrays, 1 << 12, seed=83)
    rays = pkg.tracer.make_rays(o, d, tmax)
    before, bi = s.trace_rays(rays)
    assert (bi >= 0).sum() > len(o) // 10
    s.update()
    gc.collect()
    s.update(M[::-1].copy())
    s.update(M)
    after, ai = s.trace_rays(rays)
    assert_same(after, before, "after the callers' references are gone and two updates", ai, bi)
    # the device-built scene equals the host-built one (test_gpu_ray_query.py: test_device_world_equals_host_scene), so the
    # set's hits are the composition over the cached host-built scene
    want, wi = composition(pkg, s, ["lobed_528"] * 2, o, d, tmax)
    assert_same(after, want, "DeviceWorld members against the composition", ai, wi)
    s.close()


def scene_path_of(name):
    from test_gpu_ray_query import scene_path
    return scene_path(name)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_four_thousand_instances(pkg, gpu):
    n = 4096
    rng = np.random.default_rng(7)
    lo, hi = object_box(scene(pkg, "lobed_528")[0])
    size = float((hi - lo).max())
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    M = np.zeros((n, 3, 4))
    for i in range(n):
        M[i, :, :3] = rotation(rng) * rng.uniform(0.4, 0.9)
        M[i, :, 3] = (g[i] + rng.uniform(-0.3, 0.3, 3)) * size
    M = M.astype(F)
    pick = ["lobed_528"] * n
    s = pkg.tracer.InstanceSet([scene(pkg, "lobed_528")[1]] * n, M)
    o, d, tmax = world_rays(pkg, pick, M, 1 << 12, seed=71)
    o = (rng.random((len(o), 3)) * 16 * size - 0.5 * size).astype(F)
    want, wi = composition(pkg, s, pick, o, d, tmax, max_bvh_iterations=0)
    got, gi = s.trace_rays(pkg.tracer.make_rays(o, d, tmax), max_bvh_iterations=0)
    bad = mismatches(got, want, gi, wi, cap_uv=True)
    ties = [j for j in bad if same_t_other_triangle(pkg, pick, got, gi, want, wi, j)]
    assert len(ties) == len(bad), "rays differ: " + "; ".join(f"#{j} got {got[j]} / {gi[j]} want {want[j]} / {wi[j]}"
                                                              for j in bad if j not in ties)[:2000]
    assert (wi >= 0).sum() > len(o) // 10
    s.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(pkg, gpu):
    import torch
    N = pkg._native
    lib = N.load_instance()
    sc = scene(pkg, "lobed_528")[1]
    eye = np.eye(3, 4, dtype=F)[None]
    for bad in (np.nan, np.inf):
        m = eye.copy()
        m[0, 1, 3] = bad
        with pytest.raises(N.ShrayError) as err:
            pkg.tracer.InstanceSet([sc], m)
        assert err.value.code == INVALID
    singular = eye.copy()
    singular[0, 2, :3] = [1, 0, 0]
    with pytest.raises(N.ShrayError) as err:
        pkg.tracer.InstanceSet([sc], singular)
    assert err.value.code == INVALID
    tiny = eye.copy() * F(1e-39)                  # invertible in double, its inverse overflows float
    with pytest.raises(N.ShrayError) as err:
        pkg.tracer.InstanceSet([sc], tiny)
    assert err.value.code == INVALID
    chain = pkg.Scene(chain_scene(5).desc)        # no packed tree
    with pytest.raises(N.ShrayError) as err:
        pkg.tracer.InstanceSet([sc, chain], np.concatenate([eye, eye]))
    assert err.value.code == BAD_TREE
    chain.close()
    s = pkg.tracer.InstanceSet([sc], eye)
    h = s._handle
    qp = pkg.tracer.query_params()
    d_rays = torch.zeros((65, 8), dtype=torch.float32, device="cuda")
    d_hits = torch.zeros((65, 4), dtype=torch.int32, device="cuda")
    d_inst = torch.zeros(66, dtype=torch.int32, device="cuda")
    rp, hp, ip = d_rays.data_ptr(), d_hits.data_ptr(), d_inst.data_ptr()
    dev = lib.shray_trace_instances_device
    V = C.c_void_p
    assert dev(None, C.byref(qp), V(rp), 64, V(hp), V(ip), None) == INVALID
    assert dev(h, None, V(rp), 64, V(hp), V(ip), None) == INVALID
    assert dev(h, C.byref(qp), None, 64, V(hp), V(ip), None) == INVALID
    assert dev(h, C.byref(qp), V(rp), 64, None, V(ip), None) == INVALID
    assert dev(h, C.byref(qp), V(rp), -1, V(hp), V(ip), None) == INVALID
    assert dev(h, C.byref(qp), V(rp), 0, V(hp), V(ip), None) == 0
    assert dev(h, C.byref(qp), V(rp + 4), 64, V(hp), V(ip), None) == INVALID
    assert dev(h, C.byref(qp), V(rp), 64, V(hp + 8), V(ip), None) == INVALID
    assert dev(h, C.byref(qp), V(rp), 64, V(hp), V(ip + 2), None) == INVALID
    assert dev(h, C.byref(qp), V(rp), 64, V(hp), V(ip + 4), None) == 0       # 4-byte alignment is enough for instances
    torch.cuda.synchronize()
    wrong = pkg.tracer.query_params()
    wrong.struct_size = 12
    assert dev(h, C.byref(wrong), V(rp), 64, V(hp), V(ip), None) == INVALID
    host = np.zeros(4, pkg.tracer.RAY_DTYPE)
    hits = np.zeros(4, pkg.tracer.HIT_DTYPE)
    assert lib.shray_trace_instances(h, C.byref(qp), host.ctypes.data_as(V), 4, None, None) == INVALID
    assert lib.shray_trace_instances_counters(h, C.byref(qp), host.ctypes.data_as(V), 4, hits.ctypes.data_as(V), None, None) == INVALID
    assert lib.shray_instance_set_update(h, None) == 0
    assert lib.shray_instance_set_world_to_object(h, None) == INVALID
    with pytest.raises(ValueError):
        s.update(np.zeros((2, 3, 4), F))
    s.close()
