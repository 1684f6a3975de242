"""The device update of an instance set on the GPU (include/shader_ray_instance.h: shray_instance_set_update_device): the set
it builds equals the host update's bit for bit (top-level nodes, W records, world_to_object; then hits, instances and
counters); it is ordered after a refit on its stream; an animation loop of device updates and traces without a synchronise
equals fresh host-built sets; a refused transform changes nothing and update_status names the lowest one; bad arrays are
refused at the call; host and device updates mix."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_instances import assert_same, counters_of, object_box, rotation, scene, world_rays
from test_gpu_ray_query import loaded

pytestmark = pytest.mark.gpu

F = np.float32
INVALID = -1


def arrays(s):
    """(nodes [2n - 1, 8] uint32, records [4n, 4] uint32) as the next query reads them (shrayi_instance_set_arrays)"""
    N = s._lib
    count = C.c_int32()
    assert N.shrayi_instance_set_arrays(s._handle, None, None, C.byref(count)) == 0
    nodes = np.zeros((count.value, 8), np.uint32)
    records = np.zeros((4 * s.count, 4), np.uint32)
    assert N.shrayi_instance_set_arrays(s._handle, nodes.ctypes.data_as(C.c_void_p), records.ctypes.data_as(C.c_void_p), None) == 0
    return nodes, records


def assert_same_set(a, b, what):
    na, ra = arrays(a)
    nb, rb = arrays(b)
    bad = np.nonzero((na != nb).any(1))[0]
    assert not len(bad), f"{what}: {len(bad)} of {len(na)} nodes differ; first {[(j, na[j], nb[j]) for j in bad[:3]]}"
    bad = np.nonzero((ra != rb).any(1))[0]
    assert not len(bad), f"{what}: {len(bad)} of {len(ra)} record rows differ; first {[(j, ra[j], rb[j]) for j in bad[:3]]}"
    assert np.array_equal(a.world_to_object().view(np.uint32), b.world_to_object().view(np.uint32)), what


def placements(pkg, names, n, seed):
    """n instances over the named scenes: rotations, non-uniform scales, mirrors, axis permutations, exact duplicates, zero
    translations"""
    rng = np.random.default_rng(seed)
    pick = [names[i % len(names)] for i in range(n)]
    sizes = {name: float(np.subtract(*object_box(scene(pkg, name)[0])[::-1]).max()) for name in names}
    M = np.zeros((n, 3, 4))
    for i in range(n):
        kind = rng.random()
        if kind < 0.1:
            A = np.eye(3)[rng.permutation(3)] * rng.choice([-1.0, 1.0], 3)       # a permutation with flips: exact zeros
        else:
            A = rotation(rng) @ np.diag(rng.uniform(0.5, 1.8, 3))
            if kind < 0.35:
                A = A @ np.diag([-1.0, 1.0, 1.0])
        M[i, :, :3] = A
        if rng.random() >= 0.1:
            M[i, :, 3] = rng.uniform(-1, 1, 3) * sizes[pick[i]] * (n ** (1 / 3))
    for i in range(2, n, 7):                                                     # duplicates: equal boxes and centres
        pick[i], M[i] = pick[i - 2], M[i - 2]
    return pick, M.astype(F)


def on_gpu(m):
    import torch
    return torch.from_numpy(np.ascontiguousarray(m)).cuda()


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 17, 301, 4096, 65536])
def test_device_update_is_the_host_update_bit_for_bit(pkg, gpu, n):
    names = ["lobed_528", "small_trisrc", "bunny"] if n == 17 else ["lobed_528", "small_trisrc"]
    pick, M0 = placements(pkg, names, n, seed=n)
    _, M1 = placements(pkg, names, n, seed=n + 1)
    members = [scene(pkg, p)[1] for p in pick]
    dev = pkg.tracer.InstanceSet(members, M0)
    host = pkg.tracer.InstanceSet(members, M0)
    dev.update(on_gpu(M1))
    host.update(M1)
    assert dev.update_status() == -1
    assert_same_set(dev, host, f"{n} instances")
    o, d, tmax = world_rays(pkg, pick, M1, 1 << 12, seed=n + 2)
    rays = pkg.tracer.make_rays(o, d, tmax)
    got, gi, gc = dev.trace_rays(rays, counters=True)
    want, wi, wc = host.trace_rays(rays, counters=True)
    assert_same(got, want, f"{n} instances", gi, wi)
    assert counters_of(gc) == counters_of(wc)
    if n >= 17:
        assert (wi >= 0).sum() > 0
    dev.close()
    host.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_refit_then_device_update_on_one_stream(pkg, gpu):
    import torch
    world, _, _ = loaded(pkg, "lobed_528")
    own = pkg.Scene(world.flatten())            # a scene of its own: it is refit below
    other = scene(pkg, "small_trisrc")[1]
    pick, M = placements(pkg, ["lobed_528", "small_trisrc"], 33, seed=33)
    members = [own if p == "lobed_528" else other for p in pick]
    dev = pkg.tracer.InstanceSet(members, M)
    o, d, tmax = world_rays(pkg, pick, M, 1 << 12, seed=34)
    rays = pkg.tracer.make_rays(o, d, tmax)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)).cuda()
    corners = own.geometry()["vertex_positions"].reshape(-1, 3)
    moved = np.ascontiguousarray(corners * F(1.5) + F(0.2))
    d_moved = torch.from_numpy(moved).cuda()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        hits = torch.empty((len(rays), 4), dtype=torch.int32, device="cuda")
        inst = torch.empty(len(rays), dtype=torch.int32, device="cuda")
        own.refit(d_moved, stream_ptr=stream.cuda_stream)
        dev.update_into(0, stream.cuda_stream)
        dev.trace_rays_into(d_rays.data_ptr(), len(rays), hits.data_ptr(), inst.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert dev.update_status() == -1
    host = pkg.tracer.InstanceSet(members, M)      # created after the refit: the host path over the moved scene
    want, wi = host.trace_rays(rays)
    got = hits.cpu().numpy().view(pkg.tracer.HIT_DTYPE).reshape(-1)
    assert_same(got, want, "refit + device update + trace on one stream", inst.cpu().numpy(), wi)
    assert_same_set(dev, host, "refit + device update")
    dev.close()
    host.close()
    own.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_animation_loop_without_a_synchronise(pkg, gpu):
    import torch
    pick, M = placements(pkg, ["lobed_528", "small_trisrc"], 257, seed=257)
    members = [scene(pkg, p)[1] for p in pick]
    dev = pkg.tracer.InstanceSet(members, M)
    o, d, tmax = world_rays(pkg, pick, M, 1 << 12, seed=258)
    rays = pkg.tracer.make_rays(o, d, tmax)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)).cuda()
    rng = np.random.default_rng(259)
    base = on_gpu(M)
    velocity = on_gpu((rng.normal(size=(len(M), 3)) * 0.3).astype(F))
    spin = on_gpu(np.stack([rotation(rng) for _ in range(8)]).astype(F))
    steps = []
    for t in range(8):
        m = base.clone()
        m[:, :, :3] = torch.matmul(spin[t], m[:, :, :3])
        m[:, :, 3] += velocity * float(t)
        hits = torch.empty((len(rays), 4), dtype=torch.int32, device="cuda")
        inst = torch.empty(len(rays), dtype=torch.int32, device="cuda")
        dev.update(m)
        dev.trace_rays_into(d_rays.data_ptr(), len(rays), hits.data_ptr(), inst.data_ptr(), torch.cuda.current_stream().cuda_stream)
        steps.append((m, hits, inst))
    torch.cuda.synchronize()
    assert dev.update_status() == -1
    for t, (m, hits, inst) in enumerate(steps):
        fresh = pkg.tracer.InstanceSet(members, m.cpu().numpy())
        want, wi = fresh.trace_rays(rays)
        assert_same(hits.cpu().numpy().view(pkg.tracer.HIT_DTYPE).reshape(-1), want, f"step {t}", inst.cpu().numpy(), wi)
        fresh.close()
    dev.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def bad_map(kind, m):
    m = m.copy()
    if kind == "nan":
        m[0, 1] = np.nan
    elif kind == "inf":
        m[2, 3] = np.inf
    elif kind == "singular":
        m[2, :3] = m[0, :3]
    else:                                           # invertible in double, W overflows float
        m[:, :3] = np.eye(3) * F(1e-39)
    return m


@pytest.mark.parametrize("kinds", [("nan", "singular"), ("inf", "overflow"), ("singular", "nan"), ("overflow", "inf")])
def test_a_refused_device_update_changes_nothing(pkg, gpu, kinds):
    pick, M0 = placements(pkg, ["lobed_528", "small_trisrc"], 40, seed=40)
    _, M1 = placements(pkg, ["lobed_528", "small_trisrc"], 40, seed=41)
    members = [scene(pkg, p)[1] for p in pick]
    dev = pkg.tracer.InstanceSet(members, M0)
    o, d, tmax = world_rays(pkg, pick, M0, 1 << 12, seed=42)
    rays = pkg.tracer.make_rays(o, d, tmax)
    nodes, records = arrays(dev)
    w2o = dev.world_to_object()
    hits, inst = dev.trace_rays(rays)
    bad = M1.copy()
    bad[23] = bad_map(kinds[0], bad[23])
    bad[9] = bad_map(kinds[1], bad[9])
    with pytest.raises(pkg._native.ShrayError) as err:
        pkg.tracer.InstanceSet(members, bad)       # (the host path refuses it too)
    assert err.value.code == INVALID
    dev.update(on_gpu(bad))
    assert dev.update_status() == 9
    n2, r2 = arrays(dev)
    assert np.array_equal(n2, nodes) and np.array_equal(r2, records)
    assert np.array_equal(dev.world_to_object().view(np.uint32), w2o.view(np.uint32))
    got, gi = dev.trace_rays(rays)
    assert_same(got, hits, "after a refused device update", gi, inst)
    # the kept transforms are the old ones: an update that keeps them rebuilds the same set
    dev.update_into(0)
    assert dev.update_status() == -1
    assert np.array_equal(arrays(dev)[0], nodes)
    # a valid update after it applies
    dev.update(on_gpu(M1))
    assert dev.update_status() == -1
    host = pkg.tracer.InstanceSet(members, M1)
    assert_same_set(dev, host, "a valid update after a refused one")
    dev.close()
    host.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arrays_are_refused_at_the_call(pkg, gpu):
    import torch
    N = pkg._native
    lib = N.load_instance()
    pick, M = placements(pkg, ["lobed_528"], 17, seed=17)
    members = [scene(pkg, p)[1] for p in pick]
    dev = pkg.tracer.InstanceSet(members, M)
    before = arrays(dev)
    bad = M.copy()
    bad[3] = bad_map("nan", bad[3])
    dev.update(on_gpu(bad))
    assert dev.update_status() == 3
    h, V, nbytes = dev._handle, C.c_void_p, M.nbytes
    host = np.ascontiguousarray(M)
    assert lib.shray_instance_set_update_device(h, host.ctypes.data_as(V), None) == INVALID            # host memory
    assert lib.shray_instance_set_update_device(None, V(on_gpu(M).data_ptr()), None) == INVALID        # no set
    d = torch.zeros(M.size + 1, dtype=torch.float32, device="cuda")
    assert lib.shray_instance_set_update_device(h, V(d.data_ptr() + 2), None) == INVALID               # misaligned
    # a short allocation: the last nbytes - 4 bytes of a 2 MiB hipMalloc
    hip = C.CDLL("libamdhip64.so")
    raw = C.c_void_p()
    assert hip.hipMalloc(C.byref(raw), C.c_size_t(2 << 20)) == 0
    try:
        assert lib.shray_instance_set_update_device(h, V(raw.value + (2 << 20) - nbytes + 4), None) == INVALID
        assert b"past the end" in N.load_hip().shray_last_error()
    finally:
        hip.hipFree(raw)
    if torch.cuda.device_count() > 1:                                                                   # another device's
        other = torch.from_numpy(host).to(torch.device("cuda", 1 if dev.device == 0 else 0))
        assert lib.shray_instance_set_update_device(h, V(other.data_ptr()), None) == INVALID
    with pytest.raises(ValueError):
        dev.update(on_gpu(M[:-1]))
    assert dev.update_status() == 3, "an argument error enqueues nothing: the status is the update's before it"
    assert all(np.array_equal(x, y) for x, y in zip(arrays(dev), before))
    dev.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_host_and_device_updates_mixed(pkg, gpu):
    names = ["lobed_528", "small_trisrc"]
    pick, M0 = placements(pkg, names, 65, seed=65)
    M1, M2, M3, M4 = (placements(pkg, names, 65, seed=66 + k)[1] for k in range(4))
    members = [scene(pkg, p)[1] for p in pick]
    dev = pkg.tracer.InstanceSet(members, M0)
    ref = pkg.tracer.InstanceSet(members, M1)
    # device update, then update(None): the device's transforms
    dev.update(on_gpu(M1))
    assert np.array_equal(dev.world_to_object().view(np.uint32), ref.world_to_object().view(np.uint32))
    dev.update(None)
    assert_same_set(dev, ref, "device update, then update(None)")
    # device update, then a host update: the host update alone
    dev.update(on_gpu(M2))
    dev.update(M3)
    ref.update(M3)
    assert_same_set(dev, ref, "device update, then host update")
    # host update, then a device update that keeps the transforms: the host's
    dev.update(M4)
    dev.update_into(0)
    ref.update(M4)
    assert dev.update_status() == -1
    assert_same_set(dev, ref, "host update, then device update(NULL)")
    o, d, tmax = world_rays(pkg, pick, M4, 1 << 12, seed=70)
    rays = pkg.tracer.make_rays(o, d, tmax)
    got, gi = dev.trace_rays(rays)
    want, wi = ref.trace_rays(rays)
    assert_same(got, want, "mixed updates", gi, wi)
    import torch
    if torch.cuda.device_count() > 1:                # a tensor on another device is refused before anything is enqueued
        with pytest.raises(ValueError):
            dev.update(on_gpu(M1).to(torch.device("cuda", 1 if dev.device == 0 else 0)))
    dev.close()
    ref.close()
