"""Instanced all-hits ray queries on the GPU (include/shader_ray_instance_multihit.h): one identity instance is
Scene.trace_all_hits byte for byte (records, counts, counters); a set of two against the numpy restatement
(tests/instance_multi_hit_ref.py); sets of 17 and 301 against the merge of per-scene Scene.trace_all_hits answers on rays
moved by the set's own W; translated and duplicated copies of tall_stack, where every insertion form evicts, t_K falls below
later instances' boxes and ties straddle the edge of K; record 0 against InstanceSet.trace_rays; a refit, a device update and
the query on one stream; a count split over two launches; the refusals; the counters of a multi-instance set."""
import ctypes as C

import numpy as np
import pytest

import instance_multi_hit_ref as IM
import instance_ref as I
import multi_hit_ref as M
import ray_query_ref as R
from test_gpu_instances import BAD_TREE, INVALID, random_set, rotation, scene, scene_path_of, world_rays
from test_gpu_multi_hit import assert_same_records, dev, records
from test_gpu_ray_query import loaded, random_rays
from test_oracle_kat import chain_scene

pytestmark = pytest.mark.gpu

F = np.float32
EYE = np.eye(3, 4, dtype=F)
_sets = {}


def assert_same_answer(got, want, what, k):
    """(hits, instances, counts) against (hits, instances, counts) cut at k; a None count is not compared"""
    assert_same_records(got[0], want[0][:, :k], what)
    assert np.array_equal(got[1], want[1][:, :k]), f"{what}: instances differ on {int((got[1] != want[1][:, :k]).any(1).sum())} rays"
    if got[2] is not None:
        assert np.array_equal(got[2], want[2]), f"{what}: counts differ on {int((got[2] != want[2]).sum())} rays"


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_trisrc", "lobed_528", "bunny"])
def test_one_identity_instance_is_the_all_hits_query(pkg, gpu, name):
    arrays, sc = scene(pkg, name)
    o, d, tmax = random_rays(arrays, 4000, seed=41 + len(name))      # the all-hits test's rays
    rays = pkg.tracer.make_rays(o, d, tmax)
    s = pkg.tracer.InstanceSet([sc], EYE[None])
    try:
        for k in (0, 1, 3, 5, 8, 64):
            for with_counts in (True, False):
                if k == 0 and not with_counts:
                    continue
                what = f"{name}, K {k}, counts {with_counts}"
                want, want_counts = sc.trace_all_hits(rays, max_hits=k, counts=with_counts)
                hits, inst, counts = s.trace_all_hits(rays, max_hits=k, counts=with_counts)
                if k:
                    assert_same_records(hits, want, what)
                    assert np.array_equal(inst, np.where(want["triangle"] >= 0, 0, -1)), what
                else:
                    assert hits is None and inst is None
                if with_counts:
                    assert np.array_equal(counts, want_counts), what
                else:
                    assert counts is None
            want, want_counts, want_counters = sc.trace_all_hits(rays, max_hits=k, counters=True)
            hits, inst, counts, counters = s.trace_all_hits(rays, max_hits=k, counters=True)
            if k:
                assert_same_records(hits, want, f"{name}, counting, K {k}")
            assert np.array_equal(counts, want_counts) and counters == want_counters, (name, k, counters, want_counters)
        assert np.array_equal(s.crossing_counts(rays), sc.crossing_counts(rays))
        assert (want_counts > 0).sum() > 400 and (want_counts > 1).sum() > 40
    finally:
        s.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_a_set_of_two_equals_the_restatement(pkg, gpu):
    """lobed_528 and small_trisrc, rotated, scaled non-uniformly and laid over each other: every byte of hits, instances and
    counts against the numpy restatement with the set's own W, on every ray."""
    import torch
    names = ["lobed_528", "small_trisrc"]
    rng = np.random.default_rng(22)
    Mx = np.zeros((2, 3, 4))
    for i, name in enumerate(names):
        pts = scene(pkg, name)[0].positions.reshape(-1, 3).astype(np.float64)
        lo, hi = pts.min(0), pts.max(0)
        A = rotation(rng) @ np.diag(rng.uniform(0.6, 1.7, 3)) / float((hi - lo).max())      # a world size near 1
        Mx[i, :, :3] = A
        Mx[i, :, 3] = -A @ ((lo + hi) / 2) + np.array([[0.0, 0.0, 0.0], [0.3, 0.1, -0.2]])[i]
    Mx = Mx.astype(F)
    s = pkg.tracer.InstanceSet([scene(pkg, n)[1] for n in names], Mx)
    try:
        o, d, tmax = world_rays(pkg, names, Mx, 2000, seed=23)
        rays = pkg.tracer.make_rays(o, d, tmax)
        want = IM.all_hits([scene(pkg, n)[0] for n in names], s.world_to_object(), o, d, tmax, max_hits=64, details=True)
        per = want[5]
        assert ((per[0] > 0) & (per[1] > 0)).sum() > 100, "the two overlap: many rays cross both"
        d_rays = dev(rays)
        for k in (0, 1, 2, 4, 5, 8, 64):
            for with_counts in (True, False):
                if k == 0 and not with_counts:
                    continue
                what = f"set of two, K {k}, counts {with_counts}"
                hits, inst, counts = s.trace_all_hits(rays, max_hits=k, counts=with_counts)
                d_hits, d_inst, d_counts = s.trace_all_hits(d_rays, max_hits=k, counts=with_counts)
                torch.cuda.current_stream().synchronize()
                if k:
                    assert_same_answer((hits, inst, counts), want, what + ", host path", k)
                    assert_same_answer((records(d_hits), d_inst.cpu().numpy(), d_counts.cpu().numpy() if with_counts else None), want,
                                       what + ", device path", k)
                else:
                    assert hits is None and inst is None and np.array_equal(counts, want[2]) and np.array_equal(d_counts.cpu().numpy(), want[2])
    finally:
        s.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
SETS = {17: ["lobed_528", "small_trisrc", "bunny"], 301: ["small_trisrc", "lobed_528"]}


def composed(pkg, n):
    """A set built as test_gpu_instances.random_set builds them, 2^13 of its world rays, and the answer composed from
    Scene.trace_all_hits(K = 64, counts) on the rays moved by the set's own W: per distinct scene, its instances' rays
    concatenated (a few instances a call, to bound the host arrays), then merged by the key.  Once per module."""
    if n not in _sets:
        names = SETS[n]
        pick, Mx = random_set(pkg, names, n, seed=n)
        s = pkg.tracer.InstanceSet([scene(pkg, p)[1] for p in pick], Mx)
        o, d, tmax = world_rays(pkg, pick, Mx, 1 << 13, seed=n + 1)
        W = s.world_to_object()
        rays_n = len(o)
        parts, total, most, pairs = [], np.zeros(rays_n, np.int64), 0, 0
        for name in sorted(set(pick)):
            ids = [i for i, p in enumerate(pick) if p == name]
            for at in range(0, len(ids), 16):
                chunk = ids[at:at + 16]
                moved = np.concatenate([pkg.tracer.make_rays(*I.object_rays(W[i], o, d), tmax) for i in chunk])
                hits, counts = scene(pkg, name)[1].trace_all_hits(moved, max_hits=64, counts=True)
                for j, i in enumerate(chunk):
                    parts.append(IM.held_members(hits[j * rays_n:(j + 1) * rays_n], i))
                    c = counts[j * rays_n:(j + 1) * rays_n]
                    total += c
                    most = max(most, int(c.max()))
                    pairs += int((c > 0).sum())
        members = tuple(np.concatenate(p) for p in zip(*parts))
        hits, inst = IM.first_k(*members, tmax, 64)
        _sets[n] = dict(pick=pick, set=s, o=o, d=d, tmax=tmax, rays=pkg.tracer.make_rays(o, d, tmax),
                        want=(hits, inst, total.astype(np.int32)), most=most, pairs=pairs)
    return _sets[n]


@pytest.fixture(scope="module", autouse=True)
def close_the_module_sets():
    yield
    for c in _sets.values():
        c["set"].close()
    _sets.clear()


@pytest.mark.parametrize("n", sorted(SETS))
def test_sets_equal_the_composition(pkg, gpu, n):
    c = composed(pkg, n)
    s, rays, want = c["set"], c["rays"], c["want"]
    assert c["most"] <= 64, "no instance crosses more than the composition's K on any ray: every ray is compared"
    assert (want[2] > 0).sum() > len(rays) // 10
    for k, with_counts in [(1, True), (8, True), (64, True), (1, False), (4, False), (8, False), (16, False)]:
        got = s.trace_all_hits(rays, max_hits=k, counts=with_counts)
        assert_same_answer(got, want, f"{n} instances, K {k}, counts {with_counts}", k)
    assert np.array_equal(s.crossing_counts(rays), want[2])
    # instance 2 is an exact duplicate of instance 0: its records follow instance 0's own at equal t
    hits, inst, counts = s.trace_all_hits(rays, max_hits=64)
    whole = np.nonzero((counts <= 64) & (inst == 0).any(1))[0]
    assert len(whole) >= 10          # (instance 0 is one of n: a few dozen of the 2^13 rays reach it)
    for r in whole:
        zero, two = np.nonzero(inst[r] == 0)[0], np.nonzero(inst[r] == 2)[0]
        assert len(zero) == len(two) and np.array_equal(hits[r][zero], hits[r][two]), r
        t = hits["t"][r]
        for a, b in zip(zero, two):
            assert a < b and (t[a:b + 1] == t[a]).all(), (r, a, b)
            if (t == t[a]).sum() == 2:      # no other tie at this t: the duplicate sits directly behind
                assert b == a + 1, (r, a, b)


# 4 ---------------------------------------------------------------------------------------------------------------------------
DEEP_KS = (1, 3, 8, 9, 16, 33, 64)
_deep = {}


def deep_set(pkg, tmp_path_factory):
    """eight copies of tall_stack 8 apart along z (the axial rays' direction) in an order that is not the spatial one, and two
    exact duplicates; the axial rays and some random ones"""
    if not _deep:
        world = pkg.World(M.write_mesh(pkg, str(tmp_path_factory.mktemp("instance_multihit") / "tall_stack.trisrc"), "tall_stack"))
        arrays, sc = R.SceneArrays(world.arrays()), pkg.Scene(world.flatten())
        offsets = [8.0 * z for z in (0, -3, 2, -1, 3, -4, 1, -2)] + [0.0, -32.0]      # instances 8 and 9 repeat 0 and 5
        Mx = np.tile(EYE, (10, 1, 1))
        Mx[:, 2, 3] = offsets
        n = 2500
        o, d, tmax = M.axial_rays(n, seed=16)
        ro, rd, rt = random_rays(arrays, n // 5, seed=17)
        o, d, tmax = np.concatenate([o, ro]), np.concatenate([d, rd]), np.concatenate([tmax, rt])
        _deep.update(world=world, arrays=arrays, scene=sc, set=pkg.tracer.InstanceSet([sc] * 10, Mx), o=o, d=d, tmax=tmax, n=n, want={})
    return _deep


@pytest.fixture(scope="module", autouse=True)
def close_the_deep_set():
    yield
    if _deep:
        _deep["set"].close()
        _deep["scene"].close()
        _deep["world"].close()
        _deep.clear()


@pytest.mark.parametrize("max_leaf_tests", [10, 16])
def test_eviction_and_pruning_across_instances(pkg, gpu, tmp_path_factory, max_leaf_tests):
    import torch
    c = deep_set(pkg, tmp_path_factory)
    s, o, d, tmax, n = c["set"], c["o"], c["d"], c["tmax"], c["n"]
    rays = pkg.tracer.make_rays(o, d, tmax)
    want = IM.all_hits([c["arrays"]] * 10, s.world_to_object(), o, d, tmax, max_hits=64, max_leaf_tests=max_leaf_tests)
    ties = (want[0]["t"][:, 1:] == want[0]["t"][:, :-1]) & (want[0]["triangle"][:, 1:] >= 0)
    across = ties & (want[1][:, 1:] != want[1][:, :-1])
    # equal t across the edge of K: a duplicate's record behind its original's (K = 1, 3, 9), three coincident squares (K = 8, 16)
    assert min(across[:, 0].sum(), across[:, 2].sum(), across[:, 8].sum(), ties[:, 7].sum(), ties[:, 15].sum()) > 20
    d_rays = dev(rays)
    for k in DEEP_KS:
        assert (want[2] > k).sum() > n // 4, (k, int((want[2] > k).sum()))                        # something to evict and to prune
        for with_counts in (True, False):
            what = f"tall_stack copies, leaf cap {max_leaf_tests}, K {k}, counts {with_counts}"
            got = s.trace_all_hits(rays, max_hits=k, counts=with_counts, max_leaf_tests=max_leaf_tests)
            assert_same_answer(got, want, what + ", host path", k)
            d_hits, d_inst, d_counts = s.trace_all_hits(d_rays, max_hits=k, counts=with_counts, max_leaf_tests=max_leaf_tests)
            torch.cuda.current_stream().synchronize()
            assert_same_answer((records(d_hits), d_inst.cpu().numpy(), d_counts.cpu().numpy() if with_counts else None), want,
                               what + ", device path", k)
    # without an instance buffer the records are the same (K > 8 keeps that half of its keys in scratch of its own)
    for k in (3, 16):
        d_hits = torch.full((len(rays), k, 4), -7, dtype=torch.int32, device="cuda")
        s.trace_all_hits_into(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), 0, 0, k, torch.cuda.current_stream().cuda_stream,
                              max_leaf_tests)
        torch.cuda.current_stream().synchronize()
        assert_same_records(records(d_hits), want[0][:, :k], f"no instance buffer, K {k}")
    one = s.trace_all_hits(rays, max_hits=1, counts=False, max_leaf_tests=max_leaf_tests)
    eight = s.trace_all_hits(rays, max_hits=8, counts=False, max_leaf_tests=max_leaf_tests)
    assert_same_records(one[0], eight[0][:, :1], "K = 1 against record 0 of K = 8")
    assert np.array_equal(one[1], eight[1][:, :1])


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_record_0_is_the_instanced_closest_hit(pkg, gpu):
    """InstanceSet.trace_rays without a cap against record 0 and its instance, on the 17-instance set.  Left out: rays whose two
    smallest keys have equal t within ONE instance, and rays with a NaN candidate in any instance (the restatement's flag); at
    most 1 % of the rays, which the restatement alone has to satisfy too.

    Equal t in two different instances is not left out.  The set holds an exact duplicate of instance 0, so every ray that
    reaches instance 0 first has its two smallest keys at equal t: 86 of these 4096 rays, 2.1 %, in the restatement alone, twice
    the cap.  Both queries decide such a tie by contract, for the lower instance, so record 0 must still be the closest hit; the
    only tie a closest-hit walk decides by its own visit order is between two triangles of one instance, and then record 1 is
    that instance's too (the instance sorts before the triangle).  The narrower rule compares more rays, under the same cap."""
    c = composed(pkg, 17)
    s, rays, o, d, tmax = c["set"], c["rays"][:4096], c["o"][:4096], c["d"][:4096], c["tmax"][:4096]
    ref_hits, ref_inst, ref_counts, _, nan_candidate, _ = IM.all_hits([scene(pkg, p)[0] for p in c["pick"]], s.world_to_object(), o, d,
                                                                      tmax, max_hits=2, details=True)
    ref_tie = (ref_counts >= 2) & (ref_hits["t"][:, 0] == ref_hits["t"][:, 1])
    ref_out = (ref_tie & (ref_inst[:, 0] == ref_inst[:, 1])) | nan_candidate
    print(f"the restatement: {int(ref_tie.sum())} of {len(rays)} rays with equal t in the two smallest keys, {int(ref_out.sum())} left out "
          f"({int(nan_candidate.sum())} for a NaN candidate)")
    assert ref_out.mean() <= 0.01, (int(ref_out.sum()), len(rays))
    closest, ci = s.trace_rays(rays, max_bvh_iterations=0)
    hits, inst, counts = s.trace_all_hits(rays, max_hits=2)
    left_out = ((counts >= 2) & (hits["t"][:, 0] == hits["t"][:, 1]) & (inst[:, 0] == inst[:, 1])) | nan_candidate
    print(f"{int(left_out.sum())} of {len(rays)} rays left out")
    assert left_out.mean() <= 0.01, (int(left_out.sum()), len(rays))
    keep = ~left_out
    assert np.array_equal((counts == 0)[keep], (closest["triangle"] == R.HIT_MISS)[keep])
    k = keep & (counts > 0)
    assert k.sum() > len(rays) // 20
    assert_same_records(hits[:, 0][k], closest[k], "record 0 against InstanceSet.trace_rays")
    assert np.array_equal(inst[:, 0][k], ci[k]) and np.all(ci[keep & (counts == 0)] == -1)
    across = k & (counts >= 2) & (hits["t"][:, 0] == hits["t"][:, 1])
    assert across.sum() > 20 and np.all(inst[:, 0][across] == 0) and np.all(inst[:, 1][across] == 2), "the duplicate's ties were compared"


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_refit_update_and_query_on_one_stream(pkg, gpu):
    """A device refit of a member, a device update with moved transforms and the query, enqueued on one side stream with no
    synchronisation between them, against the blocking path of a set created from the same final state."""
    import torch
    world, _, _ = loaded(pkg, "lobed_528")
    own = pkg.Scene(world.flatten())            # a scene of its own: it is refit below
    other = scene(pkg, "small_trisrc")[1]
    dw = pkg.tracer.DeviceWorld(scene_path_of("lobed_528"))
    pick, M0 = random_set(pkg, ["lobed_528", "small_trisrc", "lobed_528"], 9, seed=60)
    _, M1 = random_set(pkg, ["lobed_528", "small_trisrc", "lobed_528"], 9, seed=61)
    members = [other if p == "small_trisrc" else (own if i % 3 == 0 else dw) for i, p in enumerate(pick)]
    assert own in members and dw in members and other in members
    s = pkg.tracer.InstanceSet(members, M0)
    host = None
    try:
        o, d, tmax = world_rays(pkg, pick, M1, 1 << 12, seed=62)
        rays = pkg.tracer.make_rays(o, d, tmax)
        d_rays = dev(rays)
        corners = own.geometry()["vertex_positions"].reshape(-1, 3)
        d_moved = torch.from_numpy(np.ascontiguousarray(corners * F(1.4) + F(0.15))).cuda()
        d_maps = torch.from_numpy(M1).cuda()
        n = len(rays)
        out = {k: (torch.full((n, k, 4), -7, dtype=torch.int32, device="cuda"), torch.full((n, k), -7, dtype=torch.int32, device="cuda"))
               for k in (4, 16)}
        d_counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            own.refit(d_moved, stream_ptr=side.cuda_stream)
            s.update_into(d_maps.data_ptr(), side.cuda_stream)
            s.trace_all_hits_into(d_rays.data_ptr(), n, out[4][0].data_ptr(), out[4][1].data_ptr(), d_counts.data_ptr(), 4, side.cuda_stream)
            s.trace_all_hits_into(d_rays.data_ptr(), n, out[16][0].data_ptr(), out[16][1].data_ptr(), 0, 16, side.cuda_stream)
        side.synchronize()
        assert s.update_status() == -1
        host = pkg.tracer.InstanceSet(members, M1)      # created after the refit: the blocking path over the final state
        want = host.trace_all_hits(rays, max_hits=16)
        before = pkg.tracer.InstanceSet(members, M0)
        assert (before.trace_all_hits(rays, max_hits=1)[1] != want[1][:, :1]).sum() > 100, "the update moved something"
        before.close()
        assert (want[2] > 0).sum() > n // 10
        assert_same_answer((records(out[4][0]), out[4][1].cpu().numpy(), d_counts.cpu().numpy()), want, "one stream, K 4 with counts", 4)
        assert_same_answer((records(out[16][0]), out[16][1].cpu().numpy(), None), want, "one stream, K 16 without counts", 16)
    finally:
        s.close()
        if host is not None:
            host.close()
        own.close()
        dw.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_a_count_split_over_two_launches(pkg, gpu):
    """2^24 + 3000 rays made on the device (one launch holds 2^24), K = 1 without counts, on a one-instance set: equal on the
    device to Scene.trace_all_hits_into."""
    import torch
    arrays, sc = scene(pkg, "small_trisrc")
    s = pkg.tracer.InstanceSet([sc], EYE[None])
    try:
        n = (1 << 24) + 3000
        pts = arrays.positions.reshape(-1, 3)
        lo, hi = torch.tensor(pts.min(0), device="cuda"), torch.tensor(pts.max(0), device="cuda")
        g = torch.Generator(device="cuda").manual_seed(7)
        d_rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        d_rays[:, 0:3] = (lo + hi) / 2 + (torch.rand((n, 3), generator=g, device="cuda") * 2 - 1) * (hi - lo)
        d_rays[:, 3] = 1e7
        d_rays[:, 4:7] = torch.nn.functional.normalize(torch.randn((n, 3), generator=g, device="cuda"), dim=1)
        d_rays[:, 7] = 0
        stream = torch.cuda.current_stream().cuda_stream
        want = torch.full((n, 1, 4), -7, dtype=torch.int32, device="cuda")
        sc.trace_all_hits_into(d_rays.data_ptr(), n, want.data_ptr(), 0, 1, stream)
        got = torch.full((n, 1, 4), -9, dtype=torch.int32, device="cuda")
        got_inst = torch.full((n, 1), -9, dtype=torch.int32, device="cuda")
        s.trace_all_hits_into(d_rays.data_ptr(), n, got.data_ptr(), got_inst.data_ptr(), 0, 1, stream)
        torch.cuda.current_stream().synchronize()
        assert torch.equal(got, want)
        hit = want[:, 0, 3] >= 0
        assert int(hit.sum()) > n // 20 and int(hit[1 << 24:].sum()) > 100
        assert torch.equal(got_inst[:, 0], torch.where(hit, 0, -1).to(torch.int32))
    finally:
        s.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_device(pkg, gpu):
    import torch
    N = pkg._native
    lib = N.load_instance_multihit()
    sc = scene(pkg, "lobed_528")[1]
    chain = pkg.Scene(chain_scene(5).desc)        # no packed tree: refused when the set is created, so no query ever meets one
    with pytest.raises(N.ShrayError) as err:
        pkg.tracer.InstanceSet([sc, chain], np.concatenate([EYE[None], EYE[None]]))
    assert err.value.code == BAD_TREE
    chain.close()
    s = pkg.tracer.InstanceSet([sc], EYE[None])
    try:
        h = s._handle
        d_rays = torch.zeros((65, 8), dtype=torch.float32, device="cuda")
        d_rays[:, 6] = 1
        d_hits = torch.zeros((65 * 8 + 1, 4), dtype=torch.int32, device="cuda")
        d_inst = torch.zeros(65 * 8 + 2, dtype=torch.int32, device="cuda")
        d_counts = torch.zeros(66, dtype=torch.int32, device="cuda")
        rp, hp, ip, cp = d_rays.data_ptr(), d_hits.data_ptr(), d_inst.data_ptr(), d_counts.data_ptr()
        call, V = lib.shray_trace_instances_all_hits_device, C.c_void_p
        mp, none = pkg.tracer.multihit_params(8), pkg.tracer.multihit_params(0)
        assert call(h, C.byref(mp), V(rp + 4), 64, V(hp), V(ip), V(cp), None) == INVALID
        assert call(h, C.byref(mp), V(rp), 64, V(hp + 8), V(ip), V(cp), None) == INVALID
        assert call(h, C.byref(mp), V(rp), 64, V(hp), V(ip + 2), V(cp), None) == INVALID
        assert call(h, C.byref(mp), V(rp), 64, V(hp), V(ip), V(cp + 1), None) == INVALID
        assert call(h, C.byref(none), V(rp), 64, None, None, None, None) == INVALID
        assert call(h, C.byref(none), V(rp), 64, V(hp), V(ip), None, None) == INVALID
        assert call(h, C.byref(mp), V(rp), 64, None, V(ip), V(cp), None) == INVALID
        assert call(h, C.byref(mp), V(rp), 64, V(hp + 16), V(ip + 4), V(cp + 4), None) == 0      # 4-byte alignment is enough for these
        assert call(h, C.byref(none), V(rp), 64, None, None, V(cp), None) == 0
        assert call(h, C.byref(mp), V(rp), 0, V(hp), V(ip), V(cp), None) == 0
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            s.trace_all_hits(pkg.tracer.make_rays(np.zeros((2, 3), F), np.ones((2, 3), F)), max_hits=0, counts=False)
        for bad in (-1, 65):
            with pytest.raises(N.ShrayError):
                s.trace_all_hits(pkg.tracer.make_rays(np.zeros((2, 3), F), np.ones((2, 3), F)), max_hits=bad)
        hits, inst, counts = s.trace_all_hits(pkg.tracer.make_rays(np.zeros((0, 3), F), np.ones((0, 3), F)), max_hits=5)
        assert hits.shape == (0, 5) and inst.shape == (0, 5) and counts.shape == (0,)
    finally:
        s.close()


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_counters_of_a_multi_instance_set(pkg, gpu):
    c = composed(pkg, 17)
    s, rays = c["set"], c["rays"]
    plain = s.trace_all_hits(rays, max_hits=8)
    hits, inst, counts, counters = s.trace_all_hits(rays, max_hits=8, counters=True)
    assert_same_answer((hits, inst, counts), plain, "the counting form against the plain one", 8)
    assert_same_answer(plain, c["want"], "the plain form against the composition", 8)
    assert c["pairs"] <= counters["traversals"] <= len(rays) * s.count, (c["pairs"], counters)
    assert counters["samples"] == len(rays) and counters["bad_hits"] == 0
    assert counters["node_visits"] >= counters["traversals"] and counters["triangle_tests"] >= int(counts.sum()) > 0
