"""All-hits ray queries on the GPU (include/shader_ray_multihit.h) against the restatement (tests/multi_hit_ref.py): every
byte of every hit record and every count, for K in {0, 1, 2, 3, 4, 5, 8, 9, 64} with and without counts (the walk that skips what cannot
reach the first K against the walk that skips nothing), on the test scenes and the reference test's small meshes with the
ray query's random rays; the host and device paths, DeviceWorld, a count split over two launches, the counters, a device
refit followed by the query on the same stream, the refusal of a scene without a packed tree, trace_rays' closest hit
against record 0, and a mesh with more crossings per ray than any K holds, where eviction and pruning bite."""
import numpy as np
import pytest

import multi_hit_ref as M
import ray_query_ref as R
import refit_ref
from test_gpu_point_query import BAD_TREE, loaded, scene_path
from test_gpu_ray_query import random_rays
from test_gpu_signed_distance import moved_lobed
from test_oracle_kat import chain_scene

pytestmark = pytest.mark.gpu

F = np.float32
KS = (0, 1, 2, 3, 4, 5, 8, 9, 64)
SCENES = [("small_trisrc", 30000), ("lobed_528", 30000), ("bunny", 30000), ("quads_mixed", 30000)] + [(m, 20000) for m in M.MESHES]
_small = {}
_refs = {}


def scene_of(pkg, tmp_path_factory, name):
    """(restatement's arrays, resident scene) of a test scene or of one of the reference test's meshes"""
    if name in M.MESHES + M.DEEP_MESHES:
        if name not in _small:
            world = pkg.World(M.write_mesh(pkg, str(tmp_path_factory.mktemp("multihit") / f"{name}.trisrc"), name))
            _small[name] = (world, R.SceneArrays(world.arrays()), pkg.Scene(world.flatten()))
        return _small[name][1], _small[name][2]
    arrays, scene = loaded(pkg, name)
    return R.SceneArrays(arrays), scene


@pytest.fixture(scope="module", autouse=True)
def close_the_module_scenes():
    """the small meshes' worlds and resident scenes are this module's own: closed when its last test has run"""
    yield
    for world, _, scene in _small.values():
        scene.close()
        world.close()
    _small.clear()
    _refs.clear()


def reference(pkg, tmp_path_factory, name, n):
    """the rays and the restatement's answer for K = 64 (the first K of it is the answer for any smaller K)"""
    if name not in _refs:
        arrays, _ = scene_of(pkg, tmp_path_factory, name)
        o, d, tmax = random_rays(arrays, n, seed=41 + len(name))
        hits, counts, counters, nan_candidate = M.all_hits(arrays, o, d, tmax, max_hits=64, details=True)
        _refs[name] = (pkg.tracer.make_rays(o, d, tmax), hits, counts, counters, nan_candidate)
    return _refs[name]


def assert_same_records(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).any(1))[0]
    assert not len(bad), f"{what}: {len(bad)} of {len(got)} rays differ; first: " + "; ".join(
        f"#{i} got {got[i]} want {want[i]}" for i in bad[:3])


def dev(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(F).reshape(-1, 8).copy()).cuda()


def records(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(R.HIT_DTYPE).reshape(t.shape[0], t.shape[1])


@pytest.mark.parametrize("name, n", SCENES)
def test_every_record_and_count_equals_the_restatement(pkg, gpu, tmp_path_factory, name, n):
    import torch
    _, scene = scene_of(pkg, tmp_path_factory, name)
    rays, want, want_counts, _, _ = reference(pkg, tmp_path_factory, name, n)
    assert (want_counts > 0).sum() > n // 20 and (want_counts == 0).sum() > n // 20 and (want_counts > 1).sum() > n // 100
    d_rays = dev(rays)
    for k in KS:
        for with_counts in (True, False):
            if k == 0 and not with_counts:
                continue
            what = f"{name}, K {k}, counts {with_counts}"
            hits, counts = scene.trace_all_hits(rays, max_hits=k, counts=with_counts)
            d_hits, d_counts = scene.trace_all_hits(d_rays, max_hits=k, counts=with_counts)
            torch.cuda.current_stream().synchronize()
            if k:
                assert_same_records(hits, want[:, :k], what + ", host path")
                assert_same_records(records(d_hits), want[:, :k], what + ", device path")
            else:
                assert hits is None and d_hits is None
            if with_counts:
                assert np.array_equal(counts, want_counts), what
                assert np.array_equal(d_counts.cpu().numpy(), want_counts), what + ", device path"
            else:
                assert counts is None and d_counts is None
    assert np.array_equal(scene.crossing_counts(rays), want_counts)


DEEP_KS = (1, 3, 8, 9, 16, 33, 64)


@pytest.mark.parametrize("max_leaf_tests", [10, 16])
def test_more_crossings_than_any_k(pkg, gpu, tmp_path_factory, max_leaf_tests):
    """tall_stack (104 triangles on an axial ray, ties of three at equal t): most rays cross more surfaces than K holds, so
    every insertion form evicts and the pruned forms skip nodes.  Every byte against the restatement for K in DEEP_KS with and
    without counts, host and device paths, and the counters; with the default leaf cap (the builder leaves up to 16 triangles
    in a leaf here) and with a cap that tests them all."""
    import torch
    arrays, scene = scene_of(pkg, tmp_path_factory, "tall_stack")
    n = 20000
    o, d, tmax = M.axial_rays(n, seed=6)
    ro, rd, rt = random_rays(arrays, n // 4, seed=7)
    o, d, tmax = np.concatenate([o, ro]), np.concatenate([d, rd]), np.concatenate([tmax, rt])
    rays = pkg.tracer.make_rays(o, d, tmax)
    want, want_counts, want_counters = M.all_hits(arrays, o, d, tmax, max_hits=64, max_leaf_tests=max_leaf_tests)
    assert want_counts.max() > 64 and (want_counts == 0).sum() > 100
    ties = (want["t"][:, 1:] == want["t"][:, :-1]) & (want["triangle"][:, 1:] >= 0)
    assert ties.sum() > 1000 and ties[:, 7].sum() > 100 and ties[:, 15].sum() > 100   # equal t across the edge of K = 8 and 16
    d_rays = dev(rays)
    for k in DEEP_KS:
        assert (want_counts > k).sum() > n // 4, (k, int((want_counts > k).sum()))      # something to evict and to prune
        for with_counts in (True, False):
            what = f"tall_stack, leaf cap {max_leaf_tests}, K {k}, counts {with_counts}"
            hits, counts = scene.trace_all_hits(rays, max_hits=k, counts=with_counts, max_leaf_tests=max_leaf_tests)
            d_hits, d_counts = scene.trace_all_hits(d_rays, max_hits=k, counts=with_counts, max_leaf_tests=max_leaf_tests)
            torch.cuda.current_stream().synchronize()
            assert_same_records(hits, want[:, :k], what + ", host path")
            assert_same_records(records(d_hits), want[:, :k], what + ", device path")
            if with_counts:
                assert np.array_equal(counts, want_counts) and np.array_equal(d_counts.cpu().numpy(), want_counts), what
        hits, counts, counters = scene.trace_all_hits(rays, max_hits=k, max_leaf_tests=max_leaf_tests, counters=True)
        assert_same_records(hits, want[:, :k], f"tall_stack, counting instance, K {k}")
        assert np.array_equal(counts, want_counts)
        for key in R.COUNTER_NAMES:
            assert counters[key] == want_counters[key], (k, key, counters, want_counters)


@pytest.mark.parametrize("name", ["lobed_528", "bunny"])
def test_k1_without_counts_is_the_first_record_of_k8(pkg, gpu, tmp_path_factory, name):
    _, scene = scene_of(pkg, tmp_path_factory, name)
    rays = reference(pkg, tmp_path_factory, name, 30000)[0]
    one, _ = scene.trace_all_hits(rays, max_hits=1, counts=False)
    eight, _ = scene.trace_all_hits(rays, max_hits=8, counts=False)
    assert_same_records(one, eight[:, :1], name)


@pytest.mark.parametrize("name", ["lobed_528", "bunny", "stack_of_squares"])
def test_counters_equal_the_restatement(pkg, gpu, tmp_path_factory, name):
    _, scene = scene_of(pkg, tmp_path_factory, name)
    rays, want, want_counts, want_counters, _ = reference(pkg, tmp_path_factory, name, 30000 if name not in M.MESHES else 20000)
    for k in (0, 3, 64):
        hits, counts, counters = scene.trace_all_hits(rays, max_hits=k, counters=True)
        if k:
            assert_same_records(hits, want[:, :k], f"{name}, counting instance, K {k}")
        assert np.array_equal(counts, want_counts)
        for key in R.COUNTER_NAMES:
            assert counters[key] == want_counters[key], (k, key, counters, want_counters)
        assert counters["samples"] == len(rays) and counters["bad_hits"] == 0


def test_max_leaf_tests_is_honoured(pkg, gpu, tmp_path_factory):
    arrays, scene = scene_of(pkg, tmp_path_factory, "lobed_528")
    rays = reference(pkg, tmp_path_factory, "lobed_528", 30000)[0][:8000]
    want, want_counts, _ = M.all_hits(arrays, rays["origin"], rays["direction"], rays["tmax"], max_hits=8, max_leaf_tests=1)
    for with_counts in (True, False):
        hits, counts = scene.trace_all_hits(rays, max_hits=8, counts=with_counts, max_leaf_tests=1)
        assert_same_records(hits, want, f"one test per leaf, counts {with_counts}")
    assert (want_counts != reference(pkg, tmp_path_factory, "lobed_528", 30000)[2][:8000]).any()


def test_device_world_matches_the_restatement(pkg, gpu, tmp_path_factory):
    import torch
    rays, want, want_counts, _, _ = reference(pkg, tmp_path_factory, "lobed_528", 30000)
    dw = pkg.tracer.DeviceWorld(scene_path("lobed_528"))
    try:
        hits, counts = dw.trace_all_hits(rays, max_hits=8)
        assert_same_records(hits, want[:, :8], "DeviceWorld, host path")
        assert np.array_equal(counts, want_counts) and np.array_equal(dw.crossing_counts(rays), want_counts)
        d_rays = dev(rays)
        d_hits = torch.full((len(rays), 3, 4), -7, dtype=torch.int32, device="cuda")
        d_counts = torch.full((len(rays),), -7, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        dw.trace_all_hits_into(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), d_counts.data_ptr(), 3, stream)
        torch.cuda.current_stream().synchronize()
        assert_same_records(records(d_hits), want[:, :3], "DeviceWorld, device path")
        assert np.array_equal(d_counts.cpu().numpy(), want_counts)
        d_hits.fill_(-7)
        dw.trace_all_hits_into(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), 0, 3, stream)
        torch.cuda.current_stream().synchronize()
        assert_same_records(records(d_hits), want[:, :3], "DeviceWorld, device path without counts")
    finally:
        dw.close()


@pytest.mark.parametrize("with_counts", [True, False])
def test_a_count_split_over_two_launches(pkg, gpu, tmp_path_factory, with_counts):
    """2^24 + 3000 rays (one launch holds 2^24): rays that start far away and point away fill the buffer; the last launch's
    rays and real rays scattered over the first launch are restated."""
    import torch
    arrays, scene = scene_of(pkg, tmp_path_factory, "small_trisrc")
    n, k = (1 << 24) + 3000, 2
    o, d, tmax = random_rays(arrays, 3000 + 4096, seed=77)
    real = pkg.tracer.make_rays(o, d, tmax)
    want, want_counts, _ = M.all_hits(arrays, o, d, tmax, max_hits=k)
    far = pkg.tracer.make_rays([[1e5, 2e5, -3e5]], [[1.0, 0.0, 0.0]], 55.0)
    d_rays = dev(far).repeat(n, 1)
    d_rays[n - 3000:] = dev(real[:3000])
    sample = torch.from_numpy(np.random.default_rng(2).choice(n - 3000, 4096, replace=False)).cuda()
    d_rays[sample] = dev(real[3000:])
    d_hits = torch.full((n, k, 4), -7, dtype=torch.int32, device="cuda")
    d_counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    scene.trace_all_hits_into(d_rays.data_ptr(), n, d_hits.data_ptr(), d_counts.data_ptr() if with_counts else 0, k,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    assert_same_records(records(d_hits[n - 3000:]), want[:3000], "the last rays")
    assert_same_records(records(d_hits[sample]), want[3000:], "rays of the first launch")
    rest = torch.ones(n - 3000, dtype=torch.bool, device="cuda")
    rest[sample] = False
    miss = torch.tensor(np.array([(55.0, 0.0, 0.0, -1)], R.HIT_DTYPE).view(np.int32), device="cuda")
    assert bool((d_hits[: n - 3000][rest] == miss).all())
    if with_counts:
        assert np.array_equal(d_counts[n - 3000:].cpu().numpy(), want_counts[:3000])
        assert np.array_equal(d_counts[sample].cpu().numpy(), want_counts[3000:])
        assert bool((d_counts[: n - 3000][rest] == 0).all())
    else:
        assert bool((d_counts == -7).all())


def test_device_refit_then_query_on_the_same_stream(pkg, gpu):
    """A device refit and the query enqueued on one side stream with no synchronisation between them: the query sees the
    moved vertices and the refit boxes (restated from the refit's own restatement)."""
    import torch
    world = pkg.World(scene_path("lobed_528"))
    scene = pkg.Scene(world.flatten())
    try:
        arrays = dict(world.arrays())
        pos = moved_lobed(np.asarray(arrays["vertex_positions"], F).reshape(-1, 3))
        tree = refit_ref.TreeArrays.of(world.export_tree())
        arrays["vertex_positions"] = pos.reshape(-1)
        arrays["group_boxmin"], arrays["group_boxmax"] = refit_ref.flat_boxes(tree, refit_ref.node_boxes(tree, pos))
        moved = R.SceneArrays(arrays)
        o, d, tmax = random_rays(moved, 20000, seed=8)
        rays = pkg.tracer.make_rays(o, d, tmax)
        before, _ = scene.trace_all_hits(rays, max_hits=4)
        want, want_counts, _ = M.all_hits(moved, o, d, tmax, max_hits=4)
        d_rays, d_pos = dev(rays), torch.from_numpy(pos).cuda()
        d_hits = torch.full((len(rays), 4, 4), -7, dtype=torch.int32, device="cuda")
        d_pruned = torch.full((len(rays), 4, 4), -7, dtype=torch.int32, device="cuda")
        d_counts = torch.full((len(rays),), -7, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            scene.refit(d_pos, stream_ptr=side.cuda_stream)
            scene.trace_all_hits_into(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), d_counts.data_ptr(), 4, side.cuda_stream)
            scene.trace_all_hits_into(d_rays.data_ptr(), len(rays), d_pruned.data_ptr(), 0, 4, side.cuda_stream)
        side.synchronize()
        assert_same_records(records(d_hits), want, "after the device refit")
        assert_same_records(records(d_pruned), want, "after the device refit, without counts")
        assert np.array_equal(d_counts.cpu().numpy(), want_counts)
        assert (before["triangle"] != want["triangle"]).any(1).sum() > 1000
    finally:
        scene.close()
        world.close()


def test_refusals_and_no_ops(pkg, gpu, tmp_path_factory):
    """A scene without a packed tree (a hand-made chain) is refused with SHRAY_ERR_BAD_TREE; count 0 is a no-op."""
    hand = chain_scene(5)
    scene = pkg.Scene(hand.desc)
    rays = pkg.tracer.make_rays(np.zeros((4, 3), F), np.ones((4, 3), F))
    try:
        for call in (lambda: scene.trace_all_hits(rays), lambda: scene.trace_all_hits(rays, counts=False), lambda: scene.crossing_counts(rays),
                     lambda: scene.trace_all_hits(rays, max_hits=64, counters=True)):
            with pytest.raises(pkg._native.ShrayError) as err:
                call()
            assert err.value.code == BAD_TREE
    finally:
        scene.close()
    _, good = scene_of(pkg, tmp_path_factory, "lobed_528")
    hits, counts = good.trace_all_hits(rays[:0], max_hits=5)
    assert hits.shape == (0, 5) and counts.shape == (0,)
    for bad in (-1, 65):
        with pytest.raises(pkg._native.ShrayError):
            good.trace_all_hits(rays, max_hits=bad)


@pytest.mark.parametrize("name", ["small_trisrc", "lobed_528", "bunny"])
def test_trace_rays_closest_hit_is_record_0(pkg, gpu, tmp_path_factory, name):
    """trace_rays (kernel id 0, no iteration cap) against the all-hits query on the GPU: count == 0 iff a miss, else record
    0 is its record bit for bit.  Left out, as in tests/test_multi_hit_reference.py: rays whose first two records have equal
    t and rays that met a NaN candidate (the restatement's flag); at most 1 % of a scene's rays."""
    _, scene = scene_of(pkg, tmp_path_factory, name)
    rays, _, _, _, nan_candidate = reference(pkg, tmp_path_factory, name, 30000)
    scene.set_kernel(0)
    closest = scene.trace_rays(rays, max_bvh_iterations=0)
    hits, counts = scene.trace_all_hits(rays, max_hits=2)
    left_out = ((counts >= 2) & (hits["t"][:, 0] == hits["t"][:, 1])) | nan_candidate
    print(f"{name}: {int(left_out.sum())} of {len(rays)} rays left out")
    assert left_out.mean() <= 0.01, (name, int(left_out.sum()), len(rays))
    keep = ~left_out
    assert np.array_equal((counts == 0)[keep], (closest["triangle"] == R.HIT_MISS)[keep])
    k = keep & (counts > 0)
    assert k.sum() > len(rays) // 20
    assert_same_records(hits[:, 0][k], closest[k], f"{name}, record 0 against trace_rays")
