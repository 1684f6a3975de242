"""Caller-supplied rays at the edges of exact_div.h's operand ranges, on the GPU, bit for bit against the restatements (which
divide): the cases of tests/ray_scale_cases.py through trace_rays (kernels 0 and 1, closest and any hit, counters), through
trace_all_hits (K 1 and 8, with counts: the walk that skips nothing and its counters; without: the pruned walk), a refit that
flips the scene's flag under a caller's rays on one stream, and instances whose maps push the object-space ray across an edge
while the world-space ray is ordinary.  tests/test_ray_scale_reference.py pins the cases themselves."""
import numpy as np
import pytest

import instance_ref as I
import multi_hit_ref as M
import ray_query_ref as R
import ray_scale_cases as X
from test_gpu_instances import mismatches, same_t_other_triangle
from test_gpu_multi_hit import assert_same_records, dev, records
from test_gpu_ray_query import assert_same_hits, own_test

pytestmark = pytest.mark.gpu

F = np.float32
CASES = [(name, s) for name in X.SCENES for s in X.S_EXPONENTS]
_scenes = {}


def one_nan(h):
    """the records with every NaN of t, u, v replaced by one NaN: where float32 products overflow (S >= 2^59: inf - inf, 0 * inf)
    both sides report NaN, and which NaN (its sign and payload) is numpy's and the hardware's own business, not the contract's"""
    h = np.array(h, copy=True)
    for f in ("t", "u", "v"):
        h[f][np.isnan(h[f])] = np.nan
    return h


def same_hits(got, want, what):
    assert_same_hits(one_nan(got), one_nan(want), what)


def same_records(got, want, what):
    assert_same_records(one_nan(np.ascontiguousarray(got)), one_nan(np.ascontiguousarray(want)), what)


def resident(pkg, name, s_exp, client):
    """the scaled scene on the device, once per module and client: trace_rays' scene is refit to its own corners to read the
    flag (the library has no other getter); the all-hits scene is never refit, so that client runs on the flag that
    shray_scene_create derived"""
    key = (name, s_exp, client)
    if key not in _scenes:
        world = X.load_scaled(pkg, name, s_exp)
        _scenes[key] = (world, pkg.Scene(world.flatten()))
    return _scenes[key][1]


@pytest.fixture(scope="module", autouse=True)
def close_the_module_scenes():
    yield
    for world, scene in _scenes.values():
        scene.close()
        world.close()
    _scenes.clear()


@pytest.mark.parametrize("name, s_exp", CASES)
def test_trace_rays_equals_the_restatement(pkg, gpu, name, s_exp):
    c = X.case(pkg, name, s_exp)
    want, want_counts = X.closest(pkg, name, s_exp)
    scene = resident(pkg, name, s_exp, "closest")
    rays = pkg.tracer.make_rays(c.o, c.d, c.tmax)
    for kernel in (0, 1):
        scene.set_kernel(kernel)
        what = f"{name}, S 2^{s_exp}, kernel {kernel}"
        same_hits(scene.trace_rays(rays), want, what)
        counted, counters = scene.trace_rays(rays, counters=True)
        same_hits(counted, want, what + ", counting instance")
        for k in R.COUNTER_NAMES:
            assert counters[k] == want_counts[k], (what, k, counters, want_counts)
        # the any-hit contract (tests/test_gpu_ray_query.py: test_any_hit_contract)
        anyh = scene.trace_rays(rays, any_hit=True)
        cap = want["triangle"] == R.HIT_CAP        # (a capped closest-hit walk: the any-hit walk may have ended at a hit before)
        assert np.array_equal((anyh["triangle"] == R.HIT_MISS)[~cap], (want["triangle"] == R.HIT_MISS)[~cap]), what
        k = np.nonzero(anyh["triangle"] >= 0)[0]
        assert (anyh["t"][k] < c.tmax[k]).all()
        t, u, v = own_test(c.arrays, c.o[k], c.d[k], anyh["triangle"][k])
        for field, mine in (("t", t), ("u", u), ("v", v)):
            assert np.array_equal(anyh[field][k], mine.astype(F), equal_nan=True), (what, field)
            finite = np.isfinite(mine)
            assert np.array_equal(anyh[field][k][finite].view(np.uint32), mine.astype(F)[finite].view(np.uint32)), (what, field)
    # the flag the scene reports: a refit to its own corners rewrites it by the same rule; the table states it
    corners = scene.geometry()["vertex_positions"].reshape(-1, 3)
    assert scene.refit(np.ascontiguousarray(corners))["exact_div_ok"] == X.expected_flag(name, s_exp)
    scene.set_kernel(0)
    same_hits(scene.trace_rays(rays), want, f"{name}, S 2^{s_exp}, after the refit to its own corners")


@pytest.mark.parametrize("name, s_exp", CASES)
def test_trace_all_hits_equals_the_restatement(pkg, gpu, name, s_exp):
    import torch
    c = X.case(pkg, name, s_exp)
    want, want_counts, want_counters = X.all_hits(pkg, name, s_exp)
    scene = resident(pkg, name, s_exp, "all hits")
    rays = pkg.tracer.make_rays(c.o, c.d, c.tmax)
    d_rays = dev(rays)
    for k in (1, 8):
        for with_counts in (True, False):
            what = f"{name}, S 2^{s_exp}, K {k}, counts {with_counts}"
            hits, counts = scene.trace_all_hits(rays, max_hits=k, counts=with_counts)
            d_hits, d_counts = scene.trace_all_hits(d_rays, max_hits=k, counts=with_counts)
            torch.cuda.current_stream().synchronize()
            same_records(hits, want[:, :k], what + ", host path")
            same_records(records(d_hits), want[:, :k], what + ", device path")
            if with_counts:
                assert np.array_equal(counts, want_counts) and np.array_equal(d_counts.cpu().numpy(), want_counts), what
        hits, counts, counters = scene.trace_all_hits(rays, max_hits=k, counters=True)
        same_records(hits, want[:, :k], f"{name}, S 2^{s_exp}, counting instance, K {k}")
        assert np.array_equal(counts, want_counts)
        for key in R.COUNTER_NAMES:
            assert counters[key] == want_counters[key], (name, s_exp, k, key, counters, want_counters)


def test_a_refit_flips_the_flag_under_a_callers_rays(pkg, gpu):
    """One vertex of one triangle goes to 2^60 on the device and comes back; the queries follow each refit on the same stream
    with no host synchronisation in between.  exact_div_ok reads 1, 0, 1; each answer is the restatement's on the moved arrays
    (boxes restated by tests/refit_ref.py); the third equals the first byte for byte.  Then a scene whose flag decides answers:
    every x at 2^100 (see there)."""
    import torch
    import refit_ref
    name = "lobed_528"
    world = X.load_scaled(pkg, name, 0)
    scene = pkg.Scene(world.flatten())
    try:
        arrays = dict(world.arrays())
        tree = refit_ref.TreeArrays.of(world.export_tree())
        pos = np.asarray(arrays["vertex_positions"], F).reshape(-1, 3).copy()
        moved = pos.copy()
        moved[3 * 100 + 1, 0] = F(2.0 ** 60)

        def restated(p):
            a = dict(arrays)
            a["vertex_positions"] = p.reshape(-1)
            boxes = refit_ref.node_boxes(tree, p.reshape(-1, 3, 3))
            a["group_boxmin"], a["group_boxmax"] = refit_ref.flat_boxes(tree, boxes)
            return R.SceneArrays(a), int(refit_ref.exact_div_ok(boxes))

        c = X.case(pkg, name, 0)
        rays = pkg.tracer.make_rays(c.o, c.d, c.tmax)
        d_rays = dev(rays)
        n = len(rays)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        answers, flags, wanted = [], [], []
        with torch.cuda.stream(side):
            for step, p in enumerate((pos, moved, pos)):
                d_pos = torch.from_numpy(p).cuda()
                d_closest = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
                d_all = torch.full((n, 8, 4), -7, dtype=torch.int32, device="cuda")
                d_counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
                d_pruned = torch.full((n, 8, 4), -7, dtype=torch.int32, device="cuda")
                flags.append(scene.refit(d_pos, stream_ptr=side.cuda_stream)["exact_div_ok"])
                scene.trace_rays_into(d_rays.data_ptr(), n, d_closest.data_ptr(), side.cuda_stream)
                scene.trace_all_hits_into(d_rays.data_ptr(), n, d_all.data_ptr(), d_counts.data_ptr(), 8, side.cuda_stream)
                scene.trace_all_hits_into(d_rays.data_ptr(), n, d_pruned.data_ptr(), 0, 8, side.cuda_stream)
                answers.append((d_closest, d_all, d_counts, d_pruned, d_pos))
        side.synchronize()
        assert flags == [1, 0, 1]
        for step, p in enumerate((pos, moved, pos)):
            sa, flag = restated(p)
            assert flag == flags[step]
            want, _ = R.trace(sa, c.o, c.d, c.tmax)
            want_all, want_counts, _ = M.all_hits(sa, c.o, c.d, c.tmax, max_hits=8)
            d_closest, d_all, d_counts, d_pruned, _ = answers[step]
            got = np.ascontiguousarray(d_closest.cpu().numpy()).view(R.HIT_DTYPE).reshape(-1)
            same_hits(got, want, f"step {step}, flag {flag}")
            same_records(records(d_all), want_all, f"step {step}, all hits")
            same_records(records(d_pruned), want_all, f"step {step}, all hits without counts")
            assert np.array_equal(d_counts.cpu().numpy(), want_counts)
            wanted.append(want)
        for a, b in zip(answers[0][:4], answers[2][:4]):
            assert torch.equal(a, b)
        assert (wanted[0]["triangle"] != wanted[1]["triangle"]).any()     # the moved vertex is seen
        fast = R.fast_division(1, c.o, c.d)
        assert fast.sum() > 1000 and (~fast).sum() > 1000                 # rays that change class with the flag, and rays that do not
        # A flag the walk's answers depend on.  div_by_constant4 equals the division far beyond exact_div.h's ranges (replayed
        # with fmaf: no mismatch for divisors of 2^-60 .. 2^33 and dividends up to 2^62), so the 2^60 above can change no record
        # whichever form is taken.  With every x at 2^100 it does: a ray with an in-range origin and 0 < d.x < 2^-28 has the
        # entry quotient 2^100 / d.x = +inf and misses the root; the four operations make inf, then inf - inf = NaN of it,
        # which the walk's max() passes over, so a ray "fast" despite the flag would enter the root by its y and z alone.
        flat = pos.copy()
        flat[:, 0] = F(2.0 ** 100)
        assert scene.refit(flat)["exact_div_ok"] == 0
        sa, flag = restated(flat)
        assert flag == 0
        k = np.nonzero(fast & (np.abs(c.d[:, 0]) < F(2.0 ** -28)))[0]
        want_all, want_counts, want_counters = M.all_hits(sa, c.o[k], c.d[k], c.tmax[k], max_hits=8)
        traced = int((c.tmax[k] > 0).sum())
        assert traced > 200 and want_counters["node_visits"] == traced and (want_counts == 0).all()   # every one of them misses the root
        yz, _, loose = M.all_hits(restated(pos)[0], c.o[k], c.d[k], c.tmax[k], max_hits=8)
        assert loose["node_visits"] > 3 * traced                            # and would walk on by y and z
        hits, counts, counters = scene.trace_all_hits(rays[k], max_hits=8, counters=True)
        same_records(hits, want_all, "every x at 2^100")
        assert np.array_equal(counts, want_counts)
        for key in R.COUNTER_NAMES:
            assert counters[key] == want_counters[key], (key, counters, want_counters)
        want, want_c = R.trace(sa, c.o, c.d, c.tmax)
        for kernel in (0, 1):
            scene.set_kernel(kernel)
            got, counters = scene.trace_rays(rays, counters=True)
            same_hits(got, want, f"every x at 2^100, kernel {kernel}")
            for key in R.COUNTER_NAMES:
                assert counters[key] == want_c[key], (kernel, key, counters, want_c)
    finally:
        scene.close()
        world.close()


# object-to-world maps: one axis scaled by 2^e among identity and rigid members.  W scales that axis by 2^-e, so an ordinary
# world-space direction component u becomes u * 2^-e in object space: below 2^-40 for e = 41 and 45 (and for e = 21 when
# |u| < 2^-19), at or above 2^20 for e = -21, -41, -45 when |u| >= 2^-1, 2^-21, 2^-25.  The origin's component moves with it.
SCALE_EXPONENTS = (21, -21, 41, -41, 45, -45)


def instance_maps():
    maps = [np.eye(3, 4), [[1, 0, 0, 0.75], [0, 1, 0, -2.0], [0, 0, 1, 0.5]], [[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 3.0]],
            [[-1, 0, 0, 0.25], [0, 1, 0, 0], [0, 0, -1, 3.0]]]
    for j, e in enumerate(SCALE_EXPONENTS):
        m = np.eye(3, 4)
        m[j % 3, j % 3] = 2.0 ** e
        m[:, 3] = [(-1.5, 2.0, 0.5), (2.5, -0.5, -2.0), (0.5, 0.5, 2.5)][j % 3] if j < 3 else [(-2.5, -2.0, 0.0), (0.0, 2.5, 2.0), (2.0, -2.5, -1.0)][j % 3]
        maps.append(m)
    return np.array([np.asarray(m, np.float64) for m in maps]).astype(F)


def test_instances_whose_maps_cross_an_edge(pkg, gpu):
    """Ordinary world-space rays (unit directions, origins O(1)) through lobed_528 placed by instance_maps(): the gate is taken
    again for the object-space ray of every instance a ray enters, and within one ray's walk some instances divide and others
    do not.  Hits and instances equal instance_ref's composition of the restatement over the set's own W; the one admissible
    disagreement is tests/test_gpu_instances.py's (another triangle of the same instance at the same t)."""
    import torch
    world = X.load_scaled(pkg, "lobed_528", 0)
    scene = pkg.Scene(world.flatten())
    scene.set_kernel(0)
    s = None
    try:
        arrays = R.SceneArrays(world.arrays())
        maps = instance_maps()
        s = pkg.tracer.InstanceSet([scene] * len(maps), maps)
        W = s.world_to_object()
        # world rays: towards points of the instances' world-space meshes, from origins about them
        rng = np.random.default_rng(77)
        n = 4096
        pts = arrays.positions.reshape(-1, 3).astype(np.float64)
        which = rng.integers(0, len(maps), n)
        A, b = maps[:, :, :3].astype(np.float64), maps[:, :, 3].astype(np.float64)
        target = np.einsum("nij,nj->ni", A[which], pts[rng.integers(0, len(pts), n)]) + b[which]
        squash = np.abs(target) > 1e3                    # a mesh stretched by 2^21 and more: aim at its part near the origin
        target[squash] = rng.uniform(-3, 3, int(squash.sum()))
        o = rng.uniform(-4, 4, (n, 3))
        d = target - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        o, d = o.astype(F), d.astype(F)
        tmax = np.full(n, F(1e7))
        tmax[rng.random(n) < 0.1] = np.inf
        flag = 1
        per, fast = [], []
        for w in W:
            po, pd = I.object_rays(w, o, d)
            per.append(R.trace(arrays, po, pd, tmax, max_bvh_iterations=0)[0])
            fast.append(R.fast_division(flag, po, pd))
        want, wi = I.compose(per, tmax)
        fast = np.array(fast)
        # vacuity: best hits from "divide" instances and from "fast" ones, rays that meet both classes, every scaled map hit
        hit = np.nonzero(wi >= 0)[0]
        best_fast = fast[wi[hit], hit]
        assert best_fast.sum() >= n // 20 and (~best_fast).sum() >= n // 20, (int(best_fast.sum()), int((~best_fast).sum()))
        assert (fast.any(0) & (~fast).any(0)).sum() > n // 2
        for i, e in enumerate(SCALE_EXPONENTS, start=4):
            # 2^21: |u| 2^-21 leaves the range only below |u| = 2^-19, so nearly every ray stays "fast"; 2^-21: about half the
            # rays (|u| >= 1/2); the others: every ray divides.  Behind 2^-41 and 2^-45 the object-space origin is 2^40 and more
            # mesh sizes away, where float32 cannot resolve the mesh: no best hit comes from there, the walks are still made.
            if e == 21:
                assert fast[i].sum() >= n // 2
            else:
                assert (~fast[i]).sum() >= n // 4 and (abs(e) == 21 or (~fast[i]).all()), (e, int((~fast[i]).sum()))
            if e not in (-41, -45):
                assert (wi == i).sum() >= 100, (e, int((wi == i).sum()))
        rays = pkg.tracer.make_rays(o, d, tmax)

        def check(what):
            got, gi = s.trace_rays(rays, max_bvh_iterations=0)
            bad = mismatches(got, want, gi, wi, cap_uv=True)
            ties = [j for j in bad if same_t_other_triangle(pkg, None, got, gi, want, wi, j)]
            assert len(ties) == len(bad), what + ": rays differ: " + "; ".join(
                f"#{j} got {got[j]} / {gi[j]} want {want[j]} / {wi[j]} fast {fast[:, j].astype(int)}" for j in bad if j not in ties)[:2000]
            assert len(ties) <= n // 1000
            anyh, ai = s.trace_rays(rays, any_hit=True)
            assert np.array_equal(anyh["triangle"] == R.HIT_MISS, want["triangle"] == R.HIT_MISS), what
        check("the set as created")
        s.update(torch.from_numpy(maps).cuda())          # update_device with the same maps
        assert s.update_status() == -1
        assert np.array_equal(s.world_to_object(), W)
        check("after update_device")
        # the documented refusal: a map whose inverse overflows float
        refused = maps.copy()
        refused[4, 0, 0] = F(2.0 ** -130)
        with pytest.raises(pkg._native.ShrayError):
            pkg.tracer.InstanceSet([scene] * len(maps), refused)
    finally:
        if s is not None:
            s.close()
        scene.close()
        world.close()
