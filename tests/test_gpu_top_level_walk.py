"""The walk of an instance set's top level (shader-ray_amd/instance/top_level.h's walk_top_level), which the three instanced
queries share: closest / any hit, all hits and closest points over the SAME small sets, at the shapes where only that loop
can be wrong.  Sets of 1 (the untested root is a leaf), 2 (one branch), 3 and 5 instances (median splits of odd counts:
leaves at two depths, a leaf's sibling branch waiting on the stack), with overlapping world boxes from 3 on (an exact
duplicate: a lane's best carries from one instance into the next); 1, 63, 65 and 129 items; and waves whose lanes do not
walk: a whole wave of them, and a wave whose only walking lane is lane 37.  Every answer against the references the
queries' own tests use, as bits."""
import numpy as np
import pytest

import instance_multi_hit_ref as IM
import instance_point_ref as IP
import instance_ref as I
import ray_query_ref as R
from test_gpu_instance_multi_hit import assert_same_answer
from test_gpu_instance_point import assert_answer
from test_gpu_instances import assert_same, composition, mismatches, random_set, same_t_other_triangle, scene, world_boxes, world_rays

pytestmark = pytest.mark.gpu

F = np.float32
SETS = {1: ["small_trisrc"], 2: ["lobed_528", "small_trisrc"], 3: ["lobed_528"], 5: ["small_trisrc", "lobed_528"]}
COUNTS = (1, 63, 65, 129)
WAVE, LANE = 64, 37
ITEMS = 2 * WAVE + 1            # the masked layout: wave 0 walks nothing, wave 1 only its lane 37, then one more item
WALKERS = (WAVE + LANE, 2 * WAVE)
_cases = {}


def case(pkg, n):
    """The set of n instances, its world triangles, and the two item layouts' walking pattern; once per module."""
    if n not in _cases:
        pick, M = random_set(pkg, SETS[n], n, seed=40 + n)
        s = pkg.tracer.InstanceSet([scene(pkg, p)[1] for p in pick], M)
        positions = [np.asarray(scene(pkg, p)[0].positions, F).reshape(-1) for p in pick]
        world = [IP.map_corners(M[i], positions[i]).reshape(-1, 3, 3).astype(np.float64) for i in range(n)]
        if n >= 3:
            boxes = world_boxes(pkg, pick, M)
            assert any(np.all(boxes[a][0] <= boxes[b][1]) and np.all(boxes[b][0] <= boxes[a][1])
                       for a in range(n) for b in range(a + 1, n)), "two world boxes overlap"
        _cases[n] = dict(pick=pick, M=M, set=s, positions=positions, world=world)
    return _cases[n]


@pytest.fixture(scope="module", autouse=True)
def close_the_sets():
    yield
    for c in _cases.values():
        c["set"].close()
    _cases.clear()


def layouts(natural, masked):
    """(what, first item, count) of every launch: prefixes of the natural items, then the masked layout on its own"""
    return [(f"{k} items", 0, k) for k in COUNTS] + [("a wave of no walkers, a wave of lane 37", len(natural), len(masked))]


def rays_of(pkg, c):
    """129 of the set's world rays (mixed tmax, a few made NaN), and the masked layout: tmax 0 and NaN in turn, except on the
    two walkers, which are aimed at the middle of a triangle of the last instance from outside its box"""
    o, d, tmax = world_rays(pkg, c["pick"], c["M"], COUNTS[-1], seed=7)
    tmax[5::17] = np.nan
    mo, md, _ = world_rays(pkg, c["pick"], c["M"], ITEMS, seed=8)
    mt = np.where(np.arange(ITEMS) % 2 == 0, F(0), F(np.nan)).astype(F)
    tris = c["world"][-1]
    size = float(np.ptp(tris.reshape(-1, 3), axis=0).max())
    for k, j in enumerate(WALKERS):
        tri = tris[(k * 7) % len(tris)]
        to = tri.mean(0)
        away = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        mo[j] = to + away / np.linalg.norm(away) * 3 * size
        md[j] = (to - mo[j].astype(np.float64)) / np.linalg.norm(to - mo[j].astype(np.float64))
        mt[j] = F(1e7)
    return (o, d, tmax), (mo, md, mt)


@pytest.mark.parametrize("n", sorted(SETS))
def test_closest_and_any_hit(pkg, gpu, n):
    c = case(pkg, n)
    s, pick = c["set"], c["pick"]
    natural, masked = rays_of(pkg, c)
    o, d, tmax = (np.concatenate(p) for p in zip(natural, masked))
    want, wi = composition(pkg, s, pick, o, d, tmax, max_bvh_iterations=0)
    rays = pkg.tracer.make_rays(o, d, tmax)
    W = s.world_to_object()
    assert (wi[:COUNTS[-1]] >= 0).sum() >= 10 and all(wi[COUNTS[-1] + j] >= 0 for j in WALKERS), "the walkers hit"
    idle = np.setdiff1d(np.arange(ITEMS), WALKERS) + COUNTS[-1]
    assert np.all(wi[idle] == -1) and np.all(want["triangle"][idle] == R.HIT_MISS) and np.array_equal(
        want["t"][idle].view(np.uint32), tmax[idle].view(np.uint32)), "the reference's miss record on every lane that does not walk"
    for what, first, count in layouts(natural[0], masked[0]):
        part = slice(first, first + count)
        for counters in (False, True):
            got, gi = s.trace_rays(rays[part], max_bvh_iterations=0, counters=counters)[:2]
            bad = mismatches(got, want[part], gi, wi[part], cap_uv=True)
            ties = [j for j in bad if same_t_other_triangle(pkg, pick, got, gi, want[part], wi[part], j)]
            assert len(ties) == len(bad) and len(ties) <= count // 1000, f"{n} instances, {what}, counters {counters}: rays differ: " + "; ".join(
                f"#{j} got {got[j]} / {gi[j]} want {want[part][j]} / {wi[part][j]}" for j in bad[:5])
        # any hit: the closest query's misses, and on a hit the record of the plain any-hit query of that instance's ray
        anyh, ai = s.trace_rays(rays[part], any_hit=True, max_bvh_iterations=0)
        assert np.array_equal(anyh["triangle"] == R.HIT_MISS, want["triangle"][part] == R.HIT_MISS), (n, what)
        assert np.array_equal(ai >= 0, anyh["triangle"] >= 0), (n, what)
        miss = ai < 0
        assert_same(anyh[miss], want[part][miss], f"{n} instances, {what}, any hit's misses")
        for i in np.unique(ai[~miss]):
            k = np.nonzero(ai == i)[0]
            plain = scene(pkg, pick[i])[1].trace_rays(pkg.tracer.make_rays(*I.object_rays(W[i], o[part][k], d[part][k]), tmax[part][k]),
                                                      any_hit=True, max_bvh_iterations=0)
            assert_same(anyh[k], plain, f"{n} instances, {what}, any hit on instance {i}")


@pytest.mark.parametrize("n", sorted(SETS))
def test_all_hits(pkg, gpu, n):
    c = case(pkg, n)
    s = c["set"]
    natural, masked = rays_of(pkg, c)
    o, d, tmax = (np.concatenate(p) for p in zip(natural, masked))
    want = IM.all_hits([scene(pkg, p)[0] for p in c["pick"]], s.world_to_object(), o, d, tmax, max_hits=64)
    rays = pkg.tracer.make_rays(o, d, tmax)
    assert (want[2][:COUNTS[-1]] > 0).sum() >= 10 and all(want[2][COUNTS[-1] + j] > 0 for j in WALKERS), "the walkers cross something"
    if n >= 3:
        assert (want[1][:, 1] > want[1][:, 0]).sum() > 0, "some ray's first two crossings are on two instances"
    idle = np.setdiff1d(np.arange(ITEMS), WALKERS) + COUNTS[-1]
    assert np.all(want[2][idle] == 0) and np.all(want[1][idle] == -1)
    for what, first, count in layouts(natural[0], masked[0]):
        part = slice(first, first + count)
        cut = tuple(w[part] for w in want[:3])
        for k, with_counts in [(1, True), (8, True), (4, False), (64, False)]:
            got = s.trace_all_hits(rays[part], max_hits=k, counts=with_counts)
            assert_same_answer(got, cut, f"{n} instances, {what}, K {k}, counts {with_counts}", k)
        got = s.trace_all_hits(rays[part], max_hits=8, counters=True)
        assert_same_answer(got[:3], cut, f"{n} instances, {what}, counting form", 8)
        assert np.array_equal(s.crossing_counts(rays[part]), cut[2])


def points_of(c):
    """129 world points as the instanced closest-point tests draw them, and the masked layout: a non-finite coordinate and a
    negative max_dist2 in turn, except on the two walkers, which lie just off a triangle of the last instance"""
    import instance_point_cases as IC
    distinct = sorted(set(c["pick"]))
    of = [distinct.index(p) for p in c["pick"]]
    positions = [c["positions"][c["pick"].index(x)] for x in distinct]
    natural, _, _ = IC.world_points(positions, of, c["M"], COUNTS[-1], seed=9)
    masked, _, _ = IC.world_points(positions, of, c["M"], ITEMS, seed=10)
    masked["p"] = np.nan_to_num(masked["p"], nan=0.0, posinf=1.0, neginf=-1.0)
    masked["max_dist2"] = np.inf
    masked["p"][0::2, 1] = np.inf
    masked["max_dist2"][1::2] = -1.0
    tris = c["world"][-1]
    size = float(np.ptp(tris.reshape(-1, 3), axis=0).max())
    for k, j in enumerate(WALKERS):
        tri = tris[(k * 7) % len(tris)]
        masked["p"][j] = tri.mean(0) + size / 50
        masked["max_dist2"][j] = np.inf
    return positions, of, natural, masked


@pytest.mark.parametrize("n", sorted(SETS))
def test_closest_points(pkg, gpu, n):
    c = case(pkg, n)
    s = c["set"]
    positions, of, natural, masked = points_of(c)
    pts = np.concatenate([natural, masked])
    want, wi = IP.closest_over_instances(positions, of, c["M"], pts)
    assert (wi[:COUNTS[-1]] >= 0).sum() >= 10 and all(wi[COUNTS[-1] + j] >= 0 for j in WALKERS), "the walkers find a point"
    idle = np.setdiff1d(np.arange(ITEMS), WALKERS) + COUNTS[-1]
    assert np.all(wi[idle] == -1) and np.all(want["triangle"][idle] < 0)
    if n >= 3:
        assert len(set(wi[wi >= 0].tolist())) >= 2, "the answers come from more than one instance"
    for what, first, count in layouts(natural, masked):
        part = slice(first, first + count)
        got, gi = s.closest_points(pts[part])
        assert_answer(got, gi, want[part], wi[part], f"{n} instances, {what}")
        got, gi, counters = s.closest_points(pts[part], counters=True)
        assert_answer(got, gi, want[part], wi[part], f"{n} instances, {what}, counting form")
        walked = int((np.isfinite(pts["p"][part]).all(1) & (pts["max_dist2"][part] >= 0)).sum())
        assert counters["samples"] == count and counters["traversals"] <= walked * n
