"""The CPU side of the instanced within-radius query (include/shader_ray_instance_near.h), on
tests/instance_near_ref.py: what the nine-instance set of the GPU tests covers (tests/instance_near_cases.py); a restatement of
the pruned walk (a median tree, image-box bounds, a scrambled instance order, the reach the K-th best) that returns the brute
force byte for byte; the header's five consequences; and five mutants of the walk, each changing an answer on a named input and
none on a named control."""
import os

import numpy as np
import pytest

import instance_near_cases as NC
import instance_near_ref as IN
import instance_point_cases as IC
import instance_point_ref as IP
import near_ref as NR
import point_query_ref as R
from test_instance_point_reference import set_maps, set_points

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EYE = np.eye(3, 4, dtype=F)
KS = (1, 3, 8, 9, 64)


@pytest.fixture(scope="module")
def lobed_positions(pkg):
    world = pkg.World(os.path.join(GOLDEN, "lobed_528.trisrc"))
    try:
        return np.asarray(world.arrays()["vertex_positions"], F).copy()
    finally:
        world.close()


def same(got, want):
    return all(np.array_equal(NR.as_bits(g) if g.dtype == R.CLOSEST_DTYPE else g, NR.as_bits(w) if w.dtype == R.CLOSEST_DTYPE else w)
               for g, w in zip(got, want))


def near_points(positions, maps, n, seed):
    """set_points' points with two in three of the unlimited radii made finite, up to 30 % of the scene's extent and mostly
    small: points with no pair within, with fewer than any K kept, and with more than 64"""
    pts = set_points(positions, maps, n, seed)
    rng = np.random.default_rng(seed + 1)
    extent = float(np.linalg.norm(positions.reshape(-1, 3).max(0) - positions.reshape(-1, 3).min(0)))
    finite = np.isposinf(pts["max_dist2"]) & (np.arange(n) % 3 != 0)
    pts["max_dist2"][finite] = ((rng.random(finite.sum()) ** 2 * 0.3 * extent) ** 2).astype(F)
    return pts


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_the_nine_instance_set_covers_every_band(lobed_positions):
    """The set and points of tests/test_gpu_instance_near.py, on the brute force at K = 64: every count band, records of several
    instances under a finite radius, and cross-instance ties, each over 4 % of the points."""
    tiny = {name: np.asarray(tris, F).reshape(-1) for name, tris in IC.TINY.items()}
    positions, of, maps, kinds, names = NC.nine_instances(lambda name: lobed_positions if name == "lobed_528" else tiny[name])
    assert names == NC.NINE and kinds[4] == "duplicate of 1"
    pts, kind, radius = NC.world_points(positions, of, maps, NC.NINE_POINTS, NC.NINE_POINT_SEED)
    records, instances, counts = IN.near_over_instances(positions, of, maps, pts, 64)
    print({k: round(v, 4) for k, v in NC.assert_mixed(pts, radius, records, instances, counts, "nine instances").items()})
    total = sum(len(positions[s]) // 9 for s in of)
    assert counts.max() == total, "an unlimited radius holds every pair"


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 17])
def test_the_restated_walk_returns_the_brute_force_bytes(lobed_positions, n):
    maps = set_maps(n, seed=n)
    pts = near_points(lobed_positions, maps, 96 if n < 17 else 48, seed=n + 60)
    corners = lobed_positions.reshape(-1, 3, 3)
    order = np.random.default_rng(n).permutation(n)[::-1]       # (not the index order: the key must not lean on it)
    lo, hi = corners.reshape(-1, 3).min(0), corners.reshape(-1, 3).max(0)
    top = [IP.stored_box(M, lo, hi)[:2] for M in maps]
    prepared = IN.prepare(corners, maps, pts, top)
    brute_tests = int(NR.walked(pts).sum()) * n * len(corners)
    for k in KS:
        want = IN.near_over_instances([lobed_positions], [0] * n, maps, pts, k)
        for counts in (True, False):
            rec, inst, cnt, tests = IN.restated_walk(corners, maps, pts, order, k, counts, top_boxes=top, prepared=prepared)
            assert np.array_equal(NR.as_bits(rec), NR.as_bits(want[0])), (n, k, counts)
            assert np.array_equal(inst, want[1]), (n, k, counts)
            assert (np.array_equal(cnt, want[2]) if counts else cnt is None), (n, k, counts)
            assert tests < brute_tests, "the cull skips something"
            if not counts and k == 1:
                pruned = tests
            if counts and k == 1:
                unpruned = tests
        if k == 1:
            assert pruned < unpruned, "the K-th best prunes below max_dist2"
    shares = ((want[2] > 64).mean(), ((want[2] > 0) & (want[2] <= 64)).mean(), (want[2] == 0).mean())
    assert min(shares) > 0.1, shares


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_one_identity_instance_is_the_plain_query(lobed_positions):
    pts = near_points(lobed_positions, EYE[None], 200, seed=5)
    for k in (0, 1, 8, 64):
        rec, inst, cnt = IN.near_over_instances([lobed_positions], [0], EYE[None], pts, k)
        want, want_cnt = NR.near(lobed_positions, pts, k)
        assert np.array_equal(NR.as_bits(rec), NR.as_bits(want)) and np.array_equal(cnt, want_cnt)
        assert np.array_equal(inst, np.where(want["triangle"] >= 0, 0, -1))


def test_k_1_is_the_instanced_closest_point(lobed_positions):
    maps = set_maps(5, seed=9)
    pts = near_points(lobed_positions, maps, 200, seed=10)
    rec, inst, _ = IN.near_over_instances([lobed_positions], [0] * 5, maps, pts, 1)
    want, want_inst = IP.closest_over_instances([lobed_positions], [0] * 5, maps, pts)
    assert np.array_equal(NR.as_bits(rec[:, 0]), NR.as_bits(want)) and np.array_equal(inst[:, 0], want_inst)
    assert 0.2 < (want_inst < 0).mean() < 0.8


def test_the_records_for_k_are_a_prefix_and_the_merged_scene_splits(lobed_positions):
    maps = set_maps(5, seed=11)
    pts = near_points(lobed_positions, maps, 160, seed=12)
    full = IN.near_over_instances([lobed_positions], [0] * 5, maps, pts, 64)
    for k in (1, 3, 8, 9):
        rec, inst, cnt = IN.near_over_instances([lobed_positions], [0] * 5, maps, pts, k)
        assert np.array_equal(NR.as_bits(rec), NR.as_bits(full[0][:, :k])) and np.array_equal(inst, full[1][:, :k])
        assert np.array_equal(cnt, full[2])
    # the merged scene, split by hand: every instance has 528 triangles
    merged = np.concatenate([IP.map_corners(M, lobed_positions).reshape(-1) for M in maps])
    rec, cnt = NR.near(merged, pts, 64)
    t = rec["triangle"]
    assert np.array_equal(np.where(t >= 0, t // 528, -1), full[1]) and np.array_equal(np.where(t >= 0, t % 528, -1), full[0]["triangle"])
    for f in ("q", "dist2", "u", "v", "region"):
        assert np.array_equal(rec[f].view(np.uint32), full[0][f].view(np.uint32)), f
    assert np.array_equal(cnt, full[2])


def test_an_exact_duplicate_contributes_every_pair_again_behind_its_original(lobed_positions):
    maps = set_maps(5, seed=13)                              # map 4 is map 0
    assert np.array_equal(maps[4].view(np.uint32), maps[0].view(np.uint32))
    pts = near_points(lobed_positions, maps, 160, seed=14)
    rec, inst, cnt = IN.near_over_instances([lobed_positions], [0] * 5, maps, pts, 64)
    without = IN.near_over_instances([lobed_positions], [0] * 4, maps[:4], pts, 64)
    alone = IN.near_over_instances([lobed_positions], [0], maps[:1], pts, 0)
    assert np.array_equal(cnt, without[2] + alone[2])
    pairs = 0
    for j in range(len(pts)):
        for s in np.nonzero(inst[j] == 0)[0]:
            twin = np.nonzero((inst[j] == 4) & (rec[j]["triangle"] == rec[j, s]["triangle"]))[0]
            if len(twin):       # (the twin may have fallen off the end of the K kept)
                assert twin[0] > s and rec[j, twin[0]]["dist2"] == rec[j, s]["dist2"]
                a, b = NR.as_bits(rec[j, s:s + 1]), NR.as_bits(rec[j, twin[0]:twin[0] + 1])
                assert np.array_equal(a, b)
                pairs += 1
            else:
                assert cnt[j] > 64
        assert not ((inst[j] == 4).sum() > (inst[j] == 0).sum())
    assert pairs > 500


# 4 ---------------------------------------------------------------------------------------------------------------------------
FLAT = np.array([[[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]]], F)      # in the plane z = 0: its box bound IS its dist2 above it


def above_the_flat_triangle():
    """a point above the interior of a triangle whose box is flat, two identity copies of it, the higher visited first: when
    the lower is reached, the bound of its box (and of its exact top-level box) equals the reach"""
    pts = np.zeros(1, R.POINT_DTYPE)
    pts["p"], pts["max_dist2"] = (1.0, 1.0, 0.75), np.inf
    maps = np.stack([EYE, EYE])
    boxes = [(FLAT.reshape(-1, 3).min(0), FLAT.reshape(-1, 3).max(0))] * 2
    return pts, maps, boxes, [1, 0]


def off_surface_points(positions, maps, n, seed):
    """points off every surface with positive radii: no bound equals a reach, no two pairs tie"""
    pts = near_points(positions, maps, n, seed)
    rng = np.random.default_rng(seed)
    pts["p"] += (rng.normal(size=(n, 3)) * 0.013).astype(F)
    pts["max_dist2"] = np.where(pts["max_dist2"] == 0, F(0.3), pts["max_dist2"])
    return pts


@pytest.mark.parametrize("which", ["node_skip", "top_skip"])
def test_mutant_a_skip_at_equality_loses_the_lower_instance(lobed_positions, which):
    mutant = {which: lambda lb, reach: lb >= reach}
    pts, maps, boxes, order = above_the_flat_triangle()
    want = IN.near_over_instances([FLAT.reshape(-1)], [0, 0], maps, pts, 1)
    assert want[1][0, 0] == 0 and want[0][0, 0]["dist2"] == F(0.5625)
    rec, inst, _, _ = IN.restated_walk(FLAT, maps, pts, order, 1, False, top_boxes=boxes)
    assert same((rec, inst), want[:2])
    rec, inst, _, _ = IN.restated_walk(FLAT, maps, pts, order, 1, False, top_boxes=boxes, **mutant)
    assert inst[0, 0] == 1, "the mutant keeps the higher instance"
    # the control: nothing sits at equality
    maps = set_maps(2, seed=3)
    corners = lobed_positions.reshape(-1, 3, 3)
    pts = off_surface_points(lobed_positions, maps, 64, seed=21)
    top = [IP.stored_box(M, corners.reshape(-1, 3).min(0), corners.reshape(-1, 3).max(0))[:2] for M in maps]
    want = IN.near_over_instances([lobed_positions], [0, 0], maps, pts, 3)
    rec, inst, _, _ = IN.restated_walk(corners, maps, pts, [1, 0], 3, False, top_boxes=top, **mutant)
    assert same((rec, inst), want[:2])


def test_mutant_the_tie_by_triangle_before_instance(lobed_positions):
    mutant = dict(key=lambda d, i, t: (d, t, i))
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = np.stack([set_maps(1, seed=4)[0]] * 2)            # an exact duplicate
    pts = np.zeros(8, R.POINT_DTYPE)
    pts["p"] = IP.map_corners(maps[0], corners[::66, 0])      # exactly at mapped corners: the triangles around each tie at 0
    pts["max_dist2"] = np.inf
    want = IN.near_over_instances([lobed_positions], [0, 0], maps, pts, 4)
    assert (want[0]["dist2"][:, :4] == 0).all() and (want[1][:, :2] == 0).all(), "two triangles of instance 0 lead"
    rec, inst, _, _ = IN.restated_walk(corners, maps, pts, [1, 0], 4, False)
    assert same((rec, inst), want[:2])
    rec, inst, _, _ = IN.restated_walk(corners, maps, pts, [1, 0], 4, False, **mutant)
    assert (inst[:, 1] == 1).all(), "the mutant puts the duplicate's copy of the first triangle second"
    # the control: no two pairs tie
    maps = set_maps(2, seed=3)
    pts = off_surface_points(lobed_positions, maps, 64, seed=22)
    want = IN.near_over_instances([lobed_positions], [0, 0], maps, pts, 4)
    rec, inst, cnt, _ = IN.restated_walk(corners, maps, pts, [1, 0], 4, True, **mutant)
    assert same((rec, inst, cnt), want)


def test_mutant_the_reach_taken_one_slot_early():
    """The reach must be the K-th smallest dist2 held (slot K - 1 from 0).  Taken from the slot before it, the walk prunes what
    could still be the K-th record: three copies of the flat triangle 1, 2 and 3 below the point, K = 3, the nearest visited
    first; after two the mutant's reach is 4 and the third, whose bound is 9, is lost.  Taken from the slot after it (which
    the K kept do not have) the walk prunes by max_dist2 alone: the same answer."""
    pts = np.zeros(1, R.POINT_DTYPE)
    pts["p"], pts["max_dist2"] = (1.0, 1.0, 0.0), np.inf
    maps = np.stack([EYE] * 3)
    maps[:, 2, 3] = (-1.0, -2.0, -3.0)
    want = IN.near_over_instances([FLAT.reshape(-1)], [0, 0, 0], maps, pts, 3)
    assert want[0]["dist2"][0].tolist() == [1.0, 4.0, 9.0] and want[1][0].tolist() == [0, 1, 2]
    rec, inst, _, _ = IN.restated_walk(FLAT, maps, pts, [0, 1, 2], 3, False)
    assert same((rec, inst), want[:2])
    rec, inst, _, _ = IN.restated_walk(FLAT, maps, pts, [0, 1, 2], 3, False, reach_slot=-2)
    assert inst[0].tolist() == [0, 1, -1], "the mutant loses the third record"
    rec, inst, _, _ = IN.restated_walk(FLAT, maps, pts, [0, 1, 2], 3, False, reach_slot=0)
    assert same((rec, inst), want[:2])
    # the control: the form with counts never reads the slot
    rec, inst, cnt, _ = IN.restated_walk(FLAT, maps, pts, [0, 1, 2], 3, True, reach_slot=-2)
    assert same((rec, inst, cnt), want)


def test_mutant_n_counted_only_for_kept_records(lobed_positions):
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = set_maps(2, seed=3)
    pts = near_points(lobed_positions, maps, 64, seed=24)
    prepared = IN.prepare(corners, maps, pts)
    want = IN.near_over_instances([lobed_positions], [0, 0], maps, pts, 3)
    assert (want[2] > 3).mean() > 0.3
    rec, inst, cnt, _ = IN.restated_walk(corners, maps, pts, [1, 0], 3, True, prepared=prepared)
    assert same((rec, inst, cnt), want)
    rec, inst, cnt, _ = IN.restated_walk(corners, maps, pts, [1, 0], 3, True, count_kept_only=True, prepared=prepared)
    assert same((rec, inst), want[:2]) and (cnt != want[2]).sum() >= (want[2] > 3).sum() // 2 and (cnt <= want[2]).all()
    # the control: radii so small that no point holds more than K
    small = pts.copy()
    small["max_dist2"] = np.where(np.isfinite(pts["max_dist2"]) | np.isnan(pts["max_dist2"]), pts["max_dist2"], F(1e-4))
    small["max_dist2"] = np.where(small["max_dist2"] > 1e-4, F(1e-4), small["max_dist2"])
    want = IN.near_over_instances([lobed_positions], [0, 0], maps, small, 64)
    assert want[2].max() <= 64 and (want[2] > 0).sum() > 5
    rec, inst, cnt, _ = IN.restated_walk(corners, maps, small, [1, 0], 64, True, count_kept_only=True)
    assert same((rec, inst, cnt), want)


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["leaf_root", "one_branch", "wide_by_one"])
def test_the_counting_walk_finds_every_member(name):
    """instance_near_ref.walk_counters over a hand-shaped tree and refit_ref.node_boxes: the pairs it finds within the radius are
    the brute force's count under every kind of map (the counting form skips nothing in S), a point that is not walked counts
    nothing, a walked one counts the root, two bounds a branch entered and every triangle of a leaf entered."""
    import refit_ref
    import tree_shapes as T
    tree, vertex_data = T.build(name)
    corners = np.ascontiguousarray(vertex_data[tree.triangle_vertices][:, :, :3])
    positions = corners.reshape(-1)
    boxes = refit_ref.node_boxes(tree, corners)
    rng = np.random.default_rng(len(name))
    leaves = tree.negative < 0
    for kind in ("identity", "rotation_nonuniform", "mirror", "shear", "signed_permutation"):
        M = IC.map_of(kind, rng, positions, 1.5).astype(F)
        pts, _, _ = NC.world_points([positions], [0], M[None], 160, seed=3)
        _, _, want = IN.near_over_instances([positions], [0], M[None], pts, 0)
        w = IN.walk_counters(tree, boxes, corners, M, pts)
        assert np.array_equal(w["near"], want), (name, kind)
        go = NR.walked(pts)
        assert np.array_equal(w["traversals"], go.astype(np.int64)) and (w["node_visits"][~go] == 0).all()
        assert (w["node_visits"][go] % 2 == 1).all() and (w["node_visits"] <= tree.node_count).all()
        assert (w["leaf_visits"] <= leaves.sum()).all() and (w["triangle_tests"] >= w["near"]).all()
        unlimited = go & np.isposinf(pts["max_dist2"])
        assert (w["node_visits"][unlimited] == tree.node_count).all() and (w["triangle_tests"][unlimited] == len(corners)).all()
        # a top-level box the point is outside by more than its radius: nothing is walked, and nothing was within
        lo, hi = IP.image_box(M, boxes[0, :3], boxes[0, 3:])
        culled = IN.walk_counters(tree, boxes, corners, M, pts, top_box=(lo, hi))
        out = go & (culled["traversals"] == 0)
        assert (want[out] == 0).all() and np.array_equal(culled["near"], want)
