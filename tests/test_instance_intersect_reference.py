"""The CPU side of the instanced triangle-intersection query (include/shader_ray_instance_intersect.h), on
tests/instance_intersect_ref.py: what the nine-instance set, its queries and the placed lattice of the GPU tests cover
(tests/instance_intersect_cases.py); a restatement of the walk (a median tree, image boxes, the stored boxes as the top level,
a scrambled instance order, the instance skip of the pruned form, the own-instance skip) that returns the brute force index
for index; the header's seven consequences; and seven mutants of the walk, each changing an answer on a named input and none
on a named control where there is one."""
import os

import numpy as np
import pytest

import instance_intersect_cases as XC
import instance_intersect_ref as II
import instance_point_cases as IC
import instance_point_ref as IP
import intersect_cases as TC
import intersect_ref as IR
from test_instance_point_reference import set_maps

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


@pytest.fixture(scope="module")
def nine(lobed_positions):
    tiny = {name: np.asarray(tris, F).reshape(-1) for name, tris in IC.TINY.items()}
    positions, of, maps, kinds, names = XC.nine_instances(lambda name: lobed_positions if name == "lobed_528" else tiny[name])
    assert kinds[4] == "duplicate of 1"
    return positions, of, maps


def queries_for(positions, maps, n, seed):
    """intersect_cases' queries of every kind over the merged scene of `positions` under `maps`"""
    return XC.world_queries([positions], [0] * len(maps), maps, n, seed)


def stored(corners, maps):
    out = []
    for i, M in enumerate(maps):
        v = (corners[i] if isinstance(corners, list) else corners).reshape(-1, 3)
        out.append(IP.stored_box(M, v.min(0), v.max(0))[:2])
    return out


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


# 1: what the GPU tests' inputs cover --------------------------------------------------------------------------------------------
def test_the_nine_instance_set_and_its_queries_cover_every_band(nine):
    """The set and queries of tests/test_gpu_instance_intersect.py, on the brute force at K = 64: every band of n and held pairs
    of several instances, each over 4 % of the queries; nq, nt and the nine edge axes each first to separate some pair."""
    positions, of, maps = nine
    queries = XC.world_queries(positions, of, maps)
    assert len(queries) == 768
    merged, first = IP.merged_positions(positions, of, maps)
    code = IR.first_axis(queries, merged)
    tri, inst, n = II.from_membership(code == IR.INTERSECT, first, 64)
    s = XC.assert_mixed(queries, inst, n, code, "nine instances")
    print(s)
    assert n.max() > 64 and (~IR.walked(queries)).sum() >= 30
    assert min(s["first to separate, per axis"][:11]) >= 20


@pytest.mark.parametrize("seed", [3, 7])
def test_the_placed_lattice_makes_every_in_plane_axis_separate_first_and_is_exact(seed):
    """Three exact placements of the flat lattice and integer queries: each of the axes 12 to 17 is the first to separate some
    pair, all three instances are hit, and every pair's membership is the exact one on the world corners."""
    positions, of, maps = XC.placed_lattice()
    queries = XC.lattice_queries(seed)
    merged, first = IP.merged_positions(positions, of, maps)
    assert np.array_equal(merged, np.rint(merged)), "every world corner is an integer"
    code = IR.first_axis(queries, merged)
    per_axis = np.bincount(code[(code >= IR.AXIS0) & (code < IR.UNWALKED)].astype(np.int64) - IR.AXIS0, minlength=IR.AXES)
    print(seed, per_axis.tolist())
    assert min(per_axis[11:]) >= 1, per_axis.tolist()
    tri, inst, n = II.from_membership(code == IR.INTERSECT, first, 64)
    assert set(inst[inst >= 0].tolist()) == {0, 1, 2}
    world = merged.reshape(-1, 3, 3)
    walked = IR.walked(queries)
    for j in np.nonzero(walked)[0]:
        for t in np.nonzero((code[j] >= 3) | (code[j] == IR.INTERSECT))[0]:   # (stage 0 is comparisons only: exact by itself)
            assert (code[j, t] == IR.INTERSECT) == TC.exact_intersects(queries[j], world[t]), (j, t)
    assert (code[~walked] == IR.UNWALKED).all()


def test_the_instance_form_on_the_nine_instance_set(nine):
    """With SKIP_OWN_INSTANCE: instance 5 meets nothing; the duplicates 1 and 4 meet in all 528 triangles; instance 0 meets 6
    and 8 in 306 of its triangles; instance 8 (11 triangles) meets five instances; all but instance 5 collide."""
    positions, of, maps = nine
    met = {}
    for q in range(9):
        member, first = II.own_membership(positions, of, maps, q)
        n = member.sum(1)
        hit = sorted({int(np.searchsorted(first, c, side="right") - 1) for c in np.nonzero(member.any(0))[0]})
        met[q] = (int((n > 0).sum()), int(n.max()), hit)
        assert q not in hit
    print(met)
    assert met[5] == (0, 0, [])
    assert met[1] == (528, 29, [4]) and met[4] == (528, 29, [1])
    assert met[0][0] == 306 and met[0][2] == [6, 8]
    assert len(met[8][2]) == 5 and met[8][1] == 169
    assert II.colliding(positions, of, maps).tolist() == [q != 5 for q in range(9)]


# 2: the restated walk ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 17])
def test_the_restated_walk_returns_the_brute_force_indices(lobed_positions, n):
    maps = set_maps(n, seed=n)
    corners = lobed_positions.reshape(-1, 3, 3)
    queries = queries_for(lobed_positions, maps, 128 if n < 17 else 64, seed=n + 40)
    order = np.random.default_rng(n).permutation(n)[::-1]       # (not the index order: the key must not lean on it)
    top = stored(corners, maps)
    brute_tests = int(IR.walked(queries).sum()) * n * len(corners)
    for skip_shared in (False, True):
        member, first = II.membership([lobed_positions], [0] * n, maps, queries, skip_shared)
        for k in KS:
            want = II.from_membership(member, first, k)
            for counts in (True, False):
                tri, inst, cnt, tests, walks = II.restated_walk(corners, maps, queries, order, k, counts, skip_shared=skip_shared,
                                                                top_boxes=top)
                assert np.array_equal(tri, want[0]) and np.array_equal(inst, want[1]), (n, k, counts, skip_shared)
                assert (np.array_equal(cnt, want[2]) if counts else cnt is None), (n, k, counts, skip_shared)
                assert tests < brute_tests, "the cull skips something"
        got_any = II.restated_walk(corners, maps, queries, order, 0, True, skip_shared=skip_shared, top_boxes=top, any_only=True)
        assert np.array_equal(got_any[2], (want[2] > 0).astype(np.int32)), "ANY is n > 0"
        if not skip_shared:
            shares = ((want[2] > 64).mean(), ((want[2] > 0) & (want[2] <= 64)).mean(), (want[2] == 0).mean())
            assert min(shares) > 0.05, shares
        else:
            assert (want[2] != II.from_membership(*II.membership([lobed_positions], [0] * n, maps, queries), 0)[2]).mean() > 0.1


def test_the_instance_skip_begins_fewer_walks(lobed_positions):
    maps = set_maps(17, seed=17)
    corners = lobed_positions.reshape(-1, 3, 3)
    queries = queries_for(lobed_positions, maps, 96, seed=57)
    order = np.arange(17)
    top = stored(corners, maps)
    with_counts = II.restated_walk(corners, maps, queries, order, 1, True, top_boxes=top)
    without = II.restated_walk(corners, maps, queries, order, 1, False, top_boxes=top)
    assert same(without[:2], with_counts[:2]) and without[4] < with_counts[4] and without[3] < with_counts[3]


# 3: the consequences -----------------------------------------------------------------------------------------------------------
def test_consequence_1_one_identity_instance_is_the_plain_query(lobed_positions):
    queries = queries_for(lobed_positions, EYE[None], 300, seed=5)
    for skip_shared in (False, True):
        for k in (0, 1, 8, 64):
            tri, inst, cnt = II.intersect_over_instances([lobed_positions], [0], EYE[None], queries, k, skip_shared)
            want, want_cnt = IR.intersect(queries, lobed_positions, k, skip_shared)
            assert np.array_equal(tri, want) and np.array_equal(cnt, want_cnt)
            assert np.array_equal(inst, np.where(want >= 0, 0, -1))


def test_consequences_2_and_3_the_merged_scene_splits_and_k_is_a_prefix(lobed_positions):
    maps = set_maps(5, seed=11)
    queries = queries_for(lobed_positions, maps, 300, seed=12)
    full = II.intersect_over_instances([lobed_positions], [0] * 5, maps, queries, 64)
    for k in (1, 3, 8, 9):
        tri, inst, cnt = II.intersect_over_instances([lobed_positions], [0] * 5, maps, queries, k)
        assert np.array_equal(tri, full[0][:, :k]) and np.array_equal(inst, full[1][:, :k]) and np.array_equal(cnt, full[2])
    # the merged scene, split by hand: every instance has 528 triangles
    merged = np.concatenate([IP.map_corners(M, lobed_positions).reshape(-1) for M in maps])
    idx, cnt = IR.intersect(queries, merged, 64)
    assert np.array_equal(np.where(idx >= 0, idx // 528, -1), full[1]) and np.array_equal(np.where(idx >= 0, idx % 528, -1), full[0])
    assert np.array_equal(cnt, full[2])
    key = full[1].astype(np.int64) * 528 + full[0]
    held = full[0] >= 0
    assert ((np.diff(key, axis=1) > 0) | ~held[:, 1:]).all(), "(instance, triangle) ascends over the held slots"
    assert (held[:, 1:] <= held[:, :-1]).all(), "then -1"


def test_consequence_4_a_duplicate_contributes_every_pair_again_behind_its_original(lobed_positions):
    maps = set_maps(5, seed=13)                              # map 4 is map 0
    assert np.array_equal(maps[4].view(np.uint32), maps[0].view(np.uint32))
    queries = queries_for(lobed_positions, maps, 300, seed=14)
    member, first = II.membership([lobed_positions], [0] * 5, maps, queries)
    assert np.array_equal(member[:, :528], member[:, 4 * 528:]) and member[:, :528].sum() > 1000
    tri, inst, cnt = II.from_membership(member, first, 64)
    without = II.intersect_over_instances([lobed_positions], [0] * 4, maps[:4], queries, 64)
    alone = II.intersect_over_instances([lobed_positions], [0], maps[:1], queries, 0)
    assert np.array_equal(cnt, without[2] + alone[2])
    pairs = 0
    for j in range(len(queries)):
        for s in np.nonzero(inst[j] == 4)[0]:
            original = np.nonzero((inst[j] == 0) & (tri[j] == tri[j, s]))[0]
            assert len(original) == 1 and original[0] < s
            pairs += 1
    assert pairs > 100


def test_consequence_5_any_is_n_above_zero(lobed_positions):
    maps = set_maps(5, seed=15)
    corners = lobed_positions.reshape(-1, 3, 3)
    queries = queries_for(lobed_positions, maps, 200, seed=16)
    n = II.intersect_over_instances([lobed_positions], [0] * 5, maps, queries, 0)[2]
    for order in (np.arange(5), np.arange(5)[::-1]):
        got = II.restated_walk(corners, maps, queries, order, 0, True, top_boxes=stored(corners, maps), any_only=True)
        assert np.array_equal(got[2], (n > 0).astype(np.int32))
    assert 0.1 < (n > 0).mean() < 0.95


def test_consequence_6_the_instance_form_is_the_item_form_on_its_own_rows(nine):
    """The walk fed with instance q's world corners and told to skip q equals the item form's answer with q's pairs removed, and
    n is less by their number."""
    positions, of, maps = nine
    corners = [positions[s].reshape(-1, 3, 3) for s in of]
    top = stored(corners, maps)
    order = np.random.default_rng(6).permutation(9)
    for q, first_triangle, count in ((0, 100, 90), (1, 0, 80), (8, 0, None), (7, 0, None), (6, 500, 28)):
        queries = II.own_queries(positions, of, maps, q, first_triangle, count)
        item = II.intersect_over_instances(positions, of, maps, queries, 64)
        assert same(II.intersect_instance(positions, of, maps, q, 64, skip_own=False, first_triangle=first_triangle, count=count), item)
        got = II.restated_walk(corners, maps, queries, order, 64, True, top_boxes=top, own=q, skip_own=False, scene_of=of)
        assert same(got[:3], item), q
        want = II.intersect_instance(positions, of, maps, q, 64, first_triangle=first_triangle, count=count)
        got = II.restated_walk(corners, maps, queries, order, 64, True, top_boxes=top, own=q, skip_own=True, scene_of=of)
        assert same(got[:3], want), q
        member, first = II.membership(positions, of, maps, queries)
        own_pairs = member[:, first[q]:first[q + 1]].sum(1)
        assert np.array_equal(item[2] - want[2], own_pairs) and (own_pairs >= 1).all(), "every triangle finds itself"
        assert not (want[1] == q).any()
        for k in (1, 8, 9):
            pruned = II.restated_walk(corners, maps, queries, order, k, False, top_boxes=top, own=q, skip_own=True, scene_of=of)
            assert np.array_equal(pruned[0], want[0][:, :k]) and np.array_equal(pruned[1], want[1][:, :k])


def test_consequence_7_one_identity_instance_without_the_flag_is_the_self_form(lobed_positions):
    corners = lobed_positions.reshape(-1, 3, 3)
    for skip_shared in (False, True):
        want, want_n = IR.intersect(corners, lobed_positions, 64, skip_shared)          # the self form's restatement
        tri, inst, n = II.intersect_instance([lobed_positions], [0], EYE[None], 0, 64, skip_shared=skip_shared, skip_own=False)
        assert np.array_equal(tri, want) and np.array_equal(n, want_n) and np.array_equal(inst, np.where(want >= 0, 0, -1))
        got = II.restated_walk(corners, EYE[None], corners[:160], [0], 64, True, skip_shared=skip_shared, own=0, skip_own=False)
        assert np.array_equal(got[0], want[:160]) and np.array_equal(got[2], want_n[:160])
    assert (IR.intersect(corners, lobed_positions, 0)[1] >= 1).all(), "without SKIP_SHARED every triangle finds itself"


# 4: the mutants ----------------------------------------------------------------------------------------------------------------
def test_mutant_at_or_beyond_in_the_node_cull(lobed_positions):
    """<= culls a node whose image box only touches the query's vertex box: a triangle of the set as the query loses the
    neighbours in other leaves that touch it at a vertex with an extreme coordinate (under an axis-aligned scale the image box
    is the box of the mapped corners, so the two ends are the same bits)."""
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = np.zeros((2, 3, 4), F)
    maps[0, :, :3], maps[1, :, :3] = np.diag([0.75, 1.25, 1.5]), np.diag([-1.0, 1.0, 0.5])
    maps[1, :, 3] = (6.0, 0.5, -0.25)
    queries = II.own_queries([lobed_positions], [0, 0], maps, 0)[::3]
    want = II.intersect_over_instances([lobed_positions], [0, 0], maps, queries, 64)
    assert (want[2] > 1).all()
    right = II.restated_walk(corners, maps, queries, [1, 0], 64, True, top_boxes=stored(corners, maps))
    assert same(right[:3], want)
    wrong = II.restated_walk(corners, maps, queries, [1, 0], 64, True, top_boxes=stored(corners, maps), node_cull=II.misses_or_touches)
    assert not same(wrong[:3], want) and (wrong[2] <= want[2]).all()


def ends_by_position(M, lo, hi):
    """a mutant image box: the corner formula on (lo, lo, lo) and (hi, hi, hi), whatever the entries' signs"""
    M = np.asarray(M, F).reshape(3, 4)
    low = np.stack([IP.map_row(M[r], tuple(lo[..., c] for c in range(3))) for r in range(3)], -1)
    high = np.stack([IP.map_row(M[r], tuple(hi[..., c] for c in range(3))) for r in range(3)], -1)
    return low, high


def test_mutant_image_ends_chosen_without_the_sign(lobed_positions):
    """With a negative entry the low end needs the box's high coordinate: on the mirror and the rotations pairs are lost.  Maps
    whose entries are all positive or zero (a scale with a translation) are the control."""
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = set_maps(3, seed=23)
    assert (maps[:, :, :3] < 0).any(axis=(1, 2)).all()
    positive = np.zeros((2, 3, 4), F)
    positive[0, :, :3], positive[1, :, :3] = np.diag([0.7, 1.2, 0.9]), np.diag([1.5, 0.6, 1.1])
    positive[1, :, 3] = (0.5, -1.0, 2.0)
    for m, differs in ((maps, True), (positive, False)):
        queries = queries_for(lobed_positions, m, 128, seed=24)
        order = list(range(len(m)))[::-1]
        want = II.intersect_over_instances([lobed_positions], [0] * len(m), m, queries, 64)
        assert same(II.restated_walk(corners, m, queries, order, 64, True, top_boxes=stored(corners, m))[:3], want)
        wrong = II.restated_walk(corners, m, queries, order, 64, True, top_boxes=stored(corners, m), image_box=ends_by_position)
        assert same(wrong[:3], want) != differs, differs


def test_mutant_triangle_before_instance_in_the_key(lobed_positions):
    """(triangle, instance) keeps other pairs once a query has more than K members from two instances.  One instance is the
    control: the two keys order its pairs alike."""
    corners = lobed_positions.reshape(-1, 3, 3)
    for n, differs in ((3, True), (1, False)):
        maps = set_maps(n, seed=25)
        if n > 1:
            maps[1] = maps[0]
            maps[1, :, 3] += F(0.05)                         # beside instance 0: most queries have members of both
        queries = queries_for(lobed_positions, maps, 128, seed=26)
        want = II.intersect_over_instances([lobed_positions], [0] * n, maps, queries, 8)
        order = list(range(n))[::-1]
        assert same(II.restated_walk(corners, maps, queries, order, 8, True, top_boxes=stored(corners, maps))[:3], want)
        wrong = II.restated_walk(corners, maps, queries, order, 8, True, top_boxes=stored(corners, maps), key=II.key_triangle_first)
        assert np.array_equal(wrong[2], want[2]) and same(wrong[:2], want[:2]) != differs, differs


def test_mutant_the_instance_skip_reads_the_slot_before_the_kth(lobed_positions):
    """Reading slot K - 1 skips a higher instance while slot K is still empty, and loses its pairs.  K = 1 is the control: there
    is no slot before the first, so nothing is skipped early."""
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = set_maps(3, seed=27)
    maps[1], maps[2] = maps[0], maps[0]
    maps[1, :, 3] += F(0.05)
    maps[2, :, 3] -= F(0.05)
    queries = queries_for(lobed_positions, maps, 160, seed=28)
    order = [0, 1, 2]                                         # ascending: the lower instances' keys are held when a higher one comes
    for k, differs in ((3, True), (9, True), (1, False)):
        want = II.intersect_over_instances([lobed_positions], [0] * 3, maps, queries, k)
        assert same(II.restated_walk(corners, maps, queries, order, k, False, top_boxes=stored(corners, maps))[:2], want[:2])
        wrong = II.restated_walk(corners, maps, queries, order, k, False, top_boxes=stored(corners, maps), skip_slot=-1)
        assert same(wrong[:2], want[:2]) != differs, (k, differs)


def test_mutant_n_counted_only_for_kept_members(lobed_positions):
    """n is |S|, not the number of pairs that entered the K kept.  K = 64 with queries of at most 64 members is the control."""
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = set_maps(2, seed=29)
    queries = queries_for(lobed_positions, maps, 160, seed=30)
    n = II.intersect_over_instances([lobed_positions], [0, 0], maps, queries, 0)[2]
    assert (n > 8).mean() > 0.2
    few = queries[n <= 64]
    for qs, k, differs in ((queries, 8, True), (few, 64, False)):
        want = II.intersect_over_instances([lobed_positions], [0, 0], maps, qs, k)
        assert same(II.restated_walk(corners, maps, qs, [1, 0], k, True, top_boxes=stored(corners, maps))[:3], want)
        wrong = II.restated_walk(corners, maps, qs, [0, 1], k, True, top_boxes=stored(corners, maps), count_kept_only=True)
        assert same(wrong[:2], want[:2]) and np.array_equal(wrong[2], want[2]) != differs, differs


def test_mutant_own_judged_by_the_scene(nine):
    """"Own" is the instance index: q = 1 must still find its duplicate, instance 4, which shares its scene.  A set of distinct
    scenes (instances 0, 7 and 8 of the nine) is the control."""
    positions, of, maps = nine
    for pick, q, differs in ((list(range(9)), 1, True), ([0, 7, 8], 2, False)):
        p_of = [of[i] for i in pick]
        p_maps = maps[pick]
        corners = [positions[s].reshape(-1, 3, 3) for s in p_of]
        queries = II.own_queries(positions, p_of, p_maps, q, 0, 120)
        want = II.intersect_instance(positions, p_of, p_maps, q, 64, count=len(queries))
        assert (want[2] > 0).any()
        order = list(range(len(pick)))[::-1]
        right = II.restated_walk(corners, p_maps, queries, order, 64, True, top_boxes=stored(corners, p_maps), own=q, skip_own=True,
                                 scene_of=p_of)
        assert same(right[:3], want)
        wrong = II.restated_walk(corners, p_maps, queries, order, 64, True, top_boxes=stored(corners, p_maps), own=q, skip_own=True,
                                 scene_of=p_of, own_is=II.same_scene)
        assert same(wrong[:3], want) != differs, differs
        if differs:
            assert (want[1] == 4).any() and not (wrong[1] == 4).any()


def test_mutant_shared_corners_judged_on_object_coordinates(nine):
    """The shared-corner rule compares WORLD corners: instance 0's triangle j and instance 6's triangle t share a corner of their
    common scene, but not in the world.  Judged on object coordinates, q = 0 against instance 6 loses such pairs.  One instance
    is the control: there the object corners are equal exactly where the world corners are."""
    positions, of, maps = nine
    lobed = positions[0]
    corners = lobed.reshape(-1, 3, 3)
    for pick, differs in (([0, 6], True), ([2], False)):
        p_maps = maps[pick]
        n = len(pick)
        queries = II.own_queries([lobed], [0] * n, p_maps, 0)
        want = II.intersect_instance([lobed], [0] * n, p_maps, 0, 64, skip_shared=True, skip_own=n > 1)
        assert (want[2] > 0).any() or n == 1
        kw = dict(top_boxes=stored(corners, p_maps), skip_shared=True, own=0, skip_own=n > 1, object_queries=corners)
        right = II.restated_walk(corners, p_maps, queries, list(range(n)), 64, True, **kw)
        assert same(right[:3], want)
        wrong = II.restated_walk(corners, p_maps, queries, list(range(n)), 64, True, shared_on_object=True, **kw)
        assert same(wrong[:3], want) != differs, differs


# 5: the guard's regime --------------------------------------------------------------------------------------------------------
def test_an_instance_small_enough_for_a_wrong_top_level_cull_has_no_member():
    """a top-level cull can be wrong only for an instance whose world coordinates are all below 2^-130.  Such
    an instance is no member's home for this query: the edges of its world triangles, taken after the translation by the query's
    corner, are 0 or below 2^-128, every product in nt = e0 x e1 underflows to 0, and the degenerate rule rejects the triangle.
    So the guard (kept: the predicate is section 23's, unchanged) cannot change S here.  Shown on random maps and triangles at
    2^-132 against queries of every size that cross the origin; order-1 triangles under the same maps are the control."""
    rng = np.random.default_rng(149)
    for scale, empty in ((2.0 ** -132, True), (1.0, False)):
        members = 0
        for _ in range(300):
            M = np.zeros((3, 4), F)
            M[:, :3] = (np.eye(3) + rng.uniform(-0.5, 0.5, (3, 3))).astype(F)
            corners = (rng.uniform(-1, 1, (4, 3, 3)) * scale).astype(F)
            world = IP.map_corners(M, corners).reshape(-1, 3, 3)
            if empty:
                assert (np.abs(world) < 2.0 ** -130).all()
            size = 2.0 ** rng.integers(-140, 3, (6, 1, 1))
            queries = (rng.uniform(-1, 1, (6, 3, 3)) * size).astype(F)
            queries[:, 0] *= F(-1)                                            # (corners on both sides of the origin)
            queries = np.concatenate([queries, world])                      # and the instance's own world triangles
            members += int(IR.intersects(queries, world.reshape(-1)).sum())
        assert (members == 0) == empty, (scale, members)
