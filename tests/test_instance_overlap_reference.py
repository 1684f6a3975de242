"""The CPU side of the instanced box-overlap query (include/shader_ray_instance_overlap.h), on
tests/instance_overlap_ref.py: what the nine-instance set and the boxes of the GPU tests cover
(tests/instance_overlap_cases.py); a restatement of the walk (a median tree, image boxes, the stored boxes as the top level, a
scrambled instance order, the instance skip of the pruned form) that returns the brute force index for index; the header's five
consequences; and six mutants of the walk, each changing an answer on a named input and none on a named control."""
import os

import numpy as np
import pytest

import instance_overlap_cases as XC
import instance_overlap_ref as IO
import instance_point_cases as IC
import instance_point_ref as IP
import overlap_ref as OR
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


def boxes_for(positions, maps, n, seed):
    """overlap_cases' boxes of every kind over the merged scene of `positions` under `maps`"""
    return XC.world_boxes([positions], [0] * len(maps), maps, n, seed)


def stored(corners, maps):
    v = corners.reshape(-1, 3)
    return [IP.stored_box(M, v.min(0), v.max(0))[:2] for M in maps]


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_the_nine_instance_set_and_its_boxes_cover_every_band(lobed_positions):
    """The set and boxes of tests/test_gpu_instance_overlap.py, on the brute force at K = 64: every band of n and held pairs of
    several instances, each over 4 % of the boxes; every later axis first to separate some pair."""
    tiny = {name: np.asarray(tris, F).reshape(-1) for name, tris in IC.TINY.items()}
    positions, of, maps, kinds, names = XC.nine_instances(lambda name: lobed_positions if name == "lobed_528" else tiny[name])
    assert kinds[4] == "duplicate of 1"
    boxes = XC.world_boxes(positions, of, maps)
    assert len(boxes) == 1536
    merged, first = IP.merged_positions(positions, of, maps)
    code = OR.first_axis(merged, boxes)
    tri, inst, n = IO.from_membership(code == OR.OVERLAP, first, 64)
    s = XC.assert_mixed(boxes, inst, n, code, "nine instances")
    print(s)
    assert n.max() > 64 and (~OR.walked(boxes)).sum() >= 30


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 17])
def test_the_restated_walk_returns_the_brute_force_indices(lobed_positions, n):
    maps = set_maps(n, seed=n)
    corners = lobed_positions.reshape(-1, 3, 3)
    boxes = boxes_for(lobed_positions, maps, 160 if n < 17 else 96, seed=n + 40)
    order = np.random.default_rng(n).permutation(n)[::-1]       # (not the index order: the key must not lean on it)
    top = stored(corners, maps)
    member, first = IO.membership([lobed_positions], [0] * n, maps, boxes)
    brute_tests = int(OR.walked(boxes).sum()) * n * len(corners)
    for k in KS:
        want = IO.from_membership(member, first, k)
        for counts in (True, False):
            tri, inst, cnt, tests, walks = IO.restated_walk(corners, maps, boxes, order, k, counts, top_boxes=top)
            assert np.array_equal(tri, want[0]) and np.array_equal(inst, want[1]), (n, k, counts)
            assert (np.array_equal(cnt, want[2]) if counts else cnt is None), (n, k, counts)
            assert tests < brute_tests, "the cull skips something"
    got_any = IO.restated_walk(corners, maps, boxes, order, 0, True, top_boxes=top, any_only=True)
    assert np.array_equal(got_any[2], (want[2] > 0).astype(np.int32)), "ANY is n > 0"
    shares = ((want[2] > 64).mean(), ((want[2] > 0) & (want[2] <= 64)).mean(), (want[2] == 0).mean())
    assert min(shares) > 0.05, shares


def test_the_instance_skip_begins_fewer_walks(lobed_positions):
    maps = set_maps(17, seed=17)
    corners = lobed_positions.reshape(-1, 3, 3)
    boxes = boxes_for(lobed_positions, maps, 96, seed=57)
    order = np.arange(17)
    top = stored(corners, maps)
    with_counts = IO.restated_walk(corners, maps, boxes, order, 1, True, top_boxes=top)
    without = IO.restated_walk(corners, maps, boxes, order, 1, False, top_boxes=top)
    assert same(without[:2], with_counts[:2]) and without[4] < with_counts[4] and without[3] < with_counts[3]


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_consequence_1_one_identity_instance_is_the_plain_query(lobed_positions):
    boxes = boxes_for(lobed_positions, EYE[None], 300, seed=5)
    for k in (0, 1, 8, 64):
        tri, inst, cnt = IO.overlap_over_instances([lobed_positions], [0], EYE[None], boxes, k)
        want, want_cnt = OR.overlap(lobed_positions, boxes, k)
        assert np.array_equal(tri, want) and np.array_equal(cnt, want_cnt)
        assert np.array_equal(inst, np.where(want >= 0, 0, -1))


def test_consequences_2_and_3_the_merged_scene_splits_and_k_is_a_prefix(lobed_positions):
    maps = set_maps(5, seed=11)
    boxes = boxes_for(lobed_positions, maps, 300, seed=12)
    full = IO.overlap_over_instances([lobed_positions], [0] * 5, maps, boxes, 64)
    for k in (1, 3, 8, 9):
        tri, inst, cnt = IO.overlap_over_instances([lobed_positions], [0] * 5, maps, boxes, k)
        assert np.array_equal(tri, full[0][:, :k]) and np.array_equal(inst, full[1][:, :k]) and np.array_equal(cnt, full[2])
    # the merged scene, split by hand: every instance has 528 triangles
    merged = np.concatenate([IP.map_corners(M, lobed_positions).reshape(-1) for M in maps])
    idx, cnt = OR.overlap(merged, boxes, 64)
    assert np.array_equal(np.where(idx >= 0, idx // 528, -1), full[1]) and np.array_equal(np.where(idx >= 0, idx % 528, -1), full[0])
    assert np.array_equal(cnt, full[2])
    key = full[1].astype(np.int64) * 528 + full[0]
    held = full[0] >= 0
    assert ((np.diff(key, axis=1) > 0) | ~held[:, 1:]).all(), "(instance, triangle) ascends over the held slots"
    assert (held[:, 1:] <= held[:, :-1]).all(), "then -1"


def test_consequence_4_a_duplicate_contributes_every_pair_again_behind_its_original(lobed_positions):
    maps = set_maps(5, seed=13)                              # map 4 is map 0
    assert np.array_equal(maps[4].view(np.uint32), maps[0].view(np.uint32))
    boxes = boxes_for(lobed_positions, maps, 300, seed=14)
    member, first = IO.membership([lobed_positions], [0] * 5, maps, boxes)
    assert np.array_equal(member[:, :528], member[:, 4 * 528:]) and member[:, :528].sum() > 1000
    tri, inst, cnt = IO.from_membership(member, first, 64)
    without = IO.overlap_over_instances([lobed_positions], [0] * 4, maps[:4], boxes, 64)
    alone = IO.overlap_over_instances([lobed_positions], [0], maps[:1], boxes, 0)
    assert np.array_equal(cnt, without[2] + alone[2])
    pairs = 0
    for j in range(len(boxes)):
        for s in np.nonzero(inst[j] == 4)[0]:
            original = np.nonzero((inst[j] == 0) & (tri[j] == tri[j, s]))[0]
            assert len(original) == 1 and original[0] < s
            pairs += 1
    assert pairs > 200


def test_consequence_5_any_is_n_above_zero(lobed_positions):
    maps = set_maps(5, seed=15)
    corners = lobed_positions.reshape(-1, 3, 3)
    boxes = boxes_for(lobed_positions, maps, 200, seed=16)
    n = IO.overlap_over_instances([lobed_positions], [0] * 5, maps, boxes, 0)[2]
    for order in (np.arange(5), np.arange(5)[::-1]):
        got = IO.restated_walk(corners, maps, boxes, order, 0, True, top_boxes=stored(corners, maps), any_only=True)
        assert np.array_equal(got[2], (n > 0).astype(np.int32))
    assert 0.1 < (n > 0).mean() < 0.95


# 4: the mutants ----------------------------------------------------------------------------------------------------------------
def vertex_face_boxes(corners, M, n, seed):
    """boxes beside a leaf of the median tree with one face exactly on the leaf's extreme world vertex coordinate, the vertex
    within the face (so the box touches its triangles and only touches the leaf's image box), and as a control the same boxes
    pushed half their size into the leaf"""
    rng = np.random.default_rng(seed)
    leaves = [nd[4] for nd in IP.median_tree(corners) if nd[4] is not None]
    extent = float(np.linalg.norm(corners.reshape(-1, 3).max(0) - corners.reshape(-1, 3).min(0)))
    lo, hi, control_lo, control_hi = (np.zeros((n, 3), F) for _ in range(4))
    for j in range(n):
        w = IP.map_corners(M, corners[leaves[rng.integers(0, len(leaves))]])
        axis, upper = int(rng.integers(0, 3)), bool(rng.integers(0, 2))
        v = w[np.argmax(w[:, axis]) if upper else np.argmin(w[:, axis])]
        half = (0.01 * extent * (1 + rng.random(3))).astype(F)
        lo[j], hi[j] = v - half, v + half
        control_lo[j], control_hi[j] = lo[j], hi[j]
        if upper:                                             # the leaf's greatest coordinate on the box's lower face
            lo[j, axis] = v[axis]
        else:
            hi[j, axis] = v[axis]
    return OR.make_boxes(lo, hi), OR.make_boxes(control_lo, control_hi)


def test_mutant_at_or_beyond_in_the_node_cull(lobed_positions):
    """<= culls a node whose image box only touches the query box: a box with a face on a leaf's extreme vertex coordinate loses
    the triangles that touch it there (under an axis-aligned scale the image box is the box of the mapped corners).  Boxes that
    reach past the vertex are the control."""
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = np.zeros((2, 3, 4), F)
    maps[0, :, :3], maps[1, :, :3] = np.diag([0.75, 1.25, 1.5]), np.diag([-1.0, 1.0, 0.5])
    maps[1, :, 3] = (6.0, 0.5, -0.25)
    on_face, control = vertex_face_boxes(corners, maps[0], 120, seed=22)
    for boxes, differs in ((on_face, True), (control, False)):
        want = IO.overlap_over_instances([lobed_positions], [0, 0], maps, boxes, 64)
        assert (want[2] > 0).all()
        right = IO.restated_walk(corners, maps, boxes, [1, 0], 64, True, top_boxes=stored(corners, maps))
        assert same(right[:3], want)
        wrong = IO.restated_walk(corners, maps, boxes, [1, 0], 64, True, top_boxes=stored(corners, maps), node_cull=IO.misses_or_touches)
        assert same(wrong[:3], want) != differs, differs


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
        boxes = boxes_for(lobed_positions, m, 160, seed=24)
        order = list(range(len(m)))[::-1]
        want = IO.overlap_over_instances([lobed_positions], [0] * len(m), m, boxes, 64)
        assert same(IO.restated_walk(corners, m, boxes, order, 64, True, top_boxes=stored(corners, m))[:3], want)
        wrong = IO.restated_walk(corners, m, boxes, order, 64, True, top_boxes=stored(corners, m), image_box=ends_by_position)
        assert same(wrong[:3], want) != differs, differs


def test_mutant_triangle_before_instance_in_the_key(lobed_positions):
    """(triangle, instance) keeps other pairs once more than K touch a box and they come from two instances.  One instance is the
    control: the two keys order its pairs alike."""
    corners = lobed_positions.reshape(-1, 3, 3)
    for n, differs in ((3, True), (1, False)):
        maps = set_maps(n, seed=25)
        if n > 1:
            maps[1] = maps[0]
            maps[1, :, 3] += F(0.05)                         # beside instance 0: most boxes hold pairs of both
        boxes = boxes_for(lobed_positions, maps, 160, seed=26)
        want = IO.overlap_over_instances([lobed_positions], [0] * n, maps, boxes, 8)
        order = list(range(n))[::-1]
        assert same(IO.restated_walk(corners, maps, boxes, order, 8, True, top_boxes=stored(corners, maps))[:3], want)
        wrong = IO.restated_walk(corners, maps, boxes, order, 8, True, top_boxes=stored(corners, maps), key=IO.key_triangle_first)
        assert np.array_equal(wrong[2], want[2]) and same(wrong[:2], want[:2]) != differs, differs


def test_mutant_the_instance_skip_reads_the_slot_before_the_kth(lobed_positions):
    """Reading slot K - 1 skips a higher instance while slot K is still empty, and loses its pairs.  K = 1 is the control: there
    is no slot before the first, so nothing is skipped early."""
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = set_maps(3, seed=27)
    maps[1], maps[2] = maps[0], maps[0]
    maps[1, :, 3] += F(0.05)
    maps[2, :, 3] -= F(0.05)
    boxes = boxes_for(lobed_positions, maps, 200, seed=28)
    order = [0, 1, 2]                                         # ascending: the lower instances' keys are held when a higher one comes
    for k, differs in ((3, True), (9, True), (1, False)):
        want = IO.overlap_over_instances([lobed_positions], [0] * 3, maps, boxes, k)
        assert same(IO.restated_walk(corners, maps, boxes, order, k, False, top_boxes=stored(corners, maps))[:2], want[:2])
        wrong = IO.restated_walk(corners, maps, boxes, order, k, False, top_boxes=stored(corners, maps), skip_slot=-1)
        assert same(wrong[:2], want[:2]) != differs, (k, differs)


def test_mutant_n_counted_only_for_kept_members(lobed_positions):
    """n is |S|, not the number of pairs that entered the K kept.  K = 64 with boxes that hold at most 64 pairs is the control."""
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = set_maps(2, seed=29)
    boxes = boxes_for(lobed_positions, maps, 200, seed=30)
    n = IO.overlap_over_instances([lobed_positions], [0, 0], maps, boxes, 0)[2]
    assert (n > 8).mean() > 0.2
    few = boxes[n <= 64]
    for bx, k, differs in ((boxes, 8, True), (few, 64, False)):
        want = IO.overlap_over_instances([lobed_positions], [0, 0], maps, bx, k)
        assert same(IO.restated_walk(corners, maps, bx, [1, 0], k, True, top_boxes=stored(corners, maps))[:3], want)
        wrong = IO.restated_walk(corners, maps, bx, [0, 1], k, True, top_boxes=stored(corners, maps), count_kept_only=True)
        assert same(wrong[:2], want[:2]) and np.array_equal(wrong[2], want[2]) != differs, differs


def point_triangle_draws(scale, draws, seed=147):
    """tests/test_instance_point_scale_reference.py's draws: one corner of magnitude about `scale` under a random row of entries
    in (-1, 1) beside two rows that keep the condition small; (M, the object corner, its fp32 world corner)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(draws):
        M = np.zeros((3, 4), F)
        M[:, :3] = (np.eye(3) + rng.uniform(-1, 1, (3, 3)) * np.array([[1.0], [0.2], [0.2]])).astype(F)
        M[0, :3] = rng.uniform(-1, 1, 3)
        if abs(np.linalg.det(M[:, :3].astype(np.float64))) < 0.2:
            continue
        v = (rng.uniform(-4, 4, 3) * scale).astype(F)
        out.append((M, v, IP.map_corners(M, v)[0]))
    return out


def test_mutant_the_subnormal_guard_removed():
    """A one-corner scene at about 2^-147: the fp32 world corner can lie outside the box the top level stores (DESIGN section
    20), so a zero-extent query box on that corner, which touches the pair, is separated from the stored box by a plain
    comparison.  With the stored box as the only top-level test, the unguarded walk loses the pair in some draw and the guarded
    walk in none.  Order-1 coordinates are the control: the stored box holds the corner and the two walks agree."""
    far = np.eye(3, 4, dtype=F)
    far[:, 3] = 8.0                                           # a second instance, elsewhere: a set of one culls nothing
    for scale, differs in ((2.0 ** -147, True), (1.0, False)):
        lost = outside = 0
        draws = point_triangle_draws(scale, 1500)
        for M, v, w in draws:
            corners = np.broadcast_to(v, (1, 3, 3)).copy()
            maps = np.stack([M, far])
            top = [IP.stored_box(M, v, v)[:2], IP.stored_box(far, v, v)[:2]]
            outside += bool(((w < top[0][0]) | (w > top[0][1])).any())
            box = OR.make_boxes(w[None], w[None])
            want = IO.overlap_over_instances([corners.reshape(-1)], [0, 0], maps, box, 1)
            assert want[2][0] >= 1 and want[1][0, 0] == 0 and want[0][0, 0] == 0, "the box on the corner touches the pair"
            guarded = IO.restated_walk(corners, maps, box, [1, 0], 1, True, top_boxes=top)
            assert same(guarded[:3], want), (M, v, w, top)
            plain = IO.restated_walk(corners, maps, box, [1, 0], 1, True, top_boxes=top, top_cull=IO.misses)
            lost += not same(plain[:3], want)
        print(f"scale {scale:g}: {outside} of {len(draws)} corners outside their stored box, the unguarded walk loses {lost} pairs")
        assert (lost > 0) == differs and (outside > 0) == differs
