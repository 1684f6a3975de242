"""The CPU side of the instance-pair collision matrix (include/shader_ray_instance_pairs.h), on
tests/instance_pairs_ref.py: the nine-instance set's count matrix, cell for cell; the header's nine consequences on the brute
force; the restatement of the kernel's scheme (64-triangle workgroups per instance, cells shared between them, the two skips)
equal to the brute force in the three modes under scrambled workgroup orders; and six mutants of the scheme, each changing an
answer on a named input."""
import os

import numpy as np
import pytest

import instance_intersect_cases as XC
import instance_intersect_ref as II
import instance_pairs_ref as PR
import instance_point_cases as IC

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the ordered pairs (row, column) of the nine-instance set that have members, and how many
NINE_COUNTS = {(0, 6): 488, (0, 8): 136, (1, 4): 7488, (2, 8): 26, (3, 8): 56, (4, 1): 7488, (6, 0): 487, (6, 8): 124, (7, 8): 2,
               (8, 0): 136, (8, 2): 26, (8, 3): 56, (8, 6): 124, (8, 7): 2}


@pytest.fixture(scope="module")
def nine(pkg):
    """(positions, scene of every instance, maps, blocks, walked, the brute force (first, counts))"""
    world = pkg.World(os.path.join(GOLDEN, "lobed_528.trisrc"))
    try:
        lobed = np.asarray(world.arrays()["vertex_positions"], F).copy()
    finally:
        world.close()
    tiny = {name: np.asarray(tris, F).reshape(-1) for name, tris in IC.TINY.items()}
    positions, of, maps, kinds, names = XC.nine_instances(lambda name: lobed if name == "lobed_528" else tiny[name])
    assert kinds[4] == "duplicate of 1"
    blocks, walked = PR.memberships(positions, of, maps)
    return positions, of, maps, blocks, walked, PR.brute(blocks)


def orders(count):
    """scrambled workgroup orders: the grid's, its reverse, and two seeded permutations"""
    return [None, list(range(count - 1, -1, -1))] + [np.random.default_rng(seed).permutation(count).tolist() for seed in (5, 6)]


def same(got, want):
    return all((g is None and w is None) or (g is not None and w is not None and np.array_equal(g, w)) for g, w in zip(got, want))


def wanted(brute, mode):
    first, counts = brute
    return {PR.ANY: (None, (counts > 0).astype(np.int64)), PR.FIRST_ONLY: (first, None), PR.COUNTS: (first, counts)}[mode]


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_the_count_matrix_of_the_nine_instance_set(nine):
    """Fourteen of the 72 off-diagonal cells are set, with these counts; row and column 5 are empty; the keys are the brute
    force's smallest (ta, tb) and name a member."""
    positions, of, maps, blocks, walked, (first, counts) = nine
    want = np.zeros((9, 9), np.int64)
    for (a, b), c in NINE_COUNTS.items():
        want[a, b] = c
    assert np.array_equal(counts, want), np.argwhere(counts != want)
    assert not counts[5].any() and not counts[:, 5].any() and (counts > 0).sum() == 14
    ta, tb = PR.split_keys(first)
    assert np.array_equal(ta >= 0, counts > 0) and np.array_equal(tb >= 0, counts > 0) and np.array_equal(first == PR.NONE, counts == 0)
    for a, b in NINE_COUNTS:
        block = blocks[a][b]
        assert block[ta[a, b], tb[a, b]] and not block[:ta[a, b]].any() and not block[ta[a, b], :tb[a, b]].any()


@pytest.mark.parametrize("skip_shared", [False, True])
def test_the_torch_pair_test_is_numpys(nine, skip_shared):
    """instance_pairs_ref.intersects_torch (what the larger GPU tests brute-force with) against intersect_ref.intersects, on
    torch's CPU device: every block of the nine-instance set; SKIP_SHARED empties the twins' two cells and no other"""
    pytest.importorskip("torch")
    positions, of, maps, blocks, walked, _ = nine
    plain = blocks if not skip_shared else PR.memberships(positions, of, maps, True)[0]
    got, got_walked = PR.memberships(positions, of, maps, skip_shared, device="cpu")
    for a in range(9):
        assert np.array_equal(got_walked[a], walked[a])
        for b in range(9):
            assert np.array_equal(got[a][b], plain[a][b]), (a, b)
    if skip_shared:
        assert plain[1][4].sum() == 0 and blocks[1][4].sum() == 7488, "the twins' pairs are a triangle with itself or a neighbour"
        assert plain[0][6].sum() == blocks[0][6].sum() == 488, "parts in general position share no corner"


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_the_nine_consequences(nine):
    positions, of, maps, blocks, walked, (first, counts) = nine
    n = 9
    for a in range(n):
        member, start = II.own_membership(positions, of, maps, a, skip_own=True)
        for b in range(n):
            cols = member[:, start[b]:start[b + 1]]
            assert counts[a, b] == cols.sum(), "1: the instance form's membership summed over b's columns"
            where = np.argwhere(cols)
            want = PR.NONE if len(where) == 0 else np.uint64((int(where[0][0]) << 32) | int(where[0][1]))
            assert first[a, b] == want, "2: its smallest (row, column) in row-major order"
    any_counts = PR.restated_pairs(blocks, walked, PR.ANY)[1]
    assert np.array_equal(any_counts != 0, counts > 0) and set(np.unique(any_counts).tolist()) == {0, 1}, "3: ANY equals counts > 0"
    assert (np.diag(counts) == 0).all() and (np.diag(first) == PR.NONE).all(), "4: the diagonal is none / 0"
    u_first, u_counts = PR.brute(blocks, upper=True)
    keep = np.triu(np.ones((n, n), bool), 1)
    assert np.array_equal(u_counts, np.where(keep, counts, 0)) and np.array_equal(u_first, np.where(keep, first, PR.NONE)), "5: UPPER"
    assert same(PR.restated_pairs(blocks, walked, PR.COUNTS, upper=True), (u_first, u_counts))
    for rows in (range(0, 1), range(4, 9), range(8, 9), range(3, 3)):
        part = PR.brute(blocks, rows)
        assert np.array_equal(part[0], first[rows.start:rows.stop]) and np.array_equal(part[1], counts[rows.start:rows.stop]), "6: a sub-range"
        assert same(PR.restated_pairs(blocks, walked, PR.COUNTS, rows=rows), part)
    assert np.array_equal(counts.any(axis=1), II.colliding(positions, of, maps)), "7: a row has a member iff the instance collides"
    assert counts.any(axis=1).tolist() == [a != 5 for a in range(n)]
    assert counts[1, 4] == counts[4, 1] == 7488 and of[1] == of[4], "8: the duplicate meets its twin both ways"
    assert counts[0, 6] == 488 and counts[6, 0] == 487, "9: the matrix need not be symmetric"
    assert np.array_equal(counts > 0, (counts > 0).T), "(on this set the booleans are symmetric)"


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", PR.MODES)
def test_the_restated_scheme_equals_the_brute_force_under_any_workgroup_order(nine, mode):
    positions, of, maps, blocks, walked, brute = nine
    groups = PR.workgroups(blocks, range(9))
    assert len(groups) == 7 * 9 + 2 and groups[9] == (1, 1, 0) and groups[-1] == (8, 8, 0), "528 triangles are nine workgroups, a tiny scene one"
    culls = PR.top_culls(positions, of, maps, PR.stored_boxes_of(positions, of, maps))
    assert any(c.any() for row in culls for c in row) and not all(c.all() for row in culls for c in row), "the top level culls some lanes"
    for order in orders(len(groups)):
        assert same(PR.restated_pairs(blocks, walked, mode, order), wanted(brute, mode)), (mode, order)
        assert same(PR.restated_pairs(blocks, walked, mode, order, top_culled=culls), wanted(brute, mode)), (mode, "with the top level", order)


@pytest.mark.parametrize("name", ["one_branch", "lobed_528"])
def test_the_sparse_brute_force_and_the_walk_without_a_table_are_the_dense_ones(pkg, nine, name):
    """What tests/test_gpu_instance_pairs_tree_shapes.py compares the larger shapes with, on trees small enough for the dense
    forms (a hand-shaped tree placed twice as that test places it, and lobed_528's own tree under the nine-instance set's maps
    0 and 6): member_pairs' cells are brute()'s, pair_walk_counters is instance_intersect_ref.walk_counters summed, and the two
    placements do interpenetrate."""
    pytest.importorskip("torch")
    import refit_ref
    import tree_shapes as T
    from test_gpu_instance_pairs_tree_shapes import brute_of_two, placed_twice
    if name == "lobed_528":
        world = pkg.World(os.path.join(GOLDEN, "lobed_528.trisrc"))
        try:
            tree = refit_ref.TreeArrays.of(world.export_tree())
        finally:
            world.close()
        corners = nine[0][0].reshape(-1, 3, 3)              # (the scene's triangles are in the tree's order)
        positions, maps = nine[0][0], nine[2][[0, 6]]
    else:
        tree, vd = T.build(name)
        corners = np.ascontiguousarray(vd[tree.triangle_vertices][:, :, :3])
        positions = corners.reshape(-1)
        maps = placed_twice(name, positions)
    sparse, world = brute_of_two(positions, maps, device="cpu")
    dense = PR.brute(PR.memberships([positions], [0, 0], maps)[0])
    assert np.array_equal(sparse[0], dense[0]) and np.array_equal(sparse[1], dense[1])
    assert dense[1][0, 1] > 0 and dense[1][1, 0] > 0
    stored = PR.stored_boxes_of([positions], [0, 0], maps)
    for a, b in ((0, 1), (1, 0)):
        got, go = PR.pair_walk_counters(tree, tree.box, world[b], maps[b], world[a], stored[b])
        want = II.walk_counters(tree, tree.box, corners, maps[b], world[a], top_box=stored[b])
        assert got == {c: int(want[c].sum()) for c in PR.COUNTERS} and np.array_equal(go, want["traversals"] == 1)


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_mutants_of_the_scheme_change_an_answer(nine):
    positions, of, maps, blocks, walked, brute = nine
    first, counts = brute
    groups = PR.workgroups(blocks, range(9))
    reverse = list(range(len(groups) - 1, -1, -1))

    # the ANY skip reading the transposed cell: in grid order row 0 sets (0, 6), and row 6 then skips instance 0
    got = PR.restated_pairs(blocks, walked, PR.ANY, any_cell=lambda c, r, a, b, first_row: c[b - first_row, a])[1]
    assert got[0, 6] == 1 and got[6, 0] == 0 and counts[6, 0] == 487

    # the key with tb before ta: the minimum is another pair wherever the smallest ta does not hold the smallest tb
    got = PR.restated_pairs(blocks, walked, PR.COUNTS, key=PR.key_tb_first)[0]
    assert np.array_equal(got == PR.NONE, first == PR.NONE)
    tb_led, ta_led = PR.split_keys(got)       # (the mutant's key read as it was packed)
    ta, tb = PR.split_keys(first)
    differ = sorted(map(tuple, np.argwhere((ta_led != ta) | (tb_led != tb)).tolist()))
    print("the pair with the smallest tb is not the pair with the smallest ta in cells", differ)
    assert (1, 4) not in differ and (0, 6) in differ, "the twins meet first in (0, 0) either way; instances 0 and 6 do not"
    # ... and the first-only skip then compares a scene triangle with the lane's query triangle: in reverse order the later
    # workgroups' keys keep the earlier ones out, and the cell is not even the mutant key's minimum
    lost = PR.restated_pairs(blocks, walked, PR.FIRST_ONLY, reverse, key=PR.key_tb_first)[0]
    assert (lost != got).any()

    # "own" judged by the scene: the duplicate's twin, and every other copy of lobed_528, is never met
    got = PR.restated_pairs(blocks, walked, PR.COUNTS, scene_of=of, own_is=lambda b, a, scene_of: scene_of[b] == scene_of[a])[1]
    assert got[1, 4] == 0 and got[4, 1] == 0 and got[0, 6] == 0 and got[0, 8] == counts[0, 8]

    # UPPER as b >= a: nothing changes off the diagonal, so the input is a set whose diagonal has members -- the plain
    # membership, own pairs included (every triangle meets itself)
    full = [[b.copy() for b in row] for row in blocks]
    for a in range(9):
        member, start = II.own_membership(positions, of, maps, a, skip_own=False)
        full[a][a] = member[:, start[a]:start[a + 1]]
    assert full[0][0].trace() == 528
    got = PR.restated_pairs(full, walked, PR.COUNTS, upper=True, upper_skips=lambda b, a: b < a)[1]
    assert got[0, 0] == 0, "(own is skipped before UPPER is asked)"
    got = PR.restated_pairs(full, walked, PR.COUNTS, upper=True, upper_skips=lambda b, a: b < a, own_is=lambda b, a, s: False)[1]
    assert got[0, 0] >= 528

    # the diagonal walked: every non-degenerate triangle finds itself
    got = PR.restated_pairs(full, walked, PR.COUNTS, own_is=lambda b, a, s: False)
    assert got[1][5, 5] >= 528 and got[0][5, 5] == 0 and counts[5, 5] == 0

    # the count added only when the minimum moved: in grid order the later workgroups of a row never lower the key
    got = PR.restated_pairs(blocks, walked, PR.COUNTS, add_always=False)
    assert np.array_equal(got[0], first) and got[1][1, 4] < 7488 and got[1][7, 8] == 2
    # ... and in reverse order every workgroup lowers it: that order alone does not catch the mutant
    assert same(PR.restated_pairs(blocks, walked, PR.COUNTS, reverse, add_always=False), brute)
