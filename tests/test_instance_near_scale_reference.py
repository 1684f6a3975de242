"""The cells of tests/instance_near_scale_cases.py on the CPU, on the restatement alone (tests/instance_near_ref.py): the TABLE of
the world-scale cells; each cell's conditions (finite corners, the six shares of instance_near_cases.shares over FLOOR, the rim
pairs, count 13,152 and dist2 0 where every dist2 is 0); the small set of those two cells; the cancelling scale and the
negative zeros against their twins byte for byte; the bound property the two skips rest on, at every cell; and six mutants of
the restated walk, each of which changes an answer in a named cell and none in a named control.

Mutants (instance_near_ref.restated_walk's keywords), the cell that shows each and its control.  MEASURED on the restatement,
on the first MUTANT_POINTS = 192 points of the cell (15 rim pairs among them, 149 to 152 walked points), the instances walked
in a scrambled order, "changed" counting the points with any record, instance index or count other than the plain walk's
(which returns the brute force's bytes at every cell used here):
  a. >= in the node skip (node_skip)        K = 8 without counts.  149 (every walked point) at ("ties", -90): the reach is 0
                                            once 8 keys are held, and every bound is 0.  25 at ("world", -70).  Control: the
                                            points off every surface (kinds near and box_corner) at ("world", 0), none of 79;
                                            the whole cell is no control (5: points on a mapped corner or with radius 0 on a
                                            surface, where a bound of 0 meets a reach of 0).
  b. >= in the top-level skip (top_skip)    the same form, cells and control: 149, 17 at ("world", -70), none (3 in the whole
                                            of ("world", 0)).
  c. triangle before instance (key)         K = 1 and K = 8 without counts at ("far", 23): 20 and 56.  (41 at ("world", -70),
                                            K = 8.)  Control: ("world", 0) at K = 1, none: the only ties across instances are
                                            between a map and its exact duplicate, the same triangle, and the lower instance
                                            leads under either rule.  At K = 8 that cell is no control (16): a point nearest an
                                            edge or a corner ties on the triangles around it, in instance 1 and again in its
                                            duplicate 4, and (1, t), (1, t'), (4, t), (4, t') is not (1, t), (4, t), (1, t'), (4, t').
  d. the reach read one slot early          K = 2 without counts (the reach is then the BEST dist2, not the second): 3 at
     (reach_slot=-2)                        ("world", 40); K = 3: 4 at ("world", 0).  Few, because the nearer child is
                                            walked first and the second record mostly lies in the leaf of the first.  Control:
                                            ("ties", -90), none: either slot holds 0.  (Nor does the form with counts read
                                            the slot.)
  e. n counts only what is kept             K = 8 with counts at ("world", -70): 112.  Control: K = 64 with counts at
     (count_kept_only)                      ("world", 0), among the points whose restated count is at most 64: none of 92 (98 of the rest).
  f. < in place of <= against max_dist2     K = 8 with counts at ("world", 0): all 15 rim points whose radius is the dist2 of
     (within)                               their j-th nearest pair count fewer (and 3 points of radius 0 on a surface).
                                            At ("world", -70) 39, 7 of them neither rim nor on a surface: a radius that
                                            rounds to 0 meets a dist2 that underflows to 0.  Control: the points of
                                            ("world", 0) off every surface that are no rim points, none of 67.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import instance_near_cases as NC
import instance_near_ref as IN
import instance_near_scale_cases as NS
import instance_point_cases as IC
import instance_point_ref as IP
import instance_point_scale_cases as SC
import near_ref as NR
import point_scale_cases as PC

F = np.float32
ORDER = np.random.default_rng(9).permutation(NS.INSTANCES)[::-1]       # not the index order: the key must not lean on it
MUTANT_POINTS = 192
BOUND_POINTS = 192
OFF_SURFACE = ("near", "box_corner")
TIES = NS.ALL_ZERO[0]


@pytest.fixture(scope="module", autouse=True)
def restate_every_cell(pkg):
    """the cells and their restatements at K = 64, made once and side by side (numpy's loops release the interpreter)"""
    NS.base_points(pkg)
    NS.cell(pkg, ("world", 0))
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as pool:
        list(pool.map(lambda key: NS.restated(pkg, NS.cell(pkg, key)), NS.CELLS))


def ids(key):
    return f"{key[0]} {key[1]}"


def same_answer(a, b):
    return np.array_equal(NR.as_bits(a[0]), NR.as_bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_the_set_and_the_rim_class_are_what_the_cells_assume(pkg):
    of, maps, kinds, *_ = SC.base(pkg)
    positions = [PC.scaled_positions(pkg, name, 0) for name in NS.SCENES]
    assert sum(len(positions[s]) // 9 for s in of) == NS.TRIANGLES and len(maps) == NS.INSTANCES
    assert len(NS.TABLE) == len(SC.S_EXPONENTS) and set(NS.TABLE) <= {"c", "o"} and NS.CELLS == SC.CELLS
    assert set(NS.LOW_SHARES) <= {("far", 23)}
    assert set(NS.LOW_SHARES[("far", 23)]) <= {"count 1 to 8", "count 9 to 64", "finite radius, two or more instances held"}
    for key in NS.CELLS:
        c = NS.cell(pkg, key)
        first, second, j = c.rim.T
        assert len(c.points) == NS.POINTS and 2 * len(c.rim) * 8 >= len(c.points), f"{c}: under one point in eight is a rim point"
        assert (c.radius[first] == 1).all() and (c.radius[second] == 1).all() and len(set(first) | set(second)) == 2 * len(c.rim)
        assert [int(x) for x in j[:8]] == list(NS.RIM_J) and set(j.tolist()) == set(NS.RIM_J)
        assert np.array_equal(c.points["p"][first].view(np.uint32), c.points["p"][second].view(np.uint32))
        at, under = c.points["max_dist2"][first], c.points["max_dist2"][second]
        assert np.array_equal(under, np.nextafter(at, F(-np.inf))) and (at >= 0).all(), c      # (+inf at 2^63 and 2^64: a far point's dist2 overflows)


@pytest.mark.parametrize("key", NS.CELLS, ids=ids)
def test_a_cell_keeps_its_conditions(pkg, key):
    c = NS.cell(pkg, key)
    world = SC.world_corners(pkg, c)
    assert all(np.isfinite(w).all() for w in world), f"{c}: a mapped corner is not finite"
    records, inst, counts = NS.restated(pkg, c)
    go = NS.walked(c.points)
    assert np.array_equal(inst >= 0, records["triangle"] >= 0) and (counts[~go] == 0).all()
    assert np.array_equal((inst >= 0).sum(1), np.minimum(counts, 64))
    first, second, j = c.rim.T
    at, under = NS.rim_counts(c, counts)
    if key in NS.ALL_ZERO:
        assert go.sum() > 0.75 * len(go), c
        assert (counts[go] == NS.TRIANGLES).all() and (records["dist2"][go] == 0).all(), f"{c}: every pair of every walked point at dist2 0"
        want_inst, want_tri = NS.first_keys(pkg, c, 64)
        assert (inst[go] == want_inst).all() and (records["triangle"][go] == want_tri).all() and (want_inst == 0).all()
        for w in world:         # every dist2 of the cell is 0, not only those held
            for s in range(0, len(go), 512):
                assert (IP.pair_dist2(c.points["p"][s:s + 512][go[s:s + 512]], w)[1] == 0).all(), c
        assert (at == NS.TRIANGLES).all() and (under == 0).all() and not go[second].any()
    else:
        s = NC.shares(c.points, c.radius, records, inst, counts)
        print(f"{c}: " + ", ".join(f"{k} {v * 100:.2f} %" for k, v in s.items()))
        low = NS.LOW_SHARES.get(key, {})
        for name, share in s.items():
            if name in low:
                assert share <= NS.FLOOR, f"{c}: {name} is {share:.4f}: not low, take it out of LOW_SHARES"
                assert share >= low[name] and (share > 0) == (low[name] > 0), (c, name, share, low[name])
            else:
                assert share > NS.FLOOR, f"{c}: {name} is {share:.4f}, at or under {NS.FLOOR} (all: {s})"
        # the rim: on the dist2 of the j-th nearest pair the count is j and the pairs that tie with it; one step under, the
        # pairs strictly nearer.  The pair differs by the inclusive bound alone
        assert (at >= j).all() and (under < j).all(), c
        split = float((at != under).mean())
        print(f"{c}: {split * 100:.1f} % of {len(c.rim)} rim pairs count differently on the dist2 and one step under it")
        assert split >= NS.MIN_RIM_SPLIT, (c, split)
        held = inst >= 0
        assert len(set(inst[held].tolist())) >= 8, f"{c}: the records come from many instances"
        assert ((inst == 1).sum(1) >= (inst == 4).sum(1)).all() and (inst == 4).sum() > 100, f"{c}: the duplicate sorts behind its original"
    if key[0] == "world":
        r0, i0, n0 = NS.restated(pkg, NS.cell(pkg, ("world", 0)))
        same = PC.same_records(records, NS.scale_answer(r0, key[1], c.points)).all(1) & (inst == i0).all(1) & (counts == n0)
        print(f"{c}: {same.mean() * 100:.2f} % of the answers are the scaled k = 0 answers, {(counts == n0).mean() * 100:.2f} % of the counts")
        assert same.all() == (NS.flag(key[1]) == NS.COVARIANT), (c, float(same.mean()))
        if NS.flag(key[1]) == NS.OUTSIDE:
            assert same.mean() > 0.3, "the outside cells are not noise either"
    twin = NS.expected_cell(key)
    if twin:
        t = NS.cell(pkg, twin)
        assert same_answer((records, inst, counts), NS.restated(pkg, t)), f"{c} against {twin}"
        assert np.array_equal(NR.as_bits(c.points.view(F).reshape(-1, 8)), NR.as_bits(t.points.view(F).reshape(-1, 8))), "the rim radii are the twin's too"
        if key[0] == "cancel":      # the mapped corners themselves keep their bits
            for a, b in zip(world, SC.world_corners(pkg, t)):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        else:
            assert np.signbit(c.maps[c.maps == 0]).all() and not np.signbit(t.maps[c.maps == 0]).any()


@pytest.mark.parametrize("key", NS.ALL_ZERO, ids=ids)
def test_the_small_set_spans_five_instances_where_every_dist2_is_zero(pkg, key):
    c = NS.small_cell(pkg, key)
    assert c.names == ["one triangle", "11-triangle leaf", "one triangle", "11-triangle leaf", "lobed_528"] and c.triangles(pkg) == 552
    assert all(np.isfinite(w).all() for w in SC.world_corners(pkg, c))
    records, inst, counts = NS.restated(pkg, c)
    go = NS.walked(c.points)
    assert go.sum() > 0.75 * len(go) and (counts[go] == 552).all() and (counts[~go] == 0).all() and (records["dist2"][go] == 0).all()
    want_inst, want_tri = NS.first_keys(pkg, c, 64)
    assert (inst[go] == want_inst).all() and (records["triangle"][go] == want_tri).all()
    assert sorted(set(want_inst.tolist())) == [0, 1, 2, 3, 4] and sorted(set(want_inst[:8].tolist())) == [0, 1], "the first 64 keys span five instances, the first 8 two"
    # the restated walk carries the held keys across the instances, in a scrambled order, in both forms
    pts = c.points[:96]
    corners = [c.positions(pkg)[s].reshape(-1, 3, 3) for s in c.of]
    for k, with_counts in ((8, False), (9, False), (64, True)):
        got = IN.restated_walk(corners, c.maps, pts, [3, 0, 4, 2, 1], k, with_counts)
        assert np.array_equal(NR.as_bits(got[0]), NR.as_bits(records[:96, :k])) and np.array_equal(got[1], inst[:96, :k]), (c, k)
        assert got[2] is None or np.array_equal(got[2], counts[:96])


# 2 ---------------------------------------------------------------------------------------------------------------------------
def stored_boxes(corners, maps):
    return [IP.stored_box(maps[i], own.reshape(-1, 3).min(0), own.reshape(-1, 3).max(0))[:2] for i, own in enumerate(corners)]


def corners_of(pkg, c):
    per_scene = [p.reshape(-1, 3, 3) for p in c.positions(pkg)]
    return [per_scene[s] for s in c.of]


_trees = {}


def tree_of(own):
    if id(own) not in _trees:
        _trees[id(own)] = (own, IP.median_tree(own))
    return _trees[id(own)][1]


@pytest.mark.parametrize("key", NS.CELLS, ids=ids)
def test_no_bound_is_above_a_dist2_below_it(pkg, key):
    """What both skips rest on, whatever the reach: for every walked point of a part of the cell, every instance and every node
    of its median tree, box_bound of the node's image box is not above the dist2 of any pair below the node; and box_bound of
    the instance's stored box (place_box restated) is not above the dist2 of any pair of the instance."""
    c = NS.cell(pkg, key)
    corners = corners_of(pkg, c)
    boxes = stored_boxes(corners, c.maps)
    part = c.points[::len(c.points) // BOUND_POINTS]
    p = np.ascontiguousarray(part["p"][NS.walked(part)])
    checked = 0
    for i, own in enumerate(corners):
        tree = tree_of(own)
        M = c.maps[i]
        d2 = IP.pair_dist2(p, IP.map_corners(M, own).reshape(-1, 3, 3))[1]
        ilo, ihi = IP.image_box(M, np.stack([nd[0] for nd in tree]), np.stack([nd[1] for nd in tree]))
        lb = IP.bound(p[:, None, :], ilo[None], ihi[None])
        least = [None] * len(tree)
        for at in range(len(tree) - 1, -1, -1):         # children come after their parent
            _, _, left, right, members = tree[at]
            least[at] = d2[:, members].min(1) if members is not None else np.minimum(least[left], least[right])
        bad = lb > np.stack(least, axis=1)
        assert not bad.any(), f"{c}: instance {i}, nodes {np.nonzero(bad.any(0))[0][:5]}: an image-box bound above a dist2 below it"
        assert not (IP.bound(p, *boxes[i]) > least[0]).any(), f"{c}: instance {i}: the stored box's bound above a dist2 of the instance"
        checked += bad.size
    assert len(p) > 0.7 * BOUND_POINTS and checked > 100000


# 3 ---------------------------------------------------------------------------------------------------------------------------
def at_or_above(lb, reach):
    return lb >= reach


MUTANTS = {
    "a. >= in the node skip": dict(node_skip=at_or_above),
    "b. >= in the top-level skip": dict(top_skip=at_or_above),
    "c. triangle before instance": dict(key=lambda d, i, t: (d, t, i)),
    "d. the reach read one slot early": dict(reach_slot=-2),
    "e. n counts only what is kept": dict(count_kept_only=True),
    "f. < against max_dist2": dict(within=lambda d, max_dist2: d < max_dist2),
}
_prepared = {}


def prepared(pkg, key):
    if key not in _prepared:
        c = NS.cell(pkg, key)
        corners = corners_of(pkg, c)
        top = stored_boxes(corners, c.maps)
        pts = c.points[:MUTANT_POINTS]
        _prepared[key] = (c, corners, top, pts, IN.prepare(corners, c.maps, pts, top))
    return _prepared[key]


def walk(pkg, key, k, counts, mutant=None):
    c, corners, top, pts, prep = prepared(pkg, key)
    return IN.restated_walk(corners, c.maps, pts, ORDER, k, counts, top_boxes=top, prepared=prep, **(MUTANTS[mutant] if mutant else {}))


def changed(a, b):
    """bool per point: any record, instance index or count differs"""
    d = (a[1] != b[1]).any(1) | (NR.as_bits(a[0]) != NR.as_bits(b[0])).any(1).reshape(a[1].shape).any(1)
    return d if a[2] is None else d | (a[2] != b[2])


def plain(pkg, key, k, counts):
    """the unmutated walk, which must be the brute force, byte for byte"""
    c = NS.cell(pkg, key)
    got = walk(pkg, key, k, counts)
    want = NS.restated(pkg, c)
    assert np.array_equal(NR.as_bits(got[0]), NR.as_bits(want[0][:MUTANT_POINTS, :k])) and np.array_equal(got[1], want[1][:MUTANT_POINTS, :k]), (c, k)
    assert got[2] is None or np.array_equal(got[2], want[2][:MUTANT_POINTS]), (c, k)
    return got


def part_of(pkg, key, off_surface=False, rim=None):
    c = NS.cell(pkg, key)
    sel = np.ones(MUTANT_POINTS, bool)
    if off_surface:
        sel &= np.isin(c.kind[:MUTANT_POINTS], [IC.KINDS.index(k) for k in OFF_SURFACE])
    if rim is not None:
        is_rim = np.zeros(len(c.points), bool)
        is_rim[c.rim[:, :2].reshape(-1)] = True
        sel &= is_rim[:MUTANT_POINTS] == rim
    return sel


@pytest.mark.parametrize("mutant", ["a. >= in the node skip", "b. >= in the top-level skip"])
def test_mutant_a_skip_at_equality_culls_where_every_bound_meets_the_reach(pkg, mutant):
    n = changed(walk(pkg, TIES, 8, False, mutant), plain(pkg, TIES, 8, False))
    go = NS.walked(NS.cell(pkg, TIES).points[:MUTANT_POINTS])
    print(f"{mutant}: {int(n.sum())} of {int(go.sum())} walked points change at ties -90")
    assert np.array_equal(n, go), "every walked point loses its answer"
    n = changed(walk(pkg, ("world", -70), 8, False, mutant), plain(pkg, ("world", -70), 8, False))
    print(f"{mutant}: {int(n.sum())} points change at world -70")
    assert n.sum() >= 10
    n = changed(walk(pkg, ("world", 0), 8, False, mutant), plain(pkg, ("world", 0), 8, False))
    off = part_of(pkg, ("world", 0), off_surface=True)
    print(f"{mutant}: {int(n.sum())} points change at world 0, {int(n[off].sum())} of the {int(off.sum())} off every surface")
    assert off.sum() > 60 and n.any() and not n[off].any()


def test_mutant_the_tie_by_triangle_before_instance(pkg):
    mutant = "c. triangle before instance"
    for k in (1, 8):
        n = changed(walk(pkg, ("far", 23), k, False, mutant), plain(pkg, ("far", 23), k, False))
        print(f"{mutant}: K = {k}: {int(n.sum())} points change at far 23")
        assert n.sum() >= 10
    n = changed(walk(pkg, ("world", 0), 1, False, mutant), plain(pkg, ("world", 0), 1, False))
    assert not n.any(), f"{mutant}: {int(n.sum())} points change at its control"
    n = changed(walk(pkg, ("world", 0), 8, False, mutant), plain(pkg, ("world", 0), 8, False))
    print(f"{mutant}: K = 8: {int(n.sum())} points change at world 0 (module doc)")


def test_mutant_the_reach_read_one_slot_early(pkg):
    mutant = "d. the reach read one slot early"
    for key, k in SLOT_SHOWS:
        n = changed(walk(pkg, key, k, False, mutant), plain(pkg, key, k, False))
        print(f"{mutant}: K = {k}: {int(n.sum())} points change at {key}")
        assert n.sum() >= 2
    n = changed(walk(pkg, TIES, 2, False, mutant), plain(pkg, TIES, 2, False))
    assert not n.any(), f"{mutant}: {int(n.sum())} points change at its control"
    n = changed(walk(pkg, ("world", 40), 2, True, mutant), plain(pkg, ("world", 40), 2, True))
    assert not n.any(), "the form with counts never reads the slot"


SLOT_SHOWS = ((("world", 40), 2), (("world", 0), 3))


def test_mutant_n_counted_only_for_kept_records(pkg):
    mutant = "e. n counts only what is kept"
    base = plain(pkg, ("world", -70), 8, True)
    got = walk(pkg, ("world", -70), 8, True, mutant)
    n = changed(got, base)
    print(f"{mutant}: K = 8: {int(n.sum())} points change at world -70")
    assert not n[base[2] <= 8].any() and n.sum() > 80 and (got[2] <= base[2]).all() and not changed((got[0], got[1], None), (base[0], base[1], None)).any()
    base = plain(pkg, ("world", 0), 64, True)
    n = changed(walk(pkg, ("world", 0), 64, True, mutant), base)
    few = base[2] <= 64
    print(f"{mutant}: K = 64: {int(n.sum())} points change at world 0, {int(n[few].sum())} of the {int(few.sum())} that count at most 64")
    assert few.sum() > 60 and n.any() and not n[few].any()


def test_mutant_the_exclusive_bound_against_max_dist2(pkg):
    mutant = "f. < against max_dist2"
    c = NS.cell(pkg, ("world", 0))
    base = plain(pkg, ("world", 0), 8, True)
    got = walk(pkg, ("world", 0), 8, True, mutant)
    n = changed(got, base)
    first = c.rim[:, 0][c.rim[:, 0] < MUTANT_POINTS]
    print(f"{mutant}: {int(n.sum())} points change at world 0, {int(n[first].sum())} of the {len(first)} rim points on a dist2")
    assert len(first) >= 10 and n[first].all() and (got[2][first] < base[2][first]).all(), "every rim point on a pair's dist2 counts fewer"
    second = c.rim[:, 1][c.rim[:, 1] < MUTANT_POINTS]
    assert np.array_equal(got[2][first[:len(second)]], base[2][second]), "the mutant counts on the dist2 what is counted one step under it"
    control = part_of(pkg, ("world", 0), off_surface=True, rim=False)
    print(f"{mutant}: {int(n[control].sum())} of the {int(control.sum())} points of world 0 off every surface that are no rim points change")
    assert control.sum() > 60 and not n[control].any(), f"{mutant}: {int(n[control].sum())} points change in its control"
    n = changed(walk(pkg, ("world", -70), 8, True, mutant), plain(pkg, ("world", -70), 8, True))
    control = part_of(pkg, ("world", -70), off_surface=True, rim=False)
    print(f"{mutant}: {int(n.sum())} points change at world -70, {int(n[control].sum())} of them off every surface and no rim points")
    assert n[control].any(), "a radius that rounds to 0 meets a dist2 that underflows to 0"
