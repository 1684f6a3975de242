"""The cells of tests/instance_overlap_scale_cases.py on the CPU, on the restatement alone (tests/instance_overlap_ref.py): each
cell's conditions (finite corners, or the NaN and infinity counts of the NaN-corner cell; the six shares of
instance_overlap_cases.shares over FLOOR or at their LOW_SHARES bound; the later axes; the TABLE of the world-scale cells; the
cancelling scale and the negative zeros against their twins byte for byte); the restated walk (image boxes, stored boxes as the
top level, a scrambled instance order) against the brute force, index for index, at every cell; the guard's two neighbours on
the guard cells; the draws at 2^-147; and the mutants below, each of which changes an answer in a named cell and none in a
named control.

Mutants.  MEASURED on the restatement; "boxes" counts the boxes with any index, instance index or count other than the header's.
The arithmetic mutants (a to e) are judged on the brute force over all 1,536 boxes of a cell (a mutant of the corner formula
moves the merged scene itself); the walk's mutants (f to l) on the first WALK_BOXES = 192 boxes, the instances walked in a
scrambled order, against the plain walk, which returns the brute force's answer at every cell.
  a. fmin / fmax in min3 / max3             125 boxes at ("world", 100) (an edge product overflows, a projection is inf - inf), all
                                            1,465 walked boxes at the NaN-corner cell (190,450 pairs lost).  Control ("world", 0): 0.
  b. a NaN image end culls                  (the node test written hi >= lo && lo <= hi) every one of the 185 walked boxes at the
                                            NaN-corner cell.  Control ("world", 64): 0.
  c. a fused corner formula                 87 at ("ill", 20), 13 at ("world", 0), 1,465 at the NaN-corner cell.  Control
                                            ("negzero", 0), of order 1: 0 (each row has one nonzero entry, +-1 in the permutations
                                            and flips: nothing to fuse).  The far cells show nothing either: the translation is
                                            added unfused.
  d. subnormal results flushed              1,298 at ("subnormal", -70), 4 at ("ties", -90).  Control ("world", 0): 0.
  e. the zero entries' products added       changes no answer at any cell (asserted at ("world", 0), ("negzero", 1),
                                            ("subnormal", -70) and the NaN-corner cell): every object coordinate is finite, so a zero
                                            entry's product is +-0, and adding it moves at most the sign of a zero sum, which no
                                            comparison reads.  No GPU test can see this one either.
  f. image ends chosen without the sign     127 at ("ill", 12).  Control, the negative-zero cells: a -0 entry taken for negative
                                            (the sign bit in place of `< 0`) changes nothing at either, since a zero entry is not
                                            read whichever end is chosen.  (The mutant itself changes 66 boxes at ("negzero", 1): its
                                            flips and permutations have entries of -1.)
  g. the guard removed                      a pair lost in each of the 48 boxes of ("draws", -147).  Control ("world", 0): 0.
  h, i. the guard at 2^-110, at 2^-108      no answer changes; the instance walks (the kernel's `traversals` counter) do:
                                            instance_overlap_scale_cases.GUARD_DECISIONS.  Control ("world", -40): 0.
  k. triangle before instance in the key    K = 8 without counts: 13 at ("far", 23).  Control: the 96 boxes of ("world", 0) whose
                                            pairs are all held and of one instance: 0.
  l. the skip slot read one early           ascending instance order, without counts: 4 at ("world", 0), K = 9; 2 at ("ill", 12)
                                            and 1 at ("far", 12), K = 8; 0 at ("far", 23): the far cells do not favour it (a
                                            box there that holds K - 1 pairs of an instance nearly always holds K).  Controls:
                                            K = 1, and the form with counts: 0.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import instance_overlap_cases as XC
import instance_overlap_ref as IO
import instance_overlap_scale_cases as XS
import instance_point_ref as IP
import instance_point_scale_cases as SC
import overlap_ref as OR
from test_instance_overlap_reference import ends_by_position
from test_overlap_scale_reference import Arith, flush, fused_sub
from test_overlap_scale_reference import restate as arith_restate

F = np.float32
ORDER = np.random.default_rng(9).permutation(XS.INSTANCES)[::-1]       # not the index order: the key must not lean on it
WALK_BOXES = 192
WALK_KS = (1, 8, 9, 64)
_axes = {}


def ids(key):
    return f"{key[0]} {key[1]}"


def answer(pkg, key):
    """the restatement at K = 64 and the pairs each later axis separates first, once per cell"""
    c = XS.cell(pkg, key)
    if key not in _axes:
        merged, first = IP.merged_positions(c.positions(pkg), c.of, c.maps)
        code = OR.first_axis(merged, c.boxes)
        XS._memo[("restated", key)] = IO.from_membership(code == OR.OVERLAP, first, 64)
        _axes[key] = np.bincount(code[(code >= 0) & (code < OR.AXES)].astype(np.int64), minlength=OR.AXES)
    return XS.restated(pkg, c)


@pytest.fixture(scope="module", autouse=True)
def restate_every_cell(pkg):
    """the cells and their restatements at K = 64, made once and side by side (numpy's loops release the interpreter)"""
    XS.base_boxes(pkg)
    XS.cell(pkg, ("world", 0))
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as pool:
        list(pool.map(lambda key: answer(pkg, key), XS.CELLS))


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def changed(a, b):
    """bool per box: any index, instance index or count differs"""
    d = (a[0] != b[0]).any(1) | (a[1] != b[1]).any(1)
    return d if a[2] is None else d | (a[2] != b[2])


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_the_cells_are_what_the_files_say(pkg):
    of, maps, *_ = SC.base(pkg)
    assert sum(len(XS.unscaled(pkg)[s]) // 9 for s in of) == XS.TRIANGLES and len(maps) == XS.INSTANCES
    assert len(XS.TABLE) == len(SC.S_EXPONENTS) and set(XS.TABLE) <= {"k", "c"}
    assert XS.CELLS[:len(SC.CELLS)] == SC.CELLS and len(XS.base_boxes(pkg)) == XS.BOXES == 1536
    assert set(XS.LOW_SHARES) == {("far", 20), ("far", 23), XS.NAN_CELL} and set(XS.SHARE_COUNTS) == set(XS.CELLS)
    assert set(XS.KEPT_COUNTS) == {("world", k) for k in SC.S_EXPONENTS + (XS.FMIN_WORLD,)} | set(XS.ALL_ZERO)
    for key in XS.CELLS:
        c = XS.cell(pkg, key)
        assert len(c.boxes) == XS.BOXES and c.boxes.dtype == OR.BOX_DTYPE
        assert c.grid.any() == (key[0] in ("far", "ill")), c
        assert np.isfinite(c.maps).all(), f"{c}: every map is finite"
        if key != XS.NAN_CELL:
            assert np.array_equal(OR.walked(c.boxes), OR.walked(XS.base_boxes(pkg))) or key[0] in ("far", "ill", "negzero"), c
        else:
            base = XS.base_boxes(pkg)
            go = OR.walked(base)
            assert np.array_equal(OR.walked(c.boxes), go), "clipping to FLT_MAX keeps the walked boxes walked, the others as they were"
            assert np.array_equal(c.boxes[~go].view(np.uint32), base[~go].view(np.uint32))
            assert np.isfinite(c.boxes["lo"][go]).all() and np.isfinite(c.boxes["hi"][go]).all()
            assert (np.abs(c.boxes["hi"][go]) == XS.FLT_MAX).any(), "some ends are clipped"


@pytest.mark.parametrize("key", XS.CELLS, ids=ids)
def test_a_cell_keeps_its_conditions(pkg, key):
    c = XS.cell(pkg, key)
    world = XS.world_corners(pkg, c)
    tri, inst, n = answer(pkg, key)
    go = OR.walked(c.boxes)
    assert (n[~go] == 0).all() and np.array_equal((inst >= 0).sum(1), np.minimum(n, 64)) and np.array_equal(inst >= 0, tri >= 0)
    if key == XS.NAN_CELL:
        nan = [int(np.isnan(w).any(2).any(1).sum()) for w in world]
        inf = [int(np.isinf(w).any(2).any(1).sum()) for w in world]
        print(f"{c}: triangles with a NaN corner per instance {nan}, with an infinite corner {inf}")
        assert nan == XS.NAN_TRIANGLES and inf == XS.INF_TRIANGLES
        assert sum(x > 0 for x in nan) >= 2, "NaN corners in two or more instances"
        merged, _ = IP.merged_positions(c.positions(pkg), c.of, c.maps)
        member = OR.overlaps(merged, c.boxes)
        with_nan = np.isnan(merged.reshape(-1, 9)).any(1)
        pairs, holding = int(member[:, with_nan].sum()), int(member[:, with_nan].any(1).sum())
        print(f"{c}: {pairs} member pairs with a NaN corner, in {holding} of the {int(go.sum())} walked boxes")
        assert pairs == XS.NAN_MEMBER_PAIRS and holding == int(go.sum()) == XS.NAN_WALKED
    else:
        assert all(np.isfinite(w).all() for w in world), f"{c}: a mapped corner is not finite"
    s = XC.shares(c.boxes, inst, n)
    print(f"{c}: " + ", ".join(f"{k} {v * 100:.2f} %" for k, v in s.items()) + f"; first to separate, per axis {_axes[key].tolist()}")
    counts = tuple(int(round(v * len(c.boxes))) for v in s.values())
    assert counts == XS.SHARE_COUNTS[key], f"{c}: the six shares, in boxes of {len(c.boxes)}: {counts}, the case file says {XS.SHARE_COUNTS[key]}"
    low = XS.LOW_SHARES.get(key, {})
    for name, share in s.items():
        if name in low:
            assert share <= XS.FLOOR, f"{c}: {name} is {share:.4f}: not low, take it out of LOW_SHARES"
            assert share >= low[name] and (share > 0) == (low[name] > 0), (c, name, share, low[name])
        else:
            assert share > XS.FLOOR, f"{c}: {name} is {share:.4f}, at or under {XS.FLOOR} (all: {s})"
    if key in XS.LATER_AXES_SEPARATE:
        assert min(_axes[key][3:]) >= 1, (c, _axes[key].tolist())
    if key in XS.ALL_ZERO:
        assert (n[go] > 64).mean() > 0.3, f"{c}: the underflowed world still answers richly"
        assert _axes[key][3:].sum() == 0, f"{c}: every later product is 0: the set is stage 0's"
    if key in XS.KEPT_COUNTS:
        t0, i0, n0 = answer(pkg, ("world", 0))
        kept = (tri == t0).all(1) & (inst == i0).all(1) & (n == n0)
        print(f"{c}: {int(kept.sum())} boxes ({kept.mean() * 100:.2f} %) keep their k = 0 answer")
        assert int(kept.sum()) == XS.KEPT_COUNTS[key], (c, int(kept.sum()))
        if key[0] == "world" and key[1] in SC.S_EXPONENTS:
            assert kept.all() == (XS.flag(key[1]) == XS.KEPT), (c, float(kept.mean()))
        assert kept.mean() > 0.3, "the changed cells are not noise either"
    twin = XS.expected_cell(key)
    if twin:
        t = XS.cell(pkg, twin)
        assert same((tri, inst, n), answer(pkg, twin)), f"{c} against {twin}"
        assert np.array_equal(c.boxes.view(np.uint32), t.boxes.view(np.uint32)), "the boxes are the twin's too"
        if key[0] == "cancel":      # the mapped corners themselves keep their bits
            for a, b in zip(world, XS.world_corners(pkg, t)):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        else:
            assert np.signbit(c.maps[c.maps == 0]).all() and not np.signbit(t.maps[c.maps == 0]).any()


# 2 ---------------------------------------------------------------------------------------------------------------------------
_prepared = {}


def prepared(pkg, key):
    if key not in _prepared:
        c = XS.cell(pkg, key)
        per_scene = [p.reshape(-1, 3, 3) for p in c.positions(pkg)]
        _prepared[key] = (c, [per_scene[s] for s in c.of], XS.stored_boxes(pkg, c))
    return _prepared[key]


def walk(pkg, cell_key, k, counts, order=ORDER, **mutant):
    c, corners, top = prepared(pkg, cell_key)
    with np.errstate(all="ignore"):
        return IO.restated_walk(corners, c.maps, c.boxes[:WALK_BOXES], order, k, counts, top_boxes=top, **mutant)


def brute(pkg, key, k, counts):
    tri, inst, n = answer(pkg, key)
    return tri[:WALK_BOXES, :k], inst[:WALK_BOXES, :k], (n[:WALK_BOXES] if counts else None)


@pytest.mark.parametrize("key", XS.CELLS, ids=ids)
def test_the_restated_walk_returns_the_brute_force_indices(pkg, key):
    """What both culls rest on: with the image boxes as the nodes' boxes and instance_point_ref.stored_box as the top level the
    walk loses no pair, at any scale: it fails if an image box or a stored box stops holding its corners."""
    for k in WALK_KS:
        for counts in (True, False):
            got = walk(pkg, key, k, counts)
            assert same(got[:3], brute(pkg, key, k, counts)), (key, k, counts)
    n = answer(pkg, key)[2][:WALK_BOXES]
    assert np.array_equal(walk(pkg, key, 0, True, any_only=True)[2], (n > 0).astype(np.int32)), (key, "ANY is n > 0")


# 3: the guard ------------------------------------------------------------------------------------------------------------------
def top_level_misses(pkg, key, guard):
    """bool [walked boxes, instances]: the top level separates the instance's stored box from the box"""
    c, _, top = prepared(pkg, key)
    lo, hi = OR.lo_hi(c.boxes)
    go = OR.walked(c.boxes)
    return np.stack([IO.guarded_misses(t[0][None], t[1][None], lo, hi, guard=F(2.0 ** guard)) for t in top], 1)[go]


@pytest.mark.parametrize("key", XS.GUARD_CELLS + [("world", -40)], ids=ids)
def test_the_guard_s_neighbours_begin_other_walks(pkg, key):
    """The (box, instance) decisions of the top level that a guard of 2^-110 or of 2^-108 takes otherwise than 2^-109, over all
    the walked boxes, and the instance walks of the restated walk on the first WALK_BOXES boxes (the kernel's `traversals`
    counter): XS.GUARD_DECISIONS.  A greater guard culls less, so every differing decision is one walk more or less, and the
    counter tells the neighbours apart wherever a decision differs.  ("world", -40) is the control: no end is near the guard."""
    at = {g: top_level_misses(pkg, key, g) for g in (-110, -109, -108)}
    assert not (at[-109] & ~at[-110]).any() and not (at[-108] & ~at[-109]).any(), "a greater guard culls less"
    below, above = int((at[-110] != at[-109]).sum()), int((at[-108] != at[-109]).sum())
    walks = {g: walk(pkg, key, 1, True, top_cull=lambda *a, g=g: IO.guarded_misses(*a, guard=F(2.0 ** g)))[4] for g in (-110, -109, -108)}
    print(f"{key}: decisions that differ from 2^-109's: {below} at 2^-110, {above} at 2^-108 (of {at[-109].size}); instance walks of the first "
          f"{WALK_BOXES} boxes: {walks[-110]}, {walks[-109]}, {walks[-108]}")
    want = XS.GUARD_DECISIONS.get(key[1], (0, 0))
    assert (below, above) == want, (key, below, above)
    assert walks[-110] <= walks[-109] <= walks[-108]
    if want[0] >= 50:
        assert walks[-110] < walks[-109], key
    if want[1] >= 50:
        assert walks[-108] > walks[-109], key
    if key[0] == "world":
        assert walks[-110] == walks[-109] == walks[-108]
    for g in (-110, -108):      # neither neighbour loses a pair here: the counter alone tells them apart
        got = walk(pkg, key, 8, True, top_cull=lambda *a, g=g: IO.guarded_misses(*a, guard=F(2.0 ** g)))
        assert same(got[:3], brute(pkg, key, 8, True)), (key, g)


def test_the_draws_lose_their_pair_without_the_guard(pkg):
    """("draws", -147), the very set and boxes of the GPU test: every fp32 corner lies outside its instance's stored box; the
    guarded walk returns the brute force, the unguarded one loses pair (i, 0) of box i.  Control: ("world", 0), where the two
    walks agree."""
    c = XS.draws_cell(pkg)
    n = len(c.of)
    assert n == XS.DRAWS_KEPT >= 2 and len(c.boxes) == n
    corners = [p.reshape(-1, 3, 3) for p in c.positions(pkg)]
    top = XS.stored_boxes(pkg, c)
    w = c.boxes["lo"]
    assert np.array_equal(w.view(np.uint32), c.boxes["hi"].view(np.uint32))
    for i in range(n):
        assert np.array_equal(IP.map_corners(c.maps[i], corners[i][0, 0])[0].view(np.uint32), w[i].view(np.uint32))
        assert ((w[i] < top[i][0]) | (w[i] > top[i][1])).any(), f"draw {i}: the corner is inside its stored box"
    want = IO.overlap_over_instances(c.positions(pkg), c.of, c.maps, c.boxes, 64)
    rows = np.arange(n)
    assert ((want[1] == rows[:, None]) & (want[0] == 0)).any(1).all()
    order = np.random.default_rng(3).permutation(n)
    lost = 0
    for k, counts in ((1, True), (8, False), (64, True)):
        guarded = IO.restated_walk(corners, c.maps, c.boxes, order, k, counts, top_boxes=top)
        assert same(guarded[:3], (want[0][:, :k], want[1][:, :k], want[2] if counts else None)), (k, counts)
        plain = IO.restated_walk(corners, c.maps, c.boxes, order, k, counts, top_boxes=top, top_cull=IO.misses)
        if counts:
            lost = int((plain[2] < want[2]).sum())
            assert lost == n, f"the unguarded walk loses a pair in {lost} of {n} boxes"
    print(f"draws: the unguarded walk loses a pair in {lost} of {n} boxes, the guarded walk in none")
    assert same(walk(pkg, ("world", 0), 8, True, top_cull=IO.misses)[:3], brute(pkg, ("world", 0), 8, True)), "the control"


# 4: the arithmetic mutants -----------------------------------------------------------------------------------------------------
def fused_row(row, x):
    """map_row with every product after the first fused into the sum (one rounding), the translation added as it is"""
    row = np.asarray(row, F)
    shape = np.broadcast(x[0], x[1], x[2]).shape
    acc = None
    for c in range(3):
        if row[c] != 0:
            xc, rc = np.broadcast_to(np.asarray(x[c], F), shape), np.full(shape, row[c], F)
            acc = np.multiply(rc, xc, dtype=F) if acc is None else fused_sub(rc, xc, -acc)
    if row[3] != 0:
        acc = np.full(shape, row[3], F) if acc is None else np.add(acc, row[3], dtype=F)
    return np.zeros(shape, F) if acc is None else np.broadcast_to(acc, shape).astype(F)


def flushed_row(row, x):
    """map_row with every subnormal product and sum flushed to 0"""
    row = np.asarray(row, F)
    shape = np.broadcast(x[0], x[1], x[2]).shape
    acc = None
    for c in range(3):
        if row[c] != 0:
            prod = flush(np.multiply(row[c], np.asarray(x[c], F), dtype=F))
            acc = prod if acc is None else flush(np.add(acc, prod, dtype=F))
    if row[3] != 0:
        acc = np.full(shape, row[3], F) if acc is None else flush(np.add(acc, row[3], dtype=F))
    return np.zeros(shape, F) if acc is None else np.broadcast_to(acc, shape).astype(F)


def zeros_too_row(row, x):
    """map_row that also adds the zero entries' products and a zero translation"""
    row = np.asarray(row, F)
    shape = np.broadcast(x[0], x[1], x[2]).shape
    acc = np.multiply(row[0], np.asarray(x[0], F), dtype=F)
    for c in (1, 2):
        acc = np.add(acc, np.multiply(row[c], np.asarray(x[c], F), dtype=F), dtype=F)
    return np.broadcast_to(np.add(acc, row[3], dtype=F), shape).astype(F)


ROWS = {"c. a fused corner formula": fused_row, "d. subnormal results flushed": flushed_row, "e. the zero entries' products added": zeros_too_row}


def merged_under(pkg, c, map_row):
    p = c.positions(pkg)
    return np.concatenate([IP.map_corners(c.maps[i], p[s], map_row=map_row).reshape(-1) for i, s in enumerate(c.of)])


def boxes_changed_by_a_row(pkg, key, map_row):
    c = XS.cell(pkg, key)
    with np.errstate(all="ignore"):
        got = OR.overlaps(merged_under(pkg, c, map_row), c.boxes)
        return int((got != OR.overlaps(merged_under(pkg, c, IP.map_row), c.boxes)).any(1).sum())


@pytest.mark.parametrize("mutant", sorted(ROWS))
def test_a_mutant_of_the_corner_formula_shows_in_its_cells_and_not_in_its_control(pkg, mutant):
    for key, want in XS.ROW_MUTANTS[mutant]["cells"].items():
        got = boxes_changed_by_a_row(pkg, key, ROWS[mutant])
        print(f"{mutant}: {got} boxes change at {key}")
        assert got == want > 0, (mutant, key, got, want)
    for control in XS.ROW_MUTANTS[mutant]["controls"]:
        assert boxes_changed_by_a_row(pkg, control, ROWS[mutant]) == 0, (mutant, control)


@pytest.mark.parametrize("key", [("world", XS.FMIN_WORLD), XS.NAN_CELL, ("world", 0)], ids=ids)
def test_mutant_fmin_and_fmax_in_min3_and_max3(pkg, key):
    """a. fmin / fmax drop a NaN that the header's comparisons pass on: XS.FMIN_CHANGES boxes at ("world", 100), where an edge
    product overflows and a projection is inf - inf, every walked box at the NaN-corner cell, none at ("world", 0)."""
    c = XS.cell(pkg, key)
    merged, _ = IP.merged_positions(c.positions(pkg), c.of, c.maps)
    plain, _ = arith_restate(merged, c.boxes, Arith())
    assert np.array_equal(plain, OR.overlaps(merged, c.boxes)), "the parametrised restatement is the restatement"
    got, _ = arith_restate(merged, c.boxes, Arith(mn=np.fmin, mx=np.fmax))
    n = int((got != plain).any(1).sum())
    print(f"a. fmin / fmax: {n} boxes change at {c} ({int((got & ~plain).sum())} pairs added, {int((plain & ~got).sum())} lost)")
    assert n == XS.FMIN_CHANGES[key]
    assert (int((got & ~plain).sum()), int((plain & ~got).sum())) == XS.FMIN_PAIRS[key]


# 5: the walk's mutants ---------------------------------------------------------------------------------------------------------
def nan_culls(node_lo, node_hi, lo, hi):
    """b. the node test written as hi >= lo && lo <= hi: a NaN end fails it and the node is culled"""
    with np.errstate(invalid="ignore"):
        return ~((node_hi >= lo) & (node_lo <= hi)).all(-1)


def ends_by_sign_bit(M, lo, hi):
    """the image box with a -0 entry taken for negative (the sign bit in place of `< 0`)"""
    M = np.asarray(M, F).reshape(3, 4)
    out_lo, out_hi = [], []
    with np.errstate(all="ignore"):
        for r in range(3):
            neg = np.signbit(M[r, :3])
            out_lo.append(IP.map_row(M[r], tuple(hi[..., c] if neg[c] else lo[..., c] for c in range(3))))
            out_hi.append(IP.map_row(M[r], tuple(lo[..., c] if neg[c] else hi[..., c] for c in range(3))))
    return np.stack(out_lo, axis=-1), np.stack(out_hi, axis=-1)


def shows(pkg, cell_key, k, counts, order=ORDER, **mutant):
    base = walk(pkg, cell_key, k, counts, order)
    assert same(base[:3], brute(pkg, cell_key, k, counts)), (cell_key, k, counts)
    return changed(walk(pkg, cell_key, k, counts, order, **mutant), base)


def test_mutant_a_nan_image_end_that_culls(pkg):
    n = shows(pkg, XS.NAN_CELL, 8, True, node_cull=nan_culls)
    go = OR.walked(XS.cell(pkg, XS.NAN_CELL).boxes[:WALK_BOXES])
    print(f"b. a NaN image end that culls: {int(n.sum())} of the {int(go.sum())} walked boxes change at the NaN-corner cell")
    assert n.sum() == XS.WALK_MUTANTS["b"] and np.array_equal(n, go)
    assert not shows(pkg, ("world", 64), 8, True, node_cull=nan_culls).any(), "the control: no end is NaN"


def test_mutant_image_ends_chosen_without_the_sign(pkg):
    n = shows(pkg, ("ill", 12), 64, True, image_box=ends_by_position)
    print(f"f. image ends without the sign: {int(n.sum())} boxes change at ill 12")
    assert n.sum() == XS.WALK_MUTANTS["f"] > 0
    for key in (("negzero", 0), ("negzero", 1)):      # -0 is no negative entry: a zero entry is not read, whichever end is chosen
        assert not shows(pkg, key, 64, True, image_box=ends_by_sign_bit).any(), key
    n = shows(pkg, ("negzero", 1), 64, True, image_box=ends_by_position)
    print(f"f. image ends without the sign: {int(n.sum())} boxes change at negzero 1 (its flips and permutations have negative entries)")
    assert n.sum() == XS.WALK_MUTANTS["f at negzero"]


def test_mutant_triangle_before_instance_in_the_key(pkg):
    n = shows(pkg, ("far", 23), 8, False, key=IO.key_triangle_first)
    print(f"k. triangle before instance: {int(n.sum())} boxes change at far 23")
    assert n.sum() == XS.WALK_MUTANTS["k"] > 0
    tri, inst, cnt = brute(pkg, ("world", 0), 64, True)
    one = np.array([len(set(row[row >= 0].tolist())) <= 1 for row in inst]) & (cnt <= 64)     # every pair held, all of one instance
    n = shows(pkg, ("world", 0), 64, True, key=IO.key_triangle_first)
    print(f"k. triangle before instance: {int(n[one].sum())} of the {int(one.sum())} boxes of world 0 whose pairs are of one instance change")
    assert one.sum() == XS.WALK_MUTANTS["k control"] > 40 and not n[one].any() and n.any()


def test_mutant_the_instance_skip_reads_the_slot_before_the_kth(pkg):
    """l. In ascending instance order (the lower instances' keys are held when a higher one comes).  Few boxes show it, and
    hardly any at the far cells: there a box that holds K - 1 pairs of one instance nearly always holds K."""
    ascending = np.arange(XS.INSTANCES)
    for (key, k), want in XS.SKIP_SHOWS.items():
        n = shows(pkg, key, k, False, order=ascending, skip_slot=-1)
        print(f"l. the skip slot read one early: K = {k}: {int(n.sum())} boxes change at {key}")
        assert n.sum() == want, (key, k)
        assert not shows(pkg, key, 1, False, order=ascending, skip_slot=-1).any(), "K = 1: there is no slot before the first"
        assert not shows(pkg, key, k, True, order=ascending, skip_slot=-1).any(), "the form with counts never reads the slot"
    assert sum(XS.SKIP_SHOWS.values()) > 0
