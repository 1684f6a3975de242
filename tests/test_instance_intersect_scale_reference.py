"""The cells of tests/instance_intersect_scale_cases.py on the CPU, on the restatement alone (tests/instance_intersect_ref.py):
each cell's conditions (finite corners, or the NaN and infinity counts of the NaN-corner cell; the six shares of
instance_intersect_cases.shares over FLOOR or at their LOW_SHARES bound; the TABLE of the world-scale cells; the cancelling scale
and the negative zeros against their twins byte for byte; n = 0 and no query walked where every world coordinate underflows);
SKIP_SHARED from the same brute force; the restated walk (image boxes, stored boxes as the top level, a scrambled instance
order) against the brute force, index for index, at every cell; the instance form's queries at the far cells; and the mutants
below, each of which changes an answer in a named cell and none in a named control.

Mutants.  MEASURED on the restatement; "queries" counts the queries with any index, instance index or count other than the
header's.  The corner formula's mutants are judged on the brute force over all 256 queries of a cell, the walk's on the first
WALK_QUERIES = 192, the instances walked in a scrambled order, against the plain walk, which returns the brute force's answer
at every cell.
  a. fmin / fmax in min3 / max3             (tests/test_intersect_scale_reference.py's parametrised arithmetic on the cell's merged
                                            scene) all 248 walked queries at the NaN-corner cell (32,240 pairs lost), 167 at
                                            ("world", 64), 3 at ("world", 100) (5 pairs lost: there nearly every product has
                                            overflowed and hardly an axis separates under either rule).  Control ("world", 0): 0.
  b. a NaN image end culls                  every one of the 187 walked queries at the NaN-corner cell.  Control ("world", 64): 0.
  c. a fused corner formula                 33 at ("ill", 20), all 248 walked queries at the NaN-corner cell.  Control
                                            ("negzero", 0), of order 1: 0.
  d. subnormal results flushed              changes no answer at any cell (asserted at ("world", -70) and ("world", 0)): where a
                                            corner formula's product is subnormal the normals have long underflowed, no query
                                            is walked and n = 0 either way.  No GPU test of this query can see it; the box
                                            query's series does (1,298 boxes at its ("subnormal", -70)).
  e. the zero entries' products added       changes no answer at any cell (asserted at ("world", 0) and the NaN-corner cell), for
                                            the reason given in tests/test_instance_overlap_scale_reference.py.
  f. image ends chosen without the sign     57 at ("ill", 12).  Control, the negative-zero cells: a -0 entry taken for negative
                                            changes nothing at either.
  g, h, i. the guard removed or moved       not observable in this query on these cells (instance_intersect_scale_cases.py).
  k. triangle before instance in the key    K = 8 without counts: 9 at ("far", 23).  Control: the 97 queries of ("world", 0) whose
                                            pairs are all held and of one instance: 0.
  l. the skip slot read one early           ascending instance order, without counts, K = 8 / K = 9: 0 / 2 at ("far", 12), 0 / 1 at
                                            ("far", 20), 1 / 2 at ("far", 23); 1 at ("world", 0), K = 9.  Controls, where it shows:
                                            K = 1, and the form with counts: 0.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import instance_intersect_cases as XC
import instance_intersect_ref as II
import instance_intersect_scale_cases as TS
import instance_point_ref as IP
import instance_point_scale_cases as SC
import intersect_ref as IR
from test_instance_overlap_reference import ends_by_position
from test_instance_overlap_scale_reference import ROWS, ends_by_sign_bit, merged_under, nan_culls
from test_intersect_scale_reference import mutated

F = np.float32
ORDER = np.random.default_rng(9).permutation(TS.INSTANCES)[::-1]       # not the index order: the key must not lean on it
WALK_QUERIES = 192
WALK_KS = (1, 8, 9, 64)
_part = {}
_axes = {}


def ids(key):
    return f"{key[0]} {key[1]}"


def answer(pkg, key):
    """the restatement at K = 64 without and with SKIP_SHARED, once per cell; the membership of the first WALK_QUERIES
    queries is kept for the walks"""
    c = TS.cell(pkg, key)
    if key not in _part:
        merged, first = IP.merged_positions(c.positions(pkg), c.of, c.maps)
        code = IR.first_axis(c.queries, merged, False)
        member = code == IR.INTERSECT
        _axes[key] = np.bincount(code[(code >= IR.AXIS0) & (code < IR.UNWALKED)].astype(np.int64) - IR.AXIS0, minlength=IR.AXES)
        q, t = IR.corners_of(c.queries), merged.reshape(-1, 3, 3)
        shared = np.concatenate([II.shares_matrix(q[s:s + 32], t) for s in range(0, len(q), 32)])
        TS._memo[("restated", key, False)] = II.from_membership(member, first, 64)
        TS._memo[("restated", key, True)] = II.from_membership(member & ~shared, first, 64)
        _part[key] = [member[:WALK_QUERIES, first[i]:first[i + 1]].copy() for i in range(len(c.of))]
    return TS.restated(pkg, c)


@pytest.fixture(scope="module", autouse=True)
def restate_every_cell(pkg):
    """the cells and their restatements at K = 64, made once and side by side (numpy's loops release the interpreter)"""
    TS.base_queries(pkg)
    TS.cell(pkg, ("world", 0))
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as pool:
        list(pool.map(lambda key: answer(pkg, key), TS.CELLS))


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def changed(a, b):
    d = (a[0] != b[0]).any(1) | (a[1] != b[1]).any(1)
    return d if a[2] is None else d | (a[2] != b[2])


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_the_cells_are_what_the_files_say(pkg):
    assert len(TS.TABLE) == len(SC.S_EXPONENTS) and set(TS.TABLE) <= {"k", "c"}
    assert TS.CELLS[:len(SC.CELLS)] == SC.CELLS and len(TS.base_queries(pkg)[0]) == TS.QUERIES == 256
    base, small = TS.base_queries(pkg)
    assert small.sum() == TS.QUERIES // 4
    for key in TS.CELLS:
        c = TS.cell(pkg, key)
        assert c.queries.shape == (TS.QUERIES, 3, 3) and c.queries.dtype == F and np.array_equal(c.small, small)
        assert np.isfinite(c.maps).all(), f"{c}: every map is finite"
    c = TS.cell(pkg, TS.NAN_CELL)
    go = IR.walked(base)
    assert np.array_equal(c.queries[~go].view(np.uint32), base[~go].view(np.uint32)) and np.isfinite(c.queries[go]).all()


@pytest.mark.parametrize("key", TS.CELLS, ids=ids)
def test_a_cell_keeps_its_conditions(pkg, key):
    c = TS.cell(pkg, key)
    world = TS.world_corners(pkg, c)
    tri, inst, n = answer(pkg, key)
    go = IR.walked(c.queries)
    assert (n[~go] == 0).all() and np.array_equal((inst >= 0).sum(1), np.minimum(n, 64)) and np.array_equal(inst >= 0, tri >= 0)
    if key == TS.NAN_CELL:
        assert [int(np.isnan(w).any(2).any(1).sum()) for w in world] == TS.XS.NAN_TRIANGLES
        assert [int(np.isinf(w).any(2).any(1).sum()) for w in world] == TS.XS.INF_TRIANGLES
    else:
        assert all(np.isfinite(w).all() for w in world), f"{c}: a mapped corner is not finite"
    s = XC.shares(c.queries, inst, n)
    print(f"{c}: walked {int(go.sum())}; " + ", ".join(f"{k} {v * 100:.2f} %" for k, v in s.items()) + f"; first to separate, per axis {_axes[key].tolist()}")
    counts = tuple(int(round(v * len(c.queries))) for v in s.values()) + (int(go.sum()),)
    assert counts == TS.SHARE_COUNTS[key], f"{c}: the six shares and the walked, in queries of {len(c.queries)}: {counts}, the case file says {TS.SHARE_COUNTS[key]}"
    # instance_intersect_cases.assert_mixed's other half: nq, nt and each of the nine edge axes is first to separate some pair
    assert (min(_axes[key][:11]) >= 1) == (key in TS.ELEVEN_AXES_SEPARATE), (c, _axes[key].tolist())
    low = TS.LOW_SHARES.get(key, {})
    for name, share in s.items():
        if name in low:
            assert share <= TS.FLOOR, f"{c}: {name} is {share:.4f}: not low, take it out of LOW_SHARES"
            assert share >= low[name] and (share > 0) == (low[name] > 0), (c, name, share, low[name])
        else:
            assert share > TS.FLOOR, f"{c}: {name} is {share:.4f}, at or under {TS.FLOOR} (all: {s})"
    if key in TS.ALL_ZERO or key[0] == "guard":
        assert not go.any() and (n == 0).all(), f"{c}: every normal underflows to (0, 0, 0): no query is walked and n = 0"
    shared = TS.restated(pkg, c, True)
    assert (shared[2] <= n).all()
    if key == ("world", 0):
        assert same(shared, II.intersect_over_instances(c.positions(pkg), c.of, c.maps, c.queries, 64, True)), "SKIP_SHARED from the one brute force"
        assert (shared[2] < n).sum() > 50
    if key[0] == "world":
        t0, i0, n0 = answer(pkg, ("world", 0))
        kept = (tri == t0).all(1) & (inst == i0).all(1) & (n == n0)
        print(f"{c}: {int(kept.sum())} queries ({kept.mean() * 100:.2f} %) keep their k = 0 answer")
        assert int(kept.sum()) == TS.KEPT_COUNTS[key[1]], (c, int(kept.sum()))
        if key[1] in SC.S_EXPONENTS:
            assert kept.all() == (TS.flag(key[1]) == TS.KEPT), (c, float(kept.mean()))
        assert kept.mean() > 0.15, "the changed cells are not noise either"
    twin = TS.expected_cell(key)
    if twin:
        t = TS.cell(pkg, twin)
        assert same((tri, inst, n), answer(pkg, twin)) and same(shared, TS.restated(pkg, t, True)), f"{c} against {twin}"
        assert np.array_equal(c.queries.view(np.uint32), t.queries.view(np.uint32)), "the queries are the twin's too"
        if key[0] == "cancel":
            for a, b in zip(world, TS.world_corners(pkg, t)):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        else:
            assert np.signbit(c.maps[c.maps == 0]).all() and not np.signbit(t.maps[c.maps == 0]).any()


def test_the_draws_are_not_walked(pkg):
    """("draws", -147): the query on a draw's corner is a point: not walked, and every triangle of the set is degenerate"""
    c = TS.draws_cell(pkg)
    assert len(c.queries) == len(c.of) == TS.XS.DRAWS_KEPT and not IR.walked(c.queries).any()
    assert (II.intersect_over_instances(c.positions(pkg), c.of, c.maps, c.queries, 8)[2] == 0).all()


# 2 ---------------------------------------------------------------------------------------------------------------------------
_prepared = {}


def prepared(pkg, key):
    if key not in _prepared:
        c = TS.cell(pkg, key)
        answer(pkg, key)
        per_scene = [p.reshape(-1, 3, 3) for p in c.positions(pkg)]
        _prepared[key] = (c, [per_scene[s] for s in c.of], TS.stored_boxes(pkg, c))
    return _prepared[key]


def walk(pkg, cell_key, k, counts, order=ORDER, **mutant):
    c, corners, top = prepared(pkg, cell_key)
    with np.errstate(all="ignore"):
        return II.restated_walk(corners, c.maps, c.queries[:WALK_QUERIES], order, k, counts, top_boxes=top, members=_part[cell_key], **mutant)


def brute(pkg, cell_key, k, counts, skip_shared=False):
    tri, inst, n = TS.restated(pkg, TS.cell(pkg, cell_key), skip_shared)
    return tri[:WALK_QUERIES, :k], inst[:WALK_QUERIES, :k], (n[:WALK_QUERIES] if counts else None)


@pytest.mark.parametrize("key", TS.CELLS, ids=ids)
def test_the_restated_walk_returns_the_brute_force_indices(pkg, key):
    """What both culls rest on: with the image boxes as the nodes' boxes and instance_point_ref.stored_box as the top level the
    walk loses no pair, at any scale."""
    answer(pkg, key)
    for k in WALK_KS:
        for counts in (True, False):
            assert same(walk(pkg, key, k, counts)[:3], brute(pkg, key, k, counts)), (key, k, counts)
    assert same(walk(pkg, key, 8, True, skip_shared=True)[:3], brute(pkg, key, 8, True, True)), (key, "SKIP_SHARED")
    n = brute(pkg, key, 0, True)[2]
    assert np.array_equal(walk(pkg, key, 0, True, any_only=True)[2], (n > 0).astype(np.int32)), (key, "ANY is n > 0")


@pytest.mark.parametrize("t", SC.FAR_EXPONENTS)
def test_the_instance_form_s_queries_collapse_at_the_far_cells(pkg, t):
    """the own world corners of instances 1, 3 and 8, the queries of the instance form: at the far cells corners coincide on the
    float grid, some of the triangles are degenerate (not walked), and the rest are judged on those collapsed corners"""
    c = TS.cell(pkg, ("far", t))
    for q in TS.FORM_INSTANCES:
        rows = II.own_queries(c.positions(pkg), c.of, c.maps, q)
        coincide = int(((rows[:, 0] == rows[:, 1]).all(1) | (rows[:, 1] == rows[:, 2]).all(1) | (rows[:, 0] == rows[:, 2]).all(1)).sum())
        print(f"far {t}: instance {q}: {coincide} of {len(rows)} own triangles have two corners on one grid point, {int(IR.walked(rows).sum())} are walked")
        assert (coincide, int(IR.walked(rows).sum())) == TS.FAR_COLLAPSED[t][q], (t, q, coincide)


# 3: the mutants ----------------------------------------------------------------------------------------------------------------
def queries_changed_by_a_row(pkg, key, map_row):
    c = TS.cell(pkg, key)
    with np.errstate(all="ignore"):
        got = IR.intersects(c.queries, merged_under(pkg, c, map_row), False)
        return int((got != IR.intersects(c.queries, merged_under(pkg, c, IP.map_row), False)).any(1).sum())


@pytest.mark.parametrize("mutant", sorted(ROWS))
def test_a_mutant_of_the_corner_formula_shows_in_its_cells_and_not_in_its_control(pkg, mutant):
    for key, want in TS.ROW_MUTANTS[mutant]["cells"].items():
        got = queries_changed_by_a_row(pkg, key, ROWS[mutant])
        print(f"{mutant}: {got} queries change at {key}")
        assert got == want > 0, (mutant, key, got, want)
    for control in TS.ROW_MUTANTS[mutant]["controls"]:
        assert queries_changed_by_a_row(pkg, control, ROWS[mutant]) == 0, (mutant, control)


@pytest.mark.parametrize("key", [("world", TS.FMIN_WORLD), TS.NAN_CELL, ("world", 64), ("world", 0)], ids=ids)
def test_mutant_fmin_and_fmax_in_min3_and_max3(pkg, monkeypatch, key):
    """a. tests/test_intersect_scale_reference.py's parametrised arithmetic with fmin / fmax for the two-operand min and max (the
    query's vertex box, the triangles' boxes and every projection's min3 / max3), on the cell's merged scene: TS.FMIN_CHANGES"""
    c = TS.cell(pkg, key)
    merged, _ = IP.merged_positions(c.positions(pkg), c.of, c.maps)
    with np.errstate(all="ignore"):
        plain = IR.intersects(c.queries, merged)
        got = mutated(monkeypatch, "fmin_fmax", merged, c.queries)
    n = int((got != plain).any(1).sum())
    print(f"a. fmin / fmax: {n} queries change at {c} ({int((got & ~plain).sum())} pairs added, {int((plain & ~got).sum())} lost)")
    assert (n, int((got & ~plain).sum()), int((plain & ~got).sum())) == TS.FMIN_CHANGES[key]


def shows(pkg, cell_key, k, counts, order=ORDER, **mutant):
    base = walk(pkg, cell_key, k, counts, order)
    assert same(base[:3], brute(pkg, cell_key, k, counts)), (cell_key, k, counts)
    return changed(walk(pkg, cell_key, k, counts, order, **mutant), base)


def test_mutant_a_nan_image_end_that_culls(pkg):
    n = shows(pkg, TS.NAN_CELL, 8, True, node_cull=nan_culls)
    go = IR.walked(TS.cell(pkg, TS.NAN_CELL).queries[:WALK_QUERIES])
    print(f"b. a NaN image end that culls: {int(n.sum())} of the {int(go.sum())} walked queries change at the NaN-corner cell")
    assert n.sum() == TS.WALK_MUTANTS["b"] > 0
    assert not shows(pkg, ("world", 64), 8, True, node_cull=nan_culls).any(), "the control: no end is NaN"


def test_mutant_image_ends_chosen_without_the_sign(pkg):
    n = shows(pkg, ("ill", 12), 64, True, image_box=ends_by_position)
    print(f"f. image ends without the sign: {int(n.sum())} queries change at ill 12")
    assert n.sum() == TS.WALK_MUTANTS["f"] > 0
    for key in (("negzero", 0), ("negzero", 1)):
        assert not shows(pkg, key, 64, True, image_box=ends_by_sign_bit).any(), key


def test_mutant_triangle_before_instance_in_the_key(pkg):
    n = shows(pkg, ("far", 23), 8, False, key=II.key_triangle_first)
    print(f"k. triangle before instance: {int(n.sum())} queries change at far 23")
    assert n.sum() == TS.WALK_MUTANTS["k"] > 0
    tri, inst, cnt = brute(pkg, ("world", 0), 64, True)
    one = np.array([len(set(row[row >= 0].tolist())) <= 1 for row in inst]) & (cnt <= 64)
    n = shows(pkg, ("world", 0), 64, True, key=II.key_triangle_first)
    print(f"k. triangle before instance: {int(n[one].sum())} of the {int(one.sum())} queries of world 0 whose pairs are all held and of one instance change")
    assert one.sum() == TS.WALK_MUTANTS["k control"] > 40 and not n[one].any() and n.any()


def test_mutant_the_instance_skip_reads_the_slot_before_the_kth(pkg):
    ascending = np.arange(TS.INSTANCES)
    for (key, k), want in TS.SKIP_SHOWS.items():
        n = shows(pkg, key, k, False, order=ascending, skip_slot=-1)
        print(f"l. the skip slot read one early: K = {k}: {int(n.sum())} queries change at {key}")
        assert n.sum() == want, (key, k)
        if want:
            assert not shows(pkg, key, 1, False, order=ascending, skip_slot=-1).any(), "K = 1: there is no slot before the first"
            assert not shows(pkg, key, k, True, order=ascending, skip_slot=-1).any(), "the form with counts never reads the slot"
    assert sum(TS.SKIP_SHOWS.values()) > 0
