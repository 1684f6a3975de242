"""The cells of tests/instance_point_scale_cases.py on the CPU, on the restatement alone (tests/instance_point_ref.py): the TABLE
of the world-scale cells; each cell's conditions (finite corners, the mix of points and outcomes, the ties of the far cells, the
(0, 0) answer where every dist2 is 0); the cancelling scale and the negative zeros against their twins byte for byte; the bound
property the two culls rest on, at every cell, for every point, instance and node; and six mutants of the restated walk, each
of which changes a record in a named cell and none in a named control.

The bound property is asserted for the image box of every node of a median tree AND for the instance's stored box as
instance_point_ref.stored_box restates place_box.  With subnormal world coordinates the containment of the corners in the
stored box is not guaranteed (the margin is relative, the error of a subnormal product is half a subnormal step whatever its
size): on one-corner boxes at 2^-147 the fp32 corner falls outside its restated stored box in about 8 % of the draws
(test_a_subnormal_corner_can_leave_its_stored_box).  In the cell ("subnormal", -70) itself no corner does (measured: 0 of
355,104 coordinates; only the few corners that span a box can), and the property the cull needs holds either way, because a gap
that small squares to 0: the bound and every dist2 there are 0.

Mutants, the cell that shows each, and its control (measured on the restatement; the counts are of the cell's 1,536 points):
  a. image-box ends chosen without the entry's sign   622 records at ("world", 0); none at ("ties", -90), where the wrong
                                                       bound squares to 0 like the right one
  b. >= in place of > in the node skip                 1,327 (every walked point) at ("ties", -90); at ("world", 0) none among the
                                                       points off every surface (kinds near and box_corner).  A whole cell is
                                                       no control: each has points on a mapped corner or on a surface with radius
                                                       0, where a bound of 0 meets a best of 0 (148 records at ("world", 0))
  c. >= in the top-level skip                          1,327 at ("ties", -90); the same control (32 records at ("world", 0), all
                                                       of radius 0 or -0 on a surface)
  d. the corner formula with a fused multiply-add      180 at ("world", 0); none at ("negzero", 0), whose maps have one product
                                                       of +-1 a row
  e. zero entries read instead of skipped              2 at ("negzero", 1) (4 at ("negzero", 0), 1 at ("world", 0)): a corner
                                                       coordinate that is a zero takes the other sign, and the point on that
                                                       corner returns it as q; none at ("far", 12), where no corner is 0
  f. the tie decided by triangle before instance       176 at ("far", 23); none at ("world", 0), whose only ties across instances
                                                       are between a map and its exact duplicate (the same triangle)
"""
import functools

import numpy as np
import pytest

import instance_point_cases as IC
import instance_point_ref as IP
import instance_point_scale_cases as SC
import point_query_ref as R
import point_scale_cases as PC

F = np.float32
ORDER = np.random.default_rng(9).permutation(SC.INSTANCES)[::-1]       # not the index order: the tie rule must not lean on it
_trees = {}


def corners_of(pkg, c):
    """the object corners [T, 3, 3] of every instance's scene (one array per scene, shared by its instances)"""
    per_scene = [p.reshape(-1, 3, 3) for p in c.positions(pkg)]
    return [per_scene[s] for s in c.of]


def trees_of(pkg, c):
    """instance_point_ref.restated_walk's tree cache for the cell's scenes (a median tree per scene and scale)"""
    key = c.scene_exp
    if key not in _trees:
        _trees[key] = ({}, corners_of(pkg, c))
    return _trees[key]


def top_boxes(tree_cache, corners, maps):
    out = []
    for i, own in enumerate(corners):
        if id(own) not in tree_cache:
            tree_cache[id(own)] = (own, IP.median_tree(own))
        lo, hi = tree_cache[id(own)][1][0][:2]
        out.append(IP.stored_box(maps[i], lo, hi)[:2])
    return out


# ---- the mutants ------------------------------------------------------------------------------------------------------------
def unsigned_image_box(M, lo, hi, map_row=IP.map_row):
    """a. the low end on lo and the high end on hi, whatever the entry's sign"""
    M = np.asarray(M, F).reshape(3, 4)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(all="ignore"):
        return (np.stack([map_row(M[r], tuple(lo[..., c] for c in range(3))) for r in range(3)], axis=-1),
                np.stack([map_row(M[r], tuple(hi[..., c] for c in range(3))) for r in range(3)], axis=-1))


def at_or_above(lb, best):
    """b, c. `>=` in place of `>`"""
    return lb >= best


def fused_row(row, x):
    """d. the corner formula as a compiler contracts it: the first product rounded, every later one fused into its sum"""
    row = np.asarray(row, F)
    shape = np.broadcast(x[0], x[1], x[2]).shape
    acc = None
    for c in range(3):
        if row[c] != 0:
            xc = np.asarray(x[c], F)
            acc = np.multiply(row[c], xc, dtype=F) if acc is None else (np.float64(row[c]) * xc.astype(np.float64) + acc.astype(np.float64)).astype(F)
    if row[3] != 0:
        acc = np.full(shape, row[3], F) if acc is None else np.add(acc, row[3], dtype=F)
    if acc is None:
        acc = np.zeros(shape, F)
    return np.broadcast_to(acc, shape).astype(F)


def reading_row(row, x):
    """e. every entry read, the zeros too: three products and the translation, left to right"""
    row = np.asarray(row, F)
    shape = np.broadcast(x[0], x[1], x[2]).shape
    acc = np.multiply(row[0], np.asarray(x[0], F), dtype=F)
    for c in (1, 2):
        acc = np.add(acc, np.multiply(row[c], np.asarray(x[c], F), dtype=F), dtype=F)
    return np.broadcast_to(np.add(acc, row[3], dtype=F), shape).astype(F)


def with_row(row):
    return {"map_corners": functools.partial(IP.map_corners, map_row=row), "image_box": functools.partial(IP.image_box, map_row=row)}


MUTANTS = {
    "a. image-box ends without the sign": {"image_box": unsigned_image_box},
    "b. >= in the node skip": {"node_skip": at_or_above},
    "c. >= in the top-level skip": {"top_skip": at_or_above},
    "d. a fused corner formula": with_row(fused_row),
    "e. zero entries read": with_row(reading_row),
    "f. the tie by triangle before instance": {"triangle_first": True},
}

# mutant -> (the cell that shows it, its control cell, the control's kinds of point or None for all of them)
OFF_SURFACE = ("near", "box_corner")
SHOWS = {
    "a. image-box ends without the sign": (("world", 0), ("ties", PC.ALL_TIES_UNDERFLOW), None),
    "b. >= in the node skip": (("ties", PC.ALL_TIES_UNDERFLOW), ("world", 0), OFF_SURFACE),
    "c. >= in the top-level skip": (("ties", PC.ALL_TIES_UNDERFLOW), ("world", 0), OFF_SURFACE),
    "d. a fused corner formula": (("world", 0), ("negzero", 0), None),
    "e. zero entries read": (("negzero", 1), ("far", 12), None),
    "f. the tie by triangle before instance": (("far", 23), ("world", 0), None),
}


def walk(pkg, c, mutant=None):
    """(records, instances, triangle tests) of the restated walk over the cell, the top level as a list of stored boxes, the
    instances in a scrambled order"""
    cache, corners = trees_of(pkg, c)
    kw = dict(MUTANTS[mutant]) if mutant else {}
    return IP.restated_walk(corners, c.maps, c.points, ORDER, top_boxes=top_boxes(cache, corners, c.maps), trees=cache, **kw)


def differing(a, b):
    return (R.as_bits(a[0]) != R.as_bits(b[0])).any(1) | (np.asarray(a[1]) != np.asarray(b[1]))


_walks = {}


def plain_walk(pkg, c):
    if c.key not in _walks:
        _walks[c.key] = walk(pkg, c)
    return _walks[c.key]


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_the_base_set_is_what_the_cells_assume(pkg):
    of, maps, kinds, pts, kind, radius = SC.base(pkg)
    assert len(maps) == SC.INSTANCES and set(kinds) == set(IC.MAP_KINDS) | {"duplicate of 1"}, kinds
    assert kinds[4] == "duplicate of 1" and of[4] == of[1] and np.array_equal(maps[4].view(np.uint32), maps[1].view(np.uint32))
    assert [SC.SCENES[s] for s in of[:4]] == ["lobed_528", "small_trisrc", "lobed_528", "small_trisrc"] and len(pts) == SC.POINTS
    assert len(SC.TABLE) == len(SC.S_EXPONENTS) and set(SC.TABLE) <= {"c", "o"}
    assert len(SC.CELLS) == len(set(SC.CELLS))


@pytest.mark.parametrize("key", SC.CELLS, ids=lambda k: f"{k[0]} {k[1]}")
def test_a_cell_keeps_its_conditions(pkg, key):
    c = SC.cell(pkg, key)
    world = SC.world_corners(pkg, c)
    assert all(np.isfinite(w).all() for w in world), f"{c}: a mapped corner is not finite"
    records, inst = SC.restated(pkg, c)
    hit = records["triangle"] >= 0
    assert np.array_equal(inst >= 0, hit)
    go = SC.walked(c.points)
    if key in SC.ALL_ZERO:
        assert go.sum() > 0.8 * len(go) and np.array_equal(hit, go), f"{c}: every walked point hits"
        assert (records["dist2"][go] == 0).all() and (records["triangle"][go] == 0).all() and (inst[go] == 0).all(), f"{c}: (0, 0) on every walked point"
        for w in world:         # every dist2 of the cell is 0, not only the best
            for s in range(0, len(go), 512):
                assert (IP.pair_dist2(c.points["p"][s:s + 512][go[s:s + 512]], w)[1] == 0).all(), c
        if key[0] == "subnormal":
            tiny = F(2.0 ** -126)
            assert all((np.abs(w) < tiny).all() for w in world) and sum(int((w != 0).sum()) for w in world) > 100000
    else:
        low = SC.LOW_SHARES.get(key, {})
        try:
            IC.assert_mixed(c.points, c.kind, c.radius, records, str(c))
        except AssertionError as err:
            assert low and all(name in str(err) for name in low), err
        shares_hit = float(((c.radius == 1) & hit).mean())
        for name, least in low.items():
            assert name == "finite_radius_hit" and shares_hit >= least, (c, name, shares_hit)
        assert len(set(inst[hit].tolist())) >= 7, f"{c}: the hits come from many instances"
        assert (inst == 1).sum() > 5 and (inst == 4).sum() == 0, f"{c}: the duplicate never wins against its original"
    if key[0] == "world":
        want = SC.scale_records(SC.restated(pkg, SC.cell(pkg, ("world", 0)))[0], key[1], c.points)
        same = PC.same_records(records, want) & (inst == SC.restated(pkg, SC.cell(pkg, ("world", 0)))[1])
        print(f"{c}: {same.mean() * 100:.2f} % of the records are the scaled k = 0 records")
        assert same.all() == (SC.flag(key[1]) == SC.COVARIANT), (c, float(same.mean()))
        if SC.flag(key[1]) == SC.OUTSIDE:
            assert same.mean() > 0.4, "the outside cells are not noise either"
    if key[0] == "far":
        share = SC.tie_share(pkg, c)
        print(f"{c}: {share * 100:.1f} % of the hits have a second pair at the same dist2")
        assert share >= SC.MIN_TIE_SHARE, (c, share)
    if key[0] == "ill":
        assert len(set(inst[hit].tolist())) == 8
        k = [IP.stored_box(c.maps[i], F([-1, -1, -1]), F([1, 1, 1]))[2] for i in range(SC.INSTANCES)]
        # the margin factor 128 u cond(A), cond about 2^(2 e), passes 1 between e = 6 and e = 12 (about 0.05, 210 and 1.4e7)
        assert (max(k) > 1) == (key[1] >= 12), (c, k)
    twin = SC.expected_cell(key)
    if twin:
        t_records, t_inst = SC.restated(pkg, SC.cell(pkg, twin))
        assert np.array_equal(R.as_bits(records), R.as_bits(t_records)) and np.array_equal(inst, t_inst), f"{c} against {twin}"
        if key[0] == "cancel":      # the mapped corners themselves keep their bits
            for a, b in zip(world, SC.world_corners(pkg, SC.cell(pkg, twin))):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        else:
            assert np.signbit(c.maps[c.maps == 0]).all() and not np.signbit(SC.cell(pkg, twin).maps[c.maps == 0]).any()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SC.CELLS, ids=lambda k: f"{k[0]} {k[1]}")
def test_no_bound_is_above_a_dist2_below_it(pkg, key):
    """For every point, every instance and every node of the instance's median tree: box_bound of the node's image box is not
    above the dist2 of any pair below the node; and box_bound of the instance's stored box (place_box restated) is not above
    the dist2 of any pair of the instance.  Where every mapped corner is normal or 0 the corners also lie inside the stored box."""
    c = SC.cell(pkg, key)
    cache, corners = trees_of(pkg, c)
    boxes = top_boxes(cache, corners, c.maps)
    go = SC.walked(c.points)
    p = np.ascontiguousarray(c.points["p"][go])
    tiny = F(2.0 ** -126)
    checked = outside = 0
    for i, own in enumerate(corners):
        tree = cache[id(own)][1]
        M = c.maps[i]
        world = IP.map_corners(M, own).reshape(-1, 3, 3)
        d2 = np.concatenate([IP.pair_dist2(p[s:s + 256], world)[1] for s in range(0, len(p), 256)])
        least = [None] * len(tree)
        for at in range(len(tree) - 1, -1, -1):         # children come after their parent
            lo, hi, left, right, members = tree[at]
            least[at] = d2[:, members].min(1) if members is not None else np.minimum(least[left], least[right])
            ilo, ihi = IP.image_box(M, lo, hi)
            lb = IP.bound(p, ilo, ihi)
            assert not (lb > least[at]).any(), f"{c}: instance {i}, node {at}: an image-box bound above a dist2 below it"
            checked += len(p)
        slo, shi = boxes[i]
        assert not (IP.bound(p, slo, shi) > least[0]).any(), f"{c}: instance {i}: the stored box's bound above a dist2 of the instance"
        flat = world.reshape(-1, 3)
        out = int(((flat < slo) | (flat > shi)).sum())
        outside += out
        if (((np.abs(flat) >= tiny) | (flat == 0)).all()):
            assert out == 0, f"{c}: instance {i}: {out} normal mapped coordinates outside the restated stored box"
    print(f"{c}: {checked} bounds checked, {outside} corner coordinates outside their restated stored box")
    assert checked > 100000


def test_a_subnormal_corner_can_leave_its_stored_box():
    """One corner at about 2^-147 under a random row of entries in (-1, 1) beside two rows that keep the condition small: the
    fp32 corner is up to three half subnormal steps from its exact image, the stored box one outward rounding.  Some draws
    fall outside (why DESIGN section 20 claims the containment for normal world coordinates only); the gap is a subnormal,
    so its square is 0 and the box's bound at the corner itself, where dist2 is 0, is 0 as well."""
    rng = np.random.default_rng(147)
    outside = 0
    draws = 4000
    for _ in range(draws):
        M = np.zeros((3, 4), F)
        M[:, :3] = (np.eye(3) + rng.uniform(-1, 1, (3, 3)) * np.array([[1.0], [0.2], [0.2]])).astype(F)
        M[0, :3] = rng.uniform(-1, 1, 3)
        if abs(np.linalg.det(M[:, :3].astype(np.float64))) < 0.2:
            continue
        v = (rng.uniform(-4, 4, 3) * 2.0 ** -147).astype(F)
        w = IP.map_corners(M, v)[0]
        lo, hi, _ = IP.stored_box(M, v, v)
        out = (w < lo) | (w > hi)
        outside += bool(out.any())
        assert IP.bound(w[None], lo, hi)[0] == 0, (M, v, w, lo, hi)
        assert (np.abs(np.where(out, np.where(w < lo, lo - w, w - hi), 0)) < F(2.0 ** -146)).all()
    print(f"{outside} of {draws} draws leave the stored box")
    assert outside > 0


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted({k for row in SHOWS.values() for k in row[:2]}), ids=lambda k: f"{k[0]} {k[1]}")
def test_the_restated_walk_returns_the_brute_force_bytes_at_the_cells_the_mutants_use(pkg, key):
    c = SC.cell(pkg, key)
    got = plain_walk(pkg, c)
    assert not differing(got, SC.restated(pkg, c)).any()
    if key not in SC.ALL_ZERO:
        assert got[2] < 0.6 * int(SC.walked(c.points).sum()) * sum(len(x) for x in corners_of(pkg, c)), "the culls skip something"


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_mutant_shows_in_its_cell_and_not_in_its_control(pkg, mutant):
    shows, control, kinds = SHOWS[mutant]
    c = SC.cell(pkg, shows)
    changed = differing(walk(pkg, c, mutant), plain_walk(pkg, c))
    print(f"{mutant}: {int(changed.sum())} records differ at {c}")
    assert changed.any(), f"{mutant}: invisible at {c}"
    c = SC.cell(pkg, control)
    changed = differing(walk(pkg, c, mutant), plain_walk(pkg, c))
    if kinds:
        among = np.isin(c.kind, [IC.KINDS.index(k) for k in kinds])
        assert among.sum() > 400 and changed.any(), "the control is a part of a cell that does show the mutant"
        changed = changed[among]
    assert not changed.any(), f"{mutant}: {int(changed.sum())} records differ at its control {c}"
