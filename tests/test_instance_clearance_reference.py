"""The restatement of the instanced triangle-distance query (tests/instance_clearance_ref.py) against itself, without a GPU: what
the nine-instance set of tests/instance_clearance_cases.py covers; the restated walk (median trees, image boxes, stored boxes
as the top level, a scrambled instance order) equal to the brute force byte for byte; the header's seven consequences; the two
bounds of the walk (an image box of a wider object-space node box, and the stored top-level box) never above a pair's dist2,
over test_clearance_reference's ten families under general affine maps and over coordinates below 2^-109; and for each decision
of the walk a mutant that changes an answer on a named input and none on a named control."""
import os

import numpy as np
import pytest

import clearance_ref as CR
import instance_clearance_cases as XC
import instance_clearance_ref as XR
import instance_point_cases as IC
import instance_point_ref as IP
import point_query_ref as R
from test_clearance_reference import bound_families
from test_instance_point_reference import set_maps

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EYE = np.eye(3, 4, dtype=F)
KS = (1, 3, 8, 9, 64)
INF = F(np.inf)
_nine = {}


@pytest.fixture(scope="module")
def lobed_positions(pkg):
    world = pkg.World(os.path.join(GOLDEN, "lobed_528.trisrc"))
    try:
        return np.asarray(world.arrays()["vertex_positions"], F).copy()
    finally:
        world.close()


def bits(x):
    return CR.as_bits(x) if x.dtype == CR.PAIR_DISTANCE_DTYPE else x


def same(got, want):
    return all((g is None and w is None) or np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def nine(lobed_positions):
    """the nine-instance set, its queries, max_dist2 and the pair table, once per module"""
    if not _nine:
        tiny = {name: np.asarray(tris, F).reshape(-1) for name, tris in IC.TINY.items()}
        positions, of, maps, kinds, names = XC.nine_instances(lambda name: lobed_positions if name == "lobed_528" else tiny[name])
        queries = XC.world_queries(positions, of, maps)
        _nine["set"] = (positions, of, maps, kinds, names, queries, XC.mid_value(positions, of, maps),
                        XR.merged_table(positions, of, maps, queries))
    return _nine["set"]


def general_queries(maps, n, seed, size=0.05, reach=3.5):
    """small random world triangles in general position around the set: no bound equals a reach, no two pairs tie"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-reach, reach, (n, 1, 3))
    return (centre + rng.normal(size=(n, 3, 3)) * size).astype(F)


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_the_nine_instance_set_covers_every_class(lobed_positions):
    positions, of, maps, kinds, names, queries, mid, table = nine(lobed_positions)
    assert kinds[4] == "duplicate of 1" and len(queries) == XC.QUERIES
    records, instances, counts = XR.from_merged_table(table, queries, 64, mid)
    print({k: round(v, 4) for k, v in XC.assert_mixed(queries, mid, records, instances, counts, "nine instances").items()})
    everything = XR.from_merged_table(table, queries, 0, INF)[2]
    assert everything.max() == sum(len(positions[s]) // 9 for s in of), "+inf holds every pair"


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 17])
def test_the_restated_walk_returns_the_brute_force_bytes(lobed_positions, n):
    maps = set_maps(n, seed=n)
    merged, _ = IP.merged_positions([lobed_positions], [0] * n, maps)
    queries = XC.CC.make_queries(merged, 64 if n < 17 else 40, seed=n + 60)
    mid = XC.mid_value([lobed_positions], [0] * n, maps)
    corners = lobed_positions.reshape(-1, 3, 3)
    order = np.random.default_rng(n).permutation(n)[::-1]       # (not the index order: the key must not lean on it)
    lo, hi = corners.reshape(-1, 3).min(0), corners.reshape(-1, 3).max(0)
    top = [IP.stored_box(M, lo, hi)[:2] for M in maps]
    prepared = XR.prepare(corners, maps, queries, top)
    table = XR.merged_table([lobed_positions], [0] * n, maps, queries)
    brute = int(CR.walked(queries, mid).sum()) * n * len(corners)
    for md in (mid, INF):
        for k in KS:
            want = XR.from_merged_table(table, queries, k, md)
            for counts in (True, False):
                rec, inst, cnt, tests, _ = XR.restated_walk(corners, maps, queries, order, k, counts, md, top_boxes=top, prepared=prepared)
                assert same((rec, inst), want[:2]), (n, k, counts, md)
                assert (np.array_equal(cnt, want[2]) if counts else cnt is None), (n, k, counts, md)
                if md == mid:
                    assert tests < brute, "the cull skips something"
    members = XR.from_merged_table(table, queries, 0, mid)[2]
    assert (members == 0).mean() > 0.1 and (members > 8).mean() > 0.1, np.bincount(np.minimum(members, 65))
    a = XR.restated_walk(corners, maps, queries, order, 1, False, INF, top_boxes=top, prepared=prepared)[3]
    b = XR.restated_walk(corners, maps, queries, order, 1, True, INF, top_boxes=top, prepared=prepared)[3]
    assert a < b, "the K-th best prunes below max_dist2"
    with_shared = XR.from_merged_table(table, queries, 9, mid, skip_shared=True)
    got = XR.restated_walk(corners, maps, queries, order, 9, True, mid, skip_shared=True, top_boxes=top, prepared=prepared)
    assert same(got[:3], with_shared)
    met = XR.restated_walk(corners, maps, queries, order, 0, True, mid, any_only=True, top_boxes=top, prepared=prepared)[2]
    assert np.array_equal(met, (members > 0).astype(np.int32))     # consequence 5


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_consequences_1_and_7_one_identity_instance(lobed_positions):
    queries = XC.CC.make_queries(lobed_positions, 120, seed=5)
    mid = XC.mid_value([lobed_positions], [0], EYE[None])
    d2, _ = CR.pair_table(R.NumpyOps, queries, lobed_positions)
    shared = CR.shared_table(queries, lobed_positions)
    table = XR.merged_table([lobed_positions], [0], EYE[None], queries)
    for k in (0, 1, 8, 64):
        for skip in (False, True):
            rec, inst, cnt = XR.from_merged_table(table, queries, k, mid, skip)
            want, want_cnt = CR.from_table(queries, lobed_positions, d2, shared, k, mid, skip)
            assert same((rec, cnt), (want, want_cnt))
            assert np.array_equal(inst, np.where(want["triangle"] >= 0, 0, -1))
    # 7: the instance form without the flag is the self form
    tris = lobed_positions.reshape(-1, 3, 3)[:96]
    rec, inst, cnt = XR.clearance_instance([lobed_positions], [0], EYE[None], 0, 9, mid, skip_own=False, count=96)
    want, want_cnt = CR.clearance(lobed_positions, tris, 9, mid)
    assert same((rec, cnt), (want, want_cnt)) and (cnt >= 1).all()
    rec, inst, cnt = XR.clearance_instance([lobed_positions], [0], EYE[None], 0, 9, mid, skip_own=True, count=96)
    assert not cnt.any() and (inst == -1).all(), "one instance: nothing but its own"


def test_consequences_2_3_and_4_the_merged_scene_the_prefix_and_the_duplicate(lobed_positions):
    maps = set_maps(5, seed=13)                              # map 4 is map 0
    assert np.array_equal(maps[4].view(np.uint32), maps[0].view(np.uint32))
    merged, first = IP.merged_positions([lobed_positions], [0] * 5, maps)
    queries = XC.CC.make_queries(merged, 120, seed=14)
    mid = XC.mid_value([lobed_positions], [0] * 5, maps)
    table = XR.merged_table([lobed_positions], [0] * 5, maps, queries)
    full = XR.from_merged_table(table, queries, 64, mid)
    for k in (1, 3, 8, 9):
        rec, inst, cnt = XR.from_merged_table(table, queries, k, mid)
        assert same((rec, inst, cnt), (full[0][:, :k], full[1][:, :k], full[2]))
    # the merged scene, split by hand: every instance has 528 triangles
    by_hand = np.concatenate([IP.map_corners(M, lobed_positions).reshape(-1) for M in maps])
    rec, cnt = CR.clearance(by_hand, queries, 64, mid)
    t = rec["triangle"]
    assert np.array_equal(np.where(t >= 0, t // 528, -1), full[1]) and np.array_equal(np.where(t >= 0, t % 528, -1), full[0]["triangle"])
    for f in ("on_query", "dist2", "on_scene", "feature", "reserved"):
        assert np.array_equal(np.ascontiguousarray(rec[f]).view(np.uint32), np.ascontiguousarray(full[0][f]).view(np.uint32)), f
    assert np.array_equal(cnt, full[2])
    assert same(XR.clearance_over_instances([lobed_positions], [0] * 5, maps, queries[:40], 8, mid),
                tuple(x[:40, :8] if x.ndim == 2 else x[:40] for x in full))
    # the duplicate: every pair again at the same dist2, the lower instance first
    rec, inst, cnt = full
    without = XR.clearance_over_instances([lobed_positions], [0] * 4, maps[:4], queries, 0, mid)[2]
    alone = XR.clearance_over_instances([lobed_positions], [0], maps[:1], queries, 0, mid)[2]
    assert np.array_equal(cnt, without + alone)
    pairs = 0
    for j in range(len(queries)):
        for s in np.nonzero(inst[j] == 0)[0]:
            twin = np.nonzero((inst[j] == 4) & (rec[j]["triangle"] == rec[j, s]["triangle"]))[0]
            if len(twin):       # (the twin may have fallen off the end of the K kept)
                assert twin[0] > s
                a, b = CR.as_bits(rec[j, s:s + 1]), CR.as_bits(rec[j, twin[0]:twin[0] + 1])
                assert np.array_equal(a, b)
                pairs += 1
            else:
                assert cnt[j] > 64
        assert not ((inst[j] == 4).sum() > (inst[j] == 0).sum())
    assert pairs > 300, pairs


def test_consequence_6_the_instance_form(lobed_positions):
    positions, of, maps, kinds, names, *_ = nine(lobed_positions)
    mid = XC.mid_value(positions, of, maps)
    for q in (1, 7, 8):
        whole = XR.own_queries(positions, of, maps, q)
        some = min(48, len(whole))
        rows = whole[:some]
        table = XR.merged_table(positions, of, maps, rows)
        item = XR.from_merged_table(table, rows, 64, mid)
        plain = XR.clearance_instance(positions, of, maps, q, 64, mid, skip_own=False, count=some, table=table)
        assert same(plain, item) and (plain[2] >= 1).all()
        if q == 8:
            assert same(plain, XR.clearance_instance(positions, of, maps, q, 64, mid, skip_own=False)), "the whole instance, its own table"
        flagged = XR.clearance_instance(positions, of, maps, q, 64, mid, skip_own=True, count=some, table=table)
        assert not (flagged[1] == q).any()
        merged, first, d2, _ = table
        own_pairs = (d2[:some, first[q]:first[q + 1]] <= mid).sum(1)
        assert np.array_equal(flagged[2], plain[2] - own_pairs)
        for j in range(some):    # what is left is the item form's answer without instance q's records, in order
            keep = plain[1][j] != q
            left = plain[0][j][keep & (plain[1][j] >= 0)]
            if plain[2][j] <= 64:
                assert np.array_equal(CR.as_bits(left), CR.as_bits(flagged[0][j][:len(left)]))
    table = XR.merged_table(positions, of, maps, XR.own_queries(positions, of, maps, 1)[:8])
    nearest = XR.clearance_instance(positions, of, maps, 1, 1, INF, count=8, table=table)
    assert nearest[1].tolist() == [[4]] * 8 and (nearest[0]["dist2"] == 0).all(), "the duplicate is found, at distance 0"


# 4 ---------------------------------------------------------------------------------------------------------------------------
def affine_maps(rng, n, scale=1.0):
    maps = np.zeros((n, 3, 4), F)
    for i in range(n):
        A = IC.rotation(rng) @ np.diag(rng.uniform(0.3, 2.5, 3)) @ (np.eye(3) + np.triu(rng.normal(size=(3, 3)), 1) * 0.4)
        if i % 2:
            A = A @ np.diag([-1.0, 1.0, 1.0])
        maps[i, :, :3] = A
        maps[i, :, 3] = rng.uniform(-3, 3, 3) * scale
    return maps


def assert_bounds(name, q_object, t_object, M, stored_pairs, contained=True):
    """the pairs (M q, M t): lb <= dist2 for the image box of a wider object-space node box and for the stored box of it"""
    o = R.NumpyOps
    q = IP.map_corners(M, q_object).reshape(-1, 3, 3)
    t = IP.map_corners(M, t_object).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        d2 = CR.pair_values(q, t)[0]
    both = np.concatenate([t_object, np.roll(t_object, 1, 0)], 1)      # the node's box: this triangle and another
    nlo, nhi = both.min(1), both.max(1)
    ilo, ihi = IP.image_box(M, nlo, nhi)
    qlo, qhi = XR.query_box(q)
    image = XR.gap2(qlo, qhi, ilo, ihi)
    assert np.isfinite(d2).all() and np.isfinite(image).all(), name
    assert (image <= d2).all(), (name, "image box", int((image > d2).sum()))
    if contained:
        assert ((t >= ilo[:, None]) & (t <= ihi[:, None])).all(), (name, "a world corner outside its image box")
    rows = np.arange(0, len(q), max(1, len(q) // stored_pairs))
    stored = np.array([IP.stored_box(M, nlo[j], nhi[j])[:2] for j in rows])
    lb = XR.gap2(qlo[rows], qhi[rows], stored[:, 0], stored[:, 1])
    assert (lb <= d2[rows]).all(), (name, "stored box", int((lb > d2[rows]).sum()))
    return int((image == d2).sum()), int((image > 0).sum()), int((lb > 0).sum())


def test_the_two_bounds_never_exceed_a_pair_s_dist2():
    """lb <= dist2 bit for bit with the image box of a wider object-space node box and with the stored top-level box, over the
    ten families of the triangle-distance query's own check under random general affine maps (the huge family under maps
    without translation, so that it stays finite), and over a family with every coordinate below 2^-109, where a corner may
    leave its stored box."""
    rng = np.random.default_rng(30)
    maps = affine_maps(rng, 3)
    for name, (q, t) in bound_families(5_000, 11).items():
        for M in maps:
            if name in ("huge", "scale 2^40"):
                M = M.copy()
                M[:, 3] = 0
            eq, pos, top = assert_bounds(name, q, t, M, 400)
        print(f"{name}: {len(q)} pairs a map, the last: image lb == dist2 on {eq}, image lb > 0 on {pos}, stored lb > 0 on {top} of 400")
    # below 2^-109: subnormal corners, and queries at three scales around the bound's 2^-75
    n = 4_000
    t = (rng.uniform(-1, 1, (n, 3, 3)) * 2.0 ** -111).astype(F)
    small = affine_maps(rng, 3, scale=0.0)
    small[:, :, :3] *= F(0.25)
    for scale in (2.0 ** -111, 2.0 ** -76, 2.0 ** -70, 2.0 ** -60):
        q = (rng.uniform(-1, 1, (n, 3, 3)) * scale + rng.choice([-1.0, 1.0], (n, 1, 3)) * scale).astype(F)
        for M in small:
            # (the query is in world space already: the identity for it, the small map for the scene)
            o = R.NumpyOps
            tw = IP.map_corners(M, t).reshape(-1, 3, 3)
            assert (np.abs(tw) < 2.0 ** -109).all()
            with np.errstate(all="ignore"):
                d2 = CR.pair_values(q, tw)[0]
            both = np.concatenate([t, np.roll(t, 1, 0)], 1)
            nlo, nhi = both.min(1), both.max(1)
            ilo, ihi = IP.image_box(M, nlo, nhi)
            qlo, qhi = XR.query_box(q)
            assert (XR.gap2(qlo, qhi, ilo, ihi) <= d2).all(), ("below 2^-109, image box", scale)
            rows = np.arange(0, n, 8)
            stored = np.array([IP.stored_box(M, nlo[j], nhi[j])[:2] for j in rows])
            assert (np.abs(stored) < 2.0 ** -109).all()
            lb = XR.gap2(qlo[rows], qhi[rows], stored[:, 0], stored[:, 1])
            assert (lb <= d2[rows]).all(), ("below 2^-109, stored box", scale, int((lb > d2[rows]).sum()))
            if scale >= 2.0 ** -70:
                assert (lb > 0).any(), "the bound is not vacuous at this scale"


# 5 ---------------------------------------------------------------------------------------------------------------------------
FLAT = np.array([[[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]]], F)      # in the plane z = 0: its box bound IS its dist2 above it
ABOVE = np.array([[[1.0, 1.0, 0.75], [1.5, 1.0, 0.75], [1.0, 1.5, 0.75]]], F)  # parallel above its interior: dist2 = gap^2 = 0.5625


@pytest.mark.parametrize("which", ["node_skip", "top_skip"])
def test_mutant_a_skip_at_equality_loses_the_lower_instance(lobed_positions, which):
    mutant = {which: XR.at_or_above}
    maps = np.stack([EYE, EYE])
    boxes = [(FLAT.reshape(-1, 3).min(0), FLAT.reshape(-1, 3).max(0))] * 2
    want = XR.clearance_over_instances([FLAT.reshape(-1)], [0, 0], maps, ABOVE, 1)
    assert want[1][0, 0] == 0 and want[0][0, 0]["dist2"] == F(0.5625)
    got = XR.restated_walk(FLAT, maps, ABOVE, [1, 0], 1, False, top_boxes=boxes)
    assert same(got[:2], want[:2])
    got = XR.restated_walk(FLAT, maps, ABOVE, [1, 0], 1, False, top_boxes=boxes, **mutant)
    assert got[1][0, 0] == 1, "the mutant keeps the higher instance"
    # the control: nothing sits at equality
    maps = set_maps(2, seed=3)
    corners = lobed_positions.reshape(-1, 3, 3)
    queries = general_queries(maps, 48, seed=21)
    top = [IP.stored_box(M, corners.reshape(-1, 3).min(0), corners.reshape(-1, 3).max(0))[:2] for M in maps]
    want = XR.clearance_over_instances([lobed_positions], [0, 0], maps, queries, 3)
    assert (want[0]["dist2"] > 0).all()
    got = XR.restated_walk(corners, maps, queries, [1, 0], 3, False, top_boxes=top, **mutant)
    assert same(got[:2], want[:2])


def test_mutant_the_tie_by_triangle_before_instance(lobed_positions):
    mutant = dict(key=XR.key_triangle_first)
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = np.stack([set_maps(1, seed=4)[0]] * 2)            # an exact duplicate
    queries = IP.map_corners(maps[0], corners[::66]).reshape(-1, 3, 3)    # the world triangles themselves: they and their neighbours tie at 0
    want = XR.clearance_over_instances([lobed_positions], [0, 0], maps, queries, 4)
    assert (want[0]["dist2"][:, :4] == 0).all() and (want[1][:, :2] == 0).all(), "two triangles of instance 0 lead"
    got = XR.restated_walk(corners, maps, queries, [1, 0], 4, False)
    assert same(got[:2], want[:2])
    got = XR.restated_walk(corners, maps, queries, [1, 0], 4, False, **mutant)
    assert (got[1][:, 1] == 1).all(), "the mutant puts the duplicate's copy of the first triangle second"
    # the control: no two pairs tie
    maps = set_maps(2, seed=3)
    queries = general_queries(maps, 48, seed=22)
    want = XR.clearance_over_instances([lobed_positions], [0, 0], maps, queries, 4)
    got = XR.restated_walk(corners, maps, queries, [1, 0], 4, True, **mutant)
    assert same(got[:3], want)


def test_mutant_the_reach_taken_one_slot_early():
    """Three copies of the flat triangle 1, 2 and 3 below the query, K = 3, the nearest visited first; after two the mutant's
    reach is 4 and the third, whose bound is 9, is lost."""
    query = np.array([[[1.0, 1.0, 0.0], [1.5, 1.0, 0.0], [1.0, 1.5, 0.0]]], F)
    maps = np.stack([EYE] * 3)
    maps[:, 2, 3] = (-1.0, -2.0, -3.0)
    want = XR.clearance_over_instances([FLAT.reshape(-1)], [0, 0, 0], maps, query, 3)
    assert want[0]["dist2"][0].tolist() == [1.0, 4.0, 9.0] and want[1][0].tolist() == [0, 1, 2]
    got = XR.restated_walk(FLAT, maps, query, [0, 1, 2], 3, False)
    assert same(got[:2], want[:2])
    got = XR.restated_walk(FLAT, maps, query, [0, 1, 2], 3, False, reach_slot=-2)
    assert got[1][0].tolist() == [0, 1, -1], "the mutant loses the third record"
    got = XR.restated_walk(FLAT, maps, query, [0, 1, 2], 3, False, reach_slot=0)
    assert same(got[:2], want[:2])
    # the control: the form with counts never reads the slot
    got = XR.restated_walk(FLAT, maps, query, [0, 1, 2], 3, True, reach_slot=-2)
    assert same(got[:3], want)


def test_mutant_n_counted_only_for_kept_records(lobed_positions):
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = set_maps(2, seed=3)
    merged, _ = IP.merged_positions([lobed_positions], [0, 0], maps)
    queries = XC.CC.make_queries(merged, 48, seed=24)
    mid = XC.mid_value([lobed_positions], [0, 0], maps)
    prepared = XR.prepare(corners, maps, queries)
    want = XR.clearance_over_instances([lobed_positions], [0, 0], maps, queries, 3, mid)
    assert (want[2] > 3).mean() > 0.3
    got = XR.restated_walk(corners, maps, queries, [1, 0], 3, True, mid, prepared=prepared)
    assert same(got[:3], want)
    got = XR.restated_walk(corners, maps, queries, [1, 0], 3, True, mid, count_kept_only=True, prepared=prepared)
    assert same(got[:2], want[:2]) and (got[2] != want[2]).sum() >= (want[2] > 3).sum() // 2 and (got[2] <= want[2]).all()
    # the control: a tolerance so small that no query holds more than K
    tight = F(1e-7)
    want = XR.clearance_over_instances([lobed_positions], [0, 0], maps, queries, 64, tight)
    assert want[2].max() <= 64 and (want[2] > 0).sum() > 5
    got = XR.restated_walk(corners, maps, queries, [1, 0], 64, True, tight, count_kept_only=True, prepared=prepared)
    assert same(got[:3], want)


def test_mutant_own_judged_by_the_scene(lobed_positions):
    """The input is a duplicate instance: by its index it is another instance and is found at distance 0; judged by the scene
    it would be the query's own."""
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = np.stack([set_maps(1, seed=6)[0]] * 2 + [set_maps(1, seed=7)[0]])
    maps[2, :, 3] += F(9.0)
    rows = XR.own_queries([lobed_positions], [0, 0, 0], maps, 0, count=24)
    want = XR.clearance_instance([lobed_positions], [0, 0, 0], maps, 0, 2, INF, count=24)
    assert (want[1] == 1).all() and (want[0]["dist2"] == 0).all()
    walk = dict(own=0, skip_own=True, scene_of=[0, 0, 0])
    got = XR.restated_walk(corners, maps, rows, [2, 1, 0], 2, True, INF, **walk)
    assert same(got[:3], want)
    got = XR.restated_walk(corners, maps, rows, [2, 1, 0], 2, True, INF, own_is=XR.same_scene, **walk)
    assert (got[1] == -1).all() and not got[2].any(), "the mutant finds nothing: every instance is of the query's scene"
    # the control: every instance a scene of its own
    each = [corners, corners.copy(), corners.copy()]
    got = XR.restated_walk(each, maps, rows, [2, 1, 0], 2, True, INF, own=0, skip_own=True, own_is=XR.same_scene)
    assert same(got[:3], want)


def test_mutant_skip_shared_on_object_corners(lobed_positions):
    """The input is a translated duplicate: its world corners share nothing with the query's, its object corners everything."""
    corners = lobed_positions.reshape(-1, 3, 3)
    maps = np.stack([EYE, EYE])
    maps[1, :, 3] = (0.015625, 0.0, 0.0)
    rows = XR.own_queries([lobed_positions], [0, 0], maps, 0, count=24)
    want = XR.clearance_instance([lobed_positions], [0, 0], maps, 0, 64, INF, skip_shared=True, skip_own=False, count=24)
    without_flag = XR.clearance_instance([lobed_positions], [0, 0], maps, 0, 0, INF, skip_own=False, count=24)
    assert (want[2] < without_flag[2]).all() and (want[2] > 528).all(), "instance 0's neighbours go, instance 1 stays whole"
    walk = dict(skip_shared=True, own=0, object_queries=corners[:24])
    got = XR.restated_walk(corners, maps, rows, [1, 0], 64, True, INF, **walk)
    assert same(got[:3], want)
    got = XR.restated_walk(corners, maps, rows, [1, 0], 64, True, INF, shared_on_object=True, **walk)
    assert (got[2] < want[2]).all(), "the mutant drops instance 1's copies of the neighbours too"
    # the control: one identity instance, whose object corners are its world corners
    want = XR.clearance_instance([lobed_positions], [0], EYE[None], 0, 8, INF, skip_shared=True, skip_own=False, count=24)
    got = XR.restated_walk(corners, EYE[None], rows, [0], 8, True, INF, shared_on_object=True, **walk)
    assert same(got[:3], want)


# 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["leaf_root", "one_branch", "wide_by_one"])
def test_the_counting_walk_finds_every_member(name):
    """instance_clearance_ref.walk_counters over a hand-shaped tree and refit_ref.node_boxes: the members it finds are the brute
    force's count under every kind of map; a query that is not walked counts nothing; behind a top-level box that is out of
    reach there is no member."""
    import refit_ref
    import tree_shapes as T
    tree, vertex_data = T.build(name)
    corners = np.ascontiguousarray(vertex_data[tree.triangle_vertices][:, :, :3])
    positions = corners.reshape(-1)
    boxes = refit_ref.node_boxes(tree, corners)
    rng = np.random.default_rng(len(name))
    for kind in ("identity", "rotation_nonuniform", "mirror", "shear")[:4 if len(corners) < 100 else 2]:
        M = IC.map_of(kind, rng, positions, 1.5).astype(F)
        queries = XC.world_queries([positions], [0], M[None], 96 if len(corners) < 100 else 40, seed=3)
        mid = XC.mid_value([positions], [0], M[None]) * F(4 if len(corners) < 100 else 0.01)
        table = XR.merged_table([positions], [0], M[None], queries)
        go = CR.walked(queries, mid)
        for skip in (False, True):
            want = XR.from_merged_table(table, queries, 0, mid, skip)[2]
            w = XR.walk_counters(tree, boxes, corners, M, queries, mid, skip_shared=skip, d2s=table[2])
            assert np.array_equal(w["members"], want), (name, kind, skip)
            assert np.array_equal(w["traversals"], go.astype(np.int64)) and (w["node_visits"][~go] == 0).all()
            assert (w["node_visits"][go] % 2 == 1).all() and (w["node_visits"] <= tree.node_count).all()
            assert (w["triangle_tests"] >= w["members"]).all()
            met = XR.walk_counters(tree, boxes, corners, M, queries, mid, skip_shared=skip, any_only=True, d2s=table[2])
            assert (met["triangle_tests"] <= w["triangle_tests"]).all() and (met["node_visits"] <= w["node_visits"]).all()
            assert ((met["triangle_tests"] > 0) >= (want > 0)).all()
        lo, hi = IP.image_box(M, boxes[0, :3], boxes[0, 3:])
        culled = XR.walk_counters(tree, boxes, corners, M, queries, mid, top_box=(lo, hi), d2s=table[2])
        out = go & (culled["traversals"] == 0)
        assert (culled["members"][out] == 0).all()
