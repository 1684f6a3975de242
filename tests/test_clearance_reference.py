"""The restatement of the triangle-distance query (tests/clearance_ref.py, include/shader_ray_clearance.h) on the CPU: known
pairs (parallel triangles, a corner above a face, skew edges, an interpenetrating pair whose feature minimum is positive, the
same pair under a degenerate query), its relation to the closest-point and the intersection restatements, the prefix property
over K, membership at exactly a pair's dist2, the self form on a closed mesh, the walk's bound lb <= dist2 (DESIGN section
11's numeric check, extended to section 29's box-to-box bound), the accuracy of float32 against the same text in float64, and
a check that does not share the formula: a 64 x 64 barycentric sampling of both triangles.

Accuracy, measured on this file's own seeded pairs (ACCURACY_PAIRS random pairs in [-1, 1]^3 with offsets up to 3, kept where
the float64 dist2 exceeds 1e-6 of the squared coordinate size): the largest relative error of the float32 dist2 and its
99.99th percentile are printed by test_float32_accuracy_against_float64 and asserted at twice the values measured when the test
was written (MEASURED_MAX, MEASURED_P9999)."""
import numpy as np

import clearance_ref as CR
import intersect_cases as IC
import intersect_ref as IR
import point_query_ref as PQ

F = np.float32
ACCURACY_PAIRS = 400_000
MEASURED_MAX, MEASURED_P9999 = 5.36e-5, 1.03e-5   # (see the module doc; the asserts are at twice these)

Q0 = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]


def one(q, t):
    return CR.pair_records(np.asarray([q], F), np.asarray([t], F))[0]


def test_parallel_triangles_a_representable_distance_apart():
    for h in (1.5, 0.25, 3.0):
        r = one(Q0, [[0, 0, h], [1, 0, h], [0, 1, h]])
        assert r["dist2"] == F(h * h) and r["feature"] == 0   # every feature ties: the lowest number
        assert r["on_query"].tolist() == [0, 0, 0] and r["on_scene"].tolist() == [0, 0, h]
    r = one(Q0, [[0.25, 0.25, -2], [3, 0.25, -2], [0.25, 3, -2]])   # only the scene's corner a is under the query
    assert r["dist2"] == 4 and r["feature"] == 3 and r["on_query"].tolist() == [0.25, 0.25, 0]


def test_a_corner_above_a_face():
    r = one([[0.25, 0.25, 0.5], [0.25, 0.3, 2], [0.3, 0.25, 2]], Q0)
    assert r["dist2"] == F(0.25) and r["feature"] == 0
    assert r["on_query"].tolist() == [0.25, 0.25, 0.5] and r["on_scene"].tolist() == [0.25, 0.25, 0]
    r = one([[0.25, 0.3, 2], [0.3, 0.25, 2], [0.25, 0.25, 0.5]], Q0)
    assert r["dist2"] == F(0.25) and r["feature"] == 2


def test_skew_edges_at_a_known_distance():
    """the query's edge 0 along x in z = 0 under the scene's edge 0 along y in z = 1; everything else of either is farther"""
    q, t = [[-1, 0, 0], [1, 0, 0], [0, -3, -3]], [[0, -1, 1], [0, 1, 1], [0, 0, 5]]
    r = one(q, t)
    assert r["dist2"] == 1 and r["feature"] == 6
    assert r["on_query"].tolist() == [0, 0, 0] and r["on_scene"].tolist() == [0, 0, 1]
    r = one(q[1:] + q[:1], t[2:] + t[:2])   # the same edges are query edge 2 and scene edge 1
    assert r["dist2"] == 1 and r["feature"] == 6 + 3 * 2 + 1


PIERCED = [[-20, -20, 0], [20, -20, 0], [0, 30, 0]]
PIERCING = [[0, 0, -1], [0.5, 0, 1], [-0.5, 0.25, 1]]


def test_an_interpenetrating_pair_whose_feature_minimum_is_positive():
    """the case the intersecting stage exists for: no corner and no edge of either triangle touches the other"""
    q, t = np.asarray([PIERCING], F), np.asarray([PIERCED], F)
    d2, feature, x, y = CR.pair_features(PQ.NumpyOps, CR._corner_tuples(PQ.NumpyOps, q), CR._corner_tuples(PQ.NumpyOps, t))
    assert d2[0] == 1 and feature[0] == 0
    r = one(PIERCING, PIERCED)
    assert r["dist2"] == 0 and not np.signbit(r["dist2"]) and r["feature"] == CR.PAIR_INTERSECTING
    # the witnesses stay those of the feature minimum: points of the two triangles, not a contact point
    assert r["on_query"].tolist() == [0, 0, -1] and r["on_scene"].tolist() == [0, 0, 0]


def test_the_same_pair_with_a_degenerate_query_is_positive():
    segment = [PIERCING[0], PIERCING[1], PIERCING[1]]
    r = one(segment, PIERCED)
    assert r["dist2"] == 1 and r["feature"] == 0
    r = one(PIERCING, [PIERCED[0], PIERCED[1], PIERCED[1]])   # a degenerate scene triangle never takes the stage either
    assert r["dist2"] > 0 and r["feature"] < CR.PAIR_INTERSECTING


def random_scene(n, seed, size=0.3):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-size, size, (n, 3, 3))).astype(F)


def test_never_above_the_closest_point_query_of_its_corners():
    """a query (p, p, p) has dist2 <= closest()'s dist2; a general one <= the minimum over its three corners: exactly, because
    the corner features are in the minimum"""
    tris = random_scene(150, 1)
    pos = tris.reshape(-1)
    rng = np.random.default_rng(2)
    p = rng.uniform(-1.5, 1.5, (120, 3)).astype(F)
    points = np.zeros(len(p), PQ.POINT_DTYPE)
    points["p"], points["max_dist2"] = p, np.inf
    want = PQ.closest(pos, points)
    got, n = CR.clearance(pos, np.repeat(p[:, None, :], 3, 1), 1)
    assert (n == len(tris)).all() and (got["dist2"][:, 0] <= want["dist2"]).all()
    # (not always equal: another feature's rounding -- a scene corner against the point -- may come out a float below)
    assert (got["dist2"][:, 0] == want["dist2"]).mean() > 0.5
    queries = random_scene(120, 3, 0.5)
    got, _ = CR.clearance(pos, queries, 1)
    corners = np.zeros((3, len(queries)), F)
    for i in range(3):
        points["p"] = queries[:, i]
        corners[i] = PQ.closest(pos, points)["dist2"]
    assert (got["dist2"][:, 0] <= corners.min(0)).all() and (got["dist2"][:, 0] < corners.min(0)).sum() > 10


def test_every_member_of_the_intersection_set_is_at_zero():
    tris = random_scene(200, 4)
    queries = IC.make_queries({"vertex_positions": tris.reshape(-1)}, 200, seed=5)
    member = IR.intersects(queries, tris.reshape(-1))
    d2, feature = CR.pair_table(PQ.NumpyOps, queries, tris.reshape(-1))
    assert member.sum() > 500 and (d2[member] == 0).all() and (feature[member] == CR.PAIR_INTERSECTING).all()
    assert not (feature[~member] == CR.PAIR_INTERSECTING).any()
    # a degenerate query that touches: 0 by a feature, not by the stage
    r = one([tris[0, 0]] * 3, tris[0])
    assert r["dist2"] == 0 and r["feature"] == 0


def test_the_prefix_property_and_the_order():
    tris = random_scene(200, 6)
    queries = random_scene(40, 7, 0.5)
    queries[::2] += F(1.2)   # half of them off to one side: few members
    full, n = CR.clearance(tris.reshape(-1), queries, 64, F(0.6))
    assert (n > 64).any() and (n < 8).any()
    for k in (0, 1, 2, 4, 8, 9):
        got, gn = CR.clearance(tris.reshape(-1), queries, k, F(0.6))
        assert np.array_equal(gn, n) and np.array_equal(CR.as_bits(got), CR.as_bits(full[:, :k]))
    for row, count in zip(full, n):
        held = row[:min(count, 64)]
        key = list(zip(held["dist2"].tolist(), held["triangle"].tolist()))
        assert key == sorted(key) and (held["dist2"] <= F(0.6)).all() and (row[len(held):]["triangle"] == -1).all()
        assert (row[len(held):]["dist2"] == F(0.6)).all() and (row[len(held):]["feature"] == -1).all()


def test_max_dist2_exactly_a_pair_s_dist2_is_a_member():
    tris = random_scene(60, 8)
    queries = random_scene(30, 9, 0.5) + F(0.4)
    d2, _ = CR.pair_table(PQ.NumpyOps, queries, tris.reshape(-1))
    for row in range(0, 30, 5):
        at = np.sort(d2[row])[3]
        assert at > 0
        assert CR.clearance(tris.reshape(-1), queries[row:row + 1], 0, at)[1][0] == (d2[row] <= at).sum() >= 4
        below = np.nextafter(at, F(0))
        assert CR.clearance(tris.reshape(-1), queries[row:row + 1], 0, below)[1][0] == (d2[row] < at).sum()
    first = np.sort(d2[0])[0]
    assert CR.clearance(tris.reshape(-1), queries[:1], 0, first)[1][0] >= 1
    assert CR.clearance(tris.reshape(-1), queries[:1], 0, np.nextafter(first, F(0)))[1][0] == 0
    for bad in (F(-1), F(np.nan), F(-0.5)):
        got, n = CR.clearance(tris.reshape(-1), queries[:2], 2, bad)
        assert (n == 0).all() and (got["triangle"] == -1).all() and np.array_equal(got["dist2"].view(np.uint32), np.full((2, 2), bad, F).view(np.uint32))


def test_the_self_form_on_a_closed_mesh_with_skip_shared_has_no_zero(pkg):
    world = pkg.World(IC.scene_path("lobed_528"))
    pos = np.asarray(world.arrays()["vertex_positions"], F).copy()
    world.close()
    tris = pos.reshape(-1, 3, 3)
    got, n = CR.clearance(pos, tris, 1, np.inf, skip_shared=True)
    assert (n > 0).all() and (n < len(tris)).all() and (got["dist2"] > 0).all() and (got["feature"] < CR.PAIR_INTERSECTING).all()
    assert (got["triangle"][:, 0] != np.arange(len(tris))).all()
    got, n = CR.clearance(pos, tris[:64], 1, np.inf)
    assert (n == len(tris)).all() and (got["dist2"] == 0).all()   # without the flag every triangle finds itself or a neighbour


def bound_families(n, seed):
    """pairs for the bound check: random, small and far, an integer lattice, parallel sheets, scale 2^40, face-touching,
    corner-touching, tiny and huge triangles, points and segments"""
    rng = np.random.default_rng(seed)
    u = lambda lo, hi, *shape: rng.uniform(lo, hi, shape)
    out = {}
    out["random"] = (u(-1, 1, n, 3, 3), u(-1, 1, n, 3, 3) + u(-3, 3, n, 1, 3))
    out["small and far"] = (u(-1, 1, n, 3, 3) * 0.01, u(-1, 1, n, 3, 3) * 0.01 + u(-50, 50, n, 1, 3))
    out["lattice"] = (rng.integers(-4, 5, (n, 3, 3)), rng.integers(-4, 5, (n, 3, 3)))
    q, t = rng.integers(-4, 5, (n, 3, 3)).astype(float), rng.integers(-4, 5, (n, 3, 3)).astype(float)
    q[:, :, 2], t[:, :, 2] = 0, rng.integers(0, 3, (n, 1))
    out["parallel sheets"] = (q, t)
    out["scale 2^40"] = (u(-1, 1, n, 3, 3) * 2.0 ** 40, u(-1, 1, n, 3, 3) * 2.0 ** 40 + u(-3, 3, n, 1, 3) * 2.0 ** 40)
    q, t = u(-1, 1, n, 3, 3), u(-1, 1, n, 3, 3)
    b = rng.dirichlet((1, 1, 1), n)
    t[:, 0] = (b[:, :, None] * q).sum(1)   # a scene corner in the query's face
    out["face-touching"] = (q, t)
    q, t = u(-1, 1, n, 3, 3), u(-1, 1, n, 3, 3)
    t[:, 1] = q[:, 2]
    out["corner-touching"] = (q, t)
    out["tiny"] = (u(-1, 1, n, 1, 3) + u(-1, 1, n, 3, 3) * 1e-6, u(-1, 1, n, 1, 3) + u(-1, 1, n, 3, 3) * 1e-6)
    out["huge"] = (u(-1, 1, n, 3, 3) * 1e18, u(-1, 1, n, 3, 3) * 1e18)
    q, t = rng.integers(-3, 4, (n, 3, 3)).astype(float), u(-3, 3, n, 3, 3)
    q[::2, 1] = q[::2, 0]
    q[::4, 2] = q[::4, 0]
    t[1::3, 2] = t[1::3, 1]
    out["points and segments"] = (q, t)
    return {name: (np.asarray(q, F), np.asarray(t, F)) for name, (q, t) in out.items()}


def test_the_box_bound_never_exceeds_a_pair_s_dist2():
    """lb <= dist2 bit for bit, for the scene triangle's own vertex box and for a node's box that holds it (here: the box of the
    triangle and a second random one), with and without the intersecting stage"""
    o = PQ.NumpyOps
    for name, (q, t) in bound_families(40_000, 11).items():
        with np.errstate(all="ignore"):
            plain, feature, x, y = CR.pair_features(o, CR._corner_tuples(o, q), CR._corner_tuples(o, t))
            hit = CR.pair_intersects(q, t)
            d2, feature = np.where(hit, F(0), plain), np.where(hit, CR.PAIR_INTERSECTING, feature)
            qlo, qhi = CR.vertex_box(q)
            lo, hi = CR.vertex_box(t)
            own = CR.box_gap2(o, qlo, qhi, lo, hi)
        # the node's box: the min/max over the corners of this triangle and of another
        both = np.concatenate([t, np.roll(t, 1, 0)], 1)
        nlo = tuple(both[:, :, k].min(1) for k in range(3))
        nhi = tuple(both[:, :, k].max(1) for k in range(3))
        with np.errstate(all="ignore"):
            node = CR.box_gap2(o, qlo, qhi, nlo, nhi)
        assert np.isfinite(d2).all() and np.isfinite(own).all(), name
        assert (own <= d2).all() and (own <= plain).all(), (name, int((own > d2).sum()))
        assert (node <= own).all() and (node <= d2).all(), name
        assert (own[feature == CR.PAIR_INTERSECTING] == 0).all(), name
        for k in range(3):   # the witnesses lie in the two vertex boxes
            assert ((x[k] >= qlo[k]) & (x[k] <= qhi[k]) & (y[k] >= lo[k]) & (y[k] <= hi[k])).all(), name
        print(f"{name}: {len(q)} pairs, lb == dist2 on {int((own == d2).sum())}, lb > 0 on {int((own > 0).sum())}, intersecting {int((feature == 15).sum())}")


def accuracy_pairs(n, seed=21):
    rng = np.random.default_rng(seed)
    q = rng.uniform(-1, 1, (n, 3, 3)).astype(F)
    t = (rng.uniform(-1, 1, (n, 3, 3)) + rng.uniform(-3, 3, (n, 1, 3))).astype(F)
    return q, t


def test_float32_accuracy_against_float64():
    q, t = accuracy_pairs(ACCURACY_PAIRS)
    d32 = CR.pair_values(q, t)[0].astype(np.float64)
    d64 = CR.pair_values(q, t, CR.Float64Ops)[0]
    size2 = np.maximum(np.abs(q).max((1, 2)), np.abs(t).max((1, 2))).astype(np.float64) ** 2
    keep = d64 > 1e-6 * size2
    assert keep.mean() > 0.9
    rel = np.abs(d32[keep] - d64[keep]) / d64[keep]
    worst, p9999 = float(rel.max()), float(np.quantile(rel, 0.9999))
    print(f"float32 against float64 on {int(keep.sum())} of {len(q)} pairs: largest relative error {worst:.3g}, 99.99th percentile {p9999:.3g}")
    assert worst <= 2 * MEASURED_MAX and p9999 <= 2 * MEASURED_P9999, (worst, p9999)
    # where float64 says the pair is apart by that much, float32 does not call it intersecting
    assert (d32[keep] > 0).all()


def test_against_a_barycentric_sampling_of_both_triangles():
    """Independent of the formula: on disjoint pairs the float64 distance is never above the minimum over a 64 x 64 barycentric
    grid of either triangle, and not below it by more than two grid steps (a grid step: the longest edge / 64)."""
    q, t = accuracy_pairs(300, seed=22)
    d64 = CR.pair_values(q, t, CR.Float64Ops)[0]
    disjoint = d64 > 0
    assert disjoint.sum() > 250
    n = 64
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    inside = i + j <= n
    b = np.stack([i[inside], j[inside], n - i[inside] - j[inside]], 1) / n   # [S, 3] barycentric weights
    for row in np.nonzero(disjoint)[0]:
        Q, T = q[row].astype(np.float64), t[row].astype(np.float64)
        ps, ts = b @ Q, b @ T
        # |p - t|^2 as |p|^2 + |t|^2 - 2 p.t over all sample pairs (float64: its cancellation is far below the slack below)
        sampled = np.sqrt(max(((ps * ps).sum(1)[:, None] + (ts * ts).sum(1)[None, :] - 2.0 * (ps @ ts.T)).min(), 0.0))
        step = max(np.linalg.norm(Q - np.roll(Q, 1, 0), axis=1).max(), np.linalg.norm(T - np.roll(T, 1, 0), axis=1).max()) / n
        d = np.sqrt(d64[row])
        assert d <= sampled * (1 + 1e-9) and d >= sampled - 2 * step, (row, d, sampled, step)
