"""The within-radius restatement (tests/near_ref.py) pinned to cases known by hand: a flat grid of unit squares with a point above
it (counts and order at several radii, a radius exactly on a dist2 value), a point at a shared vertex (a tie at 0, ordered by
index, K below the tie), duplicated triangles, the radius and non-finite rules; then its two consequences (K = 1 is the
closest-point restatement in all 32 bytes; K is a prefix of any larger K) on lobed_528 with every kind of point, and a float64
check of the membership of the near set."""
import numpy as np

import near_cases
import near_ref as NR
import point_query_ref as R

F = np.float32


def grid(nx=4, ny=4):
    """unit squares in z = 0, each cut along the diagonal from (i, j) to (i + 1, j + 1): triangles 2 * (j * nx + i) + {0, 1}"""
    tris = []
    for j in range(ny):
        for i in range(nx):
            tris.append([(i, j, 0), (i + 1, j, 0), (i + 1, j + 1, 0)])
            tris.append([(i, j, 0), (i + 1, j + 1, 0), (i, j + 1, 0)])
    return np.asarray(tris, F).reshape(-1)


def points(p, max_dist2):
    p = np.asarray(p, F).reshape(-1, 3)
    out = np.zeros(len(p), R.POINT_DTYPE)
    out["p"], out["max_dist2"] = p, np.asarray(max_dist2, F)
    return out


AROUND_2_2 = [10, 11, 13, 18, 20, 21]   # the triangles with a corner at (2, 2), ascending


def is_miss(rec, pt):
    return (rec["triangle"] == -1 and rec["region"] == -1 and rec["u"] == 0 and rec["v"] == 0
            and rec["q"].view(np.uint32).tolist() == pt["p"].view(np.uint32).tolist()
            and rec["dist2"].view(np.uint32) == pt["max_dist2"].view(np.uint32))


def test_point_above_a_grid_vertex_counts_and_order():
    """p = (2, 2, 1): the six triangles around the vertex are at dist2 1 exactly; triangles 12 and 19 (their diagonal edges
    pass at planar distance sqrt(1/2)) at 1.5 exactly.  The bound is inclusive."""
    pos = grid()
    below = np.nextafter(F(1.5), F(0))
    pts = points([(2, 2, 1)] * 6, [0.5, 1.0, 1.25, below, 1.5, np.nextafter(F(1.0), F(0))])
    rec, n = NR.near(pos, pts, 8)
    assert n.tolist() == [0, 6, 6, 6, 8, 0]
    assert rec["triangle"][1].tolist() == AROUND_2_2 + [-1, -1]
    assert rec["triangle"][4].tolist() == AROUND_2_2 + [12, 19]
    assert rec["dist2"][4].tolist() == [1.0] * 6 + [1.5] * 2
    assert rec["region"][4].tolist()[6:] == [R.REGION_AC, R.REGION_AB]
    assert np.allclose(rec["q"][4][6], (2.5, 1.5, 0)) and np.allclose(rec["q"][4][7], (1.5, 2.5, 0))
    for row in (0, 5):
        assert all(is_miss(rec[row, k], pts[row]) for k in range(8))
    assert is_miss(rec[1, 6], pts[1]) and is_miss(rec[1, 7], pts[1])
    # the whole grid within a large radius, ordered by (dist2, index)
    rec, n = NR.near(pos, points([(2, 2, 1)], [np.inf]), 64)
    assert n.tolist() == [32] and (rec["triangle"][0, 32:] == -1).all()
    key = list(zip(rec["dist2"][0, :32].tolist(), rec["triangle"][0, :32].tolist()))
    assert key == sorted(key) and sorted(rec["triangle"][0, :32].tolist()) == list(range(32))


def test_point_at_a_shared_vertex_ties_at_zero_by_index():
    pos = grid()
    pts = points([(2, 2, 0)] * 2, [0.0, np.inf])
    rec, n = NR.near(pos, pts, 8)
    assert n.tolist() == [6, 32]
    for row in range(2):
        assert rec["triangle"][row, :6].tolist() == AROUND_2_2 and (rec["dist2"][row, :6] == 0).all()
    assert (rec["triangle"][0, 6:] == -1).all() and (rec["dist2"][1, 6:] > 0).all()
    rec4, n4 = NR.near(pos, pts, 4)   # K below the tie keeps the lowest indices
    assert n4.tolist() == [6, 32] and rec4["triangle"].tolist() == [AROUND_2_2[:4]] * 2


def test_duplicated_triangles_are_all_members_in_index_order():
    t = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    u = [5, 5, 5, 6, 5, 5, 5, 6, 5]
    pos = np.asarray(t + t + u + t, F)
    rec, n = NR.near(pos, points([(0.25, 0.25, 2)], [4.0]), 4)
    assert n.tolist() == [3] and rec["triangle"][0].tolist() == [0, 1, 3, -1] and (rec["dist2"][0, :3] == 4.0).all()
    assert (NR.as_bits(rec[0, 0])[0, :6] == NR.as_bits(rec[0, 1])[0, :6]).all() and rec["region"][0, :3].tolist() == [R.REGION_FACE] * 3
    rec, n = NR.near(pos, points([(0.25, 0.25, 2)], [4.0]), 2)
    assert n.tolist() == [3] and rec["triangle"][0].tolist() == [0, 1]


def test_radius_and_non_finite_rules():
    pos = grid()
    p = [(2.25, 2.5, 0), (2.25, 2.5, 0), (2.25, 2.5, 0), (2.25, 2.5, 0), (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (2.25, 2.5, 3)]
    md = [0.0, -1.0, np.nan, np.inf, np.inf, 1.0, 1.0, np.inf]
    pts = points(p, md)
    rec, n = NR.near(pos, pts, 3)
    assert n.tolist() == [1, 0, 0, 32, 0, 0, 0, 32]
    assert rec["triangle"][0].tolist() == [21, -1, -1] and rec["dist2"][0, 0] == 0 and rec["region"][0, 0] == R.REGION_FACE
    for row in (1, 2, 4, 5, 6):   # nothing is walked: miss records with max_dist2 as given (NaN and -1 kept)
        assert all(is_miss(rec[row, k], pts[row]) for k in range(3))
    assert is_miss(rec[0, 1], pts[0])
    assert (rec["triangle"][3] >= 0).all() and (rec["triangle"][7] >= 0).all()
    # K = 0: counts alone
    rec0, n0 = NR.near(pos, pts, 0)
    assert rec0.shape == (len(pts), 0) and n0.tolist() == n.tolist()
    # a dist2 that overflows to +inf is within max_dist2 = +inf, and within nothing else
    far = points([(3e19, 0, 0)] * 2, [np.inf, 3e38])
    rec, n = NR.near(pos, far, 2)
    assert n.tolist() == [32, 0] and np.isinf(rec["dist2"][0]).all() and rec["triangle"][0].tolist() == [0, 1]


def lobed(pkg):
    world = pkg.World(near_cases.scene_path("lobed_528"))
    try:
        return {k: np.array(v) for k, v in world.arrays().items() if k in ("vertex_positions", "group_boxmin", "group_boxmax")}
    finally:
        world.close()


def test_k1_is_the_closest_point_restatement_and_k_is_a_prefix(pkg):
    """On lobed_528 with the seven kinds of point: K = 1 equals point_query_ref.closest in all 32 bytes, misses included,
    with no exception; the records for K are the first K of the records for 64; the counts do not depend on K."""
    arrays = lobed(pkg)
    pts = near_cases.make_points(arrays, 3000, seed=5)
    pos = arrays["vertex_positions"]
    rec64, n64 = NR.near(pos, pts, 64)
    rec1, n1 = NR.near(pos, pts, 1)
    want = R.closest(pos, pts)
    assert (want["triangle"] >= 0).sum() > len(pts) // 2 and (want["triangle"] < 0).sum() > len(pts) // 20
    assert np.array_equal(NR.as_bits(rec1[:, 0]), R.as_bits(want))
    assert ((n64 > 64).mean() > 0.3) and ((n64 > 8) & np.isfinite(pts["max_dist2"])).mean() > 0.1
    for k in (1, 2, 3, 4, 8, 9):
        rec, n = NR.near(pos, pts, k)
        assert np.array_equal(n, n64)
        assert np.array_equal(NR.as_bits(rec), NR.as_bits(rec64[:, :k]))
    # the records are sorted by the key, members first, and hold min(n, K) members
    members = rec64["triangle"] >= 0
    assert np.array_equal(members.sum(1), np.minimum(n64, 64))
    assert (members[:, :-1] >= members[:, 1:]).all()
    both = members[:, :-1] & members[:, 1:]
    d, t = rec64["dist2"], rec64["triangle"]
    assert ((d[:, :-1] < d[:, 1:]) | ((d[:, :-1] == d[:, 1:]) & (t[:, :-1] < t[:, 1:])))[both].all()


class Float64Ops(R.NumpyOps):
    """the same formulas in float64"""

    @staticmethod
    def f(x):
        return np.asarray(x, np.float64)


def test_membership_agrees_with_float64():
    """Wherever the float64 dist2 is not within rounding of max_dist2, the fp32 near set has exactly the float64 members.
    The band: a relative 1e-4 of the larger of the two (fp32 rounds each of the few dozen operations to 6e-8 relative; the
    triangles are well shaped, so nothing amplifies it a thousandfold) plus 1e-9 for values at zero."""
    rng = np.random.default_rng(17)
    centres = rng.normal(size=(300, 1, 3)) * 2
    pos = (centres + rng.normal(size=(300, 3, 3)) * 0.5).astype(F).reshape(-1)
    p = (rng.normal(size=(400, 3)) * 2.5).astype(F)
    md = (rng.random(400) * 3).astype(F) ** 2
    pts = points(p, md)
    d32 = NR.pair_dist2(R.NumpyOps, pos, pts)
    with np.errstate(all="ignore"):
        d64 = NR.pair_dist2(Float64Ops, pos.astype(np.float64), pts)   # (stored as float32: rounding far inside the band)
    rec, n = NR.near(pos, pts, 64)
    clear = np.abs(d64.astype(np.float64) - md[:, None]) > 1e-4 * np.maximum(d64, md[:, None]) + 1e-9
    assert clear.mean() > 0.99
    assert np.array_equal((d32 <= md[:, None])[clear], (d64 <= md[:, None])[clear])
    assert np.array_equal(n, (d32 <= md[:, None]).sum(1)) and n.max() > 64 and (n == 0).any()
    for row in range(len(pts)):
        got = set(rec["triangle"][row][rec["triangle"][row] >= 0].tolist())
        assert got <= set(np.nonzero(d32[row] <= md[row])[0].tolist())
