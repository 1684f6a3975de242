"""The closest-point restatement (tests/point_query_ref.py) pinned to analytic cases: each Voronoi region of a triangle with its
region code and point, degenerate triangles (finite and deterministic), the lowest index on a tie, the max_dist2 and non-finite
point rules of a miss; a float64 check of the distances; the torch form against the numpy one; and the exactness bound of
the walk, lb <= dist2 bit for bit, on seeded random points against random triangles and their vertex boxes."""
import numpy as np
import pytest

import point_query_ref as R

F = np.float32
TRI = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], F)   # a = origin, b = +x, c = +y


def run(positions, pts, max_dist2=np.inf):
    pts = np.asarray(pts, F).reshape(-1, 3)
    points = np.zeros(len(pts), R.POINT_DTYPE)
    points["p"] = pts
    points["max_dist2"] = np.asarray(max_dist2, F)
    return R.closest(np.asarray(positions, F), points)


@pytest.mark.parametrize("p, region, q, uv", [
    ((-1, -1, 0), R.REGION_A, (0, 0, 0), (0, 0)),
    ((0, 0, 0), R.REGION_A, (0, 0, 0), (0, 0)),
    ((2, -0.5, 0.5), R.REGION_B, (1, 0, 0), (1, 0)),
    ((1, 0, 0), R.REGION_B, (1, 0, 0), (1, 0)),
    ((-0.5, 2, -3), R.REGION_C, (0, 1, 0), (0, 1)),
    ((0.5, -1, 0), R.REGION_AB, (0.5, 0, 0), (0.5, 0)),
    ((0.25, 0, 0), R.REGION_AB, (0.25, 0, 0), (0.25, 0)),
    ((-1, 0.75, 1), R.REGION_AC, (0, 0.75, 0), (0, 0.75)),
    ((1, 1, 0), R.REGION_BC, (0.5, 0.5, 0), (0.5, 0.5)),
    ((0.75, 0.25, 0), R.REGION_BC, (0.75, 0.25, 0), (0.75, 0.25)),
    ((0.25, 0.25, 0), R.REGION_FACE, (0.25, 0.25, 0), (0.25, 0.25)),
    ((0.25, 0.5, 2), R.REGION_FACE, (0.25, 0.5, 0), (0.25, 0.5)),
    ((0.125, 0.25, -3), R.REGION_FACE, (0.125, 0.25, 0), (0.125, 0.25)),
])
def test_each_region(p, region, q, uv):
    r = run(TRI, [p])[0]
    assert r["triangle"] == 0 and r["region"] == region
    assert r["q"].tolist() == list(q)
    assert (r["u"], r["v"]) == uv
    d = np.asarray(p, np.float64) - np.asarray(q, np.float64)
    assert r["dist2"] == F(d @ d)


@pytest.mark.parametrize("tri", [
    [1, 2, 3] * 3,                                 # zero area: one point three times
    [0, 0, 0, 0, 0, 0, 2, 1, 0],                   # a repeated vertex
    [0, 0, 0, 1, 1, 1, 2, 2, 2],                   # collinear
    [0, 0, 0, 2, 2, 2, 1, 1, 1],                   # collinear, the middle vertex last
    [0, 0, 0, 1e-30, 0, 0, 0, 1e-30, 0],           # tiny: products underflow
    [-3e18, 0, 0, 3e18, 1, 0, 0, 3e18, 1],         # huge: products overflow
])
def test_degenerate_triangles_are_finite_and_deterministic(tri):
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.normal(size=(200, 3)) * 3, np.asarray(tri, F).reshape(3, 3)]).astype(F)
    a = run(tri, pts)
    b = run(tri, pts)
    assert np.array_equal(R.as_bits(a), R.as_bits(b))
    assert (a["triangle"] == 0).all() and np.isfinite(a["q"]).all() and np.isfinite(a["u"]).all() and np.isfinite(a["v"]).all()
    assert ((a["dist2"] >= 0) | np.isinf(a["dist2"])).all()
    corners = np.asarray(tri, F).reshape(3, 3)
    assert (a["q"] >= corners.min(0)).all() and (a["q"] <= corners.max(0)).all()


def test_collinear_triangle_distance_is_the_segments():
    """For a degenerate (collinear) triangle the answer still lies on the segment and is close to the true distance."""
    tri = np.array([0, 0, 0, 1, 0, 0, 3, 0, 0], F)
    pts = np.array([[2, 1, 0], [-1, 0, 0], [4, 2, 0], [0.5, 0, 3]], F)
    r = run(tri, pts)
    want = [1.0, 1.0, 5.0, 9.0]
    assert np.allclose(r["dist2"], want, rtol=1e-6), r["dist2"]


def test_duplicated_triangles_lowest_index_wins():
    other = np.array([5, 5, 5, 6, 5, 5, 5, 6, 5], F)
    for order, want in (((TRI, TRI, other), 0), ((other, TRI, TRI, TRI), 1), ((other, TRI[[3, 4, 5, 6, 7, 8, 0, 1, 2]], TRI), 1)):
        pos = np.concatenate(order)
        r = run(pos, [(0.25, 0.25, 1), (0.25, 0.25, 0)])
        assert (r["triangle"] == want).all(), (want, r["triangle"])
    # the chunking must not change the tie rule: the duplicate lands in a later chunk
    pos = np.concatenate([other] * 5 + [TRI] + [other] * 5 + [TRI])
    pts = np.zeros(1, R.POINT_DTYPE)
    pts["p"] = (0.25, 0.25, 1)
    pts["max_dist2"] = np.inf
    for pairs in (1, 3, 7, 1 << 10):
        r = R.closest(pos, pts, point_chunk=1, pairs=pairs)
        assert r["triangle"][0] == 5 and r["dist2"][0] == 1


def test_max_dist2_and_non_finite_points():
    pts = [(0.25, 0.25, 0), (0.25, 0.25, 2), (0.25, 0.25, 2), (0.25, 0.25, 2), (0.25, 0.25, 2), (0.25, 0.25, 2),
           (0.25, 0.25, 0), (0.25, 0.25, 2), (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)]
    md = np.array([0, 0, 4, 3.9999998, np.inf, -1, -0.0, np.nan, np.inf, np.inf, np.inf], F)
    r = run(TRI, pts, md)
    hit = [True, False, True, False, True, False, True, False, False, False, False]
    assert ((r["triangle"] >= 0) == hit).all(), r["triangle"]
    miss = ~np.asarray(hit)
    pts = np.asarray(pts, F)
    assert (r["region"][miss] == -1).all() and (r["u"][miss] == 0).all() and (r["v"][miss] == 0).all()
    assert np.array_equal(r["q"][miss].view(np.uint32), pts[miss].view(np.uint32))
    assert np.array_equal(r["dist2"][miss].view(np.uint32), md[miss].view(np.uint32))
    assert r["dist2"][2] == 4 and r["dist2"][4] == 4 and r["dist2"][0] == 0


def random_mesh(rng, n):
    centres = rng.normal(size=(n, 1, 3)) * 4
    return (centres + rng.normal(size=(n, 3, 3)) * rng.choice([0.01, 0.3, 2.0], size=(n, 1, 1))).astype(F).reshape(-1)


def test_distances_agree_with_float64():
    """The fp32 answer is the true nearest distance to within rounding (against a dense float64 sampling of every triangle)."""
    rng = np.random.default_rng(11)
    pos = random_mesh(rng, 60)
    pts = (rng.normal(size=(300, 3)) * 5).astype(F)
    r = run(pos, pts)
    T = pos.reshape(-1, 3, 3).astype(np.float64)
    # the float64 truth: the minimum over a dense barycentric sampling is an upper bound, the fp32 answer must not beat it
    # by more than rounding, and the fp32 point must be at its stated distance
    g = np.linspace(0, 1, 41)
    uu, vv = np.meshgrid(g, g)
    keep = uu + vv <= 1
    uu, vv = uu[keep], vv[keep]
    samples = T[:, None, 0] + uu[None, :, None] * (T[:, None, 1] - T[:, None, 0]) + vv[None, :, None] * (T[:, None, 2] - T[:, None, 0])
    samples = samples.reshape(-1, 3)
    d2 = ((pts[:, None, :].astype(np.float64) - samples[None]) ** 2).sum(-1).min(1)
    assert (r["dist2"] <= d2 * (1 + 1e-5) + 1e-12).all()
    q = r["q"].astype(np.float64)
    assert np.allclose(((pts - q) ** 2).sum(1), r["dist2"], rtol=1e-5, atol=1e-12)
    assert (r["triangle"] >= 0).all()


def test_torch_restatement_matches_numpy():
    torch = pytest.importorskip("torch")
    del torch
    rng = np.random.default_rng(5)
    pos = random_mesh(rng, 97)
    pos[:9] = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1], F)   # a degenerate one
    pts = np.zeros(700, R.POINT_DTYPE)
    pts["p"] = (rng.normal(size=(700, 3)) * 5).astype(F)
    pts["max_dist2"] = np.where(rng.random(700) < 0.5, np.inf, rng.random(700) * 4).astype(F)
    pts["p"][:20] = pos.reshape(-1, 3)[:20]
    pts["p"][20, 1] = np.nan
    pts["max_dist2"][21] = -1
    a = R.closest(pos, pts, point_chunk=64, pairs=1 << 12)
    b = R.closest_torch(pos, pts, device="cpu", point_chunk=100, pairs=1 << 13)
    assert np.array_equal(R.as_bits(a), R.as_bits(b))


def test_box_bound_never_exceeds_dist2_bitwise():
    """lb(p, vertex box of a triangle) <= dist2(p, triangle) in fp32 for every pair: random points, points on the box faces
    and corners, far points (the sums overflow to +inf), and tiny and huge triangles."""
    rng = np.random.default_rng(2026)
    tris = np.concatenate([random_mesh(rng, 400).reshape(-1, 9),
                           (rng.normal(size=(50, 9)) * 1e-20).astype(F), (rng.normal(size=(50, 9)) * 1e18).astype(F)])
    corners = tris.reshape(-1, 3, 3)
    lo, hi = corners.min(1), corners.max(1)
    o = R.NumpyOps
    with np.errstate(all="ignore"):
        for kind in range(4):
            n = len(tris)
            if kind == 0:
                p = (rng.normal(size=(n, 3)) * rng.choice([0.1, 3, 1e3], size=(n, 1))).astype(F)
            elif kind == 1:   # on a face of the box: one coordinate on a plane, the others inside or out
                p = (lo + (hi - lo) * rng.random((n, 3)) * 1.5 - (hi - lo) * 0.25).astype(F)
                axis = rng.integers(0, 3, n)
                p[np.arange(n), axis] = np.where(rng.random((n, 1)) < 0.5, lo, hi)[np.arange(n), axis]
            elif kind == 2:   # at a corner
                p = np.where(rng.random((n, 3)) < 0.5, lo, hi).astype(F)
            else:             # far away
                p = (rng.normal(size=(n, 3)) * 1e19).astype(F)
            P = tuple(p[:, k] for k in range(3))
            a, b, c = (tuple(corners[:, j, k] for k in range(3)) for j in range(3))
            _, d2, _, _, _ = R.closest_on_triangles(o, P, a, b, c)
            lb = R.box_bound(o, P, tuple(lo[:, k] for k in range(3)), tuple(hi[:, k] for k in range(3)))
            assert not np.isnan(d2).any() and not np.isnan(lb).any()
            assert (lb <= d2).all(), (kind, np.nonzero(~(lb <= d2))[0][:5])
            # and for a node box that holds the triangle's box strictly
            lb_node = R.box_bound(o, P, tuple((lo[:, k] - F(1)) for k in range(3)), tuple((hi[:, k] + F(1)) for k in range(3)))
            assert (lb_node <= lb).all()
