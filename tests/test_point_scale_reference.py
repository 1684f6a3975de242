"""The cases of tests/point_scale_cases.py pinned on the CPU, so that tests/test_gpu_point_query_scale.py's references cannot
quietly be wrong: the restatements of the four point-query clients on scenes scaled by S = 2^k.

A "covariant" cell of the TABLE: the restatement on `positions * S` (numpy, the unscaled triangle order and tree) equals the
S = 1 result scaled by the exact power of two, bit for bit, for every record.  The float64 bounds the project holds at S = 1
(tests/test_point_query_reference.py, test_sdf_reference.py, test_winding_reference.py) therefore carry over unchanged.
An "outside" cell: at least one record differs from that prediction (the flag is not pessimistic), and the invariants of the
definition hold, which no scale may break.  Every cell has at least 5 % hits and 5 % misses.
"""
import math

import numpy as np
import pytest

import near_ref as NR
import point_query_ref as R
import point_scale_cases as PC
import ray_scale_cases as X
import refit_ref
import sdf_ref as SD
import winding_ref as W
from test_gpu_point_query import scene_path

F = np.float32
CASES = [(name, k) for name in PC.SCENES for k in PC.S_EXPONENTS]
REQUIRED = (-70, -64, -40, -31, -20, 0, 20, 32, 33, 40, 63, 64)
K = 64   # SHRAY_NEAR_MAX
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def closest_at(pkg, name, k):
    """(points, records) of the restatement at S = 2^k"""
    def make():
        pts = PC.points(pkg, name, k)
        return pts, R.closest(PC.scaled_positions(pkg, name, k), pts)
    return memo(("closest", name, k), make)


def near_at(pkg, name, k):
    def make():
        pts = PC.points(pkg, name, k, "near")
        return (pts,) + NR.near(PC.scaled_positions(pkg, name, k), pts, K)
    return memo(("near", name, k), make)


def derived_at(pkg, name, k):
    return memo(("derive", name, k), lambda: SD.derive(PC.scaled_positions(pkg, name, k)))


def tree_of(pkg, name):
    def make():
        world = pkg.World(scene_path(name))
        tree = refit_ref.TreeArrays.of(world.export_tree())
        return world, tree
    return memo(("tree", name), make)


def winding_at(pkg, name, k):
    """the restatement of the scene refit to positions * S: the unscaled tree, the boxes of the scaled corners"""
    def make():
        world, tree = tree_of(pkg, name)
        pos = PC.scaled_positions(pkg, name, k)
        return W.Restated(world, positions=pos, boxes=refit_ref.node_boxes(tree, pos.reshape(-1, 3)))
    return memo(("winding", name, k), make)


@pytest.fixture(scope="module", autouse=True)
def close_the_worlds():
    yield
    for key, value in _memo.items():
        if key[0] == "tree":
            value[0].close()
    _memo.clear()


def test_the_table_covers_the_cases():
    assert set(REQUIRED) <= set(PC.S_EXPONENTS) and tuple(sorted(PC.S_EXPONENTS)) == PC.S_EXPONENTS
    for client in PC.CLIENTS:
        for name in PC.SCENES:
            row = PC.TABLE[client][name]
            assert len(row) == len(PC.S_EXPONENTS) and set(row) <= {"c", "o"}, (client, name)
            assert PC.flag(client, name, 0) == PC.COVARIANT
            core = row.strip("o")            # one covariant interval around S = 1
            assert core == "c" * len(core), (client, name)


@pytest.mark.parametrize("name", PC.SCENES)
def test_scaled_positions_are_exact(pkg, name):
    """positions * S stays finite and non-zero at every k; every coordinate that is not rounding noise about 0 (a few
    hundred of 1e-17, 2^-56; the others are 0.017 and more) stays normal and back-scales to the unscaled bits at every k of the TABLE"""
    base = X.base_arrays(pkg, name).positions.reshape(-1)
    assert np.abs(base).max() < 1.72
    real = np.abs(base) >= F(2.0 ** -50)
    assert np.abs(base[real]).min() > 0.01
    for k in PC.S_EXPONENTS + (PC.ALL_TIES_UNDERFLOW,):
        pos = PC.scaled_positions(pkg, name, k)
        assert np.isfinite(pos).all() and np.array_equal(pos == 0, base == 0)
        if k != PC.ALL_TIES_UNDERFLOW:
            assert (np.abs(pos[real]) >= np.finfo(F).tiny).all()
            assert np.array_equal((pos[real].astype(np.float64) * 2.0 ** -k).astype(F).view(np.uint32), base[real].view(np.uint32))


def pair_rows(positions, pts, rows):
    """dist2 of every (point, triangle) pair for the given rows, float32 [len(rows), T]"""
    with np.errstate(all="ignore"):
        return NR.pair_dist2(R.NumpyOps, positions, pts[rows])


def closest_invariants(positions, pts, rec, what):
    """what the definition promises at any scale, for CLOSEST_DTYPE records of any shape against pts (leading axis)"""
    tris = np.asarray(positions, F).reshape(-1, 3, 3)
    T = len(tris)
    shape = rec.shape
    p = np.broadcast_to(pts["p"].reshape((shape[0],) + (1,) * (rec.ndim - 1) + (3,)), shape + (3,))
    md = np.broadcast_to(pts["max_dist2"].reshape((shape[0],) + (1,) * (rec.ndim - 1)), shape)
    tri, region = rec["triangle"], rec["region"]
    hit = tri >= 0
    assert ((tri == R.HIT_MISS) | ((tri >= 0) & (tri < T))).all(), what
    assert ((region >= -1) & (region <= 6)).all() and np.array_equal(region == -1, ~hit), what
    walked = NR.walked(pts).reshape((shape[0],) + (1,) * (rec.ndim - 1))
    assert not (hit & ~walked).any(), what
    # a miss carries p and max_dist2 as given
    miss = ~hit
    assert np.array_equal(rec["q"][miss].view(np.uint32), p[miss].view(np.uint32)), what
    assert np.array_equal(rec["dist2"][miss].view(np.uint32), md[miss].view(np.uint32)), what
    assert (rec["u"][miss] == 0).all() and (rec["v"][miss] == 0).all(), what
    # a hit: q in the vertex box of its triangle, dist2 recomputed, within the radius, no NaN
    v = tris[tri[hit]]
    q, ph = rec["q"][hit], p[hit]
    assert ((q >= v.min(1)) & (q <= v.max(1))).all(), what
    with np.errstate(all="ignore"):
        d = ph - q
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert np.array_equal(d2.view(np.uint32), rec["dist2"][hit].view(np.uint32)), what
    assert (rec["dist2"][hit] <= md[hit]).all(), what
    for f in ("q", "dist2", "u", "v"):
        assert not np.isnan(rec[f][hit]).any(), (what, f)
    clean = np.isfinite(pts["p"]).all(1) & ~np.isnan(pts["max_dist2"])
    for f in ("q", "dist2", "u", "v"):
        assert not np.isnan(rec[f][clean]).any(), (what, f)


def lowest_index_wins(positions, pts, rec, what, sample=600):
    """against the pairs themselves, on a sample of the points: the reported triangle is the first of the smallest dist2 within
    the radius, and a miss has none; returns how many sampled points had EVERY triangle at one dist2 (a full tie)"""
    rows = np.random.default_rng(3).choice(len(pts), min(sample, len(pts)), replace=False)
    d2 = pair_rows(positions, pts, rows)
    md = pts["max_dist2"][rows]
    with np.errstate(all="ignore"):
        member = (d2 <= md[:, None]) & NR.walked(pts[rows])[:, None]
    key = np.where(member, d2, F(np.inf))
    first = np.where(member & (key == key.min(1, keepdims=True)), np.arange(d2.shape[1])[None], d2.shape[1]).min(1)
    want = np.where(member.any(1), first, R.HIT_MISS)
    assert np.array_equal(rec["triangle"][rows], want), what
    full = member.all(1) & (d2 == d2[:, :1]).all(1)
    assert (rec["triangle"][rows][full] == 0).all(), what
    return int(full.sum())


@pytest.mark.parametrize("name, k", CASES)
def test_closest(pkg, name, k):
    pts1, rec1 = closest_at(pkg, name, 0)
    pts, rec = closest_at(pkg, name, k)
    hits = int((rec["triangle"] >= 0).sum())
    assert 0.05 * len(pts) <= hits <= 0.95 * len(pts), (name, k, hits)
    same = PC.same_records(rec, PC.scale_closest(rec1, k, pts))
    print(f"closest {name} k {k}: {same.mean() * 100:.3f} % covariant, {hits} hits of {len(pts)}")
    positions = PC.scaled_positions(pkg, name, k)
    if PC.flag("closest", name, k) == PC.COVARIANT:
        assert same.all(), (name, k, int((~same).sum()))
        assert np.array_equal(rec["triangle"], rec1["triangle"]) and np.array_equal(rec["region"], rec1["region"])
        assert np.array_equal(rec["u"].view(np.uint32), rec1["u"].view(np.uint32))
    else:
        assert not same.all(), (name, k, "the cell is covariant: the TABLE is pessimistic")
    closest_invariants(positions, pts, rec, (name, k))
    full = lowest_index_wins(positions, pts, rec, (name, k))
    if k >= 63:
        # make_points' far class with radius +inf: every dist2 is +inf, triangle 0 wins (a seventh of 600, 60 % of them: 51 expected)
        assert full >= 30, (name, k, full)


@pytest.mark.parametrize("name, k", CASES)
def test_near(pkg, name, k):
    pts1, rec1, n1 = near_at(pkg, name, 0)
    pts, rec, n = near_at(pkg, name, k)
    assert (n > 0).mean() >= 0.05 and (n == 0).mean() >= 0.05, (name, k)
    same = PC.same_records(rec, PC.scale_closest(rec1, k, pts)).all(1) & (n == n1)
    print(f"near {name} k {k}: {same.mean() * 100:.3f} % covariant, n > 0 {(n > 0).mean():.3f}, n > {K} {(n > K).mean():.3f}")
    positions = PC.scaled_positions(pkg, name, k)
    if PC.flag("near", name, k) == PC.COVARIANT:
        assert same.all(), (name, k, int((~same).sum()))
    else:
        assert not same.all(), (name, k, "the cell is covariant: the TABLE is pessimistic")
    closest_invariants(positions, pts, rec, (name, k))
    # kept records: min(n, K) of them, then misses; sorted by (dist2, index); the count is that of the pairs within the radius
    kept = rec["triangle"] >= 0
    assert np.array_equal(kept.sum(1), np.minimum(n, K)) and np.array_equal(kept, np.arange(K)[None] < kept.sum(1)[:, None])
    d, t = rec["dist2"], rec["triangle"]
    both = kept[:, 1:]
    assert ((d[:, :-1] < d[:, 1:]) | ((d[:, :-1] == d[:, 1:]) & (t[:, :-1] < t[:, 1:])))[both].all(), (name, k)
    rows = np.random.default_rng(4).choice(len(pts), 400, replace=False)
    d2 = pair_rows(positions, pts, rows)
    with np.errstate(all="ignore"):
        member = (d2 <= pts["max_dist2"][rows][:, None]) & NR.walked(pts[rows])[:, None]
    assert np.array_equal(n[rows], member.sum(1)), (name, k)
    # the first record is the closest-point query's: the smallest dist2, the lowest index on a tie
    key = np.where(member, d2, F(np.inf))
    first = np.where(member & (key == key.min(1, keepdims=True)), np.arange(d2.shape[1])[None], d2.shape[1]).min(1)
    assert np.array_equal(t[rows, 0], np.where(member.any(1), first, R.HIT_MISS)), (name, k)
    if k >= 63:
        full = member.all(1) & (d2 == d2[:, :1]).all(1)
        # nothing but ties, so index order (a seventh of the points are far and 35 % of the radii +inf: 20 of 400 expected)
        assert full.sum() >= 10 and (t[rows][full] == np.arange(K)[None]).all(), (name, k)


@pytest.mark.parametrize("name, k", CASES)
def test_signed_distance(pkg, name, k):
    pts1, rec1 = closest_at(pkg, name, 0)
    pts, rec = closest_at(pkg, name, k)
    d1, dk = derived_at(pkg, name, 0), derived_at(pkg, name, k)
    s1 = SD.signed(pts1, rec1, d1["sign_data"])
    sk = SD.signed(pts, rec, dk["sign_data"])
    with np.errstate(all="ignore"):
        same = PC.same_floats(sk, s1 * F(2.0 ** k))
    data_same = PC.same_floats(dk["sign_data"], d1["sign_data"])   # nhat and the pseudonormals carry S^0
    print(f"sdf {name} k {k}: values {same.mean() * 100:.3f} %, sign data {data_same.mean() * 100:.3f} % covariant, "
          f"degenerate {dk['info']['degenerate_triangles']}")
    assert 0.05 <= np.isnan(sk).mean() <= 0.95
    if PC.flag("sdf", name, k) == PC.COVARIANT:
        assert same.all() and data_same.all() and dk["info"] == d1["info"], (name, k)
    else:
        assert not (same.all() and data_same.all()), (name, k, "the cell is covariant: the TABLE is pessimistic")
    # the definition's invariants: NaN exactly on a miss; |value| = sqrtf(dist2); the weld does not depend on the scale
    hit = rec["triangle"] >= 0
    assert np.array_equal(np.isnan(sk), ~hit)
    with np.errstate(all="ignore"):
        assert np.array_equal(np.abs(sk[hit]).view(np.uint32), np.sqrt(rec["dist2"][hit]).view(np.uint32))
    assert (sk[hit & (rec["dist2"] == 0)] == 0).all() and not np.signbit(sk[hit & (rec["dist2"] == 0)]).any()
    for key in ("vertices", "edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges", "closed"):
        assert dk["info"][key] == d1["info"][key], (name, k, key)
    T = len(dk["sign_data"])
    assert 0 <= dk["info"]["degenerate_triangles"] <= T
    assert dk["info"]["degenerate_triangles"] == int((dk["sign_data"][:, 0] == 0).all(1).sum())
    assert not np.isnan(dk["sign_data"][:, 0]).any()


def away_from_the_surface(pkg, name):
    """bool per point of the cell: finite, and at least 1e-3 x extent from the unscaled surface (tests/test_winding_reference.py)"""
    def make():
        pts = PC.base_points(pkg, name).copy()
        pts["max_dist2"] = np.inf
        pos = X.base_arrays(pkg, name).positions.reshape(-1, 3)
        extent = float(np.linalg.norm(pos.max(0) - pos.min(0)))
        dist = np.sqrt(R.closest(pos.reshape(-1), pts)["dist2"].astype(np.float64))
        return np.isfinite(pts["p"]).all(1) & (dist >= 1e-3 * extent)
    return memo(("away", name), make)


@pytest.mark.parametrize("name, k", CASES)
def test_winding(pkg, name, k):
    pts = PC.points(pkg, name, k)
    finite = np.isfinite(pts["p"]).all(1)
    assert finite.mean() > 0.9 and (~finite).sum() >= 10
    w1 = memo(("w", name, 0), lambda: winding_at(pkg, name, 0).w(PC.points(pkg, name, 0), math.inf))
    ref = winding_at(pkg, name, k)
    wk = memo(("w", name, k), lambda: ref.w(pts, math.inf))
    same = PC.same_floats(wk, w1)
    nan_finite = int(np.isnan(wk[finite]).sum())
    print(f"winding {name} k {k}: exact mode {same.mean() * 100:.3f} % covariant, NaN for {nan_finite} of {int(finite.sum())} finite points")
    assert np.isnan(wk[~finite]).all()
    if PC.flag("winding", name, k) == PC.COVARIANT:
        assert same.all(), (name, k, int((~same).sum()))
        assert (w1[finite] > 0.5).mean() > 0.05 and (w1[finite] < 0.5).mean() > 0.05
        # finite beta is not covariant (the boxes' absolute pad); its inside test agrees with the exact mode's away from the surface
        if k <= PC.FINITE_BETA_MAX_EXPONENT:
            away = away_from_the_surface(pkg, name)
            w2 = ref.w(pts[away], 2.0)
            print(f"winding {name} k {k}: max |w(beta 2) - w(exact)| {np.abs(w2.astype(np.float64) - wk[away]).max():.3e} over {int(away.sum())} points")
            assert away.sum() > 1000 and np.array_equal(w2 > 0.5, wk[away] > 0.5), (name, k)
    else:
        assert not same.all(), (name, k, "the cell is covariant: the TABLE is pessimistic")
    # NaN exactly for the non-finite points, up to the scale where det = dot(a', cross(b', c')), of degree 3, meets inf - inf
    if k <= PC.EXACT_WINDING_NAN_FREE_MAX_EXPONENT:
        assert nan_finite == 0, (name, k, nan_finite)
    elif k >= PC.EXACT_WINDING_ALL_NAN_MIN_EXPONENT:
        assert nan_finite == int(finite.sum()), (name, k, nan_finite)
    if k <= PC.EXACT_WINDING_ALL_ZERO_MAX_EXPONENT:
        assert (wk[finite] == 0).all() and not np.signbit(wk[finite]).any()    # every det underflows: the zero rule, w = +0


@pytest.mark.parametrize("name", PC.SCENES)
def test_finite_beta_is_nan_where_the_far_term_overflows(pkg, name):
    """The rule found for finite beta: T_far's dot(d, m) is of degree 5 in S (m = M d, M of degree 3) and meets inf - inf long
    before the exact mode's degree 3 does.  At S = 2^20 no finite point is NaN; at S = 2^32 every finite point is, while the
    exact mode has none."""
    for k, every in ((20, False), (32, True)):
        pts = PC.points(pkg, name, k)[:400]
        finite = np.isfinite(pts["p"]).all(1)
        ref = winding_at(pkg, name, k)
        w2 = ref.w(pts, 2.0)
        assert np.isnan(w2[~finite]).all()
        assert np.isnan(w2[finite]).all() if every else not np.isnan(w2[finite]).any(), (name, k)
        assert not np.isnan(ref.w(pts, math.inf)[finite]).any()


@pytest.mark.parametrize("name", PC.SCENES)
def test_the_special_class(pkg, name):
    """S = 1, coordinates of p replaced by +-0, the smallest denormal, 2^-64, 2^63, 2^64: every value is met, the cell has hits
    and misses, and the invariants hold"""
    positions = X.base_arrays(pkg, name).positions.reshape(-1)
    pts = PC.special_points(pkg, name)
    p = pts["p"]
    for vname, value in PC.SPECIAL_VALUES:
        if value == 0:
            met = ((p == 0) & (np.signbit(p) == np.signbit(value))).any(1)
        else:
            met = (np.abs(p).view(np.uint32) == value.view(np.uint32)).any(1)
        assert met.sum() >= 100, (name, vname, int(met.sum()))
    rec = R.closest(positions, pts)
    hits = (rec["triangle"] >= 0).mean()
    assert 0.05 <= hits <= 0.95, (name, hits)
    closest_invariants(positions, pts, rec, (name, "special"))
    lowest_index_wins(positions, pts, rec, (name, "special"))
    npts = PC.special_points(pkg, name, "near")
    nrec, n = NR.near(positions, npts, K)
    assert (n > 0).mean() >= 0.05 and (n == 0).mean() >= 0.05
    closest_invariants(positions, npts, nrec, (name, "special, near"))
    sd = derived_at(pkg, name, 0)["sign_data"]
    s = SD.signed(pts, rec, sd)
    assert np.array_equal(np.isnan(s), rec["triangle"] < 0)
    w = winding_at(pkg, name, 0).w(pts, math.inf)
    finite = np.isfinite(p).all(1)
    # a coordinate of 2^63 or 2^64 puts det at degree 3 of it: NaN is the definition's answer there, and only there
    huge = (np.abs(p) >= F(2.0 ** 63)).any(1)
    assert np.isnan(w[~finite]).all() and not np.isnan(w[finite & ~huge]).any()
