"""The cases of tests/ray_scale_cases.py pinned on the CPU, so that tests/test_gpu_ray_scale.py cannot be vacuous: the scaled
scenes' flags against the table, every cell's share of hits and misses (or none at all, with a walk), the restatement's hits
against a float64 Moller-Trumbore test over all triangles, and the numpy restatement of exact_div.h's three range predicates:
where each edge value lands, and that every cell puts rays through the class it can ("fast": div_by_constant4 may be taken,
"divide": it may not)."""
import numpy as np
import pytest

import ray_query_ref as R
import ray_scale_cases as X

F = np.float32
CASES = [(name, s) for name in X.SCENES for s in X.S_EXPONENTS]


def test_edge_values_land_on_the_documented_side():
    for name, value, inside in X.EDGES:
        for v in (value, -value):
            assert bool(R.divisor_in_range(np.array([v], F))[0]) == inside, name
    for name, value, inside in X.ORIGIN_VALUES:
        for v in (value, -value):
            assert bool(R.coordinate_in_range(np.array([v], F))[0]) == inside, name
    down, up = X._down, X._up
    assert R.divisor_in_range(np.array([2.0 ** -40, up(2.0 ** -40), down(2.0 ** 20)], F)).all()
    assert not R.divisor_in_range(np.array([down(2.0 ** -40), 2.0 ** 20, 0.0, -0.0, np.inf, np.nan, 1e-45], F)).any()
    assert R.coordinate_in_range(np.array([0.0, -0.0, 2.0 ** -70, -down(2.0 ** 60)], F)).all()
    assert not R.coordinate_in_range(np.array([down(2.0 ** -70), 2.0 ** 60, -2.0 ** 60, 1e-45, np.inf, np.nan], F)).any()
    assert R.scene_exact_div_ok(np.array([[0, -1e-20, 1]], F), np.array([[down(2.0 ** 60), 3, 4]], F)) == 1
    assert R.scene_exact_div_ok(np.array([[0, 0, 0]], F), np.array([[2.0 ** 60, 1, 1]], F)) == 0
    assert R.scene_exact_div_ok(np.array([[1e-30, 0, 0]], F), np.array([[1, 1, 1]], F)) == 0
    # one term alone decides: the flag, one direction component, one origin component
    o, d = np.ones((1, 3), F), np.ones((1, 3), F)
    assert R.fast_division(1, o, d)[0] and not R.fast_division(0, o, d)[0]
    for a in range(3):
        bad = d.copy()
        bad[0, a] = F(2.0 ** 20)
        assert not R.fast_division(1, o, bad)[0]
        bad[0, a] = 0
        assert not R.fast_division(1, o, bad)[0]
        far = o.copy()
        far[0, a] = F(2.0 ** 60)
        assert not R.fast_division(1, far, d)[0]
        far[0, a] = 0
        assert R.fast_division(1, far, d)[0]


@pytest.mark.parametrize("name, s_exp", CASES)
def test_scaled_scene_and_its_flag(pkg, name, s_exp):
    """the positions are the unscaled ones times S bit for bit (asserted where the scene is loaded), and the table's flag is
    the header's rule over the boxes of the scaled positions (and over the boxes the loader made)"""
    arrays = X.scaled_arrays(pkg, name, s_exp)
    lo, hi = X.leaf_boxes(arrays)
    assert R.scene_exact_div_ok(lo, hi) == X.expected_flag(name, s_exp)
    assert R.scene_exact_div_ok(arrays.boxmin, arrays.boxmax) == X.expected_flag(name, s_exp)
    m = np.abs(np.concatenate([lo, hi]))
    assert (X.expected_flag(name, s_exp) == 0) == bool(((m != 0) & ((m < F(2.0 ** -70)) | (m >= F(2.0 ** 60)))).any())


@pytest.mark.parametrize("name, s_exp", CASES)
def test_every_cell_is_meaningful(pkg, name, s_exp):
    c = X.case(pkg, name, s_exp)
    hits, counters = X.closest(pkg, name, s_exp)
    assert counters["node_visits"] > 0
    for cell in c.cells:
        r = cell.rays
        traced = r[c.tmax[r] > 0]
        share = (hits["triangle"][traced] >= 0).mean()
        _, own = R.trace(c.arrays, c.o[r], c.d[r], c.tmax[r])
        assert own["node_visits"] > 0 and len(traced) > len(r) * 0.8, cell
        if cell.hits_possible:
            assert 0.05 <= share <= 0.95, (name, s_exp, cell, share)
        else:
            assert share == 0, (name, s_exp, cell, share)


@pytest.mark.parametrize("name, s_exp", CASES)
def test_both_classes_are_populated_where_both_can_be(pkg, name, s_exp):
    """"divide" is populated in every cell (a tenth of random_rays' directions lie on an axis: zero divisors).  "fast" needs the
    scene's flag, every direction component in [2^-40, 2^20) -- kind "uniform": |unit component| < 1, so 2^-30 <= m <= 2^20 here;
    kind "component": the edge value itself in range -- and every origin component 0 or in [2^-70, 2^60): at S = 2^-71 that asks
    all three unscaled components for a magnitude of 2 or more, which next to no origin has, so nothing is asked there."""
    c = X.case(pkg, name, s_exp)
    fast = X.fast_class(c)
    for cell in c.cells:
        f, n = int(fast[cell.rays].sum()), len(cell.rays)
        assert n - f >= 5, (name, s_exp, cell, f, n)
        if cell.kind == "origin":
            assert f >= 50, (cell, f)
            continue
        value = cell.value
        can = bool(R.divisor_in_range(np.array([value], F))[0]) if cell.kind == "component" else F(2.0 ** -30) <= value <= F(2.0 ** 20)
        if not X.expected_flag(name, s_exp) or not can:
            assert f == 0, (name, s_exp, cell, f)
        elif s_exp > -71:
            assert f >= 5, (name, s_exp, cell, f)
    if s_exp == 0:
        # the origin class: every special value is met alone on a ray, and lands where exact_div.h says
        k = c.cells[-1].rays
        for vname, value, inside in X.ORIGIN_VALUES:
            bits = np.abs(c.o[k]).view(np.uint32) == np.abs(value).view(np.uint32)
            if value == 0:
                bits = np.signbit(c.o[k]) == np.signbit(value)
                bits &= c.o[k] == 0
            assert bits.any(1).sum() >= 20, vname
            if not inside:
                assert not fast[k][bits.any(1)].any(), vname
        assert (fast[k] & (c.o[k] == 0).any(1)).sum() >= 5 and (fast[k] & (np.abs(c.o[k]) == F(2.0 ** -70)).any(1)).sum() >= 5


def float64_closest(arrays, o, d, tmax):
    """Moller-Trumbore in float64 over all triangles, vectorised: per ray the closest clearly-inside triangle (-1: none) and
    its t, and `clear`: every triangle is inside or outside by a margin and every decision of the contract has one.

    The margins.  fs:311 rejects |det| < 1e-7 and the walk keeps t in [0, min(tmax, 1e8)): a determinant within a factor 2 of
    the epsilon, a t within 1e-4 (relative) of an end or of the next crossing, leave the ray out.  u, v, u + v: 1e-4 -- a hundred
    times float32's error in them (a dozen roundings of 6e-8 each); tests/test_multi_hit_reference.py's 1e-3 leaves out more
    than a cell of a hundred rays can spare --, widened for a triangle seen edge-on (|cos| < 1e-3 between its normal and the
    ray) by 1e-3 / |cos|: the error grows with 1 / |cos|, and such a triangle's u, v are far outside anyway.
    t is measured in units of S / |direction| (a length of the unscaled scene), so one margin serves every cell."""
    v = arrays.positions.astype(np.float64)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    normal = np.cross(e1, e2)
    area2 = np.linalg.norm(normal, axis=1)
    O, D = o.astype(np.float64), d.astype(np.float64)
    n = len(O)
    best = np.full(n, -1)
    best_t = np.full(n, np.inf)
    clear = np.ones(n, bool)
    margin = 1e-4
    with np.errstate(all="ignore"):
        norm = np.linalg.norm(D, axis=1)
        limit = np.minimum(np.where(np.isnan(tmax), 0.0, tmax.astype(np.float64)), 1e8)
        for first in range(0, n, 512):
            s = slice(first, min(first + 512, n))
            p = np.cross(D[s, None, :], e2[None])
            det = (e1[None] * p).sum(2)
            cos = np.abs(det) / (area2[None] * norm[s, None])
            sv = O[s, None, :] - v[None, :, 0]
            u = (sv * p).sum(2) / det
            q = np.cross(sv, e1[None])
            w = (q * D[s, None, :]).sum(2) / det
            t = (q * e2[None]).sum(2) / det
            unit = (np.abs(O[s]).max(1) + np.abs(v).max()) / norm[s]          # the scaled scene's size, in t
            mg = margin * np.maximum(1.0, 1e-3 / cos)
            mt = margin * unit[:, None]
            lim = limit[s, None]
            counted = np.abs(det) > 2e-7
            rejected = np.abs(det) < 0.5e-7
            inside = counted & (u > mg) & (w > mg) & (u + w < 1 - mg) & (t > mt) & (t < lim * (1 - margin))
            outside = rejected | (u < -mg) | (w < -mg) | (u + w > 1 + mg) | (t < -mt) | (t > lim * (1 + margin))
            ok = (inside | outside).all(1) & np.isfinite(D[s]).all(1)
            tt = np.where(inside, t, np.inf)
            order = np.sort(tt, axis=1)[:, :2]
            ok &= ~(np.isfinite(order[:, 1]) & (order[:, 1] - order[:, 0] < margin * order[:, 1] + mt[:, 0]))
            clear[s] = ok
            idx = tt.argmin(1)
            has = np.isfinite(tt.min(1))
            best[s] = np.where(has, idx, -1)
            best_t[s] = tt.min(1)
    return best, best_t, clear


@pytest.mark.parametrize("name, s_exp", CASES)
def test_the_restatement_against_float64_over_all_triangles(pkg, name, s_exp):
    """The restatement divides in numpy and has no fast path: its closest hits equal a float64 test of all triangles wherever
    that is decided by a margin (float64_closest), in every cell.  At most 1 % of a cell's rays may be left out -- of the rays
    that do not start ON the mesh: one that does has its own triangle at t = 0 give or take rounding, inside every margin by
    construction (tests/test_multi_hit_reference.py leaves those out too); they are checked where the float64 test is clear.
    Nor of the rays with a zero direction component (random_rays' tenth on an axis): the shader's slab test divides by it, and a
    -0 sends the entry distance to +inf -- the contract (fs:204-213), not geometry.  At S >= 2^59 the float32 products of the
    triangle test overflow (S^3 > 2^128), which float64 does not restate: those scenes are miss-only in every cell
    (test_every_cell_is_meaningful) and are not compared here.
    Nor of the origin class' rays from 2^60 - 1ulp and beyond: one ulp of such an origin is 2^36 sizes of the mesh, so float32
    cannot aim at it and float64 has nothing to confirm; the restatement and the GPU still have to agree on them."""
    if s_exp >= 59:
        assert not any(cell.hits_possible for cell in X.case(pkg, name, s_exp).cells)
        return
    c = X.case(pkg, name, s_exp)
    hits, _ = X.closest(pkg, name, s_exp)
    traced = c.tmax > 0
    best, best_t, clear = float64_closest(c.arrays, c.o, c.d, c.tmax)
    if any(cell.hits_possible for cell in c.cells):
        assert c.arrays.objects[:, 1].max() <= 10             # no leaf is cut short by max_leaf_tests
    capped = hits["triangle"] == R.HIT_CAP                   # (the 400-visit cap, met in the tiny scenes: never a hit)
    got = np.where(hits["triangle"] >= 0, hits["triangle"], -1)
    far = np.abs(c.o).max(1) >= c.S * F(2.0 ** 30)            # the origin class' 2^60 and 2^61: see the docstring
    for cell in c.cells:
        r = cell.rays[traced[cell.rays] & ~c.on_surface[cell.rays] & ~(c.d[cell.rays] == 0).any(1) & ~far[cell.rays]]
        left_out = ~clear[r]
        # what the cap is taken over: at least half of the cell's traced rays (a third start on the mesh or lie on an axis), a third
        # in the origin class (a ray there has one to three special components, three of the eight values far: (5/8 + 25/64 +
        # 125/512) / 3 = 42 % have none)
        assert len(r) >= traced[cell.rays].sum() // (3 if cell.kind == "origin" else 2), (name, s_exp, cell, len(r))
        assert left_out.sum() <= max(1, len(r) // 100), (name, s_exp, cell, int(left_out.sum()), len(r))   # (1 %, or one ray of fewer than 100)
        k = r[clear[r]]
        bad = k[got[k] != best[k]]
        assert not len(bad), (name, s_exp, cell, bad[:5], got[bad[:5]], best[bad[:5]], best_t[bad[:5]], capped[bad[:5]])
        h = k[best[k] >= 0]
        assert np.allclose(hits["t"][h], best_t[h], rtol=1e-4, atol=0), (name, s_exp, cell)
        if cell.hits_possible and s_exp == 0:
            assert len(h) >= len(r) // 20, (name, s_exp, cell, len(h), len(r))
    # the rays that start on the mesh: their own triangle aside
    r = np.nonzero(traced & c.on_surface & clear & ~(c.d == 0).any(1))[0]
    assert np.array_equal(got[r], best[r])
