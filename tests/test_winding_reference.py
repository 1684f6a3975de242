"""The winding-number restatement (tests/winding_ref.py) pinned to the float64 winding number (tests/sdf_ref.py) and to
analytic values: the exact mode and beta = 2 within bounds measured on these meshes, the inside test
w > 0.5 equal to float64's away from the surface, 1, 0, -1, 2 and 5/6 where the meshes put them, and one node's far field
converging to the exact value as the distance grows."""
import math
import os

import numpy as np
import pytest

import point_query_ref as P
import sdf_ref as S
import winding_ref as W

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the restatement against float64 at points at least 1e-3 x extent from the surface: measured maxima 2.3e-6 (exact) and
# 3.1e-3 (beta 2) over these meshes
EXACT_BOUND, BETA2_BOUND = 4e-6, 5e-3
_worlds = {}


def restated(pkg, tmp_path_factory, name):
    if name not in _worlds:
        if name == "quads_mixed":
            path = os.path.join(GOLDEN, "quads_mixed.obj")
        else:
            path = W.write_mesh(pkg, str(tmp_path_factory.mktemp("winding_ref") / f"{name}.trisrc"), name)
        world = pkg.World(path)
        _worlds[name] = W.Restated(world)
        world.close()
    return _worlds[name]


def away_from_surface(ref, n, seed, margin=1e-3):
    """points in the mesh's box grown by 30 %, at least margin x extent from the surface"""
    pos = ref.positions.reshape(-1, 3)
    lo, hi = pos.min(0), pos.max(0)
    extent = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(seed)
    p = ((lo + hi) / 2 + (rng.random((n, 3)) * 2 - 1) * 0.65 * (hi - lo)).astype(F)
    pts = np.zeros(n, P.POINT_DTYPE)
    pts["p"], pts["max_dist2"] = p, np.inf
    dist = np.sqrt(P.closest(ref.positions, pts)["dist2"].astype(np.float64))
    return p[dist >= margin * extent]


@pytest.mark.parametrize("name", W.MESHES + ("quads_mixed",))
def test_exact_and_beta_2_against_float64(pkg, tmp_path_factory, name):
    ref = restated(pkg, tmp_path_factory, name)
    p = away_from_surface(ref, 4000, seed=len(name))
    assert len(p) > 3500
    w64 = S.winding_number(ref.positions, p)
    exact, approx = ref.w(p, math.inf), ref.w(p, 2.0)
    assert np.abs(exact - w64).max() <= EXACT_BOUND
    assert np.abs(approx - w64).max() <= BETA2_BOUND
    assert np.array_equal(exact > 0.5, w64 > 0.5) and np.array_equal(approx > 0.5, w64 > 0.5)


def test_analytic_values(pkg, tmp_path_factory):
    g = np.linspace(0.1, 0.9, 5)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)
    outside = np.array([[-0.5, 0.5, 0.5], [0.5, 1.7, 0.5], [2, 2, 2], [0.5, 0.5, -3], [10, -4, 7]], F)

    def check(name, p, value, shift=0.0):
        ref = restated(pkg, tmp_path_factory, name)
        q = (p + F(shift)).astype(F)
        for beta, tol in ((math.inf, EXACT_BOUND), (2.0, BETA2_BOUND)):
            assert np.abs(ref.w(q, beta) - value).max() <= tol, (name, beta, value)

    for name in ("soup", "far_cube"):
        shift = 1e4 if name == "far_cube" else 0.0
        check(name, grid, 1.0, shift)
        check(name, outside, 0.0, shift)
    check("inward_cube", grid, -1.0)
    check("inward_cube", outside, 0.0)
    check("open_cube", np.array([[0.5, 0.5, 0.5]], F), 5.0 / 6.0)
    check("two_cubes", grid[(grid > 0.5).all(1)], 2.0)
    check("two_cubes", grid[(grid < 0.5).any(1)], 1.0)
    check("two_cubes", np.array([[1.25, 1.25, 1.25], [1.4, 0.7, 0.8]], F), 1.0)
    check("two_cubes", outside[:2], 0.0)


def test_non_finite_points_and_degenerate_terms():
    """NaN for a non-finite point; a point in a triangle's plane or at its corner adds 0, not +-1/2"""
    pos, tri = S.cube()
    tris = pos[tri].astype(F)
    q = np.array([[0.5, 0.5, 0.0], [0.0, 0.0, 0.0], [3.0, 0.5, 0.0]], F)
    for t in range(len(tris)):
        if (tris[t][:, 2] == 0).all():
            terms = W.triangle_terms_at(np.repeat(tris[t:t + 1], 3, 0), q)
            assert (terms == 0).all()
    tree = type("T", (), {})()
    tree.negative, tree.positive = np.array([-1]), np.array([-1])
    tree.start, tree.triangles, tree.node_count = np.array([0]), np.array([len(tris)]), 1
    rec = W.node_records(tree, tris.reshape(-1, 3).min(0)[None], tris.reshape(-1, 3).max(0)[None], tris.reshape(-1))
    w = W.winding(tree, rec, tris.reshape(-1), np.array([[np.nan, 0, 0], [0.5, np.inf, 0.5], [0.5, 0.5, 0.5]], F), math.inf)
    assert np.isnan(w[:2]).all() and abs(w[2] - 1) < EXACT_BOUND


def test_one_nodes_far_field_converges(pkg, tmp_path_factory):
    """The open cube is one leaf: with beta = 0 every point takes the root's far field.  Its error against float64 falls as
    the fourth power of the distance (the first term left out), 16x a doubling; the cube's opening keeps w itself at the
    second power."""
    ref = restated(pkg, tmp_path_factory, "open_cube")
    assert ref.tree.node_count == 1
    u = np.random.default_rng(2).normal(size=(200, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    errors = []
    for r in (2, 4, 8, 16):
        p = (0.5 + r * u).astype(F)
        errors.append(np.abs(ref.w(p, 0.0) - S.winding_number(ref.positions, p)).max())
    ratios = np.array(errors[:-1]) / np.array(errors[1:])
    assert (ratios > 12).all(), errors
    assert errors[-1] < 2e-6
