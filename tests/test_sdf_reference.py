"""The signed-distance restatement (tests/sdf_ref.py) pinned to analytic cases: its atan_yx against the oracle's bit for bit;
the unit cube's welded topology and pseudonormal directions; the boundary, non-manifold and misoriented counts of small open
or broken meshes; the sign against the float64 winding number on closed meshes; and a fan of thin triangles at a spike's
apex, where the angle weighting is what makes the sign right."""
import os

import numpy as np
import pytest

import point_query_ref as P
import sdf_ref as S

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def points_of(p, max_dist2=np.inf):
    out = np.zeros(len(p), P.POINT_DTYPE)
    out["p"] = np.asarray(p, F).reshape(-1, 3)
    out["max_dist2"] = max_dist2
    return out


def signed_of(positions, p, sign_data=None):
    pts = points_of(p)
    rec = P.closest(positions, pts)
    sd = S.derive(positions)["sign_data"] if sign_data is None else sign_data
    return S.signed(pts, rec, sd), rec


def test_atan_yx_matches_the_oracle_bit_for_bit(oracle_mod):
    rng = np.random.default_rng(3)
    y = np.concatenate([rng.normal(size=1500) * 10.0 ** rng.integers(-6, 6, 1500), [0, -0.0, 1, -1, 0, 1e-30, 3e38, -2]])
    x = np.concatenate([rng.normal(size=1500) * 10.0 ** rng.integers(-6, 6, 1500), [0, 1, 0, 0, -1, -1e-30, 1, 2]])
    y, x = y.astype(F), x.astype(F)
    got = S.atan_yx(y, x)
    want = np.array([oracle_mod.atan2(float(a), float(b)) for a, b in zip(y, x)], F)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def test_unit_cube_topology_and_pseudonormals():
    pos, tri = S.cube()
    d = S.derive(S.corners_of(pos, tri))
    assert d["info"] == {"vertices": 8, "edges": 18, "boundary_edges": 0, "nonmanifold_edges": 0, "misoriented_edges": 0,
                         "degenerate_triangles": 0, "closed": 1}
    sd = d["sign_data"]
    centre = np.full(3, 0.5)
    corners = pos[tri]                                                       # [T, 3, 3]
    # a corner's pseudonormal points along (corner - centre): three faces, each with a right angle there
    assert np.allclose(unit(sd[:, 1:4]), unit(corners - centre), atol=1e-6)
    # an edge of the cube: the two face normals; a face diagonal: twice the face's normal
    for t in range(len(tri)):
        for e, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
            mid = (corners[t, i].astype(np.float64) + corners[t, j]) / 2
            want = np.where(np.isin(mid, (0.0, 1.0)), mid - centre, 0.0)
            assert np.allclose(unit(sd[t, 4 + e]), unit(want), atol=1e-6), (t, e)
    assert np.allclose(np.linalg.norm(sd[:, 0], axis=1), 1, atol=1e-6)


@pytest.mark.parametrize("positions, info", [
    ([0, 0, 0, 1, 0, 0, 0, 1, 0], dict(vertices=3, edges=3, boundary_edges=3, nonmanifold_edges=0, misoriented_edges=0, closed=0)),
    ([0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0],
     dict(vertices=4, edges=5, boundary_edges=4, nonmanifold_edges=0, misoriented_edges=0, closed=0)),
    ([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1],
     dict(vertices=5, edges=7, boundary_edges=6, nonmanifold_edges=1, misoriented_edges=0, closed=0)),
])
def test_open_and_non_manifold_counts(positions, info):
    got = S.derive(np.asarray(positions, F))["info"]
    assert {k: got[k] for k in info} == info and got["degenerate_triangles"] == 0


def test_a_flipped_face_is_misoriented():
    pos, tri = S.tetrahedron()
    tri = tri.copy()
    tri[3] = tri[3][::-1]
    got = S.derive(S.corners_of(pos, tri))["info"]
    assert got["misoriented_edges"] == 3 and got["boundary_edges"] == 0 and got["closed"] == 0


def test_welding_ignores_the_sign_of_zero_and_keeps_non_finite_corners_apart():
    p = np.array([[0, 0, 0], [-0.0, 0, -0.0], [1, 2, 3], [np.nan, 0, 0], [np.nan, 0, 0], [np.inf, 1, 1]], F)
    v = S.weld(p.reshape(-1))
    assert v[0] == v[1] and len({v[0], v[2], v[3], v[4], v[5]}) == 5
    assert S.derive(np.array([0, 0, 0, 1, 0, 0, 2, 0, 0], F))["info"]["degenerate_triangles"] == 1


def sample_beyond_margin(positions, n, seed, margin=1e-3):
    tris = np.asarray(positions, F).reshape(-1, 3)
    lo, hi = tris.min(0), tris.max(0)
    extent = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(seed)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    p = (c + (rng.random((n, 3)) * 2 - 1) * 1.3 * h).astype(F)
    s, rec = signed_of(positions, p)
    keep = np.abs(s) > margin * extent
    return p[keep], s[keep]


@pytest.mark.parametrize("mesh", ["cube", "tetrahedron", "fan_spike", "lobed_528"])
def test_sign_agrees_with_the_winding_number(pkg, mesh):
    if mesh == "lobed_528":
        world = pkg.World(os.path.join(GOLDEN, "lobed_528.trisrc"))
        positions = np.asarray(world.arrays()["vertex_positions"], F)
        world.close()
    else:
        positions = S.corners_of(*getattr(S, mesh)())
    assert S.derive(positions)["info"]["closed"] == 1
    p, s = sample_beyond_margin(positions, 3000 if mesh == "lobed_528" else 4000, seed=len(mesh))
    inside = S.winding_number(positions, p) > 0.5
    assert 0.02 < inside.mean() < 0.98
    assert np.array_equal(s < 0, inside)


def test_fan_at_a_spike_needs_the_angle_weights():
    """Points above the apex of a steep pyramid whose +x side is a fan of thin triangles: their nearest point is the apex.
    The angle-weighted pseudonormal signs every one right; the plain sum of the incident normals, dominated by the fan,
    calls some of them inside."""
    pos, tri = S.fan_spike()
    positions = S.corners_of(pos, tri)
    apex = pos[4].astype(np.float64)
    rng = np.random.default_rng(5)
    dirs = np.stack([-rng.uniform(0.3, 1.5, 400), (rng.random(400) * 2 - 1) * 0.05, np.ones(400)], axis=1)
    p = (apex + dirs * rng.uniform(0.05, 0.5, (400, 1))).astype(F)
    s, rec = signed_of(positions, p)
    assert (rec["region"] <= 2).all() and np.array_equal(np.unique(S.weld(positions)[3 * rec["triangle"] + rec["region"]]).size, 1)
    inside = S.winding_number(positions, p) > 0.5
    assert not inside.any() and (s > 0).all()
    wrong, _ = signed_of(positions, p, S.unweighted_sign_data(positions))
    assert (wrong < 0).any()
