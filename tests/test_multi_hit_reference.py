"""The CPU restatement of the all-hits ray query (tests/multi_hit_ref.py) pinned to analytic answers, to a float64
Moller-Trumbore test over all triangles, and to the closest-hit restatement (tests/ray_query_ref.py): record 0 is the closest
hit.  Also the monotonicity of the slab entry distance over nested boxes, which the pruned walk of the GPU kernel relies on
(DESIGN section 14)."""
import os

import numpy as np
import pytest

import helpers
import multi_hit_ref as M
import ray_query_ref as R
from test_gpu_ray_query import random_rays, scene_path
from test_ray_query_reference import hand_arrays

F = np.float32
MISS = R.HIT_MISS


@pytest.fixture(scope="module")
def meshes(pkg, tmp_path_factory):
    """the small meshes as flattened arrays (the package's own BVH build)"""
    out = {}
    for name in M.MESHES:
        world = pkg.World(M.write_mesh(pkg, str(tmp_path_factory.mktemp("multihit") / f"{name}.trisrc"), name))
        out[name] = R.SceneArrays(world.arrays())
        world.close()
    return out


def one_ray(arrays, origin, direction, tmax=1e7, **kw):
    hits, counts, _ = M.all_hits(arrays, [origin], [direction], [tmax], **kw)
    return hits[0], int(counts[0])


def test_five_squares_in_order_with_analytic_t(meshes):
    # off the diagonal x = y: exactly one triangle per square
    h, n = one_ray(meshes["stack_of_squares"], (0.25, -0.5, -2.0), (0.0, 0.0, 1.0))
    assert n == 5
    assert h["t"][:5].tolist() == [2.0, 3.0, 4.0, 5.0, 6.0]
    assert h["triangle"][:5].tolist() == [0, 2, 4, 6, 8]       # the triangle (0, 1, 2) of each square: y < x
    assert (h["triangle"][5:] == MISS).all() and (h["t"][5:] == F(1e7)).all() and (h["u"][5:] == 0).all() and (h["v"][5:] == 0).all()
    # the other side of the diagonal, from above: the squares in the opposite order
    h, n = one_ray(meshes["stack_of_squares"], (-0.5, 0.25, 5.5), (0.0, 0.0, -1.0), max_hits=3)
    assert n == 5 and h["t"].tolist() == [1.5, 2.5, 3.5] and h["triangle"].tolist() == [9, 7, 5]
    # a direction that is not normalised scales t
    h, n = one_ray(meshes["stack_of_squares"], (0.25, -0.5, -2.0), (0.0, 0.0, 4.0), max_hits=2)
    assert n == 5 and h["t"].tolist() == [0.5, 0.75]


def test_cube_from_outside_and_inside(meshes):
    cube = meshes["closed_cube"]
    h, n = one_ray(cube, (0.3, 0.4, -1.0), (0.0, 0.0, 1.0))
    assert n == 2 and h["t"][:2].tolist() == [1.0, 2.0] and (h["triangle"][:2] >= 0).all() and h["triangle"][2] == MISS
    h, n = one_ray(cube, (0.3, 0.4, 0.5), (0.0, 0.0, 1.0))
    assert n == 1 and h["t"][0] == F(0.5)
    _, n = one_ray(cube, (0.3, 0.4, 0.5), (0.0, 0.0, 1.0), max_hits=0)   # counts only
    assert n == 1


def test_coincident_triangles_are_both_reported_ordered_by_index(meshes):
    h, n = one_ray(meshes["coincident"], (0.5, 0.25, -1.0), (0.0, 0.0, 1.0), max_hits=4)
    assert n == 3
    assert h["t"].tolist()[:3] == [1.0, 1.0, 2.0] and h["triangle"].tolist() == [0, 1, 2, MISS]
    assert h["u"][0] == h["u"][1] and h["v"][0] == h["v"][1]
    h, n = one_ray(meshes["coincident"], (0.5, 0.25, -1.0), (0.0, 0.0, 1.0), max_hits=1)
    assert n == 3 and h["triangle"].tolist() == [0]


def test_tmax_cuts_the_list_and_excludes_a_hit_at_tmax(meshes):
    stack = meshes["stack_of_squares"]
    h, n = one_ray(stack, (0.25, -0.5, -2.0), (0.0, 0.0, 1.0), tmax=4.5)
    assert n == 3 and h["t"][:3].tolist() == [2.0, 3.0, 4.0] and (h["t"][3:] == F(4.5)).all() and (h["triangle"][3:] == MISS).all()
    h, n = one_ray(stack, (0.25, -0.5, -2.0), (0.0, 0.0, 1.0), tmax=4.0)
    assert n == 2 and h["t"][:2].tolist() == [2.0, 3.0] and h["triangle"][2] == MISS and h["t"][2] == F(4.0)
    h, n = one_ray(stack, (0.25, -0.5, -2.0), (0.0, 0.0, 1.0), tmax=np.inf)
    assert n == 5 and (h["t"][5:] == F(np.inf)).all()


@pytest.mark.parametrize("tmax", [0.0, -0.0, -1.5, np.nan, -np.inf])
def test_tmax_not_positive_is_no_walk(meshes, tmax):
    hits, counts, counters = M.all_hits(meshes["closed_cube"], [(0.3, 0.4, -1.0)], [(0.0, 0.0, 1.0)], [tmax], max_hits=3)
    assert counts[0] == 0 and (hits["triangle"] == MISS).all() and (hits["u"] == 0).all() and (hits["v"] == 0).all()
    assert np.array_equal(hits["t"][0].view(np.uint32), np.full(3, F(tmax)).view(np.uint32))
    assert counters == {"node_visits": 0, "leaf_visits": 0, "triangle_tests": 0, "traversals": 0, "bad_hits": 0}


def test_leaf_cap_limits_the_triangles_tested():
    # one leaf of 14 parallel triangles: only the first ten are tested, whatever K
    tris = [[[0, 0, z], [1, 0, z], [0, 1, z]] for z in range(14)]
    arrays = hand_arrays(helpers.single_leaf_scene(tris))
    hits, counts, counters = M.all_hits(arrays, [(0.25, 0.25, -1.0)], [(0.0, 0.0, 1.0)], [1e7], max_hits=16)
    assert counts[0] == 10 and hits["triangle"][0].tolist() == list(range(10)) + [MISS] * 6
    assert hits["t"][0][:10].tolist() == [float(z + 1) for z in range(10)]
    assert counters == {"node_visits": 1, "leaf_visits": 1, "triangle_tests": 10, "traversals": 1, "bad_hits": 0}
    hits, counts, _ = M.all_hits(arrays, [(0.25, 0.25, -1.0)], [(0.0, 0.0, 1.0)], [1e7], max_hits=16, max_leaf_tests=3)
    assert counts[0] == 3 and hits["triangle"][0][:4].tolist() == [0, 1, 2, MISS]


def test_more_crossings_than_k_keeps_the_first_k(pkg, tmp_path):
    """tall_stack: an axial ray off the diagonal crosses 104 triangles, three at equal t on every seventh level; every K keeps
    the first K of the one sorted list, and the count does not depend on K.  (The builder leaves up to 16 of these triangles in
    a leaf, so the analytic counts need max_leaf_tests = 16; with the default 10 some are not tested, by contract.)"""
    world = pkg.World(M.write_mesh(pkg, str(tmp_path / "tall_stack.trisrc"), "tall_stack"))
    arrays = R.SceneArrays(world.arrays())
    world.close()
    levels = [lv for lv in range(80) for _ in range(3 if lv % 7 == 0 else 1)]
    want_t = [F(1.0) + F(lv) * F(0.1) for lv in levels]
    full, n = one_ray(arrays, (0.25, -0.5, -1.0), (0.0, 0.0, 1.0), max_hits=128, max_leaf_tests=16)
    assert n == 104 and len(levels) == 104
    assert np.allclose(full["t"][:104], want_t, rtol=1e-6) and (np.diff(full["t"][:104]) >= 0).all()
    assert full["triangle"][:104].tolist() == [2 * i for i in range(104)]          # triangle (0, 1, 2) of each square, in file order
    assert (full["triangle"][104:] == MISS).all()
    for k in (1, 3, 8, 9, 16, 64):
        h, n = one_ray(arrays, (0.25, -0.5, -1.0), (0.0, 0.0, 1.0), max_hits=k, max_leaf_tests=16)
        assert n == 104 and np.array_equal(h.view(np.uint32), np.ascontiguousarray(full[:k]).view(np.uint32))
    # from above the list is reversed in t, but equal t (level 77, triangles 198, 200, 202) still sort by ascending triangle index
    down, n = one_ray(arrays, (0.25, -0.5, 9.0), (0.0, 0.0, -1.0), max_hits=128, max_leaf_tests=16)
    assert n == 104 and down["triangle"][:4].tolist() == [206, 204, 198, 200] and down["triangle"][101:104].tolist() == [0, 2, 4]
    o, d, tmax = M.axial_rays(4000, seed=1)
    _, capped, _ = M.all_hits(arrays, o, d, tmax, max_hits=0)
    _, counts, _ = M.all_hits(arrays, o, d, tmax, max_hits=0, max_leaf_tests=16)
    assert (capped > 64).sum() > 400 and (counts > 64).sum() > 400 and (counts == 0).sum() > 0 and (capped < counts).sum() > 400


def loaded(pkg, name):
    world = pkg.World(scene_path(name))
    try:
        return R.SceneArrays(world.arrays())
    finally:
        world.close()


def test_against_float64_over_all_triangles(pkg):
    """lobed_528: for rays that miss every edge, every plane-parallel case and every range end by a clear margin, the same
    triangles in the same order as a float64 Moller-Trumbore test of all 528 triangles."""
    arrays = loaded(pkg, "lobed_528")
    n = 6000
    o, d, _ = random_rays(arrays, n, seed=3)
    tmax = np.full(n, F(1e7))
    v = arrays.positions.astype(np.float64)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    O, D = o.astype(np.float64), d.astype(np.float64)
    K = 16
    hits, counts, _ = M.all_hits(arrays, o, d, tmax, max_hits=K)
    margin = 1e-3
    checked = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            p = np.cross(D[i], e2)
            det = (e1 * p).sum(1)
            s = O[i] - v[:, 0]
            u = (s * p).sum(1) / det
            q = np.cross(s, e1)
            w = (q * D[i]).sum(1) / det
            t = (q * e2).sum(1) / det
            inside = (u > margin) & (w > margin) & (u + w < 1 - margin) & (t > margin)
            outside = (u < -margin) | (w < -margin) | (u + w > 1 + margin) | (t < -margin)
            clear = (np.abs(det) > 1e-4).all() and (inside | outside).all() and np.isfinite(D[i]).all() and (np.abs(D[i]) > 1e-3).all()
            ts = np.sort(t[inside])
            if not clear or (len(ts) > 1 and np.diff(ts).min() < margin) or len(ts) > K:
                continue
            checked += 1
            want = np.nonzero(inside)[0][np.argsort(t[inside])]
            assert counts[i] == len(want), (i, counts[i], want)
            assert hits["triangle"][i][:len(want)].tolist() == want.tolist(), i
            assert np.allclose(hits["t"][i][:len(want)], np.sort(t[inside]), rtol=1e-4, atol=1e-5)
    assert checked > n // 6, checked   # (a third of the rays start on the surface and are never clear)


@pytest.mark.parametrize("name", ["small_trisrc", "lobed_528", "bunny"])
def test_record_0_is_the_closest_hit(pkg, name):
    """Agreement with the closest-hit restatement (no iteration cap): count == 0 iff the closest hit is a miss, else record
    0 equals it in t, u, v bits and in the triangle.  Left out: rays whose first two records have equal t (the closest-hit
    walk keeps the first in ITS visit order) and rays that met a NaN candidate (the closest-hit walk may have accepted it).
    At most 1 % of a scene's rays may be left out."""
    arrays = loaded(pkg, name)
    n = 20000
    o, d, tmax = random_rays(arrays, n, seed=29 + len(name))
    closest, _ = R.trace(arrays, o, d, tmax, max_bvh_iterations=0)
    hits, counts, _, nan_candidate = M.all_hits(arrays, o, d, tmax, max_hits=2, details=True)
    tie = (counts >= 2) & (hits["t"][:, 0] == hits["t"][:, 1])
    left_out = tie | nan_candidate
    assert left_out.mean() <= 0.01, (name, int(tie.sum()), int(nan_candidate.sum()), n)
    keep = ~left_out
    assert np.array_equal((counts == 0)[keep], (closest["triangle"] == MISS)[keep])
    k = keep & (counts > 0)
    assert k.sum() > n // 20 and (keep & (counts == 0)).sum() > n // 20 and (counts > 2).sum() > 50
    first = hits[:, 0]
    assert np.array_equal(first["triangle"][k], closest["triangle"][k])
    for f in ("t", "u", "v"):
        assert np.array_equal(np.ascontiguousarray(first[f][k]).view(np.uint32), np.ascontiguousarray(closest[f][k]).view(np.uint32)), f
    # and K = 1 is the first record of any larger K
    h1, _, _ = M.all_hits(arrays, o[:2000], d[:2000], tmax[:2000], max_hits=1)
    assert np.array_equal(h1[:, 0].view(np.uint32), np.ascontiguousarray(hits[:2000, 0]).view(np.uint32))


def test_an_accepted_t_is_never_below_its_leafs_r0_and_counts_match_records(pkg):
    arrays = loaded(pkg, "lobed_528")
    o, d, tmax = random_rays(arrays, 8000, seed=5)
    hits, counts, _ = M.all_hits(arrays, o, d, tmax, max_hits=M.MULTIHIT_MAX)
    real = hits["triangle"] >= 0
    assert np.array_equal(real.sum(1), np.minimum(counts, M.MULTIHIT_MAX))
    t = np.where(real, hits["t"], np.inf)
    assert (t[:, 1:] >= t[:, :-1]).all()                       # sorted, the misses last
    assert (hits["t"][real] >= 0).all() and (hits["t"] < tmax[:, None])[real].all()


def test_entry_distance_is_monotone_over_nested_boxes():
    """The pruning argument: for a box inside another, the inner r0 is never below the outer r0
    whenever the outer box can be entered at all (its r0 is finite), for random rays, axis-aligned rays with +-0 components
    and rays grazing a face or starting on a plane -- in float32, as the kernel computes it.  r0 itself is never NaN."""
    rng = np.random.default_rng(12)
    n = 400000
    centre = rng.normal(size=(n, 3)) * 3
    half = rng.random((n, 3)) * 2 + 1e-3
    olo, ohi = (centre - half).astype(F), (centre + half).astype(F)
    a, b = np.sort(rng.random((2, n, 3)), axis=0)
    snap = rng.random((n, 3)) < 0.2                                  # an inner plane on the outer one
    ilo = np.where(snap, olo, olo + (ohi - olo) * a.astype(F)).astype(F)
    ihi = np.where(rng.random((n, 3)) < 0.2, ohi, olo + (ohi - olo) * b.astype(F)).astype(F)
    ilo, ihi = np.clip(ilo, olo, ohi), np.clip(ihi, olo, ohi)
    ihi = np.maximum(ihi, ilo)
    o = (centre + rng.normal(size=(n, 3)) * 4).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    kind = rng.integers(0, 4, n)
    k = np.nonzero(kind == 1)[0]                                     # axis-aligned, +-0 elsewhere
    z = np.where(rng.random((len(k), 3)) < 0.5, F(0.0), F(-0.0)).astype(F)
    z[np.arange(len(k)), rng.integers(0, 3, len(k))] = np.where(rng.random(len(k)) < 0.5, F(1), F(-1))
    d[k] = z
    k = np.nonzero(kind >= 2)[0]                                     # the origin on a plane of the inner or outer box
    ax = rng.integers(0, 3, len(k))
    planes = np.stack([olo, ohi, ilo, ihi])[rng.integers(0, 4, len(k)), k, ax]
    o[k, ax] = planes
    g = k[: len(k) // 2]                                             # and grazing: no motion across that plane
    d[g, ax[: len(g)]] = np.where(rng.random(len(g)) < 0.5, F(0.0), F(-0.0))
    r0o, r1o = M.slab_range(olo, ohi, o, d)
    r0i, r1i = M.slab_range(ilo, ihi, o, d)
    assert not np.isnan(r0o).any() and not np.isnan(r0i).any()
    enterable = r0o < np.inf
    bad = enterable & ~(r0o <= r0i)
    assert not bad.any(), (int(bad.sum()), o[bad][:3], d[bad][:3])
    assert enterable.sum() > n // 2 and (r0o < r0i).sum() > n // 10 and ((r0o == r0i) & (r0o > 0)).sum() > 1000
    # and the exit distance is monotone the other way, so an inner box entered implies ... nothing the walk relies on;
    # the walk only needs: outer not entered => inner not visited (by construction), outer r0 <= inner r0 (above)
