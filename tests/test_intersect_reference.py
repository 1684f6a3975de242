"""The triangle-intersection restatement (tests/intersect_ref.py) against a truth that shares nothing with it: on
integer-lattice inputs, where every fp32 operation of include/shader_ray_intersect.h is exact, a clip of the query by the scene
triangle's plane and in-plane edges in fractions.Fraction (intersect_cases.exact_intersects); then cases known by hand, the
prefix and count rules, the queries that are not walked, and the range of scales 2^k over which the set does not change."""
import numpy as np
import pytest

import intersect_cases as IC
import intersect_ref as IR

F = np.float32
SCALE_RANGE = (-33, 29)   # include/shader_ray_intersect.h, DESIGN section 19


def lattice_pairs(n, seed):
    """integer corners in [-6, 6]: a quarter each of random pairs, pairs coplanar in z = 0, T built from integer combinations of
    Q's edges and shifted by -1, 0 or +1 along x, and pairs that share a corner"""
    rng = np.random.default_rng(seed)

    def near(a, reach):
        return np.clip(a + rng.integers(-reach, reach + 1, a.shape), -6, 6)

    def triangles(m, reach=5):
        a = rng.integers(-6, 7, (m, 3))
        return np.stack([a, near(a, reach), near(a, reach)], 1)

    m = n // 4
    q, t = triangles(n), triangles(n)
    t[:m] = np.clip(q[:m] + rng.integers(-3, 4, (m, 1, 3)) + rng.integers(-3, 4, (m, 3, 3)), -6, 6)   # random, near each other
    q[m:2 * m, :, 2] = 0                                                                              # coplanar in z = 0
    t[m:2 * m] = np.clip(q[m:2 * m] + rng.integers(-4, 5, (m, 3, 3)), -6, 6)
    t[m:2 * m, :, 2] = 0
    s = slice(2 * m, 3 * m)                                                                           # combinations of Q's edges
    q[s] = triangles(m, 2)
    f0, f2 = q[s, 1] - q[s, 0], q[s, 0] - q[s, 2]
    coef = rng.integers(-1, 3, (m, 3, 2))
    t[s] = q[s, :1] + coef[:, :, :1] * f0[:, None, :] - coef[:, :, 1:] * f2[:, None, :]
    t[s, :, 0] += rng.integers(-1, 2, (m, 1))
    inside = (np.abs(t[s]) <= 6).all((1, 2))
    t[s] = np.where(inside[:, None, None], t[s], np.clip(t[s], -6, 6))
    s = slice(3 * m, n)                                                                               # a shared corner
    rows = np.arange(n - 3 * m)
    t[s][rows, rng.integers(0, 3, len(rows))] = q[s][rows, rng.integers(0, 3, len(rows))]
    return q, t


def test_lattice_pairs_equal_the_exact_clip():
    n = 40000
    q, t = lattice_pairs(n, seed=19)
    assert n >= 40000 and np.abs(q).max() <= 6 and np.abs(t).max() <= 6
    # every pair through first_axis itself, the function the GPU tests compare with: blocks of queries against the blocks' own
    # triangles, the pair being the diagonal
    q32, t32, block = q.astype(F), t.astype(F), 80
    code, shared = (np.concatenate([np.diagonal(IR.first_axis(q32[s:s + block], t32[s:s + block].reshape(-1), skip)) for s in range(0, n, block)])
                    for skip in (False, True))
    assert code.shape == (n,)
    bad_q = np.array([IC.exact_degenerate(x) for x in q])
    bad_t = np.array([IC.exact_degenerate(x) for x in t])
    # the degenerate rule: such a query is not walked, such a scene triangle is not a member
    assert np.array_equal(code == IR.UNWALKED, bad_q) and np.array_equal(IR.walked(q32), ~bad_q)
    assert not (code[bad_t] == IR.INTERSECT).any() and (code[bad_t & ~bad_q] <= IR.DEGENERATE).all()
    assert (code[~bad_t & ~bad_q] != IR.DEGENERATE).all()
    good = np.nonzero(~bad_q & ~bad_t)[0]
    truth = np.array([IC.exact_intersects(q[i], t[i]) for i in good])
    firsts = np.bincount(code[good][code[good] >= 0], minlength=IR.UNWALKED)
    print(f"lattice: {n} pairs, intersecting {truth.mean():.3f}, degenerate queries {bad_q.mean():.3f}, degenerate scene triangles "
          f"{bad_t.mean():.3f}, first rejecting stage {firsts.tolist()}")
    assert truth.mean() > 1 / 3
    assert all(firsts[k] >= 1 for k in IR.STAGES), firsts
    wrong = good[(code[good] == IR.INTERSECT) != truth]
    assert len(wrong) == 0, (len(wrong), q[wrong[:3]], t[wrong[:3]], code[wrong[:3]])
    # SKIP_SHARED takes out exactly the pairs with a common corner
    common = (q[:, :, None, :] == t[:, None, :, :]).all(3).any((1, 2))
    assert common[3 * (n // 4):].all() and common.mean() < 0.5
    assert np.array_equal(shared == IR.INTERSECT, (code == IR.INTERSECT) & ~common)
    assert ((shared == IR.SHARED) == (common & ~bad_q)).all()   # (a common corner passes stage 0)


def one(q, t, skip_shared=False):
    return int(IR.first_axis(np.asarray(q, F).reshape(1, 3, 3), np.asarray(t, F).reshape(-1), skip_shared)[0, 0])


def test_analytic_cases():
    A0 = IR.AXIS0
    floor = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
    # piercing: a triangle standing in the plane x = 1 through the floor
    assert one([(1, 1, -1), (1, 2, -1), (1, 1, 1)], floor) == IR.INTERSECT
    # touching at a corner: the query's corner on the floor's face, on its edge, on its corner; and just above
    assert one([(1, 1, 0), (2, 1, 3), (1, 2, 3)], floor) == IR.INTERSECT
    assert one([(2, 0, 0), (2, -1, 3), (3, -1, 3)], floor) == IR.INTERSECT
    assert one([(0, 0, 0), (-1, -1, 3), (-2, -1, 3)], floor) == IR.INTERSECT
    assert one([(1, 1, np.nextafter(F(0), F(1))), (2, 1, 3), (1, 2, 3)], floor) == 2
    # along an edge: two triangles hinged on the floor's edge y = 0, and an edge lying across the face
    assert one([(0, 0, 0), (4, 0, 0), (2, -3, 2)], floor) == IR.INTERSECT
    assert one([(1, 1, 0), (2, 1, 0), (1, 1, 3)], floor) == IR.INTERSECT
    # an edge through a face: the query's edge pierces the floor, its third corner far above
    assert one([(1, 1, -1), (1.5, 1, 1), (9, 9, 9)], floor) == IR.INTERSECT
    # coplanar: overlapping, one inside the other, disjoint (only an in-plane axis can tell: nq and nt see one plane)
    assert one([(1, 1, 0), (6, 1, 0), (1, 6, 0)], floor) == IR.INTERSECT
    assert one([(0.5, 0.5, 0), (1.5, 0.5, 0), (0.5, 1.5, 0)], floor) == IR.INTERSECT
    assert one([(-1, -1, 0), (9, -1, 0), (-1, 9, 0)], floor) == IR.INTERSECT
    assert one([(3, 3, 0), (5, 2.5, 0), (2.5, 5, 0)], floor) >= A0 + 11       # vertex boxes meet, beyond the hypotenuse
    assert one([(3, 3, 0), (5, 2.5, 0), (2.5, 5, 0)], floor) != IR.INTERSECT
    assert one([(5, 0, 0), (6, 0, 0), (5, 1, 0)], floor) == 0
    # parallel planes: the query's plane separates first
    assert one([(0, 0, 1), (4, 0, 1), (0, 4, 1)], floor) == 2                  # (stage 0 sees it already)
    assert one([(0, 0, 1), (4, 0, 3), (0, 4, 3)], [(0, 0, 0), (4, 0, 2), (0, 4, 2)]) == A0
    # only the scene triangle's plane separates: the query straddles nothing of the floor's plane ... above it, tilted
    assert one([(1, 1, 3), (3, 1, 4), (1, 3, 5)], [(-4, -4, -2), (8, -4, -2), (-4, 8, 6)]) in (A0, A0 + 1)
    # an edge pair separates: two long thin triangles passing each other like skew lines
    skew = one([(-3, 0, 0.5), (3, 0.2, 0.5), (3, -0.2, 0.7)], [(0, -3, 0), (0.2, 3, 0), (-0.2, 3, 0.1)])
    assert skew != IR.INTERSECT
    # identical triangles; with SKIP_SHARED not a member
    assert one(floor, floor) == IR.INTERSECT and one(floor, floor, True) == IR.SHARED
    # SKIP_SHARED: one common corner is enough; -0 equals +0; a NaN corner equals nothing
    fan = [(0, 0, 0), (-4, 0, 0), (0, -4, 1)]
    assert one(fan, floor) == IR.INTERSECT and one(fan, floor, True) == IR.SHARED
    minus = [(-0.0, -0.0, 0.0), (-4, 0, 0), (0, -4, 1)]
    assert one(minus, floor, True) == IR.SHARED
    assert one([(1, 1, -1), (1, 2, -1), (1, 1, 1)], floor, True) == IR.INTERSECT            # nothing shared: still a member
    nan_scene = [(np.nan, 0, 0), (4, 0, 0), (0, 4, 0)]
    assert one([(4, 0, 0), (5, 1, 0), (5, -1, 1)], nan_scene, True) == IR.SHARED             # its finite corner (4, 0, 0) is shared
    assert one([(9, 9, 9), (5, 1, 0), (5, -1, 1)], nan_scene, True) != IR.SHARED
    # degenerate: a point or segment query is not walked, a point or segment in the scene is not a member
    assert one([(1, 1, 0)] * 3, floor) == IR.UNWALKED
    assert one([(1, 1, -1), (1, 1, 1), (1, 1, 1)], floor) == IR.UNWALKED                    # the segment pierces the floor all the same
    assert one([(1, 1, -1), (1, 2, -1), (1, 1, 1)], [(1, 1, 0)] * 3) == IR.DEGENERATE
    assert one([(1, 1, -1), (1, 2, -1), (1, 1, 1)], [(0, 1.5, 0), (4, 1.5, 0), (2, 1.5, 0)]) == IR.DEGENERATE
    # a non-finite query is not walked
    for bad in (np.nan, np.inf, -np.inf):
        assert one([(1, 1, -1), (1, bad, -1), (1, 1, 1)], floor) == IR.UNWALKED
    q = IR.make_triangles([[(1, 1, -1), (1, 2, -1), (1, 1, 1)], [(1, 1, 0)] * 3, [(np.inf, 0, 0), (1, 0, 0), (0, 1, 0)]])
    assert IR.walked(q).tolist() == [True, False, False]
    out, n = IR.intersect(q, np.asarray(floor, F).reshape(-1), 4)
    assert n.tolist() == [1, 0, 0] and out.tolist() == [[0, -1, -1, -1], [-1] * 4, [-1] * 4]


@pytest.fixture(scope="module")
def lobed(pkg):
    world = pkg.World(IC.scene_path("lobed_528"))
    pos = np.asarray(world.arrays()["vertex_positions"], F)
    queries = IC.make_queries({"vertex_positions": pos}, 1200, seed=5)
    return pos, queries, IR.first_axis(queries, pos)


def test_prefix_counts_and_unwalked_queries(lobed):
    pos, queries, code = lobed
    IC.assert_interesting(code, "lobed_528")
    member = code == IR.INTERSECT
    want64, n = IR.intersect(queries, pos, 64)
    assert np.array_equal(n, member.sum(1)) and n.dtype == np.int32 and want64.dtype == np.int32
    for k in (0, 1, 2, 3, 4, 8, 9, 63):
        got, nk = IR.intersect(queries, pos, k)
        assert got.shape == (len(queries), k) and np.array_equal(got, want64[:, :k]) and np.array_equal(nk, n)
    for row in np.nonzero(n)[0][:200]:
        kept = want64[row][want64[row] >= 0]
        assert len(kept) == min(n[row], 64) and (np.diff(kept) > 0).all() and member[row, kept].all()
        assert not member[row, :kept[-1]].sum() > len(kept) and (want64[row, len(kept):] == -1).all()
    bad = ~IR.walked(queries)
    assert bad.sum() > 20 and (n[bad] == 0).all() and (want64[bad] == -1).all() and (code[bad] == IR.UNWALKED).all()
    # the forms of a query array agree
    same = IR.first_axis(IR.make_triangles(queries), pos)
    assert np.array_equal(same, code) and np.array_equal(IR.first_axis(queries.reshape(-1, 9), pos), code)
    # SKIP_SHARED on the scene's own triangles takes out each triangle and its neighbours, and nothing else on this mesh
    own = pos.reshape(-1, 3, 3)[:200]
    with_, without = IR.intersects(own, pos, True), IR.intersects(own, pos, False)
    assert without[np.arange(200), np.arange(200)].all() and without.sum(1).min() >= 4 and not with_.any()


SCALE_SCENES = ("lobed_528", "small_trisrc")
_scale_cache = {}


def set_kept_at(pkg, name, k):
    """whether the scene `name`, its largest coordinate 1.7, and its queries keep every query's set when both are scaled by 2^k"""
    if name not in _scale_cache:
        pos = np.asarray(pkg.World(IC.scene_path(name)).arrays()["vertex_positions"], F)
        pos = (pos * F(1.7 / np.abs(pos).max())).astype(F)
        queries = IC.make_queries({"vertex_positions": pos}, 600, seed=3)
        base = IR.intersects(queries, pos)
        assert 0.2 < base.any(1).mean() < 0.95
        _scale_cache[name] = (pos, queries, base)
    pos, queries, base = _scale_cache[name]
    s = F(2.0 ** k)
    with np.errstate(all="ignore"):
        return np.array_equal(IR.intersects(queries * s, pos * s), base)


@pytest.mark.parametrize("name", SCALE_SCENES)
def test_the_set_does_not_change_with_the_scale(pkg, name):
    """Scenes whose largest coordinate is 1.7, scaled with their queries by 2^k: the set is the unscaled one at both ends of the
    measured range (the header's) and at k = +-8."""
    for k in (SCALE_RANGE[0], -8, 8, SCALE_RANGE[1]):
        assert set_kept_at(pkg, name, k), k


def test_the_scale_range_is_the_measured_one(pkg):
    """The header's range is the intersection of the scenes' own: one step outside either end some scene's set changes."""
    for k in (SCALE_RANGE[0] - 1, SCALE_RANGE[1] + 1):
        kept = {name: set_kept_at(pkg, name, k) for name in SCALE_SCENES}
        print(f"k = {k}: set kept {kept}")
        assert not all(kept.values()), k


def test_walk_counters_by_hand_on_the_two_leaf_tree():
    """test_gpu_uniform_leaf.two_leaf_scene as arrays (test_overlap_reference.two_leaf_tree): a query through the band both
    leaves share, one in the left leaf, one in the right, one beside the root and a segment"""
    from test_overlap_reference import two_leaf_tree
    tree, node_boxes, corners = two_leaf_tree()
    q = np.asarray([[(0, -4.9, -1.9), (0.05, -4.9, 0.9), (-0.05, -4.8, 0.9)],      # in the band, through every z
                    [(-5, -4.5, -1.9), (-4.5, -4.5, 0.9), (-4.5, -4.4, 0.9)],       # the left leaf only
                    [(4, -4.5, -1.9), (4.5, -4.5, 0.9), (4.5, -4.4, 0.9)],          # the right leaf only
                    [(7, 0, 0), (8, 0, 0), (7, 1, 0)],                              # beside the root
                    [(0, -4.9, -1.9), (0, -4.9, 0.9), (0, -4.9, 0.9)]], F)           # a segment: not walked
    member = IR.intersects(q, corners.reshape(-1))
    assert member.sum(1).tolist() == [8, 3, 5, 0, 0]
    c = IR.walk_counters(tree, node_boxes, corners, q)
    assert c["node_visits"].tolist() == [3, 3, 3, 1, 0]
    assert c["leaf_visits"].tolist() == [2, 1, 1, 0, 0]
    assert c["triangle_tests"].tolist() == [8, 3, 5, 0, 0]
    assert c["stack"].tolist() == [1, 0, 0, 0, 0]
    a = IR.walk_counters(tree, node_boxes, corners, q, any_only=True)
    assert a["leaf_visits"].tolist() == [1, 1, 1, 0, 0] and a["triangle_tests"].tolist() == [1, 1, 1, 0, 0]
    assert a["node_visits"].tolist() == [3, 3, 3, 1, 0]
