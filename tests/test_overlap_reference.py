"""The box-overlap restatement (tests/overlap_ref.py) against a truth that shares nothing with it: on integer-lattice inputs,
where every fp32 operation of include/shader_ray_overlap.h is exact, a clip of the triangle against the box's six closed
half-spaces in fractions.Fraction; then cases known by hand, the prefix and count rules, the boxes that are not walked, and
the range of scales 2^k over which the set does not change."""
from fractions import Fraction

import numpy as np
import pytest

import overlap_cases as OC
import overlap_ref as OR

F = np.float32
SCALE_RANGE = (-27, 44)   # include/shader_ray_overlap.h, DESIGN section 17


def clip_overlaps(tri, lo, hi):
    """the triangle (three integer corners) clipped against the closed box, in exact rationals: non-empty means overlap"""
    poly = [tuple(Fraction(int(x)) for x in p) for p in tri]
    for axis in range(3):
        for bound, sign in ((Fraction(lo[axis]), -1), (Fraction(hi[axis]), 1)):
            def inside(p):
                return sign * (p[axis] - bound) <= 0
            out = []
            for i, p in enumerate(poly):
                q = poly[(i + 1) % len(poly)]
                if inside(p):
                    out.append(p)
                if inside(p) != inside(q):
                    t = (bound - p[axis]) / (q[axis] - p[axis])
                    out.append(tuple(p[j] + t * (q[j] - p[j]) for j in range(3)))
            poly = out
            if not poly:
                return False
    return True


def lattice_pairs(n, seed):
    """triangle corners in {-8 .. 8}^3 (a share of them points and segments) and box bounds at multiples of 1/2 in the same
    range (a share of zero extent), the box placed about the triangle so that neither answer is rare"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, (n, 3))
    b = np.clip(a + rng.integers(-5, 6, (n, 3)), -8, 8)
    c = np.clip(a + rng.integers(-5, 6, (n, 3)), -8, 8)
    kind = rng.random(n)
    c = np.where((kind < 0.06)[:, None], b, c)          # a segment
    b = np.where((kind < 0.02)[:, None], a, b)          # a point (with c = b = a)
    c = np.where((kind < 0.02)[:, None], a, c)
    tri = np.stack([a, b, c], 1)
    centre = tri.mean(1) + rng.normal(size=(n, 3)) * 2.5
    half = rng.integers(0, 7, (n, 3)) / 2.0 * (rng.random((n, 3)) < 0.85)
    lo = np.clip(np.round((centre - half) * 2) / 2, -8, 8)
    hi = np.clip(lo + np.round(half * 4) / 2, -8, 8)
    return tri, lo, hi


def test_lattice_pairs_equal_the_exact_clip():
    n = 24000
    tri, lo, hi = lattice_pairs(n, seed=12)
    assert n >= 20000 and (lo <= hi).all() and (lo * 2 == np.round(lo * 2)).all() and (hi * 2 == np.round(hi * 2)).all()
    # every pair through first_axis itself, the function the GPU tests compare with: blocks of boxes against the blocks'
    # own triangles, the pair being the diagonal
    t32, block = tri.astype(F), 400
    code = np.concatenate([np.diagonal(OR.first_axis(t32[s:s + block].reshape(-1), OR.make_boxes(lo[s:s + block], hi[s:s + block])))
                           for s in range(0, n, block)])
    assert code.shape == (n,) and (code != OR.UNWALKED).all()
    truth = np.array([clip_overlaps(tri[i], [Fraction(int(x * 2), 2) for x in lo[i]], [Fraction(int(x * 2), 2) for x in hi[i]])
                      for i in range(n)])
    share = truth.mean()
    firsts = np.bincount(code[code >= 0], minlength=OR.AXES)
    print(f"lattice: {n} pairs, overlap {share:.3f}, degenerate triangles {(np.ptp(tri, axis=1) == 0).all(1).mean():.3f}, "
          f"zero-extent boxes {(lo == hi).any(1).mean():.3f}, first separating axis {firsts.tolist()}")
    assert 0.2 < share < 0.8
    assert (firsts >= 1).all(), firsts
    wrong = np.nonzero((code == OR.OVERLAP) != truth)[0]
    assert len(wrong) == 0, (len(wrong), tri[wrong[:3]], lo[wrong[:3]], hi[wrong[:3]], code[wrong[:3]])


def one(tri, lo, hi):
    return int(OR.first_axis(np.asarray(tri, F).reshape(-1), OR.make_boxes([lo], [hi]))[0, 0])


def test_analytic_cases():
    unit = ((0, 0, 0), (1, 1, 1))
    # touching counts: a triangle in the plane x = 1, one that touches the corner (1, 1, 1) only, one just beyond
    assert one([(1, 0, 0), (1, 1, 0), (1, 0, 1)], *unit) == OR.OVERLAP
    assert one([(1, 1, 1), (2, 1, 1), (1, 2, 2)], *unit) == OR.OVERLAP
    assert one([(np.nextafter(F(1), F(2)), 0, 0), (2, 1, 0), (2, 0, 1)], *unit) == 0
    # a triangle lying in a box face, inside it and larger than it
    assert one([(0.25, 0.25, 1), (0.75, 0.25, 1), (0.25, 0.75, 1)], *unit) == OR.OVERLAP
    assert one([(-5, -5, 0), (9, -5, 0), (-5, 9, 0)], *unit) == OR.OVERLAP
    # a large triangle that contains the whole box's cross-section
    assert one([(-10, -10, 0.5), (20, -10, 0.5), (-10, 20, 0.5)], *unit) == OR.OVERLAP
    # the plane cuts the corner (1, 1, .) of the box but the edges pass outside: only an edge axis separates.  In z = 0.5 the
    # corners (1.2, 0.9), (0.9, 1.2) and (3, 3): the vertex box reaches into the box, the plane z = 0.5 crosses it, the edge
    # from (1.2, 0.9) to (0.9, 1.2) lies on x + y = 2.1 beyond the corner
    assert one([(1.2, 0.9, 0.5), (0.9, 1.2, 0.5), (3, 3, 0.5)], *unit) == 4 + 2          # edge e0 with the box's z
    # a tilted one whose plane passes through the box: again no box axis and not the plane
    code = one([(1.3, 0.8, 0.2), (0.8, 1.3, 0.8), (3, 3, 0.5)], *unit)
    assert code >= 4, code
    # the plane alone: the vertex box covers the box, the plane passes beside it
    assert one([(3, -1, -1), (-1, 3, -1), (3, 3, 3)], (0, 0, 0), (0.25, 0.25, 0.25)) == 3
    # points and segments
    assert one([(0.5, 0.5, 0.5)] * 3, *unit) == OR.OVERLAP
    assert one([(2, 2, 2)] * 3, *unit) == 0
    assert one([(-1, 0.5, 0.5), (2, 0.5, 0.5), (2, 0.5, 0.5)], *unit) == OR.OVERLAP
    assert one([(1.5, -1, 0.5), (1.5, -1, 0.5), (-1, 1.5, 0.5)], *unit) == OR.OVERLAP      # the segment x + y = 0.5 .. crosses the box
    assert one([(2.5, -1, 0.5), (2.5, -1, 0.5), (-1, 2.5, 0.5)], (0, 0, 0), (0.5, 0.5, 1)) >= 4   # x + y = 1.5 passes the corner (0.5, 0.5)
    # zero-extent boxes: a point on the triangle, beside it, a segment through it
    tri = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
    assert one(tri, (1, 1, 0), (1, 1, 0)) == OR.OVERLAP
    assert one(tri, (1, 1, 0.5), (1, 1, 0.5)) == 2
    assert one(tri, (3, 3, 0), (3, 3, 0)) >= 4
    assert one(tri, (1, 1, -1), (1, 1, 1)) == OR.OVERLAP


@pytest.fixture(scope="module")
def lobed(pkg):
    world = pkg.World(OC.scene_path("lobed_528"))
    arrays = world.arrays()
    boxes = OC.make_boxes(arrays, 1500, seed=5)
    return np.asarray(arrays["vertex_positions"], F), boxes, OR.first_axis(arrays["vertex_positions"], boxes)


def test_prefix_counts_and_unwalked_boxes(lobed):
    pos, boxes, code = lobed
    member = code == OR.OVERLAP
    want64, n = OR.overlap(pos, boxes, 64)
    assert np.array_equal(n, member.sum(1)) and n.dtype == np.int32 and want64.dtype == np.int32
    for k in (0, 1, 2, 3, 4, 8, 9, 63):
        got, nk = OR.overlap(pos, boxes, k)
        assert got.shape == (len(boxes), k) and np.array_equal(got, want64[:, :k]) and np.array_equal(nk, n)
    for row in np.nonzero(n)[0][:200]:
        kept = want64[row][want64[row] >= 0]
        assert len(kept) == min(n[row], 64) and (np.diff(kept) > 0).all() and member[row, kept].all()
        assert not member[row, :kept[-1]].sum() > len(kept) and (want64[row, len(kept):] == -1).all()
    bad = ~OR.walked(boxes)
    assert bad.sum() > 20 and (n[bad] == 0).all() and (want64[bad] == -1).all() and (code[bad] == OR.UNWALKED).all()
    hand = OR.make_boxes([(0, 0, 0), (0, np.nan, 0), (0, 0, 0), (-np.inf, 0, 0), (0, 0, 0)], [(1, -1, 1), (1, 1, 1), (1, 1, np.inf), (1, 1, 1), (0, 0, 0)])
    assert OR.walked(hand).tolist() == [False, False, False, False, True]
    assert OR.overlap(pos, hand[:4], 4)[1].tolist() == [0, 0, 0, 0]


def scaled(boxes, s):
    out = boxes.copy()
    out["lo"], out["hi"] = boxes["lo"] * s, boxes["hi"] * s
    return out


SCALE_SCENES = ("lobed_528", "small_trisrc")
_scale_cache = {}


def set_kept_at(pkg, name, k):
    """whether the scene `name`, its largest coordinate 1.7, and its boxes keep every box's set when both are scaled by 2^k"""
    if name not in _scale_cache:
        pos = np.asarray(pkg.World(OC.scene_path(name)).arrays()["vertex_positions"], F)
        pos = (pos * F(1.7 / np.abs(pos).max())).astype(F)
        boxes = OC.make_boxes({"vertex_positions": pos}, 1500, seed=3)
        base = OR.overlaps(pos, boxes)
        assert 0.2 < base.any(1).mean() < 0.95
        _scale_cache[name] = (pos, boxes, base)
    pos, boxes, base = _scale_cache[name]
    s = F(2.0 ** k)
    return np.array_equal(OR.overlaps(pos * s, scaled(boxes, s)), base)


@pytest.mark.parametrize("name", SCALE_SCENES)
def test_the_set_does_not_change_with_the_scale(pkg, name):
    """Scenes whose largest coordinate is 1.7, scaled with their boxes by 2^k: the set is the unscaled one at both ends of the
    measured range (the header's) and at k = +-8."""
    for k in (SCALE_RANGE[0], -8, 8, SCALE_RANGE[1]):
        assert set_kept_at(pkg, name, k), k


def test_the_scale_range_is_the_measured_one(pkg):
    """The header's range is the intersection of the scenes' own: one step outside either end some scene's set changes (not
    every scene's: each holds a step or two further on one side)."""
    for k in (SCALE_RANGE[0] - 1, SCALE_RANGE[1] + 1):
        kept = {name: set_kept_at(pkg, name, k) for name in SCALE_SCENES}
        print(f"k = {k}: set kept {kept}")
        assert not all(kept.values()), k


# the walk's restatement (overlap_ref.walk_counters) ------------------------------------------------------------------------------

def two_leaf_tree():
    """test_gpu_uniform_leaf.two_leaf_scene as arrays: a branch over a leaf of 3 and a leaf of 5 triangles, its hand-made boxes"""
    import refit_ref
    left = [[[-6, -5, z], [0.2, -5, z], [-3, 5, z]] for z in (-0.5, 0.25, -1.0)]
    right = [[[-0.2, -5, z], [6, -5, z], [3, 5, z]] for z in (0.0, -0.75, 0.5, -0.25, -1.5)]
    i32 = lambda *x: np.array(x, np.int32)
    tree = refit_ref.TreeArrays(i32(-1, 0, 0), i32(1, -1, -1), i32(2, -1, -1), None, None, i32(0, 0, 3), i32(0, 3, 5), None)
    boxes = np.array([[-6.5, -6, -2, 6.5, 6, 1], [-6.5, -6, -2, 0.25, 6, 1], [-0.25, -6, -2, 6.5, 6, 1]], F)
    return tree, boxes, np.asarray(left + right, F)


def test_walk_counters_by_hand_on_the_two_leaf_tree():
    tree, node_boxes, corners = two_leaf_tree()
    # the band both leaves share, the left leaf, the right leaf, beside the root, and an inverted box
    band = OR.make_boxes([(-0.1, -5.0, -2.0), (-6.0, -4.0, -2.0), (0.5, -4.0, -2.0), (7.0, 0.0, 0.0), (1.0, 0.0, 0.0)],
                         [(0.1, -4.75, 1.0), (-4.0, -3.0, 1.0), (4.0, -3.0, 1.0), (8.0, 1.0, 1.0), (0.0, 1.0, 1.0)])
    member = OR.overlaps(corners.reshape(-1), band)
    assert member.sum(1).tolist() == [8, 3, 5, 0, 0]
    c = OR.walk_counters(tree, node_boxes, corners, band)
    assert c["node_visits"].tolist() == [3, 3, 3, 1, 0]      # the root, then both children of an entered branch; nothing unwalked
    assert c["leaf_visits"].tolist() == [2, 1, 1, 0, 0]
    assert c["triangle_tests"].tolist() == [8, 3, 5, 0, 0]
    assert c["stack"].tolist() == [1, 0, 0, 0, 0]             # the positive leaf waits only where both overlap
    a = OR.walk_counters(tree, node_boxes, corners, band, any_only=True)
    assert member[0, 0] and member[1, 0] and member[2, 3]     # the first triangle of the first leaf entered touches
    assert a["node_visits"].tolist() == [3, 3, 3, 1, 0] and a["leaf_visits"].tolist() == [1, 1, 1, 0, 0]
    assert a["triangle_tests"].tolist() == [1, 1, 1, 0, 0] and a["stack"].tolist() == [1, 0, 0, 0, 0]
    # ANY walks on while nothing touches: a box in the left leaf's node box, under its triangles (z = -1.75), touches none
    under = OR.make_boxes([(-5.0, -4.0, -1.9)], [(-4.0, -3.0, -1.75)])
    assert not OR.overlaps(corners.reshape(-1), under).any()
    a = OR.walk_counters(tree, node_boxes, corners, under, any_only=True)
    assert (a["node_visits"][0], a["leaf_visits"][0], a["triangle_tests"][0]) == (3, 1, 3)


def test_walk_counters_on_a_root_that_is_a_leaf():
    import tree_shapes
    tree, vd = tree_shapes.build("leaf_root")
    corners = vd[tree.triangle_vertices][:, :, :3]
    root = tree.box[0]
    boxes = OR.make_boxes([root[:3], root[3:] + F(1), (np.nan, 0, 0)], [root[3:], root[3:] + F(2), (1, 1, 1)])
    member = OR.overlaps(corners.reshape(-1), boxes)
    assert member.sum(1).tolist() == [3, 0, 0]
    for any_only, tests in ((False, 3), (True, 1)):
        c = OR.walk_counters(tree, tree.box, corners, boxes, any_only=any_only, member=member)
        assert c["node_visits"].tolist() == [1, 1, 0] and c["leaf_visits"].tolist() == [1, 0, 0]
        assert c["triangle_tests"].tolist() == [tests, 0, 0] and c["stack"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("name", ["wide_by_one", "mixed_spine"])
def test_walk_counters_equal_the_closed_form(name):
    """The counting form's visited set does not depend on the order: a node is entered iff it and every ancestor overlap the
    box, so node_visits = 1 + 2 (branches entered), leaf_visits = the leaves entered, triangle_tests = their triangles --
    computed here node by node over all boxes at once, with no stack and no order.  The greatest stack depth any box reaches
    is the shape's deepest (overlap_shape_cases.deepest_stack), reached by the root's own box."""
    import overlap_shape_cases as SH
    import tree_shapes
    tree, vd = tree_shapes.build(name)
    corners = vd[tree.triangle_vertices][:, :, :3]
    boxes = SH.shape_boxes(tree, corners, tree.box, seed=3)
    lo, hi = OR.lo_hi(boxes)
    entered = np.zeros((tree.node_count, len(boxes)), bool)
    for k in range(tree.node_count):
        nb = tree.box[k]
        inside = ~((nb[3:] < lo) | (nb[:3] > hi)).any(1)
        entered[k] = inside & OR.walked(boxes) & (entered[tree.parent[k]] if k else True)
    branch = tree.negative >= 0
    c = OR.walk_counters(tree, tree.box, corners, boxes)
    assert np.array_equal(c["node_visits"], np.where(OR.walked(boxes), 1 + 2 * entered[branch].sum(0), 0))
    assert np.array_equal(c["leaf_visits"], entered[~branch].sum(0))
    assert np.array_equal(c["triangle_tests"], (entered[~branch] * tree.triangles[~branch][:, None]).sum(0))
    assert c["leaf_visits"].sum() > 10 * len(boxes) and (c["node_visits"] == 1).sum() > 20
    whole = np.nonzero((boxes["lo"] == tree.box[0, :3]).all(1) & (boxes["hi"] == tree.box[0, 3:]).all(1))[0]
    assert len(whole) == 1 and c["stack"].max() == c["stack"][whole[0]] == SH.deepest_stack(tree)
    assert c["node_visits"][whole[0]] == tree.node_count
    # ANY never does more than the counting form, and does less wherever something touches early
    member = OR.overlaps(corners.reshape(-1), boxes)
    a = OR.walk_counters(tree, tree.box, corners, boxes, any_only=True, member=member)
    for key in OR.COUNTERS:
        assert (a[key] <= c[key]).all()
    none = ~member.any(1)
    assert all(np.array_equal(a[key][none], c[key][none]) for key in OR.COUNTERS) and a["triangle_tests"].sum() < c["triangle_tests"].sum() / 10
