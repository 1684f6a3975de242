"""The hand-shaped trees of tests/tree_shapes.py, on the CPU: every shape has the height profile its table claims (so that it
sits on the edge of the bottom-up schedule it is named for), is a valid pre-order BVH of its triangles, and the module's
TAIL_WIDTH is the kernels' kTailBlock; and the restatements the GPU tests compare with agree with brute force on the shapes:
the winding number's tree walk in its exact mode is the plain sum over the triangles in order, and the closest point does not
depend on how the triangles are cut into chunks, nor could a box of the tree hide it."""
import os
import re

import numpy as np
import pytest

import point_query_ref as R
import refit_ref
import tree_shapes as T
import winding_ref as W

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_built = {}


def shape(name):
    if name not in _built:
        _built[name] = T.build(name)
    return _built[name]


def corners_of(tree, vd):
    return vd[tree.triangle_vertices][:, :, :3]


def some_points(corners, n, seed):
    """points on the triangles, near them, about the scene and far from it"""
    rng = np.random.default_rng(seed)
    verts = corners.reshape(-1, 3).astype(np.float64)
    lo, hi = verts.min(0), verts.max(0)
    t = rng.integers(0, len(corners), n)
    b = rng.random((n, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    v = corners[t].astype(np.float64)
    p = v[:, 0] + b[:, :1] * (v[:, 1] - v[:, 0]) + b[:, 1:] * (v[:, 2] - v[:, 0])
    kind = rng.integers(0, 4, n)
    p[kind == 1] += rng.normal(size=((kind == 1).sum(), 3)) * 0.3
    box = kind == 2
    p[box] = lo + (hi - lo) * (rng.random((box.sum(), 3)) * 1.5 - 0.25)
    p[kind == 3] = (lo + hi) / 2 + rng.normal(size=((kind == 3).sum(), 3)) * 50 * np.linalg.norm(hi - lo)
    at = rng.random(n) < 0.1
    p[at] = verts[rng.integers(0, len(verts), at.sum())]
    return p.astype(F)


@pytest.mark.parametrize("name", T.NAMES)
def test_height_profiles_are_the_tables(name):
    tree, vd = shape(name)
    nodes, branches = T.PROFILES[name]
    profile = T.height_profile(tree)
    assert tree.node_count == nodes and profile.sum() == nodes, name
    assert list(profile[1:]) == branches, f"{name}: branches per height {list(profile[1:])}"
    assert profile[0] == (nodes + 1) // 2 and len(profile) - 1 <= 16, name
    assert np.array_equal(T.heights(tree), W.heights(tree))
    # where the schedule's edges are: the heights above the tail width, and the tail's first height
    wide = [int(c) for c in profile[1:] if c > T.TAIL_WIDTH]
    assert all(c > T.TAIL_WIDTH for c in profile[1:1 + len(wide)]), name      # (the wide heights come first)
    tail_first = int(profile[1 + len(wide)]) if len(profile) > 1 + len(wide) else None
    assert (wide, tail_first) == {"leaf_root": ([], None), "one_branch": ([], 1), "tail_full": ([], 1024), "wide_by_one": ([1025], 512),
                                  "two_wide": ([4096, 2048], 1024), "lopsided": ([4096, 2048], 1024),
                                  "mixed_spine": ([2054, 1026], 512)}[name]


def test_mixed_children():
    """the branches whose children the two mechanisms wrote: wide_by_one's root, each of mixed_spine's four spine branches"""
    for name, expected in (("wide_by_one", [(12, 1, 11)]), ("mixed_spine", [(13, 1, 12), (14, 2, 13), (15, 1, 14), (16, 2, 15)]),
                           ("two_wide", []), ("lopsided", []), ("tail_full", [])):
        tree, _ = shape(name)
        h, profile = T.heights(tree), T.height_profile(tree)
        wide = np.concatenate([[False], profile[1:] > T.TAIL_WIDTH])
        b = np.nonzero(tree.negative >= 0)[0]
        hn, hp = h[tree.negative[b]], h[tree.positive[b]]
        mixed = b[(hn > 0) & (hp > 0) & (wide[hn] != wide[hp])]
        found = sorted((int(h[k]), int(min(h[tree.negative[k]], h[tree.positive[k]])), int(max(h[tree.negative[k]], h[tree.positive[k]])))
                       for k in mixed)
        assert found == expected, name


def test_spine3_is_the_spine_the_walks_are_tested_on():
    """7 nodes, one branch at each of the heights 1 to 3; the root's branch child is its negative one, that branch's branch
    child its positive one, and the deepest branch holds two leaves: four leaves of 1, 2, 3 and 1 triangles"""
    tree, _ = shape("spine3")
    h = T.heights(tree)
    assert tree.node_count == 7 and list(T.height_profile(tree)) == [4, 1, 1, 1] and h[0] == 3
    n1 = tree.negative[0]
    assert h[n1] == 2 and h[tree.positive[0]] == 0
    n2 = tree.positive[n1]
    assert h[n2] == 1 and h[tree.negative[n1]] == 0 and h[tree.negative[n2]] == h[tree.positive[n2]] == 0
    assert tree.triangles[tree.negative < 0].tolist() == [1, 2, 3, 1] and "spine3" not in T.NAMES


@pytest.mark.parametrize("name", T.NAMES + tuple(T.WALK_SHAPES))
def test_the_arrays_are_a_valid_preorder_bvh(name):
    tree, vd = shape(name)
    n = tree.node_count
    leaf = tree.negative < 0
    assert tree.parent[0] == -1 and np.array_equal(leaf, tree.positive < 0)
    # pre-order: a branch's negative child follows it, its positive child follows the negative subtree
    size = np.ones(n, np.int64)
    for k in range(n - 1, -1, -1):
        if not leaf[k]:
            size[k] = 1 + size[tree.negative[k]] + size[tree.positive[k]]
    b = np.nonzero(~leaf)[0]
    assert size[0] == n
    assert np.array_equal(tree.negative[b], b + 1) and np.array_equal(tree.positive[b], b + 1 + size[tree.negative[b]])
    assert np.array_equal(tree.parent[tree.negative[b]], b) and np.array_equal(tree.parent[tree.positive[b]], b)
    # every triangle in exactly one leaf, the leaves in order; 1, 2, 3 triangles by turns
    leaves = np.nonzero(leaf)[0]
    count, start = tree.triangles[leaves], tree.start[leaves]
    t_count = len(tree.triangle_vertices)
    assert np.array_equal(start, np.cumsum(count) - count) and count.sum() == t_count
    assert np.array_equal(count, 1 + np.arange(len(leaves)) % 3) if n > 1 else count[0] == 3
    assert np.all(tree.triangles[b] == 0)
    # every vertex is some corner; the indices are not the identity
    assert np.array_equal(np.sort(tree.triangle_vertices.reshape(-1)), np.arange(len(vd)))
    assert t_count < 2 or not np.array_equal(tree.triangle_vertices.reshape(-1), np.arange(len(vd)))
    # boxes: the restated ones; children's inside their parent's; split on x with the negative child at lower x
    corners = corners_of(tree, vd)
    assert np.array_equal(tree.box.view(np.uint32), refit_ref.node_boxes(tree, corners).view(np.uint32))
    for child in (tree.negative[b], tree.positive[b]):
        assert np.all(tree.box[child, :3] >= tree.box[b, :3]) and np.all(tree.box[child, 3:] <= tree.box[b, 3:])
    assert np.all(tree.box[tree.negative[b], 3] < tree.box[tree.positive[b], 0])
    assert np.all(tree.direction[b] == (1, 0, 0)) and np.all(tree.direction[leaves] == 0)
    # the geometry: coordinates in range, z varies, both windings, unit normals that differ
    assert corners.min() >= 2.0 ** -3 and corners.max() <= 2.0 ** 12 and refit_ref.exact_div_ok(tree.box)
    assert np.all((corners[1:, :, 2] != corners[:-1, :, 2]).all(1)) and np.all(corners[:, 0, 2] != corners[:, 1, 2])
    nx = W.triangle_terms(corners.reshape(-1))[0][:, 0]
    assert (nx > 0).any() and (nx < 0).any()
    normals = vd[:, 6:9].astype(np.float64)
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-6) and len(np.unique(normals, axis=0)) == len(normals)


def test_tail_width_is_the_kernels():
    """the shapes are built around 1024; when kTailBlock changes they must move with it"""
    for path in ("refit/refit.hip", "winding/winding.hip"):
        with open(os.path.join(ROOT, "shader-ray_amd", path)) as f:
            found = re.findall(r"^constexpr int kTailBlock = (\d+);", f.read(), re.M)
        assert found == [str(T.TAIL_WIDTH)], (path, found)


@pytest.mark.parametrize("name", T.NAMES)
def test_exact_winding_walk_is_the_sum_over_triangles(name):
    tree, vd = shape(name)
    corners = corners_of(tree, vd)
    ref = W.Restated.of_tree(tree, corners, tree.box)
    q = some_points(corners, 200, seed=3)
    got = ref.w(q, np.inf)
    with np.errstate(all="ignore"):
        terms = np.stack([W.triangle_terms_at(corners, np.broadcast_to(p, (len(corners), 3))) for p in q])
    want = np.cumsum(np.concatenate([np.zeros((len(q), 1), F), terms], axis=1), axis=1, dtype=F)[:, -1]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


@pytest.mark.parametrize("name", T.NAMES)
def test_closest_point_does_not_depend_on_the_partition(name):
    tree, vd = shape(name)
    corners = corners_of(tree, vd)
    pts = np.zeros(200, R.POINT_DTYPE)
    pts["p"], pts["max_dist2"] = some_points(corners, 200, seed=4), np.inf
    want = R.closest(corners.reshape(-1), pts)
    assert (want["triangle"] >= 0).all()
    again = R.closest(corners.reshape(-1), pts, point_chunk=64, pairs=64 * 257)     # 257 triangles at a time
    assert np.array_equal(R.as_bits(want), R.as_bits(again)), name
    # no box on the winner's path bounds it away: the header's box bound of the winner's leaf and of the root is at most dist2
    leaves = np.nonzero(tree.negative < 0)[0]
    leaf_of = np.repeat(leaves, tree.triangles[leaves])[want["triangle"]]
    p = tuple(pts["p"][:, k] for k in range(3))
    for node in (leaf_of, np.zeros(len(pts), np.int64)):
        with np.errstate(all="ignore"):
            bound = R.box_bound(R.NumpyOps, p, tuple(tree.box[node, k] for k in range(3)), tuple(tree.box[node, 3 + k] for k in range(3)))
        assert np.all(bound <= want["dist2"]), name
