"""Hand-shaped canonical trees at the edges of the bottom-up schedule (csrc/tree_order.h: for_each_level) that the refit and the
winding-number derivation run: one launch for the leaves, one launch per height of more than TAIL_WIDTH branches, one
workgroup of TAIL_WIDTH threads for the remaining heights.  Pure numpy.

`build(name)` returns (refit_ref.TreeArrays, vertex_data float32 [V, 9]) in pre-order (root = node 0; a node, its negative
subtree, its positive subtree).  P(k) is the perfect tree of 2^k leaves:

  leaf_root     one leaf of 3 triangles            1 node       no branch pass at all; height 0
  one_branch    P(1)                               3 nodes      the tail is the root only
  tail_full     P(11)                              4095 nodes   height 1 has exactly 1024 branches: everything is in the tail,
                                                                whose first height fills every thread of the workgroup
  wide_by_one   root { P(11), P(1) }               4099 nodes   height 1 has 1025: one wide launch whose last workgroup has one
                                                                live thread, the tail starts at height 2; the root's children
                                                                are P(1)'s root (written by the wide launch) and P(11)'s root
                                                                (written by the tail, ten heights later)
  two_wide      P(13)                              16383 nodes  heights 1 and 2 are wide, the tail starts at height 3 with 1024
  lopsided      a spine of 13 branches: branch i   16383 nodes  P(13)'s profile (spine branch i and P(i)'s root are both of
                from the bottom has P(i) as its                 height i, so height h has (2^(13-h) - 1) + 1 branches) in a
                negative child and the branch                   tree whose subtrees' sizes halve from the root down: the nodes
                below as its positive one; the                  of one height are spread over thirteen subtrees of the
                bottom's positive child is a leaf               pre-order
  mixed_spine   four spine branches over P(12),    8215 nodes   heights 1 and 2 are wide (2054 and 1026), the tail starts at
                with negative children P(1),                    height 3; every spine branch (heights 13 to 16) combines a
                P(2), P(1), P(2)                                child a wide launch wrote with a child the tail wrote; siblings'
                                                                heights differ by up to 14

The geometry makes each tree a legitimate BVH of its triangles: the triangles lie along x in leaf order, disjoint in x, every
branch splits on direction (1, 0, 0) with its negative child at lower x (a leaf's direction is 0, as the builder leaves it), and
the boxes are refit_ref.node_boxes.  Leaf j holds 1 + (j % 3) triangles (leaf_root's single leaf: 3), y and z vary from corner
to corner, four triangles in ten are wound the other way (the second of every three and a
seeded tenth), the normals are seeded unit vectors, and the vertices are stored in
a seeded permutation so that triangle_vertices is not the identity.  Coordinates stay within [2^-3, 2^12] (exact_div_ok = 1).
Scene creation asks nothing else of these trees: its proof that the link tables are one canonical tree holds for any binary
tree flattened by shray_flatten_device."""
from __future__ import annotations

import numpy as np

import refit_ref

F = np.float32
TAIL_WIDTH = 1024           # kTailBlock of refit/refit.hip and winding/winding.hip (test_tree_shapes_reference pins it)
PITCH, WIDTH = 0.2, 0.15    # a triangle's slot along x and how much of it the triangle takes

LEAF = ("P", 0)


def P(k):
    return ("P", k)


def B(negative, positive):
    return ("B", negative, positive)


def _lopsided():
    spine = LEAF
    for i in range(13):
        spine = B(P(i), spine)
    return spine


def _mixed_spine():
    spine = P(12)
    for k in (1, 2, 1, 2):
        spine = B(P(k), spine)
    return spine


SHAPES = {
    "leaf_root": lambda: LEAF,
    "one_branch": lambda: P(1),
    "tail_full": lambda: P(11),
    "wide_by_one": lambda: B(P(11), P(1)),
    "two_wide": lambda: P(13),
    "lopsided": _lopsided,
    "mixed_spine": _mixed_spine,
}
NAMES = tuple(SHAPES)

# Shapes for the walks alone (test_gpu_packed_walk.py), outside NAMES: the schedule's tests do not run over them.
#   spine3   a spine of height 3 that leans to the negative side once and to the positive side once: root { N1, leaf },
#            N1 { leaf, N2 }, N2 { leaf, leaf } -- 7 nodes; a walk down it holds two stack entries at once, and a pop can
#            return a branch whose own sibling still waits
WALK_SHAPES = {
    "spine3": lambda: B(B(LEAF, B(LEAF, LEAF)), LEAF),
}

# name -> (nodes, branches per height from 1 up): what the module's table claims
PROFILES = {
    "leaf_root": (1, []),
    "one_branch": (3, [1]),
    "tail_full": (4095, [1 << (11 - h) for h in range(1, 12)]),
    "wide_by_one": (4099, [1025] + [1 << (11 - h) for h in range(2, 12)] + [1]),
    "two_wide": (16383, [1 << (13 - h) for h in range(1, 14)]),
    "lopsided": (16383, [1 << (13 - h) for h in range(1, 14)]),
    "mixed_spine": (8215, [2054, 1026] + [1 << (12 - h) for h in range(3, 13)] + [1, 1, 1, 1]),
}


def _preorder(spec):
    """(parent, negative, positive) int32 of the tree `spec` describes"""
    parent, negative, positive = [], [], []

    def visit(s, up):
        k = len(parent)
        parent.append(up)
        negative.append(-1)
        positive.append(-1)
        if s[0] == "P" and s[1] == 0:
            return k
        kids = (P(s[1] - 1), P(s[1] - 1)) if s[0] == "P" else s[1:]
        negative[k] = visit(kids[0], k)
        positive[k] = visit(kids[1], k)
        return k

    visit(spec, -1)
    return np.array(parent, np.int32), np.array(negative, np.int32), np.array(positive, np.int32)


def heights(tree) -> np.ndarray:
    h = np.zeros(tree.node_count, np.int64)
    for k in range(tree.node_count - 1, -1, -1):   # pre-order: children come after their parent
        if tree.negative[k] >= 0:
            h[k] = 1 + max(h[tree.negative[k]], h[tree.positive[k]])
    return h


def height_profile(tree) -> np.ndarray:
    """the number of nodes of each height, 0 (the leaves) to the root's"""
    return np.bincount(heights(tree))


def build(name):
    every = {**SHAPES, **WALK_SHAPES}
    parent, negative, positive = _preorder(every[name]())
    n = len(parent)
    leaf = np.nonzero(negative < 0)[0]                       # in pre-order: from lower x to higher
    count = 1 + np.arange(len(leaf)) % 3 if n > 1 else np.array([3])
    start, triangles = np.zeros(n, np.int32), np.zeros(n, np.int32)
    start[leaf], triangles[leaf] = np.cumsum(count) - count, count
    T = int(count.sum())

    rng = np.random.default_rng(1000 + tuple(every).index(name))
    corners = np.empty((T, 3, 3), np.float64)
    x0 = 1.0 + PITCH * np.arange(T)
    corners[:, :, 0] = x0[:, None] + WIDTH * np.array([0.0, 1.0, 0.5]) * (0.6 + 0.4 * rng.random((T, 3)))
    corners[:, :, 1] = (5.0 + 6.0 * rng.random(T))[:, None] + 5.0 * (rng.random((T, 3)) - 0.5)
    corners[:, :, 2] = (5.0 + 6.0 * rng.random(T))[:, None] + 5.0 * (rng.random((T, 3)) - 0.5)
    e0, e1 = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
    flipped = (e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1] < 0) != ((np.arange(T) % 3 == 1) | (rng.random(T) < 0.1))
    corners[flipped] = corners[flipped][:, [0, 2, 1]]           # the face normal points to +x, of four triangles in ten to -x
    normals = rng.standard_normal((T, 3, 3))
    normals /= np.linalg.norm(normals, axis=2, keepdims=True)

    perm = rng.permutation(3 * T).astype(np.int32)           # corner c is vertex perm[c]
    vertex_data = np.zeros((3 * T, 9), F)
    vertex_data[perm, 0:3] = corners.reshape(-1, 3).astype(F)
    vertex_data[perm, 3:6] = rng.random((3 * T, 3)).astype(F)
    vertex_data[perm, 6:9] = normals.reshape(-1, 3).astype(F)
    triangle_vertices = perm.reshape(T, 3).copy()

    direction = np.zeros((n, 3), F)
    direction[negative >= 0, 0] = 1.0
    tree = refit_ref.TreeArrays(parent, negative, positive, np.zeros((n, 6), F), direction, start, triangles, triangle_vertices)
    tree.box = refit_ref.node_boxes(tree, vertex_data[triangle_vertices][:, :, :3])
    return tree, vertex_data
