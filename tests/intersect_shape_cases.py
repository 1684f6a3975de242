"""The query triangles of the triangle-intersection tests over the hand-shaped trees of tests/tree_shapes.py
(tests/test_intersect_shape_reference.py on the CPU, tests/test_gpu_intersect_tree_shapes.py on the GPU).  No test and no GPU in
here.

intersect_cases.make_queries sizes its slicers by the whole scene, and a shape is a strip of up to 16,384 triangles along x, one
per 0.2, disjoint in x, in leaf order: a run of consecutive triangles is an x-slab, and a seam of the tree
(overlap_shape_cases.seams) is a triangle index.  The walk's cull sees only a query's VERTEX BOX, so the kinds below are made by
their vertex boxes, as overlap_shape_cases.shape_boxes makes its boxes; what the triangle inside the box then meets is the
restatement's business.  shape_triangles mixes, from a tree and the corners it is to be asked about (the loaded ones or deformed
ones):

  whole      corners lo and hi of the root's box and a third corner inside it: the vertex box is exactly the root's box, every node
             is entered and the walk holds overlap_shape_cases.deepest_stack(tree) entries; and a wider one
  slab       a sheet of nearly constant y whose vertex box is the x-slab over a run of 1, 9, 65 or about 1,000 consecutive
             triangles, across every seam and at random places: from z below the shape to an apex far above it, so that it is
             nearly as wide as the run where the triangles are; and the same clipped to a part of the z range
  medium     sheets over runs of 10 to 60 and of 70 to 300 triangles (the queries that meet more than 8 and more than 64)
  gap        a sheet strictly between two consecutive triangles in x (n = 0 on the loaded corners), at the seams too
  face       a triangle whose largest x is exactly a node box's lower x-face, or whose smallest x its upper x-face (entered:
             touching counts), and one float short of it (not entered)
  own        the shape's own triangles
  small      small slicers near random surface points
  far        triangles away from everything
  unwalked   a NaN, +inf or -inf coordinate, a point, a segment
"""
import numpy as np

import intersect_ref as IR
from overlap_shape_cases import RUNS, seams

F = np.float32
APEX = 1000.0


def face_triangles(b):
    """three triangles about the node box b [6]: its largest x exactly on the box's lower x-face, its smallest x exactly on the
    upper one (both entered: touching counts), and the first one float short of the face (not entered)"""
    b = np.asarray(b, F)
    return [((b[0] - F(1), b[1], b[2]), (b[0], b[4], b[5]), (b[0] - F(0.5), b[1], b[5])),
            ((b[3], b[1], b[2]), (b[3] + F(1), b[4], b[5]), (b[3] + F(0.5), b[1], b[5])),
            ((b[0] - F(1), b[1], b[2]), (np.nextafter(b[0], F(-np.inf)), b[4], b[5]), (b[0] - F(0.5), b[1], b[5]))]


def shape_triangles(tree, corners, node_boxes, seed, small=350, own=100):
    """about 650 + `small` + `own` query triangles float32 [n, 3, 3] of every kind of the module doc, for `tree` over `corners`
    [T, 3, 3] whose nodes' boxes are `node_boxes` [n, 6]; queries 0 and 1 are the whole query and the wider one, the rest are
    shuffled"""
    rng = np.random.default_rng(seed)
    c = np.asarray(corners, F).reshape(-1, 3, 3)
    n_tri = len(c)
    xlo, xhi = c[:, :, 0].min(1), c[:, :, 0].max(1)
    nb = np.asarray(node_boxes, F).reshape(-1, 6)
    root = nb[0]
    ylo, yhi, zlo, zhi = float(root[1]), float(root[4]), float(root[2]), float(root[5])
    out = []

    def add(a, b, cc):
        out.append((a, b, cc))

    def sheet(x0, x1, clipped):
        """vertex box [x0, x1] in x: the base from (x0, y, z0) to (x1, y', z0), the apex above the middle"""
        y = ylo + (yhi - ylo) * (0.25 + 0.5 * rng.random())
        dy = 0.3 * (rng.random() - 0.5)
        if clipped:
            z0, z1 = np.sort(zlo + (zhi - zlo) * rng.random(2))
        else:
            z0, z1 = zlo - 1.0, APEX
        add((x0, y, z0), (x1, y + dy, z0), (0.5 * (float(x0) + float(x1)), y - dy, z1))

    def slab(first, run, clipped):
        first = int(np.clip(first, 0, max(n_tri - run, 0)))
        last = min(first + run, n_tri)
        sheet(float(xlo[first:last].min()), float(xhi[first:last].max()), clipped)

    add(root[:3], root[3:], (0.5 * (float(root[0]) + float(root[3])), ylo + 0.25 * (yhi - ylo), zlo + 0.75 * (zhi - zlo)))
    add(root[:3] - F(3), root[3:] + F(3), (0.5 * (float(root[0]) + float(root[3])), ylo + 0.25 * (yhi - ylo), zlo + 0.75 * (zhi - zlo)))
    joints = seams(tree)
    for run in RUNS:
        for at in joints:
            for clipped in (False, True):
                slab(at - run // 2 - (run == 1 and clipped), run, clipped)       # across the seam (a run of 1: either side of it)
        for _ in range(12):
            slab(rng.integers(0, n_tri), run, bool(rng.integers(0, 2)))
    for low, high, count in ((10, 61, 130), (70, 301, 140)):
        for _ in range(count):
            slab(rng.integers(0, n_tri), int(rng.integers(low, high)), rng.random() < 0.3)
    between = [t - 1 for t in joints if t > 0] + list(rng.integers(0, max(n_tri - 1, 1), 40))
    for t in between:                                                            # strictly between triangles t and t + 1
        if t + 1 < n_tri and xhi[t] < xlo[t + 1]:
            sheet(np.nextafter(xhi[t], F(np.inf)), np.nextafter(xlo[t + 1], F(-np.inf)), False)
    for k in [0] + list(rng.integers(0, len(nb), 20)):
        for tri in face_triangles(nb[k]):
            add(*tri)
    for t in rng.integers(0, n_tri, own):
        add(*c[t])
    for _ in range(40):
        centre = np.array([xlo.min() - 50, ylo, zlo]) + rng.choice([-1.0, 1.0], 3) * (20 + 500 * rng.random(3))
        add(*(centre + 10 * rng.random((3, 3))))
    t = rng.integers(0, n_tri, small)
    b = rng.random((small, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    v = c[t].astype(np.float64)
    on = v[:, 0] + b[:, :1] * (v[:, 1] - v[:, 0]) + b[:, 1:] * (v[:, 2] - v[:, 0])
    size = np.array([0.3, 1.5, 1.5]) * (0.05 + rng.random((small, 1, 1)) ** 2)
    slicers = on[:, None, :] + rng.normal(size=(small, 3, 3)) * size
    for i in range(small):
        add(*slicers[i])
    for i in range(40):                                                          # not walked
        bad = slicers[i].astype(F).copy()
        if i % 4 == 0:
            bad[1] = bad[2] = bad[0]                                             # a point
        elif i % 4 == 1:
            bad[2] = bad[1]                                                      # a segment
        else:
            bad[i % 3, (i // 3) % 3] = (np.nan, np.inf, -np.inf)[i % 3]
        add(*bad)
    q = np.array(out, np.float64).astype(F)
    order = np.concatenate([[0, 1], 2 + rng.permutation(len(q) - 2)])
    return np.ascontiguousarray(q[order])
