"""The boxes of the box-overlap tests over the hand-shaped trees of tests/tree_shapes.py (tests/test_overlap_reference.py on the
CPU, tests/test_gpu_overlap_tree_shapes.py on the GPU).  No test and no GPU in here.

overlap_cases.make_boxes sizes its heavy kinds by the nearest centroids of every triangle, too much for 32k triangles.  A
shape's triangles lie along x in leaf order, one per 0.2, so a run of consecutive triangles is an x-slab and a seam of the tree
(where a branch's two subtrees meet: P(11) and P(1) in wide_by_one, every spine joint of lopsided and mixed_spine, the
splits down either flank of a perfect tree) is a triangle index.  shape_boxes mixes, from a tree and the corners it is to be asked
about (the loaded ones or deformed ones: a run is then the slab over those triangles' x, whatever else has moved into it):

  whole      the root's box exactly (every face on a node box's face) and a wider one: the walk holds one entry a level
  slab       x-slabs over runs of 1, 9, 65 and about 1,000 consecutive triangles, across every seam and at random places, open
             in y and z, and clipped to a part of the y and z range
  medium     slabs over runs of 10 to 60 and of 70 to 300 triangles (the boxes that hold more than 8 and more than 64)
  inside     a slab strictly inside one triangle's x-range
  gap        a slab strictly between two consecutive triangles (n = 0 on the loaded corners), at the seams too
  vertex     zero-extent boxes at vertices
  face       a box whose upper or lower x-face is exactly a node box's lower or upper x-face (entered: touching counts), and
             one float beyond it (not entered)
  far        boxes away from everything
  small      boxes near random surface points
  unwalked   inverted, NaN and infinite boxes
"""
import numpy as np

import overlap_ref as OR

F = np.float32
RUNS = (1, 9, 65, 1000)
OPEN = (-1000.0, 1000.0)


def seams(tree) -> list:
    """the triangle indices where the two subtrees of a branch meet, for every branch on the path from the root through positive
    children (the spine of lopsided and mixed_spine, then the perfect subtree's own) and on the path through negative ones"""
    first = np.zeros(tree.node_count, np.int64)        # a node's first triangle
    for k in range(tree.node_count - 1, -1, -1):
        first[k] = tree.start[k] if tree.negative[k] < 0 else first[tree.negative[k]]
    out = set()
    for side in (tree.positive, tree.negative):
        k = 0
        while tree.negative[k] >= 0:
            out.add(int(first[tree.positive[k]]))
            k = side[k]
    return sorted(out)


def deepest_stack(tree) -> int:
    """the most stack entries any walk of the tree can hold: an entry is held for every branch on the path whose negative child
    the path takes (the positive one waits), so the greatest number of negative turns down to a branch, that branch's included"""
    turns = np.zeros(tree.node_count, np.int64)
    best = 0
    for k in range(tree.node_count):                   # pre-order: a parent comes before its children
        if tree.negative[k] >= 0:
            best = max(best, int(turns[k]) + 1)
            turns[tree.negative[k]] = turns[k] + 1
            turns[tree.positive[k]] = turns[k]
    return best


def shape_boxes(tree, corners, node_boxes, seed, small=400):
    """about 600 + `small` BOX_DTYPE boxes of every kind of the module doc, for `tree` over `corners` [T, 3, 3] whose nodes' boxes
    are `node_boxes` [n, 6]"""
    rng = np.random.default_rng(seed)
    c = np.asarray(corners, F).reshape(-1, 3, 3)
    n_tri = len(c)
    xlo, xhi = c[:, :, 0].min(1), c[:, :, 0].max(1)
    root = np.asarray(node_boxes, F)[0]
    ylo, yhi, zlo, zhi = float(root[1]), float(root[4]), float(root[2]), float(root[5])
    lo, hi = [], []

    def add(l, h):
        lo.append(l)
        hi.append(h)

    def slab(first, run, clipped):
        first = int(np.clip(first, 0, max(n_tri - run, 0)))
        last = min(first + run, n_tri)
        x0, x1 = float(xlo[first:last].min()), float(xhi[first:last].max())
        if clipped:
            ys, zs = np.sort(ylo + (yhi - ylo) * rng.random(2)), np.sort(zlo + (zhi - zlo) * rng.random(2))
            add((x0, ys[0], zs[0]), (x1, ys[1], zs[1]))
        else:
            add((x0,) + OPEN[:1] * 2, (x1,) + OPEN[1:] * 2)

    add(root[:3], root[3:])
    add(root[:3] - F(3), root[3:] + F(3))
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
    for t in rng.integers(0, n_tri, 30):                                         # inside one triangle's x-range
        w = float(xhi[t] - xlo[t])
        add((float(xlo[t]) + 0.3 * w,) + OPEN[:1] * 2, (float(xlo[t]) + 0.6 * w,) + OPEN[1:] * 2)
    between = [t - 1 for t in joints if t > 0] + list(rng.integers(0, max(n_tri - 1, 1), 40))
    for t in between:                                                            # strictly between triangles t and t + 1
        if t + 1 < n_tri and xhi[t] < xlo[t + 1]:
            add((np.nextafter(xhi[t], F(np.inf)),) + OPEN[:1] * 2, (np.nextafter(xlo[t + 1], F(-np.inf)),) + OPEN[1:] * 2)
    verts = c.reshape(-1, 3)
    for v in verts[rng.integers(0, len(verts), 50)]:
        add(v, v)
    nb = np.asarray(node_boxes, F).reshape(-1, 6)
    for k in rng.integers(0, len(nb), 20):
        b = nb[k]
        add((b[0] - F(1), b[1], b[2]), (b[0], b[4], b[5]))                                       # its upper x-face on the node's lower one
        add((b[3], b[1], b[2]), (b[3] + F(1), b[4], b[5]))                                       # its lower x-face on the node's upper one
        add((b[0] - F(1), b[1], b[2]), (np.nextafter(b[0], F(-np.inf)), b[4], b[5]))             # one float short of it
    for _ in range(40):
        centre = np.array([xlo.min() - 50, ylo, zlo]) + rng.choice([-1.0, 1.0], 3) * (20 + 500 * rng.random(3))
        half = 10 * rng.random(3)
        add(centre - half, centre + half)
    t = rng.integers(0, n_tri, small)
    b = rng.random((small, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    v = c[t].astype(np.float64)
    on = v[:, 0] + b[:, :1] * (v[:, 1] - v[:, 0]) + b[:, 1:] * (v[:, 2] - v[:, 0])
    half = np.array([0.3, 1.5, 1.5]) * rng.random((small, 3)) ** 2
    centre = on + rng.normal(size=(small, 3)) * half
    for i in range(small):
        add(centre[i] - half[i], centre[i] + half[i])
    for i in range(40):                                                          # not walked
        l, h = (centre[i] - half[i]).astype(F), (centre[i] + half[i]).astype(F)
        axis = i % 3
        if i % 4 == 0:
            l[axis], h[axis] = h[axis] + F(1), l[axis]
        elif i % 2:
            l[axis] = (np.nan, -np.inf)[i % 4 == 1]
        else:
            h[axis] = (np.nan, np.inf)[i % 8 == 2]
        add(l, h)
    boxes = OR.make_boxes(np.array(lo, F), np.array(hi, F))
    return boxes[rng.permutation(len(boxes))]
