"""CPU restatement of the instance set's top-level build (include/shader_ray_instance.h), in the two forms the library has.

- median_build: the host update's recursion.  A node over ids splits on the axis of the longest centroid extent (the lowest
  axis on a tie) at the object median, the first count // 2 ids in (centre[axis], id) order going left, -0 equal to +0.  Its
  children are allocated side by side, in pre-order: a node's pair is at the end of the array when the node is visited.
- presorted_build: the device update's level-by-level form.  The ids are sorted once per axis by (centre, id); at each level
  every segment that still holds two or more ids picks its axis from its first and last entries in each list, flags the first
  half of its chosen list, and stable-partitions all three lists by those flags, with positions from one exclusive scan.  Node
  positions come from the counts alone: the root is node 0 with its pair at 1, a left child's pair follows its parent's
  (pair + 2), and a right child's follows the left subtree (pair + 2 * (count // 2)).

Both return, per node, ("leaf", id) or ("branch", axis, pair).
"""
from __future__ import annotations

import numpy as np


def _order(centres, ids, axis):
    key = np.asarray(centres, np.float64)[ids, axis] + 0.0          # -0 sorts with +0
    return ids[np.lexsort((ids, key))]


def median_build(centres) -> list:
    centres = np.asarray(centres, np.float64)
    n = len(centres)
    nodes = [None]

    def build(ids, at):
        if len(ids) == 1:
            nodes[at] = ("leaf", int(ids[0]))
            return
        c = centres[ids]
        extent = c.max(0) - c.min(0)
        axis = 0
        for a in (1, 2):
            if extent[a] > extent[axis]:
                axis = a
        ordered = _order(centres, ids, axis)
        half = len(ids) // 2
        pair = len(nodes)
        nodes.extend([None, None])
        nodes[at] = ("branch", axis, pair)
        build(ordered[:half], pair)
        build(ordered[half:], pair + 1)

    build(np.arange(n), 0)
    return nodes


def segment_at(p: int, n: int, depth: int):
    """(first, count, node, pair) of the segment holding sorted position p after `depth` levels"""
    first, count, node, pair = 0, n, 0, 1
    for _ in range(depth):
        if count < 2:
            break
        half = count // 2
        if p < first + half:
            first, count, node, pair = first, half, pair, pair + 2
        else:
            first, count, node, pair = first + half, count - half, pair + 1, pair + 2 * half
    return first, count, node, pair


def presorted_build(centres) -> list:
    centres = np.asarray(centres, np.float64)
    n = len(centres)
    ids = np.arange(n)
    lists = [_order(centres, ids, c) for c in range(3)]
    nodes = [None] * (2 * n - 1)
    depth = 0
    while (1 << depth) < n:
        depth += 1
    for d in range(depth):
        segs = [segment_at(p, n, d) for p in range(n)]
        left_of = np.zeros(n, np.uint32)
        for p, (first, count, node, pair) in enumerate(segs):       # iu_split
            if count < 2:
                continue
            last = first + count - 1
            extent = [centres[lists[c][last], c] - centres[lists[c][first], c] for c in range(3)]
            axis = 0
            for a in (1, 2):
                if extent[a] > extent[axis]:
                    axis = a
            left_of[lists[axis][p]] = 1 if p - first < count // 2 else 0
            if p == first:
                nodes[node] = ("branch", axis, pair)
        splits = np.array([s[1] >= 2 for s in segs])
        flags = np.concatenate([np.where(splits, left_of[lists[c]], 0) for c in range(3)]).astype(np.int64)   # iu_flags
        offsets = np.concatenate([[0], np.cumsum(flags)[:-1]])                               # the exclusive scan
        out = [np.empty(n, np.int64) for _ in range(3)]
        for c in range(3):                                                                   # iu_scatter
            for p, (first, count, _, _) in enumerate(segs):
                at = c * n
                if count < 2:
                    out[c][p] = lists[c][p]
                    continue
                before = offsets[at + p] - offsets[at + first]
                q = first + before if flags[at + p] else first + count // 2 + (p - first - before)
                out[c][q] = lists[c][p]
        lists = out
    assert all(np.array_equal(lists[0], lists[c]) for c in (1, 2))
    for p in range(n):                                                                       # iu_leaves
        nodes[segment_at(p, n, depth)[2]] = ("leaf", int(lists[0][p]))
    return nodes
