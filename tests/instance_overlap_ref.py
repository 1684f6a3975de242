"""Restatement of the instanced box-overlap query (include/shader_ray_instance_overlap.h), for the tests.

The header's definition: overlap_ref.overlap, unchanged, on the merged scene whose positions are the mapped corners in instance
order (instance_point_ref.merged_positions), the merged triangle index then split into (instance, triangle of the member
scene).  The merged scene's ascending index is the header's key (instance, triangle) by construction.

restated_walk is the kernel's walk in numpy and plain python, one box at a time, over a median-split tree per instance whose
boxes are replaced by their image boxes, with instance_point_ref.stored_box as the top level (a list of its leaves), a scrambled
instance order, and every decision the kernel takes replaceable (the node cull, the image box, the top-level cull and its
guard, the key, the slot the instance skip reads, what n counts), so that tests/test_instance_overlap_reference.py can show
which input catches which mistake.  walk_counters is the counting form's walk of ONE instance over a refit_ref.TreeArrays:
overlap_ref.walk_counters on the image boxes and the world corners, for the boxes that the top level lets in.
"""
from __future__ import annotations

import numpy as np

import instance_point_ref as IP
import overlap_ref as OR

F = np.float32
COUNTERS = IP.COUNTERS
GUARD = F(2.0 ** -109)      # the kernel's kGuard


def split(indices, first):
    """the merged scene's indices as (the member's own triangle indices, instances), -1 where there is none"""
    t = np.asarray(indices, np.int64)
    inst = np.where(t >= 0, np.searchsorted(first, t, side="right") - 1, -1)
    return np.where(t >= 0, t - first[np.maximum(inst, 0)], -1).astype(np.int32), inst.astype(np.int32)


def membership(scene_positions, scene_of_instance, maps, boxes):
    """(bool [n boxes, merged triangles], each instance's first merged triangle): the header's set S per box"""
    merged, first = IP.merged_positions(scene_positions, scene_of_instance, maps)
    return OR.overlaps(merged, boxes), first


def from_membership(member, first, k):
    """(int32 triangles [n, k], int32 instances [n, k], int32 counts [n]) of membership()'s result"""
    idx, n = OR.from_set(member, k)
    tri, inst = split(idx, first)
    return tri, inst, n


def overlap_over_instances(scene_positions, scene_of_instance, maps, boxes, k):
    """The header's answer: (int32 triangles [n, k], int32 instances [n, k], int32 counts [n]).  scene_positions: one
    vertex_positions array per distinct scene; scene_of_instance: its index for every instance; maps [n, 3, 4]; boxes: BOX_DTYPE
    or [n, 6] / [n, 8] float32."""
    merged, first = IP.merged_positions(scene_positions, scene_of_instance, maps)
    idx, n = OR.overlap(merged, boxes, k)
    tri, inst = split(idx, first)
    return tri, inst, n


def misses(node_lo, node_hi, lo, hi):
    """the kernel's node cull: some axis has node.hi < lo or node.lo > hi (false for a NaN on either side); boxes [..., 3] that
    broadcast against each other, bool [...]"""
    with np.errstate(invalid="ignore"):
        return ((node_hi < lo) | (node_lo > hi)).any(-1)


def misses_or_touches(node_lo, node_hi, lo, hi):
    """a mutant: <= in the node cull (a box that only touches is skipped)"""
    with np.errstate(invalid="ignore"):
        return ((node_hi <= lo) | (node_lo >= hi)).any(-1)


def guarded_misses(stored_lo, stored_hi, lo, hi, guard=GUARD):
    """the kernel's top-level cull: an axis separates only when the stored float and the query float it is compared with are
    not both below the guard in magnitude"""
    with np.errstate(invalid="ignore"):
        below = (stored_hi < lo) & ~((np.abs(stored_hi) < guard) & (np.abs(lo) < guard))
        above = (stored_lo > hi) & ~((np.abs(stored_lo) < guard) & (np.abs(hi) < guard))
        return (below | above).any(-1)


def key_instance_first(i, t):
    return (i, t)


def key_triangle_first(i, t):
    return (t, i)


def restated_walk(corners, maps, boxes, order, k, counts, *, node_cull=misses, image_box=IP.image_box, top_boxes=None,
                  top_cull=guarded_misses, key=key_instance_first, skip_slot=0, count_kept_only=False, any_only=False):
    """The kernel's walk, one box at a time: the instances in `order`; with `top_boxes` (one (lo, hi) per instance) and more
    than one instance, an instance is entered only when top_cull does not separate its box from the query box; without counts
    (and k > 0) a box that holds a key in slot k + skip_slot (1-based: the K-th) skips an instance above that key's; in an
    instance the median tree of the object corners, a node entered unless node_cull separates its IMAGE box from the query box,
    every triangle of an entered leaf mapped and tested by overlap_ref, n counted for every touching pair and the pair's key
    inserted into the sorted K smallest.  `corners` is one [t, 3, 3] array for every instance or a list with one per instance.
    With any_only a box stops at its first touching pair (n is 1 or 0).  The keyword arguments replace one decision each (the
    tests' mutants).  Returns (triangles [n, k], instances [n, k], counts [n] or None, triangle tests, instance walks)."""
    lo, hi = OR.lo_hi(boxes)
    lo, hi = np.ascontiguousarray(lo, F), np.ascontiguousarray(hi, F)
    n = len(lo)
    walk = OR.walked(boxes)
    prune = not counts and k > 0 and not any_only
    per_instance = isinstance(corners, (list, tuple))
    trees, per = {}, []
    for i in range(len(maps)):
        own = corners[i] if per_instance else corners
        if id(own) not in trees:
            trees[id(own)] = (own, IP.median_tree(own))
        tree = trees[id(own)][1]
        M = np.asarray(maps[i], F)
        ilo, ihi = image_box(M, np.stack([nd[0] for nd in tree]), np.stack([nd[1] for nd in tree]))
        member = OR.overlaps(IP.map_corners(M, own).reshape(-1), boxes)
        culled = np.asarray(node_cull(ilo[None], ihi[None], lo[:, None], hi[:, None]))
        out = None
        if top_boxes is not None and len(maps) > 1:
            out = np.asarray(top_cull(np.asarray(top_boxes[i][0], F)[None], np.asarray(top_boxes[i][1], F)[None], lo, hi))
        per.append((tree, culled, out, member))
    triangles, instances = np.full((n, k), -1, np.int32), np.full((n, k), -1, np.int32)
    found = np.zeros(n, np.int32)
    tests = walks = 0
    for j in range(n):
        if not walk[j]:
            continue
        held = []   # sorted keys, at most k
        members = 0
        for i in order:
            if any_only and members:
                break
            tree, culled, out, member = per[i]
            if out is not None and out[j]:
                continue
            cull = culled[j]
            slot = k - 1 + skip_slot
            if prune and 0 <= slot < len(held) and int(i) > (held[slot][0] if key is key_instance_first else held[slot][1]):
                continue
            walks += 1
            stack = [] if cull[0] else [0]
            while stack and not (any_only and members):
                at = stack.pop()
                _, _, left, right, ids = tree[at]
                if ids is None:
                    for child in (right, left):
                        if not cull[child]:
                            stack.append(child)
                    continue
                for t in ids:
                    tests += 1
                    if not member[j, t]:
                        continue
                    kk = key(int(i), int(t))
                    kept = k > 0 and (len(held) < k or kk < held[-1])
                    if kept or not count_kept_only:
                        members += 1
                    if any_only:
                        break
                    if kept:
                        held.append(kk)
                        held.sort()
                        del held[k:]
        found[j] = members
        for s, kk in enumerate(held):
            instances[j, s], triangles[j, s] = kk if key is key_instance_first else (kk[1], kk[0])
    return triangles, instances, (found if counts or any_only else None), tests, walks


def walk_counters(tree, node_boxes, corners, M, boxes, top_box=None, any_only=False):
    """The counting form's walk of ONE instance, over a refit_ref.TreeArrays `tree` (pre-order) whose nodes' boxes are
    `node_boxes` float32 [n, 6] (what octant copy 7 of the packed tree holds) and whose triangles are the object `corners`
    [T, 3, 3] in the tree's order.  A walked box enters the instance unless guarded_misses separates `top_box` (lo, hi: the box
    the top level stores for it; None: a set of one instance, which never culls) from it.  Then overlap_ref.walk_counters on the
    nodes' IMAGE boxes and the mapped corners.  Returns a dict of int64 [n boxes]: node_visits, leaf_visits, triangle_tests,
    traversals (1 where the instance is walked) and `touching` (the instance's pairs in the box, counted over every box)."""
    M = np.asarray(M, F).reshape(3, 4)
    nb = np.asarray(node_boxes, F).reshape(-1, 6)
    lo, hi = OR.lo_hi(boxes)
    go = OR.walked(boxes)
    if top_box is not None:
        slo, shi = np.asarray(top_box[0], F), np.asarray(top_box[1], F)
        go = go & ~guarded_misses(slo[None], shi[None], lo, hi)
    ilo, ihi = IP.image_box(M, nb[:, :3], nb[:, 3:])
    world = IP.map_corners(M, corners).reshape(-1, 3, 3)
    member = OR.overlaps(world.reshape(-1), boxes)
    rows = np.nonzero(go)[0]
    picked = np.ascontiguousarray(np.asarray(boxes)[rows])
    w = OR.walk_counters(tree, np.concatenate([ilo, ihi], axis=1), world, picked, any_only=any_only, member=member[rows])
    out = {name: np.zeros(len(lo), np.int64) for name in COUNTERS}
    for name in OR.COUNTERS:
        out[name][rows] = w[name]
    out["traversals"][rows] = 1
    out["touching"] = member.sum(1).astype(np.int64)
    return out
