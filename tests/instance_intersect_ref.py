"""Restatement of the instanced triangle-intersection query (include/shader_ray_instance_intersect.h), for the tests.

The header's definition: intersect_ref.intersect, unchanged, on the merged scene whose positions are the mapped corners in
instance order (instance_point_ref.merged_positions), the merged triangle index then split into (instance, triangle of the
member scene) by instance_overlap_ref.split.  The merged scene's ascending index is the header's key (instance, triangle) by
construction.  The instance form's queries are instance q's rows of the merged scene; with SKIP_OWN_INSTANCE instance q's
columns of the membership are cleared.

restated_walk is the kernel's walk in numpy and plain python, one query at a time, over a median-split tree per instance whose
boxes are replaced by their image boxes, with instance_point_ref.stored_box as the top level (a list of its leaves), a scrambled
instance order, and every decision the kernel takes replaceable (the node cull, the image box, the top-level cull and its
guard, the key, the slot the instance skip reads, what n counts, what "own" means, which corners the shared-corner rule
compares), so that tests/test_instance_intersect_reference.py can show which input catches which mistake.  walk_counters is the
counting form's walk of ONE instance over a refit_ref.TreeArrays: intersect_ref.walk_counters on the image boxes and the world
corners, for the queries that the top level lets in.
"""
from __future__ import annotations

import numpy as np

import instance_overlap_ref as IO
import instance_point_ref as IP
import intersect_ref as IR

F = np.float32
COUNTERS = IP.COUNTERS
GUARD = IO.GUARD
SKIP_OWN_INSTANCE = 4        # SHRAY_INTERSECT_SKIP_OWN_INSTANCE

split = IO.split
misses = IO.misses
misses_or_touches = IO.misses_or_touches
guarded_misses = IO.guarded_misses
key_instance_first = IO.key_instance_first
key_triangle_first = IO.key_triangle_first


def vertex_box(queries):
    """(lo, hi), float32 [n, 3] each: min3 / max3 of the corners, as the header's comparisons give them"""
    q = IR.corners_of(queries)
    with np.errstate(invalid="ignore"):
        return IR._min3(q[:, 0], q[:, 1], q[:, 2]), IR._max3(q[:, 0], q[:, 1], q[:, 2])


def membership(scene_positions, scene_of_instance, maps, queries, skip_shared=False):
    """(bool [n queries, merged triangles], each instance's first merged triangle): the header's set S per query"""
    merged, first = IP.merged_positions(scene_positions, scene_of_instance, maps)
    return IR.intersects(queries, merged, skip_shared), first


def from_membership(member, first, k):
    """(int32 triangles [n, k], int32 instances [n, k], int32 counts [n]) of membership()'s result"""
    idx, n = IR.from_set(member, k)
    tri, inst = split(idx, first)
    return tri, inst, n


def intersect_over_instances(scene_positions, scene_of_instance, maps, queries, k, skip_shared=False):
    """The header's answer for the item forms: (int32 triangles [n, k], int32 instances [n, k], int32 counts [n]).
    scene_positions: one vertex_positions array per distinct scene; scene_of_instance: its index for every instance; maps
    [n, 3, 4]; queries: TRIANGLE_DTYPE or [n, 3, 3] / [n, 9] / [n, 12] float32, world space."""
    merged, first = IP.merged_positions(scene_positions, scene_of_instance, maps)
    idx, n = IR.intersect(queries, merged, k, skip_shared)
    tri, inst = split(idx, first)
    return tri, inst, n


def own_queries(scene_positions, scene_of_instance, maps, q, first_triangle=0, count=None):
    """the instance form's queries, float32 [count, 3, 3]: instance q's rows of the merged scene"""
    merged, first = IP.merged_positions(scene_positions, scene_of_instance, maps)
    rows = merged.reshape(-1, 3, 3)[first[q]:first[q + 1]]
    return rows[first_triangle:] if count is None else rows[first_triangle:first_triangle + count]


def own_membership(scene_positions, scene_of_instance, maps, q, skip_shared=False, skip_own=True, first_triangle=0, count=None):
    """membership() of the instance form: with skip_own, no pair of instance q is a member"""
    queries = own_queries(scene_positions, scene_of_instance, maps, q, first_triangle, count)
    member, first = membership(scene_positions, scene_of_instance, maps, queries, skip_shared)
    if skip_own:
        member = member.copy()
        member[:, first[q]:first[q + 1]] = False
    return member, first


def intersect_instance(scene_positions, scene_of_instance, maps, q, k, skip_shared=False, skip_own=True, first_triangle=0, count=None):
    """The header's answer for the instance form (consequence 6)"""
    return from_membership(*own_membership(scene_positions, scene_of_instance, maps, q, skip_shared, skip_own, first_triangle, count), k)


def colliding(scene_positions, scene_of_instance, maps):
    """bool [instances]: instance i has a triangle that intersects a triangle of another instance"""
    return np.array([bool(own_membership(scene_positions, scene_of_instance, maps, q)[0].any()) for q in range(len(maps))])


def same_instance(i, q, scene_of):
    return i == q


def same_scene(i, q, scene_of):
    """a mutant: "own" judged by the scene, not by the instance index"""
    return scene_of[i] == scene_of[q]


def shares_matrix(q, t):
    """bool [Q, T]: some corner of t [T, 3, 3] equals (three ==) some corner of q [Q, 3, 3]"""
    with np.errstate(invalid="ignore"):
        return (q[:, None, :, None, :] == t[None, :, None, :, :]).all(-1).any((-1, -2))


def restated_walk(corners, maps, queries, order, k, counts, *, skip_shared=False, own=None, skip_own=False, scene_of=None,
                  object_queries=None, node_cull=misses, image_box=IP.image_box, top_boxes=None, top_cull=guarded_misses,
                  key=key_instance_first, skip_slot=0, count_kept_only=False, any_only=False, own_is=same_instance,
                  shared_on_object=False, members=None):
    """The kernel's walk, one query at a time: the instances in `order`; an instance that own_is(i, own, scene_of) says is the
    query's own is not walked when skip_own; with `top_boxes` (one (lo, hi) per instance) and more than one instance, an
    instance is entered only when top_cull does not separate its box from the query's vertex box; without counts (and k > 0) a
    query that holds a key in slot k + skip_slot (1-based: the K-th) skips an instance above that key's; in an instance the
    median tree of the object corners, a node entered unless node_cull separates its IMAGE box from the query's vertex box,
    every triangle of an entered leaf mapped and tested by intersect_ref, n counted for every member and the pair's key
    inserted into the sorted K smallest.  `corners` is one [t, 3, 3] array for every instance or a list with one per instance.
    `queries` are world triangles (the instance form passes own_queries' and `own`).  With any_only a query stops at its first
    member (n is 1 or 0).  With shared_on_object the shared-corner rule compares `object_queries` with the object corners (a
    mutant).  The keyword arguments replace one decision each.  `members`: one bool [n, t] per instance, the brute force's
    intersect_ref.intersects(queries, world corners) where the caller holds it already.  Returns (triangles [n, k], instances
    [n, k], counts [n] or None, triangle tests, instance walks)."""
    q = IR.corners_of(queries)
    lo, hi = vertex_box(q)
    n = len(q)
    walk = IR.walked(q)
    prune = not counts and k > 0 and not any_only
    per_instance = isinstance(corners, (list, tuple))
    if scene_of is None:
        scene_of = list(range(len(maps))) if per_instance else [0] * len(maps)
    trees, per = {}, []
    for i in range(len(maps)):
        mine = corners[i] if per_instance else corners
        if id(mine) not in trees:
            trees[id(mine)] = (mine, IP.median_tree(mine))
        tree = trees[id(mine)][1]
        M = np.asarray(maps[i], F)
        ilo, ihi = image_box(M, np.stack([nd[0] for nd in tree]), np.stack([nd[1] for nd in tree]))
        world = IP.map_corners(M, mine).reshape(-1, 3, 3)
        member = IR.intersects(q, world.reshape(-1), False) if members is None else np.asarray(members[i], bool)
        if skip_shared:
            member = member & ~(shares_matrix(np.asarray(object_queries, F).reshape(-1, 3, 3), np.asarray(mine, F)) if shared_on_object
                                else shares_matrix(q, world))
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
            if skip_own and own is not None and own_is(int(i), own, scene_of):
                continue
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


def walk_counters(tree, node_boxes, corners, M, queries, top_box=None, skip_shared=False, any_only=False):
    """The counting form's walk of ONE instance, over a refit_ref.TreeArrays `tree` (pre-order) whose nodes' boxes are
    `node_boxes` float32 [n, 6] (what octant copy 7 of the packed tree holds) and whose triangles are the object `corners`
    [T, 3, 3] in the tree's order.  A walked query enters the instance unless guarded_misses separates `top_box` (lo, hi: the
    box the top level stores for it; None: a set of one instance, which never culls) from its vertex box.  Then
    intersect_ref.walk_counters on the nodes' IMAGE boxes and the mapped corners.  Returns a dict of int64 [n queries]:
    node_visits, leaf_visits, triangle_tests, traversals (1 where the instance is walked) and `members` (the instance's pairs
    of the query, counted over every query)."""
    M = np.asarray(M, F).reshape(3, 4)
    nb = np.asarray(node_boxes, F).reshape(-1, 6)
    q = IR.corners_of(queries)
    lo, hi = vertex_box(q)
    go = IR.walked(q)
    if top_box is not None:
        slo, shi = np.asarray(top_box[0], F), np.asarray(top_box[1], F)
        go = go & ~guarded_misses(slo[None], shi[None], lo, hi)
    ilo, ihi = IP.image_box(M, nb[:, :3], nb[:, 3:])
    world = IP.map_corners(M, corners).reshape(-1, 3, 3)
    member = IR.intersects(q, world.reshape(-1), skip_shared)
    rows = np.nonzero(go)[0]
    w = IR.walk_counters(tree, np.concatenate([ilo, ihi], axis=1), world, np.ascontiguousarray(q[rows]), skip_shared=skip_shared,
                         any_only=any_only, member=member[rows])
    out = {name: np.zeros(len(q), np.int64) for name in COUNTERS}
    for name in IR.COUNTERS:
        out[name][rows] = w[name]
    out["traversals"][rows] = 1
    out["members"] = member.sum(1).astype(np.int64)
    return out
