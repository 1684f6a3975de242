"""Restatement of the instanced within-radius query (include/shader_ray_instance_near.h), for the tests.

The header's definition: near_ref.near, unchanged, on the merged scene whose positions are the mapped corners in instance
order (instance_point_ref.merged_positions), the merged triangle index then split into (instance, triangle of the member
scene) by instance_point_ref.split_index.  The merged scene's key (dist2, merged index) is the header's (dist2, instance,
triangle) by construction.

restated_walk is the kernel's walk in numpy and plain python, one point at a time, over a median-split tree per instance, with
every decision the kernel takes replaceable (the two skips, the tie rule, the slot the reach is read from, what n counts, the
membership test against max_dist2), so that tests/test_instance_near_reference.py and
tests/test_instance_near_scale_reference.py can show which input catches which mistake.  walk_counters is the counting form's
walk of ONE instance, one point at a time, over a refit_ref.TreeArrays: its node visits, leaf visits and triangle tests, and
whether the point walks the instance at all (the top level's stored box, when one is given).
"""
from __future__ import annotations

import numpy as np

import instance_point_ref as IP
import near_ref as NR
import point_query_ref as R

F = np.float32
COUNTERS = IP.COUNTERS


def near_over_instances(scene_positions, scene_of_instance, maps, points, k, device=None):
    """The header's answer: (CLOSEST_DTYPE records [n, k], int32 instances [n, k], int32 counts [n]).  scene_positions: one
    vertex_positions array per distinct scene; scene_of_instance: its index for every instance; maps [n, 3, 4]; points:
    POINT_DTYPE or [n, 4] float32.  With `device` the pairs' dist2 are computed through near_ref.near_torch there."""
    merged, first = IP.merged_positions(scene_positions, scene_of_instance, maps)
    records, counts = NR.near(merged, points, k) if device is None else NR.near_torch(merged, points, k, device=device)
    flat, inst = IP.split_index(records.reshape(-1), first)
    return flat.reshape(records.shape), inst.reshape(records.shape), counts


def above(lb, reach):
    """the kernel's skip: the bound is strictly above the reach (false for a NaN on either side)"""
    return lb > reach


def key_instance_first(d, i, t):
    return (d, i, t)


def at_or_under(d, max_dist2):
    """the kernel's membership: dist2 <= max_dist2, inclusive (false for a NaN on either side)"""
    return d <= max_dist2


def prepare(corners, maps, points, top_boxes=None):
    """what restated_walk needs per instance, for all points at once: (median tree of the object corners, image-box bounds
    [n, nodes], dist2 of every pair [n, T], world corners, top-level box bounds [n] or None)"""
    per_instance = isinstance(corners, (list, tuple))
    trees = {}
    pts = NR.as_points(points)
    n = len(pts)
    p = np.ascontiguousarray(pts["p"])
    per = []
    for i in range(len(maps)):
        own = corners[i] if per_instance else corners
        if id(own) not in trees:
            trees[id(own)] = (own, IP.median_tree(own))
        tree = trees[id(own)][1]
        M = np.asarray(maps[i], F)
        lo, hi = np.stack([nd[0] for nd in tree]), np.stack([nd[1] for nd in tree])
        ilo, ihi = IP.image_box(M, lo, hi)
        with np.errstate(all="ignore"):
            lbs = IP.bound(p[:, None, :], ilo[None], ihi[None])
            world = IP.map_corners(M, own).reshape(-1, 3, 3)
            d2 = IP.pair_dist2(p, world)[1]
            top = None if top_boxes is None else IP.bound(p, np.asarray(top_boxes[i][0], F), np.asarray(top_boxes[i][1], F))
        per.append((tree, np.asarray(lbs).tolist(), np.broadcast_to(d2, (n, len(world))), world, top))
    return per


def restated_walk(corners, maps, points, order, k, counts, *, node_skip=above, top_boxes=None, top_skip=above,
                  key=key_instance_first, reach_slot=-1, count_kept_only=False, within=at_or_under, prepared=None):
    """The kernel's walk, one point at a time: the instances in `order`; with `top_boxes` (one (lo, hi) per instance: the top
    level as a list of its leaves) an instance is entered only when the bound of its box is not above the point's reach; in an
    instance the median tree of the object corners, a node skipped only when the bound of its IMAGE box is above the reach,
    the nearer child first, every triangle of a visited leaf mapped and tested, n counted for every pair `within` max_dist2 and
    the pair's key inserted into the sorted K best.  The reach is max_dist2 with `counts` (or k == 0), else the dist2 of the
    held slot k + reach_slot (0-based: the K-th smallest), max_dist2 while that slot is empty.  `corners` is one [t, 3, 3]
    array for every instance or a list with one per instance.  The keyword arguments replace one decision each (the tests'
    mutants); `prepared` is prepare()'s result for the same corners, maps, points and top boxes, to share it between calls.
    Returns (records [n, k], instances [n, k], counts [n] or None, triangle tests)."""
    pts = NR.as_points(points)
    n = len(pts)
    p = np.ascontiguousarray(pts["p"])
    md = pts["max_dist2"]
    walk = NR.walked(pts)
    prune = not counts and k > 0
    per = prepared if prepared is not None else prepare(corners, maps, pts, top_boxes)
    records = np.zeros((n, k), R.CLOSEST_DTYPE)
    records["q"], records["dist2"] = p[:, None, :], md[:, None]
    records["triangle"], records["region"] = R.HIT_MISS, R.REGION_NONE
    instances = np.full((n, k), -1, np.int32)
    found = np.zeros(n, np.int32)
    tests = 0
    for j in range(n):
        if not walk[j]:
            continue
        held = []   # sorted keys, at most k
        mdj = md[j]
        reach = mdj
        members = 0
        for i in order:
            tree, lbs, d2, _, top = per[i]
            if top is not None and len(maps) > 1 and top_skip(top[j], reach):
                continue
            lb = lbs[j]
            stack = [] if node_skip(lb[0], reach) else [0]
            while stack:
                at = stack.pop()
                if prune and node_skip(lb[at], reach):   # the reach has dropped below it since the push
                    continue
                _, _, left, right, ids = tree[at]
                if ids is None:
                    near, far = (right, left) if lb[right] < lb[left] else (left, right)
                    if node_skip(lb[near], reach):
                        continue
                    if not node_skip(lb[far], reach):
                        stack.append(far)
                    stack.append(near)
                    continue
                for t in ids:
                    tests += 1
                    d = d2[j, t]
                    if not within(d, mdj):
                        continue
                    kk = key(d, int(i), int(t))
                    kept = k > 0 and (len(held) < k or kk < held[-1])
                    if kept or not count_kept_only:
                        members += 1
                    if kept:
                        held.append(kk)
                        held.sort()
                        del held[k:]
                        if prune:
                            slot = k + reach_slot
                            reach = held[slot][0] if 0 <= slot < len(held) else mdj
        found[j] = members
        for s, kk in enumerate(held):
            i, t = (kk[1], kk[2]) if key is key_instance_first else (kk[2], kk[1])
            q, d, u, v, region = IP.pair_dist2(p[j:j + 1], per[i][3][t:t + 1])
            records[j, s] = (tuple(np.ravel(c)[0] for c in q), np.ravel(d)[0], np.ravel(u)[0], np.ravel(v)[0], t, np.ravel(region)[0])
            instances[j, s] = i
    return records, instances, (found if counts else None), tests


def walk_counters(tree, node_boxes, corners, M, points, top_box=None, device=None):
    """The counting form's walk of ONE instance, one point at a time in plain python, over a refit_ref.TreeArrays `tree`
    (pre-order) whose nodes' boxes are `node_boxes` float32 [n, 6] (what octant copy 7 of the packed tree holds) and whose
    triangles are the object `corners` [T, 3, 3] in the tree's order.  A walked point enters the instance unless the bound of
    `top_box` (lo, hi: the box the top level stores for it; None: a set of one instance, which never culls) is above its
    max_dist2.  Then the root's image bound is counted and tested; both children of an entered branch are counted; the child
    with the smaller bound is entered first and the other kept if its bound is not above max_dist2 (the reach never drops, so
    a kept node is always entered); every triangle of an entered leaf is tested.  Returns a dict of int64 [n points]:
    node_visits, leaf_visits, triangle_tests, traversals (1 where the instance is walked) and `near` (pairs within
    max_dist2).  With `device` the pairs' dist2 are computed there (point_query_ref.TorchOps: the same bits)."""
    M = np.asarray(M, F).reshape(3, 4)
    nb = np.asarray(node_boxes, F).reshape(-1, 6)
    pts = NR.as_points(points)
    p = np.ascontiguousarray(pts["p"])
    md = pts["max_dist2"]
    n = len(p)
    go = NR.walked(pts)
    if top_box is not None:
        with np.errstate(all="ignore"):
            go = go & ~(IP.bound(p, np.asarray(top_box[0], F), np.asarray(top_box[1], F)) > md)
    ilo, ihi = IP.image_box(M, nb[:, :3], nb[:, 3:])
    world = IP.map_corners(M, corners).reshape(-1, 3, 3)
    lbs = np.empty((n, len(nb)), F)
    d2s = np.empty((n, len(world)), F)
    ops = IP.O if device is None else R.TorchOps(device)
    chunk = max(1, (1 << 21) // max(1, len(world)))
    for s in range(0, n, chunk):
        lbs[s:s + chunk] = IP.bound(p[s:s + chunk, None, :], ilo[None], ihi[None])
        d = IP.pair_dist2(p[s:s + chunk], world, ops)[1]
        d2s[s:s + chunk] = d if device is None else d.cpu().numpy()
    negative, positive = tree.negative.tolist(), tree.positive.tolist()
    start, count = tree.start.tolist(), tree.triangles.tolist()
    out = {name: np.zeros(n, np.int64) for name in COUNTERS}
    out["near"] = np.zeros(n, np.int64)
    for j in range(n):
        if not go[j]:
            continue
        lb, d2, reach = lbs[j].tolist(), d2s[j], float(md[j])
        nodes, leaves, tests, near = 1, 0, 0, 0
        stack = [] if lb[0] > reach else [0]
        while stack:
            cur = stack.pop()
            if negative[cur] < 0:
                leaves += 1
                tests += count[cur]
                near += int((d2[start[cur]:start[cur] + count[cur]] <= md[j]).sum())
                continue
            nodes += 2
            n0, n1 = negative[cur], positive[cur]
            nr, fr = (n1, n0) if lb[n1] < lb[n0] else (n0, n1)
            if not lb[nr] > reach:
                if not lb[fr] > reach:
                    stack.append(fr)
                stack.append(nr)
        out["node_visits"][j], out["leaf_visits"][j], out["triangle_tests"][j], out["traversals"][j] = nodes, leaves, tests, 1
        out["near"][j] = near
    return out
