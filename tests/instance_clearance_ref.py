"""Restatement of the instanced triangle-distance query (include/shader_ray_instance_clearance.h), for the tests.

The header's definition: clearance_ref.clearance, unchanged, on the merged scene whose positions are the mapped corners in
instance order (instance_point_ref.merged_positions), the merged triangle index then split into (instance, triangle of the
member scene) by instance_overlap_ref.split.  The merged scene's key (dist2, merged index) is the header's (dist2, instance,
triangle) by construction.  The instance form's queries are instance q's rows of the merged scene; with SKIP_OWN_INSTANCE
instance q's columns of the pair table are no members.

restated_walk is the kernel's walk in numpy and plain python, one query at a time, over a median-split tree per instance whose
boxes are replaced by their image boxes, with instance_point_ref.stored_box as the top level (a list of its leaves), a
scrambled instance order, and every decision the kernel takes replaceable (the two skips, the tie rule, the slot the reach is
read from, what n counts, what "own" means, which corners the shared-corner rule compares), so that
tests/test_instance_clearance_reference.py can show which input catches which mistake.  walk_counters is the counting form's
walk of ONE instance, one query at a time, over a refit_ref.TreeArrays.
"""
from __future__ import annotations

import numpy as np

import clearance_ref as CR
import instance_overlap_ref as IO
import instance_point_ref as IP
import intersect_ref as IR
import point_query_ref as R

F = np.float32
COUNTERS = IP.COUNTERS
SKIP_OWN_INSTANCE = 4        # SHRAY_CLEARANCE_SKIP_OWN_INSTANCE
PAIR_DISTANCE_DTYPE = CR.PAIR_DISTANCE_DTYPE

split = IO.split


def split_records(records, first):
    """the merged scene's records as (records with the member's own triangle index, int32 instances of the same shape)"""
    out = records.copy()
    tri, inst = split(records["triangle"], first)
    out["triangle"] = tri
    return out, inst


def merged_table(scene_positions, scene_of_instance, maps, queries, o=R.NumpyOps, pairs=1 << 18):
    """(merged positions, each instance's first merged triangle, dist2 [n, T], shared [n, T]) of a query set: the brute force's
    pair table, to be computed once and shared"""
    merged, first = IP.merged_positions(scene_positions, scene_of_instance, maps)
    d2, _ = CR.pair_table(o, queries, merged, pairs=pairs)
    d2.setflags(write=False)
    return merged, first, d2, CR.shared_table(queries, merged)


def from_merged_table(table, queries, k, max_dist2=np.inf, skip_shared=False, without=None):
    """The header's answer from merged_table()'s result: (records [n, k], int32 instances [n, k], int32 counts [n]).
    `without`: an instance whose pairs are no members (the instance form's SKIP_OWN_INSTANCE)."""
    merged, first, d2, shared = table
    if without is not None:
        d2 = d2.copy()
        d2[:, first[without]:first[without + 1]] = np.nan   # (a NaN is within no max_dist2)
    records, counts = CR.from_table(queries, merged, d2, shared, k, max_dist2, skip_shared)
    out, inst = split_records(records, first)
    return out, inst, counts


def clearance_over_instances(scene_positions, scene_of_instance, maps, queries, k, max_dist2=np.inf, skip_shared=False, o=R.NumpyOps):
    """The header's answer for the item forms: (PAIR_DISTANCE_DTYPE records [n, k], int32 instances [n, k], int32 counts [n]).
    scene_positions: one vertex_positions array per distinct scene; scene_of_instance: its index for every instance; maps
    [n, 3, 4]; queries: anything intersect_ref.corners_of takes, world space."""
    merged, first = IP.merged_positions(scene_positions, scene_of_instance, maps)
    records, counts = CR.clearance(merged, queries, k, max_dist2, skip_shared, o)
    out, inst = split_records(records, first)
    return out, inst, counts


def own_queries(scene_positions, scene_of_instance, maps, q, first_triangle=0, count=None):
    """the instance form's queries, float32 [count, 3, 3]: instance q's rows of the merged scene"""
    merged, first = IP.merged_positions(scene_positions, scene_of_instance, maps)
    rows = merged.reshape(-1, 3, 3)[first[q]:first[q + 1]]
    return rows[first_triangle:] if count is None else rows[first_triangle:first_triangle + count]


def clearance_instance(scene_positions, scene_of_instance, maps, q, k, max_dist2=np.inf, skip_shared=False, skip_own=True,
                       first_triangle=0, count=None, o=R.NumpyOps, table=None):
    """The header's answer for the instance form (consequence 6): the item form fed with instance q's rows of the merged scene;
    with skip_own the pairs of instance q are removed.  `table`: merged_table() of own_queries(..., q) (the whole instance)."""
    queries = own_queries(scene_positions, scene_of_instance, maps, q)
    if table is None:
        table = merged_table(scene_positions, scene_of_instance, maps, queries, o)
    stop = None if count is None else first_triangle + count
    rows = slice(first_triangle, stop)
    merged, first, d2, shared = table
    return from_merged_table((merged, first, d2[rows], shared[rows]), queries[rows], k, max_dist2, skip_shared, q if skip_own else None)


def within(scene_positions, scene_of_instance, maps, max_dist2, o=R.NumpyOps, tables=None):
    """bool [instances]: instance i has a triangle within max_dist2 of a triangle of another instance.  `tables`: one
    merged_table() of own_queries(..., q) per instance q, to share them between calls."""
    return np.array([bool(clearance_instance(scene_positions, scene_of_instance, maps, q, 0, max_dist2, o=o,
                                             table=None if tables is None else tables[q])[2].any()) for q in range(len(maps))])


# ---- the walk ---------------------------------------------------------------------------------------------------------------
def above(lb, reach):
    """the kernel's skip: the bound is strictly above the reach (false for a NaN on either side)"""
    return lb > reach


def at_or_above(lb, reach):
    """a mutant: a bound that equals the reach is skipped"""
    return lb >= reach


def key_instance_first(d, i, t):
    return (d, i, t)


def key_triangle_first(d, i, t):
    """a mutant: the tie broken by the triangle before the instance"""
    return (d, t, i)


def same_instance(i, q, scene_of):
    return i == q


def same_scene(i, q, scene_of):
    """a mutant: "own" judged by the scene, not by the instance index"""
    return scene_of[i] == scene_of[q]


def query_box(queries):
    """(lo, hi), float32 [n, 3] each: min3 / max3 of the corners"""
    q = IR.corners_of(queries)
    with np.errstate(invalid="ignore"):
        return IR._min3(q[:, 0], q[:, 1], q[:, 2]), IR._max3(q[:, 0], q[:, 1], q[:, 2])


def gap2(qlo, qhi, lo, hi):
    """clearance_ref.box_gap2 on [..., 3] arrays that broadcast: float32"""
    cols = lambda a: tuple(a[..., k] for k in range(3))
    with np.errstate(all="ignore"):
        return np.asarray(CR.box_gap2(R.NumpyOps, cols(qlo), cols(qhi), cols(lo), cols(hi)), F)


def shares_matrix(q, t):
    """bool [Q, T]: some corner of t [T, 3, 3] equals (three ==) some corner of q [Q, 3, 3]"""
    with np.errstate(invalid="ignore"):
        return (q[:, None, :, None, :] == t[None, :, None, :, :]).all(-1).any((-1, -2))


def prepare(corners, maps, queries, top_boxes=None, o=R.NumpyOps):
    """what restated_walk needs per instance, for all queries at once: (median tree of the object corners, image-box bounds
    [n, nodes], dist2 of every pair [n, T], world corners, top-level box bounds [n] or None)"""
    per_instance = isinstance(corners, (list, tuple))
    q = IR.corners_of(queries)
    lo, hi = query_box(q)
    trees, per = {}, []
    for i in range(len(maps)):
        mine = corners[i] if per_instance else corners
        if id(mine) not in trees:
            trees[id(mine)] = (mine, IP.median_tree(mine))
        tree = trees[id(mine)][1]
        M = np.asarray(maps[i], F)
        ilo, ihi = IP.image_box(M, np.stack([nd[0] for nd in tree]), np.stack([nd[1] for nd in tree]))
        lbs = gap2(lo[:, None], hi[:, None], ilo[None], ihi[None])
        world = IP.map_corners(M, mine).reshape(-1, 3, 3)
        d2 = CR.pair_table(o, q, world.reshape(-1))[0]
        top = None if top_boxes is None else gap2(lo, hi, np.asarray(top_boxes[i][0], F)[None], np.asarray(top_boxes[i][1], F)[None])
        per.append((tree, lbs.tolist(), d2, world, top, np.asarray(mine, F).reshape(-1, 3, 3)))
    return per


def restated_walk(corners, maps, queries, order, k, counts, max_dist2=np.inf, *, skip_shared=False, own=None, skip_own=False,
                  scene_of=None, object_queries=None, node_skip=above, top_boxes=None, top_skip=above, key=key_instance_first,
                  reach_slot=-1, count_kept_only=False, any_only=False, own_is=same_instance, shared_on_object=False, prepared=None):
    """The kernel's walk, one query at a time: the instances in `order`; an instance that own_is(i, own, scene_of) says is the
    query's own is not walked when skip_own; with `top_boxes` (one (lo, hi) per instance: the top level as a list of its
    leaves) and more than one instance, an instance is entered only when the bound of its box is not above the query's reach;
    in an instance the median tree of the object corners, a node skipped only when the bound of its IMAGE box is above the
    reach, the nearer child first, every triangle of a visited leaf mapped and tested (after the shared-corner rule on world
    corners), n counted for every pair with dist2 <= max_dist2 and the pair's key inserted into the sorted K best.  The reach
    is max_dist2 with `counts` (or k == 0, or any_only), else the dist2 of the held slot k + reach_slot (0-based: the K-th
    smallest), max_dist2 while that slot is empty.  With any_only a query stops at its first member (n is 1 or 0).  `corners`
    is one [t, 3, 3] array for every instance or a list with one per instance.  With shared_on_object the shared-corner rule
    compares `object_queries` with the object corners (a mutant).  The keyword arguments replace one decision each;
    `prepared` is prepare()'s result for the same corners, maps, queries and top boxes.
    Returns (records [n, k], instances [n, k], counts [n] or None, triangle tests, instance walks)."""
    q = IR.corners_of(queries)
    n = len(q)
    md = F(max_dist2)
    walk = CR.walked(q, md)
    prune = not counts and k > 0 and not any_only
    per_instance = isinstance(corners, (list, tuple))
    if scene_of is None:
        scene_of = list(range(len(maps))) if per_instance else [0] * len(maps)
    per = prepared if prepared is not None else prepare(corners, maps, q, top_boxes)
    shared = None
    if skip_shared:
        if shared_on_object:
            oq = np.asarray(object_queries, F).reshape(-1, 3, 3)
            shared = [shares_matrix(oq, p[5]) for p in per]
        else:
            shared = [shares_matrix(q, p[3]) for p in per]
    records = CR.miss_records(n, k, md)
    instances = np.full((n, k), -1, np.int32)
    found = np.zeros(n, np.int32)
    tests = walks = 0
    winners = []
    for j in range(n):
        if not walk[j]:
            continue
        held = []   # sorted keys, at most k
        reach = md
        members = 0
        for i in order:
            if any_only and members:
                break
            if skip_own and own is not None and own_is(int(i), own, scene_of):
                continue
            tree, lbs, d2, _, top, _ = per[i]
            if top is not None and len(maps) > 1 and top_skip(top[j], reach):
                continue
            walks += 1
            lb = lbs[j]
            stack = [] if node_skip(lb[0], reach) else [0]
            while stack and not (any_only and members):
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
                    if shared is not None and shared[i][j, t]:
                        continue
                    tests += 1
                    d = d2[j, t]
                    if not d <= md:
                        continue
                    kk = key(d, int(i), int(t))
                    kept = k > 0 and (len(held) < k or kk < held[-1])
                    if kept or not count_kept_only:
                        members += 1
                    if any_only:
                        break
                    if kept:
                        held.append(kk)
                        held.sort()
                        del held[k:]
                        if prune:
                            slot = k + reach_slot
                            reach = held[slot][0] if 0 <= slot < len(held) else md
        found[j] = members
        for s, kk in enumerate(held):
            i, t = (kk[1], kk[2]) if key is key_instance_first else (kk[2], kk[1])
            winners.append((j, s, i, t))
    if winners:   # the winners' records, computed again pair by pair (in one call)
        wj, ws, wi, wt = (np.asarray(c) for c in zip(*winners))
        world = np.stack([per[i][3][t] for i, t in zip(wi, wt)])
        rec = CR.pair_records(q[wj], world)
        rec["triangle"] = wt
        records[wj, ws] = rec
        instances[wj, ws] = wi
    return records, instances, (found if counts or any_only else None), tests, walks


def walk_counters(tree, node_boxes, corners, M, queries, max_dist2, top_box=None, skip_shared=False, any_only=False, o=R.NumpyOps,
                  d2s=None):
    """The counting form's walk of ONE instance, one query at a time in plain python, over a refit_ref.TreeArrays `tree`
    (pre-order) whose nodes' boxes are `node_boxes` float32 [n, 6] (what octant copy 7 of the packed tree holds) and whose
    triangles are the object `corners` [T, 3, 3] in the tree's order.  A walked query enters the instance unless the bound of
    `top_box` (lo, hi: the box the top level stores for it; None: a set of one instance, which never culls) is above
    max_dist2.  Then the root's image bound is counted and tested; both children of an entered branch are counted; the child
    with the smaller bound is entered first and the other kept if its bound is not above max_dist2; in an entered leaf a
    triangle that shares a corner (skip_shared) or whose own world vertex box is beyond max_dist2 is passed over, every other
    one is tested.  With any_only the walk stops at its first member.  Returns a dict of int64 [n queries]: node_visits,
    leaf_visits, triangle_tests, traversals (1 where the instance is walked), `members` (the instance's pairs of the query
    within max_dist2, over every walked query), and float32 [n] `top_bound` (nan without a top box) and `least` (the
    smallest dist2 of a pair of the query, +inf where there is none).  `d2s`: the pair table of the queries over the world
    corners (clearance_ref.pair_table), where the caller holds it already."""
    M = np.asarray(M, F).reshape(3, 4)
    nb = np.asarray(node_boxes, F).reshape(-1, 6)
    q = IR.corners_of(queries)
    n = len(q)
    md = F(max_dist2)
    lo, hi = query_box(q)
    walked = CR.walked(q, md)
    go = walked.copy()
    top_bound = np.full(n, np.nan, F)
    if top_box is not None:
        top_bound = gap2(lo, hi, np.asarray(top_box[0], F)[None], np.asarray(top_box[1], F)[None])
        with np.errstate(invalid="ignore"):
            go &= ~(top_bound > md)
    ilo, ihi = IP.image_box(M, nb[:, :3], nb[:, 3:])
    world = IP.map_corners(M, corners).reshape(-1, 3, 3)
    lbs = gap2(lo[:, None], hi[:, None], ilo[None], ihi[None])
    if d2s is None:
        d2s = CR.pair_table(o, q, world.reshape(-1), pairs=1 << (18 if o.xp is np else 22))[0]
    wlo, whi = world.min(1), world.max(1)
    own_gap = gap2(lo[:, None], hi[:, None], wlo[None], whi[None])
    with np.errstate(invalid="ignore"):
        candidate = ~(own_gap > md)
        if skip_shared:
            candidate &= ~shares_matrix(q, world)
        member = candidate & (d2s <= md) & walked[:, None]
    negative, positive = tree.negative.tolist(), tree.positive.tolist()
    start, count = tree.start.tolist(), tree.triangles.tolist()
    out = {name: np.zeros(n, np.int64) for name in COUNTERS}
    out["members"] = member.sum(1).astype(np.int64)
    out["top_bound"] = top_bound
    with np.errstate(invalid="ignore"):
        out["least"] = np.where(walked, np.where(np.isnan(d2s), np.inf, d2s).min(1) if d2s.shape[1] else np.inf, np.inf).astype(F)
    reach = float(md)
    for j in range(n):
        if not go[j]:
            continue
        lb, cand, mem = lbs[j].tolist(), candidate[j], member[j]
        nodes, leaves, tests, done = 1, 0, 0, False
        stack = [] if lb[0] > reach else [0]
        while stack and not done:
            cur = stack.pop()
            if negative[cur] < 0:
                leaves += 1
                for t in range(start[cur], start[cur] + count[cur]):
                    if not cand[t]:
                        continue
                    tests += 1
                    if any_only and mem[t]:
                        done = True
                        break
                continue
            nodes += 2
            n0, n1 = negative[cur], positive[cur]
            nr, fr = (n1, n0) if lb[n1] < lb[n0] else (n0, n1)
            if not lb[nr] > reach:
                if not lb[fr] > reach:
                    stack.append(fr)
                stack.append(nr)
        out["node_visits"][j], out["leaf_visits"][j], out["triangle_tests"][j], out["traversals"][j] = nodes, leaves, tests, 1
    return out
