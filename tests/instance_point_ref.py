"""Restatement of the instanced closest-point query (include/shader_ray_instance_point.h), for the tests.

The header's definition: every corner of instance i's scene goes to the world by the caller's object_to_world floats (the
products of the nonzero entries only, left to right, then the translation if it is nonzero; elementwise float32, no FMA), and
the answer is point_query_ref.closest, unchanged, on the merged scene whose positions are the mapped corners in instance
order.  The merged triangle index then splits into (instance, triangle of the member scene), and the merged scene's lowest
index on a tie is the lowest instance, then the lowest triangle, by construction.

image_box is the box the walk culls with: per world axis the same corner formula on the ends of the object box that make it
smallest and largest, chosen by the signs of the map's entries.

restated_walk is the kernel's walk in numpy over a median-split tree, all points at once, with every decision the kernel takes
replaceable (the corner formula, the image box, the two skips, the tie rule), so that tests/test_instance_point_scale_reference.py
can show which cell of tests/instance_point_scale_cases.py catches which mistake.  stored_box restates the instance library's
place_box (the box the top level culls with).  walk_counters is instance_walk itself for one instance, one point at a time,
over a refit_ref.TreeArrays: its node visits, leaf visits and triangle tests.
"""
from __future__ import annotations

import numpy as np

import point_query_ref as R

F = np.float32


def map_row(row, x):
    """row r of M applied to the coordinate arrays x = (x0, x1, x2): elementwise float32, nonzero entries only, left to right"""
    row = np.asarray(row, F)
    shape = np.broadcast(x[0], x[1], x[2]).shape
    acc = None
    for c in range(3):
        if row[c] != 0:
            prod = np.multiply(row[c], np.asarray(x[c], F), dtype=F)
            acc = prod if acc is None else np.add(acc, prod, dtype=F)
    if row[3] != 0:
        acc = np.full(shape, row[3], F) if acc is None else np.add(acc, row[3], dtype=F)
    if acc is None:
        acc = np.zeros(shape, F)
    return np.broadcast_to(acc, shape).astype(F)


def map_corners(M, positions, map_row=map_row):
    """the world corners, float32 [n, 3], of object corners `positions` (any shape of 3 n floats) under M [3, 4]"""
    M = np.asarray(M, F).reshape(3, 4)
    v = np.asarray(positions, F).reshape(-1, 3)
    x = (v[:, 0], v[:, 1], v[:, 2])
    with np.errstate(all="ignore"):
        return np.stack([map_row(M[r], x) for r in range(3)], axis=1)


def image_box(M, lo, hi, map_row=map_row):
    """(lo, hi), float32 [..., 3] each, of the image of the boxes lo, hi [..., 3] under M"""
    M = np.asarray(M, F).reshape(3, 4)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    out_lo, out_hi = [], []
    with np.errstate(all="ignore"):
        for r in range(3):
            low = tuple(hi[..., c] if M[r, c] < 0 else lo[..., c] for c in range(3))
            high = tuple(lo[..., c] if M[r, c] < 0 else hi[..., c] for c in range(3))
            out_lo.append(map_row(M[r], low))
            out_hi.append(map_row(M[r], high))
    return np.stack(out_lo, axis=-1), np.stack(out_hi, axis=-1)


def merged_positions(scene_positions, scene_of_instance, maps):
    """the merged scene: the mapped corners in instance order (9 floats a triangle), and each instance's first triangle"""
    maps = np.asarray(maps, F).reshape(-1, 3, 4)
    parts, first = [], [0]
    for i, s in enumerate(scene_of_instance):
        parts.append(map_corners(maps[i], scene_positions[s]).reshape(-1))
        first.append(first[-1] + len(parts[-1]) // 9)
    return np.concatenate(parts), np.asarray(first, np.int64)


def split_index(records, first):
    """the merged scene's records as (records with the member's own triangle index, instances)"""
    out = records.copy()
    t = records["triangle"].astype(np.int64)
    inst = np.where(t >= 0, np.searchsorted(first, t, side="right") - 1, -1)
    out["triangle"] = np.where(t >= 0, t - first[np.maximum(inst, 0)], -1)
    return out, inst.astype(np.int32)


def closest_over_instances(scene_positions, scene_of_instance, maps, points, device=None):
    """The header's answer: (CLOSEST_DTYPE records, int32 instances).  scene_positions: one vertex_positions array per distinct
    scene; scene_of_instance: its index for every instance; maps [n, 3, 4]; points: POINT_DTYPE or [n, 4] float32.  With
    `device`, the brute force runs through point_query_ref.closest_torch there (for more pairs than numpy should take)."""
    merged, first = merged_positions(scene_positions, scene_of_instance, maps)
    records = R.closest(merged, points) if device is None else R.closest_torch(merged, points, device=device)
    return split_index(records, first)


# ---- the walk ---------------------------------------------------------------------------------------------------------------
O = R.NumpyOps


def columns(a):
    return tuple(a[..., k] for k in range(3))


def bound(p, lo, hi):
    """box_bound for points p [n, 3] against boxes lo, hi [..., 3] that broadcast against them: float32"""
    with np.errstate(all="ignore"):
        return R.box_bound(O, columns(p), columns(lo), columns(hi))


def pair_dist2(p, corners, ops=O):
    """(q, dist2, u, v, region), each [n points, t triangles], of the header's per-triangle formula on world corners [t, 3, 3]"""
    with np.errstate(all="ignore"):
        p, corners = ops.f(p), ops.f(corners)
        tri = lambda k: tuple(corners[None, :, k, c] for c in range(3))
        return R.closest_on_triangles(ops, tuple(p[:, c:c + 1] for c in range(3)), tri(0), tri(1), tri(2))


def median_tree(corners, leaf=6):
    """A median-split tree over triangles [t, 3, 3] with the exact minima and maxima of the vertices below every node: a list
    of (lo, hi, left, right, triangle ids or None), the root first."""
    nodes = []

    def build(ids):
        at = len(nodes)
        v = corners[ids].reshape(-1, 3)
        nodes.append(None)
        if len(ids) <= leaf:
            nodes[at] = (v.min(0), v.max(0), -1, -1, ids)
            return at
        c = corners[ids].mean(1)
        axis = int(np.argmax(c.max(0) - c.min(0)))
        order = ids[np.argsort(c[:, axis], kind="stable")]
        left, right = build(order[:len(order) // 2]), build(order[len(order) // 2:])
        nodes[at] = (v.min(0), v.max(0), left, right, None)
        return at

    build(np.arange(len(corners)))
    return nodes


def above(lb, best):
    """the kernel's skip: the bound is strictly above the best (false for a NaN on either side)"""
    return lb > best


def restated_walk(corners, maps, points, order, *, map_corners=map_corners, image_box=image_box, node_skip=above,
                  top_boxes=None, top_skip=above, triangle_first=False, trees=None):
    """The kernel's walk in numpy, all points at once: per instance (in `order`) the tree of the object corners, a node skipped
    for a point only when the bound of its IMAGE box is above the point's best dist2, a leaf's triangles mapped and tested in
    turn with the header's "better" rule on (dist2, instance, triangle).  `corners` is one [t, 3, 3] array for every instance
    or a list with one per instance.  With `top_boxes` (one (lo, hi) per instance: the top level as a list of its leaves) an
    instance is entered by a point only when the bound of its box is not above the point's best.  The keyword arguments
    replace one decision each (the tests' mutants); `triangle_first` orders a tie by (triangle, instance).
    Returns (records, instances, triangle tests)."""
    per_instance = isinstance(corners, (list, tuple))
    trees = {} if trees is None else trees
    n = len(points)
    p = np.ascontiguousarray(points["p"])
    md = points["max_dist2"]
    with np.errstate(invalid="ignore"):
        walk = np.isfinite(p).all(1) & (md >= 0)
    best = md.copy()
    tri, inst = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    q, u, v, region = p.copy(), np.zeros(n, F), np.zeros(n, F), np.full(n, -1, np.int64)
    tests = 0

    def visit(tree, own, M, i, at, ids):
        nonlocal tests
        lo, hi, left, right, members = tree[at]
        ilo, ihi = image_box(M, lo, hi)
        with np.errstate(invalid="ignore"):
            ids = ids[~node_skip(bound(p[ids], ilo, ihi), best[ids])]
        if not len(ids):
            return
        if members is None:
            l_lo, l_hi = image_box(M, *tree[left][:2])
            r_lo, r_hi = image_box(M, *tree[right][:2])
            first = p[ids[:1]]
            with np.errstate(invalid="ignore"):
                near, far = (right, left) if bound(first, r_lo, r_hi)[0] < bound(first, l_lo, l_hi)[0] else (left, right)
            visit(tree, own, M, i, near, ids)
            visit(tree, own, M, i, far, ids)
            return
        world = map_corners(M, own[members]).reshape(-1, 3, 3)
        cq, d2, cu, cv, cr = pair_dist2(p[ids], world)
        tests += d2.size
        for k, t in enumerate(members):
            d = d2[:, k]
            b, bt, bi = best[ids], tri[ids], inst[ids]
            with np.errstate(invalid="ignore"):
                first_key, second_key = ((t < bt), (t == bt) & (i < bi)) if triangle_first else ((i < bi), (i == bi) & (t < bt))
                better = np.where(bt < 0, d <= b, (d < b) | ((d == b) & (first_key | second_key)))
            w = ids[better]
            best[w], tri[w], inst[w] = d[better], t, i
            for c in range(3):
                q[w, c] = np.broadcast_to(cq[c], d2.shape)[better, k]
            u[w], v[w], region[w] = np.broadcast_to(cu, d2.shape)[better, k], np.broadcast_to(cv, d2.shape)[better, k], np.broadcast_to(cr, d2.shape)[better, k]

    for i in order:
        own = corners[i] if per_instance else corners
        if id(own) not in trees:
            trees[id(own)] = (own, median_tree(own))
        ids = np.nonzero(walk)[0]
        if top_boxes is not None:
            with np.errstate(invalid="ignore"):
                ids = ids[~top_skip(bound(p[ids], np.asarray(top_boxes[i][0], F), np.asarray(top_boxes[i][1], F)), best[ids])]
        visit(trees[id(own)][1], own, np.asarray(maps[i], F), int(i), 0, ids)
    out = np.zeros(n, R.CLOSEST_DTYPE)
    out["q"], out["dist2"], out["u"], out["v"], out["triangle"], out["region"] = q, best, u, v, tri, region
    return out, inst.astype(np.int32), tests


MARGIN_ULPS = 128.0 * 2.0 ** -24     # instance.hip's kMarginUlps: 128 u


def stored_box(M, lo, hi):
    """The instance library's place_box restated: (lo, hi, k) of the box the top level stores for an instance whose member's
    root box is lo, hi under M.  The eight corners' images in double, widened by k (|image| + |b|) with k = 128 u ||A|| ||W||
    (infinity norms, W the float32 rounding of the double inverse), then rounded outward to float32."""
    M64 = np.asarray(M, F).reshape(3, 4).astype(np.float64)
    A = M64[:, :3]
    W = np.linalg.inv(A).astype(F).astype(np.float64)
    condition = np.abs(A).sum(1).max() * np.abs(W).sum(1).max()
    ends = np.stack([np.asarray(lo, F), np.asarray(hi, F)]).astype(np.float64)
    corners = np.array([[ends[(c >> a) & 1, a] for a in range(3)] for c in range(8)])
    y = corners @ A.T + M64[:, 3]
    blo, bhi = y.min(0), y.max(0)
    k = MARGIN_ULPS * condition
    reach = max(np.abs(blo).max(), np.abs(bhi).max()) + np.abs(M64[:, 3]).max()
    blo, bhi = blo - k * reach, bhi + k * reach
    flo, fhi = blo.astype(F), bhi.astype(F)
    flo = np.where(flo.astype(np.float64) > blo, np.nextafter(flo, F(-np.inf)), flo)
    fhi = np.where(fhi.astype(np.float64) < bhi, np.nextafter(fhi, F(np.inf)), fhi)
    return flo.astype(F), fhi.astype(F), k


COUNTERS = ("node_visits", "leaf_visits", "triangle_tests", "traversals")


def walk_counters(tree, node_boxes, corners, M, points, device=None):
    """instance_walk itself for ONE instance, one point at a time in plain python, over a refit_ref.TreeArrays `tree`
    (pre-order) whose nodes' boxes are `node_boxes` float32 [n, 6] (refit_ref.node_boxes: what octant copy 7 of the packed tree
    holds) and whose triangles are the object `corners` [T, 3, 3] in the tree's order: the root's image bound is counted and
    tested; both children of an entered branch are counted; the child with the smaller image bound is entered first, the
    negative child on a tie; the other is kept only if its bound is not above the best, and tested again when it is popped;
    every triangle of an entered leaf is tested in index order with the header's "better" rule.  A one-instance set never
    consults its top level, so this is the whole of a point's work.  Returns a dict of int64 [n points]: node_visits,
    leaf_visits, triangle_tests, traversals (1 for a walked point), and `triangle`, the walk's answer (-1: none).
    With `device` the pairs' dist2 are computed there (point_query_ref.TorchOps: the same bits)."""
    M = np.asarray(M, F).reshape(3, 4)
    nb = np.asarray(node_boxes, F).reshape(-1, 6)
    p = np.ascontiguousarray(points["p"])
    md = points["max_dist2"]
    n = len(p)
    with np.errstate(invalid="ignore"):
        go = np.isfinite(p).all(1) & (md >= 0)
    ilo, ihi = image_box(M, nb[:, :3], nb[:, 3:])
    world = map_corners(M, corners).reshape(-1, 3, 3)
    lbs = np.empty((n, len(nb)), F)
    d2s = np.empty((n, len(world)), F)
    ops = O if device is None else R.TorchOps(device)
    chunk = max(1, (1 << 21) // max(1, len(world)))
    for s in range(0, n, chunk):
        lbs[s:s + chunk] = bound(p[s:s + chunk, None, :], ilo[None], ihi[None])
        d = pair_dist2(p[s:s + chunk], world, ops)[1]
        d2s[s:s + chunk] = d if device is None else d.cpu().numpy()
    negative, positive = tree.negative.tolist(), tree.positive.tolist()
    start, count = tree.start.tolist(), tree.triangles.tolist()
    out = {name: np.zeros(n, np.int64) for name in COUNTERS}
    out["triangle"] = np.full(n, -1, np.int64)
    for j in range(n):
        if not go[j]:
            continue
        lb, d2 = lbs[j].tolist(), d2s[j].tolist()
        best, tri = float(md[j]), -1
        nodes, leaves, tests = 1, 0, 0
        stack = []
        cur = -1 if lb[0] > best else 0
        while cur >= 0:
            nxt = -1
            if negative[cur] < 0:
                leaves += 1
                for t in range(start[cur], start[cur] + count[cur]):
                    tests += 1
                    d = d2[t]
                    if (d <= best) if tri < 0 else (d < best or (d == best and t < tri)):
                        best, tri = d, t
            else:
                nodes += 2
                n0, n1 = negative[cur], positive[cur]
                second = lb[n1] < lb[n0]
                near, far = (n1, n0) if second else (n0, n1)
                if not lb[near] > best:
                    if not lb[far] > best:
                        stack.append(far)
                    nxt = near
            while nxt < 0 and stack:
                e = stack.pop()
                if not lb[e] > best:
                    nxt = e
            cur = nxt
        out["node_visits"][j], out["leaf_visits"][j], out["triangle_tests"][j], out["traversals"][j] = nodes, leaves, tests, 1
        out["triangle"][j] = tri
    return out
