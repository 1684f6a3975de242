"""Numpy restatement of include/shader_ray_overlap.h: which triangles touch an axis-aligned box.

Written from the header's text: fp32 throughout, every product and sum its own rounding (numpy contracts nothing), sums left
to right, min and max as the comparisons x < y ? x : y and x > y ? x : y, every test a comparison that a NaN fails.  Vectorised
over triangles (and over blocks of boxes).

  first_axis(positions, boxes) -> int8 [n_boxes, n_triangles]: the first of the 13 axes, in the header's order, that separates
                                  the pair (0-2 the box's x, y, z; 3 the plane; 4 + 3 e + j edge e with box axis j), OVERLAP
                                  (-1) when none does, UNWALKED (13) for every pair of a box that is not walked
  overlaps(positions, boxes)   -> bool [n_boxes, n_triangles]
  overlap(positions, boxes, k) -> (int32 [n_boxes, k], int32 [n_boxes]): the k smallest indices then -1, and the count
  walk_counters(tree, node_boxes, corners, boxes, any_only) -> the walk's own work per box: node visits,
                                  leaf visits, triangle tests and the greatest stack depth
"""
import numpy as np

F = np.float32
BOX_DTYPE = np.dtype([("lo", F, 3), ("pad0", F), ("hi", F, 3), ("pad1", F)])
OVERLAP, UNWALKED = -1, 13
AXES = 13
MISS = -1


def make_boxes(lo, hi):
    lo = np.asarray(lo, F).reshape(-1, 3)
    out = np.zeros(len(lo), BOX_DTYPE)
    out["lo"], out["hi"] = lo, np.asarray(hi, F).reshape(-1, 3)
    return out


def lo_hi(boxes):
    """(lo, hi) float32 [n, 3] of a BOX_DTYPE array or of [n, 6] / [n, 8] floats"""
    boxes = np.asarray(boxes)
    if boxes.dtype.names:
        return np.ascontiguousarray(boxes["lo"], F).reshape(-1, 3), np.ascontiguousarray(boxes["hi"], F).reshape(-1, 3)
    a = np.asarray(boxes, F)
    return (a[:, 0:3], a[:, 3:6]) if a.shape[1] == 6 else (a[:, 0:3], a[:, 4:7])


def walked(boxes):
    """bool [n]: every coordinate finite and lo <= hi on every axis"""
    lo, hi = lo_hi(boxes)
    return np.isfinite(lo).all(1) & np.isfinite(hi).all(1) & ~(lo > hi).any(1)


def _min(x, y):
    return np.where(x < y, x, y)


def _max(x, y):
    return np.where(x > y, x, y)


def _min3(x, y, z):
    return _min(_min(x, y), z)


def _max3(x, y, z):
    return _max(_max(x, y), z)


def _stage0(tris, lo, hi):
    """bool [B, T, 3]: box axis j separates, for boxes (lo, hi) [B, 3] against tris [T, 3, 3]"""
    a, b, c = (tris[:, k, :] for k in range(3))
    least, most = _min3(a, b, c)[None], _max3(a, b, c)[None]   # [1, T, 3]
    return (least > hi[:, None, :]) | (most < lo[:, None, :])


def _later(tri, lo, hi):
    """int8 [P]: the first of axes 3 to 12 that separates pair p, triangle tri [P, 3, 3] and box (lo, hi) [P, 3], or OVERLAP"""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    half = F(0.5)
    sep = {}
    # translation
    m = half * lo + half * hi
    h = half * hi - half * lo
    v0, v1, v2 = a - m, b - m, c - m
    e0, e1, e2 = v1 - v0, v2 - v1, v0 - v2
    X, Y, Z = 0, 1, 2
    # stage 1
    nx = e0[:, Y] * e1[:, Z] - e0[:, Z] * e1[:, Y]
    ny = e0[:, Z] * e1[:, X] - e0[:, X] * e1[:, Z]
    nz = e0[:, X] * e1[:, Y] - e0[:, Y] * e1[:, X]
    d = (nx * v0[:, X] + ny * v0[:, Y]) + nz * v0[:, Z]
    r = (h[:, X] * np.abs(nx) + h[:, Y] * np.abs(ny)) + h[:, Z] * np.abs(nz)
    sep[3] = (d > r) | (d < -r)
    # stage 2
    for k, e in enumerate((e0, e1, e2)):
        for j, (u, w) in enumerate(((Y, Z), (Z, X), (X, Y))):   # axis j: p = e.u * v.w - e.w * v.u, r = h.u |e.w| + h.w |e.u|
            p = [e[:, u] * v[:, w] - e[:, w] * v[:, u] for v in (v0, v1, v2)]
            r = h[:, u] * np.abs(e[:, w]) + h[:, w] * np.abs(e[:, u])   # (on y the header names the terms the other way round: a + b is b + a)
            sep[4 + 3 * k + j] = (_min3(*p) > r) | (_max3(*p) < -r)
    code = np.full(len(tri), OVERLAP, np.int8)
    for axis in range(AXES - 1, 2, -1):
        code = np.where(sep[axis], np.int8(axis), code)
    return code


def first_axis(positions, boxes, pairs_per_block=1 << 22):
    """Stage 0 for every pair; the later stages for the pairs that pass it (the set does not depend on that: the header)."""
    tris = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
    lo, hi = lo_hi(boxes)
    lo, hi = np.ascontiguousarray(lo, F), np.ascontiguousarray(hi, F)
    out = np.empty((len(lo), len(tris)), np.int8)
    step = max(1, pairs_per_block // max(1, len(tris)))
    with np.errstate(all="ignore"):
        for s in range(0, len(lo), step):
            sep = _stage0(tris, lo[s:s + step], hi[s:s + step])
            code = np.where(sep[..., 0], np.int8(0), np.where(sep[..., 1], np.int8(1), np.int8(2)))
            bi, ti = np.nonzero(~sep.any(2))
            code[bi, ti] = _later(tris[ti], lo[s + bi], hi[s + bi])
            out[s:s + step] = code
    out[~walked(boxes)] = UNWALKED
    return out


def overlaps(positions, boxes):
    return first_axis(positions, boxes) == OVERLAP


def from_set(member, k):
    """(indices int32 [n, k], counts int32 [n]) of a bool [n, triangles] membership"""
    n = member.sum(1).astype(np.int32)
    out = np.full((len(member), k), MISS, np.int32)
    if k:
        for row in np.nonzero(n)[0]:
            first = np.flatnonzero(member[row])[:k]
            out[row, :len(first)] = first
    return out, n


def overlap(positions, boxes, k):
    return from_set(overlaps(positions, boxes), k)


COUNTERS = ("node_visits", "leaf_visits", "triangle_tests")


def walk_counters(tree, node_boxes, corners, boxes, any_only=False, member=None):
    """The walk itself, one box at a time in plain python: over a refit_ref.TreeArrays `tree` (pre-order) whose
    nodes' boxes are `node_boxes` float32 [n, 6] (refit_ref.node_boxes: the min/max fold the scene stores), the triangles being
    `corners` [T, 3, 3] in the tree's order.  A node is entered iff the six comparisons pass; the root is tested once, both
    children of an entered branch are tested (two node visits), the walk descends into the negative child when it overlaps and
    pushes the positive one when both do, else into the positive one, else it pops; every triangle of a visited leaf is tested,
    in index order; with `any_only` the walk ends at the first triangle that touches.  A box that is not walked visits nothing.

    `member` is overlaps(corners, boxes) where the caller holds it already (only `any_only` looks at it).
    Returns a dict of int64 [n_boxes]: node_visits, leaf_visits, triangle_tests and `stack`, the greatest number of stack
    entries held at once."""
    lo, hi = lo_hi(boxes)
    go = walked(boxes)
    if any_only and member is None:
        member = overlaps(corners, boxes)
    nb = np.asarray(node_boxes, F).reshape(-1, 6).tolist()
    negative, positive = tree.negative.tolist(), tree.positive.tolist()
    start, count = tree.start.tolist(), tree.triangles.tolist()
    out = {name: np.zeros(len(lo), np.int64) for name in COUNTERS + ("stack",)}

    for b in range(len(lo)):
        if not go[b]:
            continue
        l0, l1, l2 = lo[b].tolist()
        h0, h1, h2 = hi[b].tolist()

        def enters(k):
            x = nb[k]
            return not (x[3] < l0 or x[0] > h0 or x[4] < l1 or x[1] > h1 or x[5] < l2 or x[2] > h2)

        nodes, leaves, tests, deepest = 1, 0, 0, 0
        stack = []
        cur = 0 if enters(0) else -1
        while cur >= 0:
            nxt = -1
            if negative[cur] < 0:
                leaves += 1
                if any_only:
                    row = member[b, start[cur]:start[cur] + count[cur]]
                    hit = np.flatnonzero(row)
                    tests += int(hit[0]) + 1 if len(hit) else count[cur]
                    if len(hit):
                        break
                else:
                    tests += count[cur]
            else:
                nodes += 2
                in0, in1 = enters(negative[cur]), enters(positive[cur])
                if in0 and in1:
                    stack.append(positive[cur])
                    deepest = max(deepest, len(stack))
                nxt = negative[cur] if in0 else positive[cur] if in1 else -1
            if nxt < 0 and stack:
                nxt = stack.pop()
            cur = nxt
        out["node_visits"][b], out["leaf_visits"][b], out["triangle_tests"][b], out["stack"][b] = nodes, leaves, tests, deepest
    return out
