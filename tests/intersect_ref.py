"""Numpy restatement of include/shader_ray_intersect.h: which scene triangles intersect a query triangle.

Written from the header's text: fp32 throughout, every product and sum its own rounding (numpy contracts nothing), the dot
product (x x' + y y') + z z', min and max as the comparisons x < y ? x : y and x > y ? x : y, every test a comparison that a NaN
fails.  Vectorised over pairs.

  first_axis(queries, positions, skip_shared) -> int8 [n_queries, n_triangles]: the first stage, in the header's order, that
                                  rejects the pair: 0-2 the vertex boxes' x, y, z; SHARED (3) a shared corner (only with
                                  skip_shared); DEGENERATE (4) a scene triangle with a zero normal; AXIS0 + a (5 .. 21) the
                                  a-th of the seventeen axes; INTERSECT (-1) when none does; UNWALKED (22) for every pair of
                                  a query that is not walked
  intersects(queries, positions, skip_shared) -> bool [n_queries, n_triangles]
  intersect(queries, positions, k, skip_shared) -> (int32 [n_queries, k], int32 [n_queries]): the k smallest indices then -1,
                                  and the count
  walk_counters(tree, node_boxes, corners, queries, ...) -> the walk's own work per query: node visits,
                                  leaf visits, triangle tests and the greatest stack depth
"""
import numpy as np

F = np.float32
TRIANGLE_DTYPE = np.dtype([("a", F, 3), ("pad0", F), ("b", F, 3), ("pad1", F), ("c", F, 3), ("pad2", F)])
INTERSECT, SHARED, DEGENERATE, AXIS0, UNWALKED = -1, 3, 4, 5, 22
AXES = 17
STAGES = tuple(range(3)) + tuple(range(AXIS0, AXIS0 + AXES))   # the 3 + 17 separating axes
MISS = -1
AXIS_NAMES = ("nq", "nt") + tuple(f"f{i} x e{j}" for i in range(3) for j in range(3)) + tuple(f"nq x f{i}" for i in range(3)) + \
    tuple(f"nt x e{j}" for j in range(3))


def make_triangles(corners):
    corners = np.asarray(corners, F).reshape(-1, 3, 3)
    out = np.zeros(len(corners), TRIANGLE_DTYPE)
    out["a"], out["b"], out["c"] = corners[:, 0], corners[:, 1], corners[:, 2]
    return out


def corners_of(queries):
    """float32 [n, 3, 3] of a TRIANGLE_DTYPE array, of [n, 3, 3] / [n, 9] floats (a, b, c) or of [n, 12] (shray_triangle)"""
    queries = np.asarray(queries)
    if queries.dtype.names:
        return np.stack([np.ascontiguousarray(queries[k], F).reshape(-1, 3) for k in ("a", "b", "c")], 1)
    a = np.asarray(queries, F)
    if a.ndim == 2 and a.shape[1] == 12:
        return np.ascontiguousarray(a.reshape(-1, 3, 4)[:, :, :3])
    return np.ascontiguousarray(a).reshape(-1, 3, 3)


def _min(x, y):
    return np.where(x < y, x, y)


def _max(x, y):
    return np.where(x > y, x, y)


def _min3(x, y, z):
    return _min(_min(x, y), z)


def _max3(x, y, z):
    return _max(_max(x, y), z)


def _cross(x, y):
    return np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], 1)


def _dot(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


def _all_zero(x):
    return (x == 0).all(1)


def query_normal(q):
    """nq [n, 3] of query corners [n, 3, 3]"""
    with np.errstate(all="ignore"):
        o = q[:, 0]
        q0, q1, q2 = q[:, 0] - o, q[:, 1] - o, q[:, 2] - o
        return _cross(q1 - q0, q2 - q1)


def walked(queries):
    """bool [n]: every coordinate finite and a normal that is not (0, 0, 0)"""
    q = corners_of(queries)
    return np.isfinite(q).all((1, 2)) & ~_all_zero(query_normal(q))


def _stage0(q, tris):
    """bool [Q, T, 3]: axis j of the two vertex boxes separates"""
    lo, hi = _min3(q[:, 0], q[:, 1], q[:, 2]), _max3(q[:, 0], q[:, 1], q[:, 2])
    least, most = _min3(tris[:, 0], tris[:, 1], tris[:, 2])[None], _max3(tris[:, 0], tris[:, 1], tris[:, 2])[None]
    return (least > hi[:, None, :]) | (most < lo[:, None, :])


def shares_corner(q, t):
    """bool [P]: some corner of t [P, 3, 3] equals (three ==) some corner of q [P, 3, 3]"""
    return (q[:, :, None, :] == t[:, None, :, :]).all(3).any((1, 2))


def _later(q, t, skip_shared):
    """int8 [P]: the first stage after stage 0 that rejects pair p, query q [P, 3, 3] and scene triangle t [P, 3, 3]"""
    o = q[:, 0]
    q0, q1, q2 = q[:, 0] - o, q[:, 1] - o, q[:, 2] - o
    v0, v1, v2 = t[:, 0] - o, t[:, 1] - o, t[:, 2] - o
    f = (q1 - q0, q2 - q1, q0 - q2)
    e = (v1 - v0, v2 - v1, v0 - v2)
    nq, nt = _cross(f[0], f[1]), _cross(e[0], e[1])
    axes = [nq, nt] + [_cross(f[i], e[j]) for i in range(3) for j in range(3)] + [_cross(nq, f[i]) for i in range(3)] + \
        [_cross(nt, e[j]) for j in range(3)]
    code = np.full(len(q), INTERSECT, np.int8)
    for k in range(AXES - 1, -1, -1):
        A = axes[k]
        s = [_dot(A, v) for v in (v0, v1, v2)]
        p = [_dot(A, x) for x in (q0, q1, q2)]
        sep = (_min3(*s) > _max3(*p)) | (_max3(*s) < _min3(*p))
        code = np.where(sep, np.int8(AXIS0 + k), code)
    code = np.where(_all_zero(nt), np.int8(DEGENERATE), code)
    if skip_shared:
        code = np.where(shares_corner(q, t), np.int8(SHARED), code)
    return code


def first_axis(queries, positions, skip_shared=False, pairs_per_block=1 << 21):
    """Stage 0 for every pair; the later stages for the pairs that pass it (the set does not depend on that: the header)."""
    q = corners_of(queries)
    tris = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
    out = np.empty((len(q), len(tris)), np.int8)
    step = max(1, pairs_per_block // max(1, len(tris)))
    with np.errstate(all="ignore"):
        for s in range(0, len(q), step):
            sep = _stage0(q[s:s + step], tris)
            code = np.where(sep[..., 0], np.int8(0), np.where(sep[..., 1], np.int8(1), np.int8(2)))
            qi, ti = np.nonzero(~sep.any(2))
            code[qi, ti] = _later(q[s + qi], tris[ti], skip_shared)
            out[s:s + step] = code
    out[~walked(q)] = UNWALKED
    return out


def intersects(queries, positions, skip_shared=False):
    return first_axis(queries, positions, skip_shared) == INTERSECT


def from_set(member, k):
    """(indices int32 [n, k], counts int32 [n]) of a bool [n, triangles] membership"""
    n = member.sum(1).astype(np.int32)
    out = np.full((len(member), k), MISS, np.int32)
    if k:
        for row in np.nonzero(n)[0]:
            first = np.flatnonzero(member[row])[:k]
            out[row, :len(first)] = first
    return out, n


def intersect(queries, positions, k, skip_shared=False):
    return from_set(intersects(queries, positions, skip_shared), k)


COUNTERS = ("node_visits", "leaf_visits", "triangle_tests")


def walk_counters(tree, node_boxes, corners, queries, skip_shared=False, any_only=False, member=None):
    """The walk itself, one query at a time in plain python: over a refit_ref.TreeArrays `tree` (pre-order)
    whose nodes' boxes are `node_boxes` float32 [n, 6], the triangles being `corners` [T, 3, 3] in the tree's order.  A node is
    entered iff the six comparisons of its box with the query's vertex box pass; the root is tested once, both children of an
    entered branch are tested (two node visits), the walk descends into the negative child when it overlaps and pushes the
    positive one when both do, else into the positive one, else it pops; every triangle of a visited leaf is tested, in index
    order; with `any_only` the walk ends at the first member.  A query that is not walked visits nothing.

    `member` is intersects(queries, corners, skip_shared) where the caller holds it already (only `any_only` looks at it).
    Returns a dict of int64 [n_queries]: node_visits, leaf_visits, triangle_tests and `stack`, the greatest number of stack
    entries held at once."""
    q = corners_of(queries)
    lo, hi = _min3(q[:, 0], q[:, 1], q[:, 2]), _max3(q[:, 0], q[:, 1], q[:, 2])
    go = walked(q)
    if any_only and member is None:
        member = intersects(q, corners, skip_shared)
    nb = np.asarray(node_boxes, F).reshape(-1, 6).tolist()
    negative, positive = tree.negative.tolist(), tree.positive.tolist()
    start, count = tree.start.tolist(), tree.triangles.tolist()
    out = {name: np.zeros(len(q), np.int64) for name in COUNTERS + ("stack",)}

    for b in range(len(q)):
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
                    hit = np.flatnonzero(member[b, start[cur]:start[cur] + count[cur]])
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
