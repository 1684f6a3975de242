"""Restatement of the triangle-distance query (include/shader_ray_clearance.h), for the tests.

The header's definition, brute force over (query, triangle) pairs in chunks.  Every operation is an elementwise ufunc over
point_query_ref's NumpyOps / TorchOps (float32, every product and sum its own rounding; TorchOps computes each in float64 and
rounds, which is exact for + - * /), so a GPU can brute-force scenes too large for numpy; Float64Ops runs the same text in
float64 for the accuracy tests.  The corner features are point_query_ref.closest_on_triangles (the closest-point query's
arithmetic, not restated here), the intersecting stage is intersect_ref's pair test (stage 0, the degenerate scene triangle,
the seventeen axes; never its shared-corner stage), the edge features are restated here from the header's text.

  pair_features(o, q, t)        -> (dist2, feature, x, y) of the feature minimum per pair, without the intersecting stage
  pair_records(q, t)            -> PAIR_DISTANCE_DTYPE [P] of pairs q[P, 3, 3], t[P, 3, 3], with the intersecting stage
  pair_table(o, queries, positions) -> (dist2 float32 [n, T], feature int8 [n, T]) with the intersecting stage
  clearance(positions, queries, k, max_dist2, skip_shared) -> (PAIR_DISTANCE_DTYPE [n, k], int32 [n])
  box_gap2(o, qlo, qhi, lo, hi) -> the walk's bound
"""
from __future__ import annotations

import numpy as np

import intersect_ref as IR
import point_query_ref as R

F = np.float32
PAIR_INTERSECTING, MISS = 15, -1
PAIR_DISTANCE_DTYPE = np.dtype([("on_query", F, 3), ("dist2", F), ("on_scene", F, 3), ("triangle", np.int32), ("feature", np.int32),
                                ("reserved", np.int32, 3)])


class Float64Ops:
    """the same text in float64 numpy: what the float32 answer is measured against"""
    xp = np

    @staticmethod
    def f(x):
        return np.asarray(x, np.float64)

    add, sub, mul, div = np.add, np.subtract, np.multiply, np.divide
    where, isfinite = np.where, np.isfinite


def _clamp01(o, s):
    zero, one = o.f(0.0), o.f(1.0)
    s = o.where(o.isfinite(s), s, zero)
    return o.where(s < zero, zero, o.where(s > one, one, s))


def edge_edge(o, P, Qe, Rr, S):
    """One edge feature per pair: (x (3 arrays), y (3 arrays), dist2) of the segments (P, Qe) and (Rr, S)."""
    zero, one = o.f(0.0), o.f(1.0)
    d1 = tuple(o.sub(Qe[k], P[k]) for k in range(3))
    d2 = tuple(o.sub(S[k], Rr[k]) for k in range(3))
    r = tuple(o.sub(P[k], Rr[k]) for k in range(3))
    A, E, f, c, b = R._dot(o, d1, d1), R._dot(o, d2, d2), R._dot(o, d2, r), R._dot(o, d1, r), R._dot(o, d1, d2)
    a_pos, e_pos = A > zero, E > zero
    den = o.sub(o.mul(A, E), o.mul(b, b))
    s_general = o.where(den != zero, _clamp01(o, o.div(o.sub(o.mul(b, f), o.mul(c, E)), den)), zero)
    t_general = o.div(o.add(o.mul(b, s_general), f), E)
    t_general = o.where(o.isfinite(t_general), t_general, zero)
    s_low, s_high = _clamp01(o, o.div(-c, A)), _clamp01(o, o.div(o.sub(b, c), A))
    below, above = t_general < zero, t_general > one
    s_both = o.where(below, s_low, o.where(above, s_high, s_general))
    t_both = o.where(below, zero, o.where(above, one, t_general))
    s = o.where(a_pos & e_pos, s_both, o.where(a_pos, s_low, zero))
    t = o.where(a_pos & e_pos, t_both, o.where(e_pos & ~a_pos, _clamp01(o, o.div(f, E)), zero))
    x, y, d = [], [], []
    for k in range(3):
        xk = o.add(P[k], o.mul(d1[k], s))
        xk = R._sel_min(o, R._sel_max(o, xk, R._sel_min(o, P[k], Qe[k])), R._sel_max(o, P[k], Qe[k]))
        yk = o.add(Rr[k], o.mul(d2[k], t))
        yk = R._sel_min(o, R._sel_max(o, yk, R._sel_min(o, Rr[k], S[k])), R._sel_max(o, Rr[k], S[k]))
        x.append(xk), y.append(yk), d.append(o.sub(xk, yk))
    return tuple(x), tuple(y), R._dot(o, d, d)


def pair_features(o, q, t):
    """The fifteen features in order against a running minimum (a later one replaces it only when its dist2 is less).  q, t:
    three corners each, a corner a tuple of three arrays; everything broadcasts together.  Returns (dist2, feature, x, y)."""
    best = None

    def offer(number, x, y, d2):
        nonlocal best
        if best is None:
            best = [d2, o.where(d2 == d2, number, number), list(x), list(y)]   # (an integer array of the pairs' shape)
            return
        take = d2 < best[0]
        best[0] = o.where(take, d2, best[0])
        best[1] = o.where(take, number, best[1])
        best[2] = [o.where(take, x[k], best[2][k]) for k in range(3)]
        best[3] = [o.where(take, y[k], best[3][k]) for k in range(3)]

    for i in range(3):
        point, d2 = R.closest_on_triangles(o, q[i], t[0], t[1], t[2])[:2]
        offer(i, q[i], point, d2)
    for j in range(3):
        point, d2 = R.closest_on_triangles(o, t[j], q[0], q[1], q[2])[:2]
        offer(3 + j, point, t[j], d2)
    for i in range(3):
        for j in range(3):
            x, y, d2 = edge_edge(o, q[i], q[(i + 1) % 3], t[j], t[(j + 1) % 3])
            offer(6 + 3 * i + j, x, y, d2)
    return best[0], best[1], tuple(best[2]), tuple(best[3])


def _corner_tuples(o, tris):
    """[..., 3, 3] -> three corners, each a tuple of three arrays"""
    return tuple(tuple(tris[..., i, k] for k in range(3)) for i in range(3))


def pair_intersects(q, t):
    """bool [P]: the intersecting stage of pairs q[P, 3, 3], t[P, 3, 3] (any float dtype): a query that is not degenerate, the
    vertex boxes, a scene triangle that is not degenerate, the seventeen axes"""
    with np.errstate(all="ignore"):
        lo, hi = IR._min3(q[:, 0], q[:, 1], q[:, 2]), IR._max3(q[:, 0], q[:, 1], q[:, 2])
        least, most = IR._min3(t[:, 0], t[:, 1], t[:, 2]), IR._max3(t[:, 0], t[:, 1], t[:, 2])
        apart = ((least > hi) | (most < lo)).any(1)
        return ~apart & ~IR._all_zero(IR.query_normal(q)) & np.isfinite(q).all((1, 2)) & (IR._later(q, t, False) == IR.INTERSECT)


def pair_records(q, t, o=R.NumpyOps):
    """PAIR_DISTANCE_DTYPE [P] of pairs q[P, 3, 3], t[P, 3, 3], with the intersecting stage; `triangle` is left 0"""
    d2, feature, x, y = pair_values(q, t, o)
    out = np.zeros(len(d2), PAIR_DISTANCE_DTYPE)
    out["on_query"], out["on_scene"] = np.stack(x, 1), np.stack(y, 1)
    out["dist2"], out["feature"] = d2, feature
    return out


def pair_values(q, t, o=R.NumpyOps):
    """(dist2 [P], feature [P], x (3 arrays), y (3 arrays)) of pairs q[P, 3, 3], t[P, 3, 3] in the ops' precision, with the
    intersecting stage (numpy ops only)"""
    with np.errstate(all="ignore"):
        q, t = o.f(q).reshape(-1, 3, 3), o.f(t).reshape(-1, 3, 3)
        d2, feature, x, y = pair_features(o, _corner_tuples(o, q), _corner_tuples(o, t))
        d2, feature = np.broadcast_to(d2, (len(q),)).copy(), np.broadcast_to(feature, (len(q),)).astype(np.int32).copy()
        hit = pair_intersects(q, t)
        d2[hit], feature[hit] = 0.0, PAIR_INTERSECTING
        return d2, feature, tuple(np.broadcast_to(a, (len(q),)) for a in x), tuple(np.broadcast_to(a, (len(q),)) for a in y)


def walked(queries, max_dist2):
    """bool [n]: every coordinate finite, max_dist2 neither NaN nor negative"""
    with np.errstate(all="ignore"):
        return np.isfinite(IR.corners_of(queries)).all((1, 2)) & bool(F(max_dist2) >= F(0.0))


def pair_table(o, queries, positions, pairs: int = 1 << 18):
    """(dist2 float32 [n, T], feature int8 [n, T]) of every (query, triangle) pair, with the intersecting stage, the features in
    chunks of about `pairs` pairs"""
    q = IR.corners_of(queries)
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
    Q = o.f(q)
    qc = tuple(tuple(Q[:, i, k][:, None] for k in range(3)) for i in range(3))
    P = o.f(pos)
    d2 = np.empty((len(q), len(pos)), F)
    feature = np.empty((len(q), len(pos)), np.int8)
    step = max(1, pairs // max(1, len(q)))
    host = (lambda a: a) if o.xp is np else (lambda a: a.cpu().numpy())
    with np.errstate(all="ignore"):
        for t0 in range(0, len(pos), step):
            T = P[t0:t0 + step]
            tc = tuple(tuple(T[:, j, k][None, :] for k in range(3)) for j in range(3))
            d, f = pair_features(o, qc, tc)[:2]
            d2[:, t0:t0 + step] = host(d)
            feature[:, t0:t0 + step] = host(f)
    hit = IR.first_axis(q, pos.reshape(-1)) == IR.INTERSECT   # (a degenerate or non-finite query has none)
    d2[hit], feature[hit] = 0.0, PAIR_INTERSECTING
    return d2, feature


def shared_table(queries, positions):
    """bool [n, T]: some corner of the scene triangle == some corner of the query (SHRAY_CLEARANCE_SKIP_SHARED)"""
    q = IR.corners_of(queries)
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
    out = np.empty((len(q), len(pos)), bool)
    step = max(1, (1 << 21) // max(1, len(pos)))
    with np.errstate(all="ignore"):
        for s in range(0, len(q), step):
            out[s:s + step] = (q[s:s + step, None, :, None, :] == pos[None, :, None, :, :]).all(4).any((2, 3))
    return out


def miss_records(n, k, max_dist2):
    out = np.zeros((n, k), PAIR_DISTANCE_DTYPE)
    out["dist2"] = F(max_dist2)
    out["triangle"] = out["feature"] = MISS
    return out


def from_table(queries, positions, d2, shared, k, max_dist2, skip_shared=False):
    """The header's outputs from a pair_table's dist2 and a shared_table: (PAIR_DISTANCE_DTYPE [n, k], int32 [n]).  The
    winners' records are computed again, pair by pair, in float32 numpy."""
    q = IR.corners_of(queries)
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
    md = F(max_dist2)
    with np.errstate(all="ignore"):
        member = (d2 <= md) & walked(q, md)[:, None]
    if skip_shared:
        member &= ~shared
    counts = member.sum(1).astype(np.int32)
    records = miss_records(len(q), k, md)
    win_q, win_slot, win_t = [], [], []
    if k:
        for row in np.nonzero(counts)[0]:
            idx = np.nonzero(member[row])[0]
            first = idx[np.argsort(d2[row, idx], kind="stable")][:k]   # stable: the lower index wins a tie
            win_q += [row] * len(first)
            win_slot += list(range(len(first)))
            win_t += first.tolist()
    if win_t:
        wq, ws, wt = np.asarray(win_q), np.asarray(win_slot), np.asarray(win_t)
        rec = pair_records(q[wq], pos[wt])
        rec["triangle"] = wt
        assert np.array_equal(rec["dist2"].view(np.uint32), d2[wq, wt].view(np.uint32))
        records[wq, ws] = rec
    return records, counts


def clearance(positions, queries, k: int, max_dist2=np.inf, skip_shared: bool = False, o=R.NumpyOps):
    """The header's answer, brute force.  positions: the scene's vertex_positions (9 floats a triangle); queries: anything
    intersect_ref.corners_of takes.  Returns (PAIR_DISTANCE_DTYPE [n, k], int32 [n])."""
    d2, _ = pair_table(o, queries, positions)
    return from_table(queries, positions, d2, shared_table(queries, positions) if skip_shared else None, k, max_dist2, skip_shared)


def box_gap2(o, qlo, qhi, lo, hi):
    """The walk's bound: dot(g, g), g per axis the gap between the query's vertex box and a box (0 where they meet)."""
    zero = o.f(0.0)
    g = tuple(o.where(qlo[k] > hi[k], o.sub(qlo[k], hi[k]), o.where(lo[k] > qhi[k], o.sub(lo[k], qhi[k]), zero)) for k in range(3))
    return R._dot(o, g, g)


def vertex_box(tris):
    """(lo, hi), each a tuple of three arrays, of triangles [..., 3, 3], by the header's min and max"""
    lo = tuple(IR._min3(tris[..., 0, k], tris[..., 1, k], tris[..., 2, k]) for k in range(3))
    hi = tuple(IR._max3(tris[..., 0, k], tris[..., 1, k], tris[..., 2, k]) for k in range(3))
    return lo, hi


def as_bits(records: np.ndarray) -> np.ndarray:
    """PAIR_DISTANCE_DTYPE records of any shape as [records, 12] uint32 words (the 48 bytes of each)"""
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 12)
