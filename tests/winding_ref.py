"""Restatement of the winding-number query (include/shader_ray_winding.h), for the tests.

numpy float32, one rounding per operation, in the header's order: the per-triangle terms, the node records built bottom-up
(leaves summing their triangles one at a time, branches by height), and the walk, vectorised over points: the (point, node)
pairs of one depth at a time decide far or near, and each point's terms (a far node's, or a near leaf's triangles') are then
added one at a time in pre-order, node by node and triangle by triangle, which is the order of the device's depth-first
walk.  Every constant is a float32.  The tree is the pre-order arrays of shray_tree_desc (refit_ref.TreeArrays) with the
node boxes in pre-order (scene_ref.node_boxes, or refit_ref.node_boxes after a refit).

Also small meshes whose winding numbers are known: an open cube, two interpenetrating cubes, an inward-wound cube, the cube
moved by 1e4 on every axis, and a soup with duplicate and degenerate triangles.
"""
from __future__ import annotations

import numpy as np

import scene_ref
import sdf_ref
from refit_ref import TreeArrays

F = np.float32
DATA_FLOATS = 20
K4 = F(1.0 / (4.0 * np.pi))
K2 = F(1.0 / (2.0 * np.pi))
_dot, _cross, atan_yx = sdf_ref._dot, sdf_ref._cross, sdf_ref.atan_yx


def triangle_terms(positions):
    """per triangle: N_t [T, 3], A_t [T], x_t [T, 3]"""
    t = np.asarray(positions, F).reshape(-1, 3, 3)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    with np.errstate(all="ignore"):
        n = _cross(b - a, c - a)
        return (n * F(0.5)).astype(F), (F(0.5) * np.sqrt(_dot(n, n))).astype(F), (((a + b) + c) / F(3)).astype(F)


def heights(tree: TreeArrays) -> np.ndarray:
    h = np.zeros(tree.node_count, np.int64)
    for k in range(tree.node_count - 1, -1, -1):   # pre-order: children come after their parent
        if tree.negative[k] >= 0:
            h[k] = 1 + max(h[tree.negative[k]], h[tree.positive[k]])
    return h


def _centre(A, S, lo, hi):
    with np.errstate(all="ignore"):
        return np.where((A == F(0))[:, None], (lo + hi) * F(0.5), S / A[:, None]).astype(F)


def _radius(P, lo, hi):
    e = None
    for c in range(8):
        k = np.stack([np.where(c & 1, hi[:, 0], lo[:, 0]), np.where(c & 2, hi[:, 1], lo[:, 1]), np.where(c & 4, hi[:, 2], lo[:, 2])], 1)
        with np.errstate(all="ignore"):
            d = k - P
            ec = _dot(d, d)
        e = ec if e is None else np.where(e > ec, e, ec)
    return np.sqrt(e).astype(F)


def node_records(tree: TreeArrays, lo, hi, positions) -> np.ndarray:
    """float32 [n, 20]: { P, r, N, A, M (row-major), 0, 0, 0 } per node in pre-order; lo, hi float32 [n, 3] the node boxes"""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    Nt, At, xt = triangle_terms(positions)
    n = tree.node_count
    P, N, M = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros((n, 3, 3), F)
    A, r = np.zeros(n, F), np.zeros(n, F)
    leaf = np.nonzero(tree.negative < 0)[0]
    count, start = tree.triangles[leaf].astype(np.int64), tree.start[leaf].astype(np.int64)
    S = np.zeros((len(leaf), 3), F)
    LA, LN = np.zeros(len(leaf), F), np.zeros((len(leaf), 3), F)
    with np.errstate(all="ignore"):
        for j in range(int(count.max()) if len(leaf) else 0):
            s = count > j
            t = start[s] + j
            LA[s] = LA[s] + At[t]
            S[s] = S[s] + xt[t] * At[t][:, None]
            LN[s] = LN[s] + Nt[t]
        LP = _centre(LA, S, lo[leaf], hi[leaf])
        LM = np.zeros((len(leaf), 3, 3), F)
        for j in range(int(count.max()) if len(leaf) else 0):
            s = count > j
            t = start[s] + j
            LM[s] = LM[s] + (xt[t] - LP[s])[:, :, None] * Nt[t][:, None, :]
    A[leaf], P[leaf], N[leaf], M[leaf] = LA, LP, LN, LM
    r[leaf] = _radius(LP, lo[leaf], hi[leaf])
    h = heights(tree)
    for level in range(1, int(h.max()) + 1 if n else 0):
        b = np.nonzero(h == level)[0]
        cn, cp = tree.negative[b], tree.positive[b]
        with np.errstate(all="ignore"):
            A[b] = A[cn] + A[cp]
            S = P[cn] * A[cn][:, None] + P[cp] * A[cp][:, None]
            P[b] = _centre(A[b], S, lo[b], hi[b])
            N[b] = N[cn] + N[cp]
            M[b] = (M[cn] + (P[cn] - P[b])[:, :, None] * N[cn][:, None, :]) + (M[cp] + (P[cp] - P[b])[:, :, None] * N[cp][:, None, :])
        r[b] = _radius(P[b], lo[b], hi[b])
    out = np.zeros((n, DATA_FLOATS), F)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7], out[:, 8:17] = P, r, N, A, M.reshape(n, 9)
    return out


def far_terms(rec, d, d2):
    """the header's T_far for (record, d, d2) rows"""
    M = rec[:, 8:17]
    with np.errstate(all="ignore"):
        length = np.sqrt(d2)
        i3 = F(1) / (d2 * length)
        i5 = i3 / d2
        tr = (M[:, 0] + M[:, 4]) + M[:, 8]
        m = np.stack([(M[:, 3 * i] * d[:, 0] + M[:, 3 * i + 1] * d[:, 1]) + M[:, 3 * i + 2] * d[:, 2] for i in range(3)], 1)
        return ((((_dot(rec[:, 4:7], d) + tr) * i3) - ((F(3) * _dot(d, m)) * i5)) * K4).astype(F)


def triangle_terms_at(corners, q):
    """the header's T_t for rows of (corners [k, 3, 3], q [k, 3])"""
    with np.errstate(all="ignore"):
        a, b, c = corners[:, 0] - q, corners[:, 1] - q, corners[:, 2] - q
        det = _dot(a, _cross(b, c))
        la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
        den = (((la * lb) * lc + _dot(a, b) * lc) + _dot(a, c) * lb) + _dot(b, c) * la
        return np.where(det == F(0), F(0), atan_yx(det, den) * K2).astype(F)


def _walk(tree, records, corners, q, beta):
    """w of the finite points q [P, 3]"""
    P = len(q)
    pid, node = np.arange(P), np.zeros(P, np.int64)
    parts = []   # (point, node, triangle or -1, term)
    while len(pid):
        rec = records[node]
        with np.errstate(all="ignore"):
            d = rec[:, 0:3] - q[pid]
            d2 = _dot(d, d)
            br = beta * rec[:, 3]
            far = d2 > br * br
        if far.any():
            parts.append((pid[far], node[far], np.full(int(far.sum()), -1), far_terms(rec[far], d[far], d2[far])))
        near = ~far
        leaf = near & (tree.negative[node] < 0)
        if leaf.any():
            lp, ln = pid[leaf], node[leaf]
            cnt = tree.triangles[ln].astype(np.int64)
            rp, rn = np.repeat(lp, cnt), np.repeat(ln, cnt)
            first = np.repeat(np.cumsum(cnt) - cnt, cnt)
            t = np.repeat(tree.start[ln].astype(np.int64), cnt) + (np.arange(int(cnt.sum())) - first)
            parts.append((rp, rn, t, triangle_terms_at(corners[t], q[rp])))
        branch = near & (tree.negative[node] >= 0)
        pid = np.concatenate([pid[branch], pid[branch]])
        node = np.concatenate([tree.negative[node[branch]], tree.positive[node[branch]]]).astype(np.int64)
    if not parts:
        return np.zeros(P, F)
    p, n, t, v = (np.concatenate(x) for x in zip(*parts))
    order = np.lexsort((t, n, p))
    p, v = p[order], v[order]
    counts = np.bincount(p, minlength=P)
    rank = np.arange(len(p)) - np.repeat(np.cumsum(counts) - counts, counts)
    terms = np.zeros((P, int(counts.max()) + 1), F)   # a column of +0 first: the sum starts from +0
    terms[p, rank + 1] = v
    return np.cumsum(terms, axis=1, dtype=F)[:, -1].astype(F)   # (accumulate adds one term at a time, left to right)


def winding(tree: TreeArrays, records, positions, points, beta=2.0, chunk_terms=1 << 21) -> np.ndarray:
    """w(q; beta) of each point (POINT_DTYPE or float [n, 3]), float32; NaN for a point with a non-finite coordinate"""
    q = np.asarray(points["p"] if getattr(points, "dtype", None) is not None and points.dtype.names else points, F).reshape(-1, 3)
    corners = np.asarray(positions, F).reshape(-1, 3, 3)
    beta = F(beta)
    out = np.full(len(q), np.nan, F)
    live = np.nonzero(np.isfinite(q).all(1))[0]
    step = max(1, chunk_terms // max(1, len(corners))) if np.isinf(beta) else 256
    for s in range(0, len(live), step):
        idx = live[s:s + step]
        out[idx] = _walk(tree, records, corners, q[idx], beta)
    return out


def winding_signed(records_closest, w) -> np.ndarray:
    """the header's winding-signed distance of closest-point records (point_query_ref.CLOSEST_DTYPE) given w"""
    d2 = np.asarray(records_closest["dist2"], F)
    hit = records_closest["triangle"] >= 0
    with np.errstate(all="ignore"):
        d = np.sqrt(d2)
        out = np.where((np.asarray(w, F) > F(0.5)) & (d2 > F(0)), -d, d).astype(F)
    return np.where(hit, out, F(np.nan)).astype(F)


class Restated:
    """a loaded world's tree, boxes and corners, and its node records"""

    def __init__(self, world, positions=None, boxes=None):
        self.tree = TreeArrays.of(world.export_tree())
        arrays = world.arrays()
        self.positions = np.asarray(arrays["vertex_positions"] if positions is None else positions, F).reshape(-1)
        if boxes is None:
            lo, hi = scene_ref.node_boxes(self.tree, arrays["group_boxmin"], arrays["group_boxmax"])
        else:
            lo, hi = boxes[:, :3], boxes[:, 3:]
        self.records = node_records(self.tree, lo, hi, self.positions)

    @classmethod
    def of_tree(cls, tree: TreeArrays, positions, boxes) -> "Restated":
        """the same from a tree that no world holds: its pre-order arrays, the corners float32 [T * 9] in the tree's triangle
        order and the node boxes float32 [n, 6] in pre-order"""
        self = cls.__new__(cls)
        self.tree = tree
        self.positions = np.asarray(positions, F).reshape(-1)
        boxes = np.asarray(boxes, F).reshape(-1, 6)
        self.records = node_records(tree, boxes[:, :3], boxes[:, 3:], self.positions)
        return self

    def w(self, points, beta=2.0):
        return winding(self.tree, self.records, self.positions, points, beta)


# small meshes, outward winding unless said: (positions float32 [V, 3], triangles int32 [T, 3])
def open_cube():
    """the unit cube without its top face (z = 1): 5/6 at the centre"""
    pos, tri = sdf_ref.cube()
    keep = [t for t in tri if not (pos[t][:, 2] == 1).all()]
    return pos, np.array(keep, np.int32)


def two_cubes():
    """the unit cube and its copy moved by 0.5 on every axis: 2 in their overlap [0.5, 1]^3"""
    pos, tri = sdf_ref.cube()
    return np.concatenate([pos, pos + F(0.5)]).astype(F), np.concatenate([tri, tri + len(pos)]).astype(np.int32)


def inward_cube():
    pos, tri = sdf_ref.cube()
    return pos, tri[:, ::-1].copy()


def far_cube():
    """the unit cube moved by 1e4 on every axis"""
    pos, tri = sdf_ref.cube()
    return (pos + F(1e4)).astype(F), tri


def soup():
    """the unit cube plus a face listed twice and then twice reversed (they cancel), a triangle with collinear corners and one
    whose corners coincide: still 1 inside and 0 outside"""
    pos, tri = sdf_ref.cube()
    extra = np.array([[0.2, 0.3, 0.5], [0.4, 0.3, 0.5], [0.9, 0.3, 0.5], [0.5, 0.5, 0.5]], F)
    p = np.concatenate([pos, extra]).astype(F)
    e = len(pos)
    t = np.concatenate([tri, [tri[4], tri[4], tri[4][::-1], tri[4][::-1], [e, e + 1, e + 2], [e + 3, e + 3, e + 3]]]).astype(np.int32)
    return p, t


MESHES = ("open_cube", "two_cubes", "inward_cube", "far_cube", "soup")


def write_mesh(pkg, path, name):
    """the mesh as a trisrc file (normals +z: a degenerate triangle has none of its own)"""
    pos, tri = globals()[name]()
    pkg.scenes.write_trisrc(path, pos, tri, normals=np.tile(np.array([0, 0, 1], F), (len(pos), 1)))
    return path
