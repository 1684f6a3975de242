"""Restatement of the closest-point query (include/shader_ray_point.h), for the tests.

The header's brute-force definition, vectorised over (point, triangle) pairs in chunks: Ericson's closest point on a
triangle in its order of tests, the non-finite quotients replaced by 0, the clamp to the triangle's vertex box, then the
smallest dist2 <= max_dist2 with the lowest triangle index on a tie.  Every operation is an elementwise float32 ufunc (no
np.dot, einsum or sum: their summation order is not the contract's); dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z.

The same code runs on torch tensors (closest_torch): each fp32 operation is computed in float64 and rounded to float32.
That is exact for + - * / by the double-rounding theorem (53 >= 2 * 24 + 2), so a GPU can brute-force scenes too large
for numpy.  The tests check the two against each other.
"""
from __future__ import annotations

import numpy as np

F = np.float32
HIT_MISS = -1
REGION_A, REGION_B, REGION_C, REGION_AB, REGION_AC, REGION_BC, REGION_FACE, REGION_NONE = 0, 1, 2, 3, 4, 5, 6, -1
POINT_DTYPE = np.dtype([("p", np.float32, 3), ("max_dist2", np.float32)])
CLOSEST_DTYPE = np.dtype([("q", np.float32, 3), ("dist2", np.float32), ("u", np.float32), ("v", np.float32), ("triangle", np.int32),
                          ("region", np.int32)])


class NumpyOps:
    """float32 numpy: every ufunc rounds once to float32"""
    xp = np

    @staticmethod
    def f(x):
        return np.asarray(x, F)

    add, sub, mul, div = np.add, np.subtract, np.multiply, np.divide
    where, isfinite = np.where, np.isfinite


class TorchOps:
    """float32 torch tensors, each operation computed in float64 and rounded to float32 (exact for + - * /)"""

    def __init__(self, device):
        import torch
        self.xp = torch
        self.device = device

    def f(self, x):
        return self.xp.as_tensor(np.asarray(x, F), device=self.device)

    def add(self, a, b):
        return (a.double() + b.double()).float()

    def sub(self, a, b):
        return (a.double() - b.double()).float()

    def mul(self, a, b):
        return (a.double() * b.double()).float()

    def div(self, a, b):
        return (a.double() / b.double()).float()

    def where(self, c, a, b):
        return self.xp.where(c, a, b)

    def isfinite(self, a):
        return self.xp.isfinite(a)


def _dot(o, x, y):
    return o.add(o.add(o.mul(x[0], y[0]), o.mul(x[1], y[1])), o.mul(x[2], y[2]))


def _sel_min(o, x, y):
    return o.where(x < y, x, y)


def _sel_max(o, x, y):
    return o.where(x > y, x, y)


def closest_on_triangles(o, p, a, b, c):
    """Per pair: (q (3 arrays), dist2, u, v, region).  p, a, b, c: tuples of 3 float32 arrays that broadcast together."""
    zero, one = o.f(0.0), o.f(1.0)
    ab = tuple(o.sub(b[k], a[k]) for k in range(3))
    ac = tuple(o.sub(c[k], a[k]) for k in range(3))
    ap = tuple(o.sub(p[k], a[k]) for k in range(3))
    bp = tuple(o.sub(p[k], b[k]) for k in range(3))
    cp = tuple(o.sub(p[k], c[k]) for k in range(3))
    d1, d2 = _dot(o, ab, ap), _dot(o, ac, ap)
    d3, d4 = _dot(o, ab, bp), _dot(o, ac, bp)
    d5, d6 = _dot(o, ab, cp), _dot(o, ac, cp)
    vc = o.sub(o.mul(d1, d4), o.mul(d3, d2))
    vb = o.sub(o.mul(d5, d2), o.mul(d1, d6))
    va = o.sub(o.mul(d3, d6), o.mul(d5, d4))
    d43, d56 = o.sub(d4, d3), o.sub(d5, d6)
    in_a = (d1 <= zero) & (d2 <= zero)
    in_b = ~in_a & (d3 >= zero) & (d4 <= d3)
    taken = in_a | in_b
    in_ab = ~taken & (vc <= zero) & (d1 >= zero) & (d3 <= zero)
    taken = taken | in_ab
    in_c = ~taken & (d6 >= zero) & (d5 <= d6)
    taken = taken | in_c
    in_ac = ~taken & (vb <= zero) & (d2 >= zero) & (d6 <= zero)
    taken = taken | in_ac
    in_bc = ~taken & (va <= zero) & (d43 >= zero) & (d56 >= zero)
    in_face = ~(taken | in_bc)

    def fin(s):
        return o.where(o.isfinite(s), s, zero)

    s_ab = fin(o.div(d1, o.sub(d1, d3)))
    s_ac = fin(o.div(d2, o.sub(d2, d6)))
    s_bc = fin(o.div(d43, o.add(d43, d56)))
    den = o.div(one, o.add(o.add(va, vb), vc))
    fu, fv = o.mul(vb, den), o.mul(vc, den)
    ok = o.isfinite(fu) & o.isfinite(fv)
    fu, fv = o.where(ok, fu, zero), o.where(ok, fv, zero)

    u = o.where(in_b, one, o.where(in_ab, s_ab, o.where(in_bc, o.sub(one, s_bc), o.where(in_face, fu, zero))))
    u = o.where(in_a | in_c | in_ac, zero, u)
    v = o.where(in_c, one, o.where(in_ac, s_ac, o.where(in_bc, s_bc, o.where(in_face, fv, zero))))
    v = o.where(in_a | in_b | in_ab, zero, v)
    region = o.where(in_a, REGION_A, o.where(in_b, REGION_B, o.where(in_ab, REGION_AB, o.where(
        in_c, REGION_C, o.where(in_ac, REGION_AC, o.where(in_bc, REGION_BC, REGION_FACE))))))
    q, d = [], []
    for k in range(3):
        qk = o.where(in_a, a[k], o.where(in_b, b[k], o.where(in_c, c[k], o.where(
            in_ab, o.add(a[k], o.mul(ab[k], s_ab)), o.where(
                in_ac, o.add(a[k], o.mul(ac[k], s_ac)), o.where(
                    in_bc, o.add(b[k], o.mul(o.sub(c[k], b[k]), s_bc)),
                    o.add(o.add(a[k], o.mul(ab[k], fu)), o.mul(ac[k], fv))))))))
        lo = _sel_min(o, _sel_min(o, a[k], b[k]), c[k])
        hi = _sel_max(o, _sel_max(o, a[k], b[k]), c[k])
        qk = _sel_min(o, _sel_max(o, qk, lo), hi)
        q.append(qk)
        d.append(o.sub(p[k], qk))
    return tuple(q), _dot(o, d, d), u, v, region


def box_bound(o, p, lo, hi):
    """The header's box bound: dot(g, g), g per axis the distance from p to the box's slab (0 inside it)."""
    zero = o.f(0.0)
    g = tuple(o.where(p[k] < lo[k], o.sub(lo[k], p[k]), o.where(p[k] > hi[k], o.sub(p[k], hi[k]), zero)) for k in range(3))
    return _dot(o, g, g)


def _closest(o, positions, points, point_chunk, pairs):
    xp = o.xp
    pos = o.f(np.asarray(positions, F).reshape(-1, 9))
    pts = np.ascontiguousarray(points)
    if pts.dtype != POINT_DTYPE:
        pts = np.ascontiguousarray(np.asarray(pts, F).reshape(-1, 4)).view(POINT_DTYPE).reshape(-1)
    n, t_count = len(pts), len(pos)
    out = np.zeros(n, CLOSEST_DTYPE)
    tri_chunk = max(1, pairs // max(1, point_chunk))
    for s in range(0, n, point_chunk):
        pc = pts[s:s + point_chunk]
        m = len(pc)
        P = o.f(pc["p"])
        md = o.f(pc["max_dist2"])
        p = tuple(P[:, k:k + 1] for k in range(3))
        best_d = md.clone() if xp is not np else md.copy()
        best_t = xp.full((m,), -1, dtype=xp.int64) if xp is np else xp.full((m,), -1, dtype=xp.int64, device=o.device)
        best_q = [P[:, k].clone() if xp is not np else P[:, k].copy() for k in range(3)]
        best_u, best_v = o.f(np.zeros(m)), o.f(np.zeros(m))
        best_r = xp.full((m,), -1, dtype=xp.int64) if xp is np else xp.full((m,), -1, dtype=xp.int64, device=o.device)
        walk = o.isfinite(P[:, 0]) & o.isfinite(P[:, 1]) & o.isfinite(P[:, 2]) & (md >= o.f(0.0))
        rows = xp.arange(m) if xp is np else xp.arange(m, device=o.device)
        for t0 in range(0, t_count, tri_chunk):
            T = pos[t0:t0 + tri_chunk]
            a = tuple(T[None, :, k] for k in range(3))
            b = tuple(T[None, :, 3 + k] for k in range(3))
            c = tuple(T[None, :, 6 + k] for k in range(3))
            q, d2, u, v, region = closest_on_triangles(o, p, a, b, c)
            qual = (d2 <= md[:, None]) & walk[:, None]
            inf = o.f(np.inf)
            key = o.where(qual, d2, inf)
            dmin = key.min(axis=1) if xp is np else key.min(dim=1).values
            hit = qual & (d2 == dmin[:, None])
            anyq = hit.any(axis=1) if xp is np else hit.any(dim=1)
            idx = hit.argmax(axis=1) if xp is np else hit.to(xp.int8).argmax(dim=1)
            had = best_t >= 0
            take = anyq & (~had | (dmin < best_d))
            best_d = o.where(take, dmin, best_d)
            best_t = o.where(take, idx + t0, best_t)
            for k in range(3):
                best_q[k] = o.where(take, q[k][rows, idx], best_q[k])
            best_u = o.where(take, u[rows, idx], best_u)
            best_v = o.where(take, v[rows, idx], best_v)
            best_r = o.where(take, region[rows, idx], best_r)

        def host(x):
            return x if xp is np else x.cpu().numpy()

        sl = out[s:s + m]
        sl["q"] = np.stack([host(best_q[k]) for k in range(3)], axis=1)
        sl["dist2"] = host(best_d)
        sl["u"], sl["v"] = host(best_u), host(best_v)
        sl["triangle"] = host(best_t)
        sl["region"] = host(best_r)
        out[s:s + m] = sl
    return out


def closest(positions, points, point_chunk: int = 256, pairs: int = 1 << 18) -> np.ndarray:
    """The header's answer for every point, brute force in float32 numpy.  positions: the scene's vertex_positions (9 floats a
    triangle); points: a POINT_DTYPE array or [n, 4] float32.  Returns a CLOSEST_DTYPE array."""
    with np.errstate(all="ignore"):
        return _closest(NumpyOps, positions, points, point_chunk, pairs)


def closest_torch(positions, points, device="cuda", point_chunk: int = 1024, pairs: int = 1 << 24) -> np.ndarray:
    """closest() on torch tensors on `device`: each fp32 operation in float64, rounded to float32 (exact: module doc)."""
    return _closest(TorchOps(device), positions, points, point_chunk, pairs)


def as_bits(records: np.ndarray) -> np.ndarray:
    """CLOSEST_DTYPE records as [n, 8] uint32 words (the 32 bytes of each record)"""
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 8)
