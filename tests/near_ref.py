"""Restatement of the within-radius query (include/shader_ray_near.h), for the tests.

The header's definition, brute force: dist2 for every (point, triangle) pair by point_query_ref.closest_on_triangles (the
closest-point query's arithmetic, not restated here), chunked; the near set S = {i : dist2_i <= max_dist2}; n = |S|; the first
K members by a stable sort on (dist2, index); their records rebuilt by the same function on the same pairs, and miss records
behind them.  near_torch computes the pairs on torch tensors (point_query_ref.TorchOps: each fp32 operation in float64,
rounded to float32, which is exact), so that a GPU can brute-force scenes too large for numpy; the selection is numpy in both.
"""
from __future__ import annotations

import numpy as np

import point_query_ref as R

F = np.float32
POINT_DTYPE, CLOSEST_DTYPE = R.POINT_DTYPE, R.CLOSEST_DTYPE


def as_points(points) -> np.ndarray:
    pts = np.ascontiguousarray(points)
    if pts.dtype != POINT_DTYPE:
        pts = np.ascontiguousarray(np.asarray(pts, F).reshape(-1, 4)).view(POINT_DTYPE).reshape(-1)
    return pts


def walked(pts) -> np.ndarray:
    """the points that are walked at all: finite p, max_dist2 neither NaN nor negative"""
    with np.errstate(all="ignore"):
        return np.isfinite(pts["p"]).all(1) & (pts["max_dist2"] >= F(0.0))


def pair_dist2(o, positions, pts, pairs: int = 1 << 18) -> np.ndarray:
    """dist2 of every (point, triangle) pair as float32 numpy [len(pts), triangles], in chunks of about `pairs` pairs"""
    pos = o.f(np.asarray(positions, F).reshape(-1, 9))
    P = o.f(pts["p"])
    p = tuple(P[:, k:k + 1] for k in range(3))
    out = np.empty((len(pts), len(pos)), F)
    step = max(1, pairs // max(1, len(pts)))
    for t0 in range(0, len(pos), step):
        T = pos[t0:t0 + step]
        a, b, c = (tuple(T[None, :, 3 * j + k] for k in range(3)) for j in range(3))
        d2 = R.closest_on_triangles(o, p, a, b, c)[1]
        out[:, t0:t0 + step] = d2 if o.xp is np else d2.cpu().numpy()
    return out


def _near(o, positions, points, k, point_chunk, pairs):
    pts = as_points(points)
    pos = np.asarray(positions, F).reshape(-1, 3, 3)
    n = len(pts)
    records = np.zeros((n, k), CLOSEST_DTYPE)
    records["q"] = pts["p"][:, None, :]
    records["dist2"] = pts["max_dist2"][:, None]
    records["triangle"], records["region"] = R.HIT_MISS, R.REGION_NONE
    counts = np.zeros(n, np.int32)
    win_point, win_slot, win_tri = [], [], []
    for s in range(0, n, point_chunk):
        pc = pts[s:s + point_chunk]
        d2 = pair_dist2(o, positions, pc, pairs)
        member = (d2 <= pc["max_dist2"][:, None]) & walked(pc)[:, None]
        counts[s:s + len(pc)] = member.sum(1)
        for row in np.nonzero(member.any(1))[0]:
            idx = np.nonzero(member[row])[0]                         # ascending triangle index
            first = idx[np.argsort(d2[row, idx], kind="stable")][:k]   # stable: the lower index wins a tie
            win_point += [s + row] * len(first)
            win_slot += list(range(len(first)))
            win_tri += first.tolist()
    if win_tri:
        wp, ws, wt = np.asarray(win_point), np.asarray(win_slot), np.asarray(win_tri)
        p = tuple(pts["p"][wp, j] for j in range(3))
        a, b, c = (tuple(pos[wt, corner, j] for j in range(3)) for corner in range(3))
        q, d2, u, v, region = R.closest_on_triangles(R.NumpyOps, p, a, b, c)
        rec = np.zeros(len(wt), CLOSEST_DTYPE)
        rec["q"] = np.stack(q, axis=1)
        rec["dist2"], rec["u"], rec["v"], rec["triangle"], rec["region"] = d2, u, v, wt, region
        records[wp, ws] = rec
    return records, counts


def near(positions, points, k: int, point_chunk: int = 256, pairs: int = 1 << 18):
    """The header's answer, brute force in float32 numpy.  positions: the scene's vertex_positions (9 floats a triangle);
    points: a POINT_DTYPE array or [n, 4] float32.  Returns (CLOSEST_DTYPE [n, k], int32 [n])."""
    with np.errstate(all="ignore"):
        return _near(R.NumpyOps, positions, points, k, point_chunk, pairs)


def near_torch(positions, points, k: int, device="cuda", point_chunk: int = 512, pairs: int = 1 << 24):
    """near() with the pairs' dist2 computed on torch tensors on `device` (exact: module doc)."""
    with np.errstate(all="ignore"):
        return _near(R.TorchOps(device), positions, points, k, point_chunk, pairs)


def as_bits(records: np.ndarray) -> np.ndarray:
    """CLOSEST_DTYPE records of any shape as [records, 8] uint32 words (the 32 bytes of each)"""
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 8)
