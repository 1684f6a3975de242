"""Restatement of the instanced closest-point query (include/shader_ray_instance_point.h), for the tests.

The header's definition: every corner of instance i's scene goes to the world by the caller's object_to_world floats (the
products of the nonzero entries only, left to right, then the translation if it is nonzero; elementwise float32, no FMA), and
the answer is point_query_ref.closest, unchanged, on the merged scene whose positions are the mapped corners in instance
order.  The merged triangle index then splits into (instance, triangle of the member scene), and the merged scene's lowest
index on a tie is the lowest instance, then the lowest triangle, by construction.

image_box is the box the walk culls with: per world axis the same corner formula on the ends of the object box that make it
smallest and largest, chosen by the signs of the map's entries.
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


def map_corners(M, positions):
    """the world corners, float32 [n, 3], of object corners `positions` (any shape of 3 n floats) under M [3, 4]"""
    M = np.asarray(M, F).reshape(3, 4)
    v = np.asarray(positions, F).reshape(-1, 3)
    x = (v[:, 0], v[:, 1], v[:, 2])
    with np.errstate(all="ignore"):
        return np.stack([map_row(M[r], x) for r in range(3)], axis=1)


def image_box(M, lo, hi):
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
