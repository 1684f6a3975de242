"""Restatement of the instanced winding-number query (include/shader_ray_instance_winding.h), for the tests.

It composes the restatements that exist and adds the orientation and the sum:
  - W is the set's world-to-object floats (instance_ref.world_to_object on the CPU, InstanceSet.world_to_object() on the GPU);
  - the orientation s_i is the sign of det of W's linear part, in float64 in the header's order (a product of two float32 is
    exact there; the rest rounds once per operation, left to right);
  - the object point is instance_sdf_ref.object_points (the object ray's rule);
  - the term w_i is winding_ref.Restated.w of the member at p_o (NaN for a non-finite p_o), negated when s_i < 0;
  - the sum starts from +0 and adds the terms one at a time, instances ascending, in float32; a non-finite world point is NaN
    with no term;
  - the containing instance is the lowest i whose term is above 0.5, else -1;
  - the winding-signed distance is winding_ref.winding_signed of instance_point_ref.closest_over_instances' records with that
    sum, computed for hits only.
A member is a winding_ref.Restated (its tree, node records and corners).  `signs`, when given, replaces the orientations: the
tests use it to show that a restatement without them is wrong.
"""
from __future__ import annotations

import numpy as np

import instance_point_ref as IP
import instance_sdf_ref as IS
import winding_ref as WR

F = np.float32
D = np.float64


def determinants(W) -> np.ndarray:
    """the header's det of each W [n, 3, 4] float32, float64 [n]"""
    w = np.asarray(W, F).reshape(-1, 3, 4).astype(D)
    with np.errstate(all="ignore"):
        return (w[:, 0, 0] * (w[:, 1, 1] * w[:, 2, 2] - w[:, 1, 2] * w[:, 2, 1])
                - w[:, 0, 1] * (w[:, 1, 0] * w[:, 2, 2] - w[:, 1, 2] * w[:, 2, 0])
                + w[:, 0, 2] * (w[:, 1, 0] * w[:, 2, 1] - w[:, 1, 1] * w[:, 2, 0]))


def orientations(W) -> np.ndarray:
    """s_i: float32 [n], -1 where det < 0, else +1"""
    return np.where(determinants(W) < 0, F(-1), F(1)).astype(F)


def points_of(points) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(points["p"] if getattr(points, "dtype", None) is not None and points.dtype.names else points,
                                           F).reshape(-1, 3))


def terms(members, scene_of_instance, W, p, beta=2.0, signs=None) -> np.ndarray:
    """t_i of the finite world points p [n, 3]: float32 [instances, n]"""
    W = np.asarray(W, F).reshape(-1, 3, 4)
    s = orientations(W) if signs is None else np.asarray(signs, F)
    out = np.zeros((len(W), len(p)), F)
    for i in range(len(W)):
        w_i = members[scene_of_instance[i]].w(IS.object_points(W[i], p), beta)      # (NaN for a non-finite p_o)
        out[i] = -w_i if s[i] < 0 else w_i
    return out


def winding_over_instances(members, scene_of_instance, W, points, beta=2.0, signs=None):
    """The header's answer: (float32 w [n], int32 containing instance [n])"""
    p = points_of(points)
    w = np.full(len(p), np.nan, F)
    containing = np.full(len(p), -1, np.int32)
    live = np.nonzero(np.isfinite(p).all(1))[0]
    if len(live) == 0:
        return w, containing
    t = terms(members, scene_of_instance, W, p[live], beta, signs)
    acc = np.zeros(len(live), F)
    first = np.full(len(live), -1, np.int32)
    with np.errstate(all="ignore"):
        for i in range(len(t)):
            acc = (acc + t[i]).astype(F)
            first = np.where((first < 0) & (t[i] > F(0.5)), np.int32(i), first).astype(np.int32)
    w[live], containing[live] = acc, first
    return w, containing


def winding_signed_over_instances(members, scene_of_instance, maps, W, points, beta=2.0, device=None, closest=None):
    """The header's winding-signed distance: (float32 values, CLOSEST_DTYPE records, int32 instances).  `closest`, when given,
    is instance_point_ref.closest_over_instances' (records, instances), already restated."""
    positions = [m.positions for m in members]
    records, inst = closest if closest is not None else IP.closest_over_instances(positions, scene_of_instance, maps, points, device=device)
    hit = np.nonzero(records["triangle"] >= 0)[0]
    w = np.zeros(len(records), F)
    if len(hit):
        w[hit] = winding_over_instances(members, scene_of_instance, W, points_of(points)[hit], beta)[0]
    return WR.winding_signed(records, w), records, inst
