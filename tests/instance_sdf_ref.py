"""Restatement of the instanced signed distance query (include/shader_ray_instance_sdf.h), for the tests.

It composes three restatements and adds nothing of its own but the last rule:
  1. the closest part is instance_point_ref.closest_over_instances: world records and instances;
  2. the object point is instance_ref.object_vectors on the set's W (row by row, nonzero entries only, left to right, the
     translation last if it is nonzero);
  3. the object sign is sdf_ref.signed of point_query_ref.closest at {p_o, +inf} on the member's positions, with
     sdf_ref.derive's sign data;
  4. the value is -sqrt(world dist2) when that sign is negative and the world dist2 is above 0, else +sqrt(world dist2), NaN on
     a miss.

signed_with_world_normals is the variant the tests show to be wrong: the sign taken in world space from the world record's
own feature, with the member's pseudonormal carried to the world like a normal (by the inverse transpose of the map).
"""
from __future__ import annotations

import numpy as np

import instance_point_ref as IP
import instance_ref as IR
import point_query_ref as R
import sdf_ref as S

F = np.float32


def object_points(W, p):
    """p [n, 3] through one W [3, 4] by the object ray's rule: float32 [n, 3]"""
    with np.errstate(all="ignore"):
        return IR.object_vectors(W, p, True)


def object_sign(positions, sign_data, p_o):
    """shray_signed_distance's value on one member for the points {p_o, +inf}: float32 [n], NaN for a non-finite p_o"""
    pts = np.zeros(len(p_o), R.POINT_DTYPE)
    pts["p"], pts["max_dist2"] = p_o, np.inf
    return S.signed(pts, R.closest(positions, pts), sign_data), pts


def signed_over_instances(scene_positions, scene_of_instance, maps, W, points, device=None, sign_data=None):
    """The header's answer: (float32 values, CLOSEST_DTYPE records, int32 instances).  scene_positions, scene_of_instance, maps
    and points as for instance_point_ref.closest_over_instances; W [n, 3, 4] is the set's world-to-object floats (on the GPU:
    InstanceSet.world_to_object()); sign_data, when given, is one sdf_ref.derive(...)["sign_data"] per distinct scene."""
    records, inst = IP.closest_over_instances(scene_positions, scene_of_instance, maps, points, device=device)
    if sign_data is None:
        sign_data = [S.derive(p)["sign_data"] for p in scene_positions]
    W = np.asarray(W, F).reshape(-1, 3, 4)
    p = np.ascontiguousarray(np.asarray(points["p"], F))
    with np.errstate(all="ignore"):
        d = np.sqrt(records["dist2"].astype(F))
    out = np.where(inst >= 0, d, F(np.nan)).astype(F)
    for i in sorted(set(inst[inst >= 0].tolist())):
        at = np.nonzero(inst == i)[0]
        s = scene_of_instance[i]
        sigma, _ = object_sign(scene_positions[s], sign_data[s], object_points(W[i], p[at]))
        with np.errstate(invalid="ignore"):
            inside = (sigma < F(0)) & (records["dist2"][at] > F(0))
        out[at] = np.where(inside, -d[at], d[at])
    return out, records, inst


def signed_with_world_normals(scene_positions, scene_of_instance, maps, points, sign_data=None):
    """The wrong variant: sigma = dot(p - q, N_w) in world space, with N_w the member's pseudonormal of the WORLD record's
    (triangle, region) carried to the world by the inverse transpose of the map's linear part (in float64)."""
    records, inst = IP.closest_over_instances(scene_positions, scene_of_instance, maps, points)
    if sign_data is None:
        sign_data = [S.derive(p)["sign_data"] for p in scene_positions]
    maps = np.asarray(maps, np.float64).reshape(-1, 3, 4)
    p = np.asarray(points["p"], np.float64)
    d = np.sqrt(records["dist2"].astype(np.float64))
    out = np.where(inst >= 0, d, np.nan)
    for i in sorted(set(inst[inst >= 0].tolist())):
        at = np.nonzero(inst == i)[0]
        region = records["region"][at]
        slot = np.where(region == 6, 0, region + 1)
        n_o = sign_data[scene_of_instance[i]][records["triangle"][at], slot].astype(np.float64)
        n_w = n_o @ np.linalg.inv(maps[i][:, :3])            # rows: (A^-T n)^T = n^T A^-1
        sigma = ((p[at] - records["q"][at].astype(np.float64)) * n_w).sum(1)
        out[at] = np.where((sigma < 0) & (records["dist2"][at] > 0), -d[at], d[at])
    return out.astype(F), records, inst
