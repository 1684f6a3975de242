"""Restatement of the instanced signed distance query (include/shader_ray_instance_sdf.h), for the tests.

It composes three restatements and adds nothing of its own but the last rule:
  1. the closest part is instance_point_ref.closest_over_instances: world records and instances;
  2. the object point is instance_ref.object_vectors on the set's W (row by row, nonzero entries only, left to right, the
     translation last if it is nonzero);
  3. the object sign is sdf_ref.signed of point_query_ref.closest at {p_o, +inf} on the member's positions, with
     sdf_ref.derive's sign data;
  4. the value is -sqrt(world dist2) when that sign is negative and the world dist2 is above 0, else +sqrt(world dist2), NaN on
     a miss.

signed_parts gives the intermediate results of those steps per point, and values_of applies rule 4 to them with the
pseudonormal of a chosen (triangle, slot); with object_slots that is signed_over_instances' answer (the CPU tests pin it).

signed_with_world_normals is the variant the tests show to be wrong: the sign taken in world space from the world record's
own feature, with the member's pseudonormal carried to the world like a normal (by the inverse transpose of the map).
WRONG_VARIANTS are six more, each the header's rule with another pseudonormal slot read.
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


def object_closest(positions, p_o, device=None):
    """(the points {p_o, +inf}, their closest-point records on one member); brute force on `device` through torch when given"""
    pts = np.zeros(len(p_o), R.POINT_DTYPE)
    pts["p"], pts["max_dist2"] = p_o, np.inf
    return pts, (R.closest(positions, pts) if device is None else R.closest_torch(positions, pts, device=device))


def object_sign(positions, sign_data, p_o, device=None):
    """shray_signed_distance's value on one member for the points {p_o, +inf}: float32 [n], NaN for a non-finite p_o"""
    pts, records = object_closest(positions, p_o, device)
    return S.signed(pts, records, sign_data), pts


def signed_parts(scene_positions, scene_of_instance, maps, W, points, device=None, sign_data=None, closest=None):
    """The intermediate results of the header's answer, per point, as a dict: "records" and "instances" (step 1), "d" (sqrtf of
    the world dist2), "scene" (the member scene of the hit's instance, -1 on a miss), "p_o" (step 2, float32 [n, 3]),
    "object" (step 3's CLOSEST_DTYPE records of {p_o, +inf} on the member; triangle -1 on a miss or for a non-finite p_o) and
    "sign_data" (one [T, 7, 3] per distinct scene).  Arguments as for signed_over_instances; `closest`, when given, is step 1's
    (records, instances), already restated."""
    records, inst = closest if closest is not None else IP.closest_over_instances(scene_positions, scene_of_instance, maps, points, device=device)
    if sign_data is None:
        sign_data = [S.derive(p)["sign_data"] for p in scene_positions]
    W = np.asarray(W, F).reshape(-1, 3, 4)
    p = np.ascontiguousarray(np.asarray(points["p"], F))
    n = len(p)
    with np.errstate(all="ignore"):
        d = np.sqrt(records["dist2"].astype(F))
    p_o = np.full((n, 3), np.nan, F)
    obj = np.zeros(n, R.CLOSEST_DTYPE)
    obj["triangle"], obj["region"] = R.HIT_MISS, R.REGION_NONE
    scene = np.full(n, -1, np.int64)
    for i in sorted(set(inst[inst >= 0].tolist())):
        at = np.nonzero(inst == i)[0]
        scene[at] = scene_of_instance[i]
        p_o[at] = object_points(W[i], p[at])
        obj[at] = object_closest(scene_positions[scene_of_instance[i]], p_o[at], device)[1]
    return dict(records=records, instances=inst, d=d, scene=scene, p_o=p_o, object=obj, sign_data=sign_data)


def object_slots(parts):
    """(triangle, slot) of the pseudonormal the header reads for each point: the OBJECT record's triangle and region"""
    region = parts["object"]["region"]
    return parts["object"]["triangle"], np.where(region == R.REGION_FACE, 0, region + 1)


def sigma_of(parts, triangle, slot):
    """dot(p_o - q_o, N) with N the sign data's [triangle, slot] of each point's member scene: float32 [n], NaN where the point
    has no object record"""
    obj = parts["object"]
    ok = (obj["triangle"] >= 0) & (np.asarray(triangle) >= 0)
    nrm = np.zeros((len(obj), 3), F)
    for s in sorted(set(parts["scene"][ok].tolist())):
        at = np.nonzero(ok & (parts["scene"] == s))[0]
        nrm[at] = parts["sign_data"][s][np.asarray(triangle)[at], np.clip(np.asarray(slot)[at], 0, 6)]
    with np.errstate(all="ignore"):
        sigma = S._dot(parts["p_o"] - obj["q"], nrm)
    return np.where(ok, sigma, F(np.nan)).astype(F)


def values_of(parts, pick=object_slots):
    """the header's rule 4 on the intermediate results, with the pseudonormal that `pick` selects: float32 values.  With
    object_slots it is signed_over_instances' answer."""
    triangle, slot = pick(parts)
    sigma = sigma_of(parts, triangle, slot)
    d = parts["d"]
    with np.errstate(invalid="ignore"):
        inside = (sigma < F(0)) & (parts["object"]["dist2"] > F(0)) & (parts["records"]["dist2"] > F(0))
    return np.where(parts["instances"] >= 0, np.where(inside, -d, d), F(np.nan)).astype(F)


def signed_over_instances(scene_positions, scene_of_instance, maps, W, points, device=None, sign_data=None):
    """The header's answer: (float32 values, CLOSEST_DTYPE records, int32 instances).  scene_positions, scene_of_instance, maps
    and points as for instance_point_ref.closest_over_instances; W [n, 3, 4] is the set's world-to-object floats (on the GPU:
    InstanceSet.world_to_object()); sign_data, when given, is one sdf_ref.derive(...)["sign_data"] per distinct scene; with
    `device` both brute forces (the world one and the members' object ones) run there through torch."""
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
        sigma, _ = object_sign(scene_positions[s], sign_data[s], object_points(W[i], p[at]), device)
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


# The variants the tests show to be wrong, each a `pick` for values_of: a kernel that read another pseudonormal than the
# header's.  tests/instance_sdf_cases.py measures how many values of its points each one changes.
def _remap(table):
    table = np.asarray(table)

    def pick(parts):
        triangle, slot = object_slots(parts)
        return triangle, table[np.clip(slot, 0, 6)]
    return pick


def _world_feature(parts):
    region = parts["records"]["region"]
    return parts["records"]["triangle"], np.where(region == R.REGION_FACE, 0, region + 1)


#                                          face a  b  c  AB AC BC
WRONG_VARIANTS = {
    "face normal for every region": _remap([0, 0, 0, 0, 0, 0, 0]),
    "vertex a for every vertex": _remap([0, 1, 1, 1, 4, 5, 6]),
    "AC and BC swapped": _remap([0, 1, 2, 3, 4, 6, 5]),
    "edge slots shifted by one": _remap([0, 1, 2, 3, 5, 6, 4]),
    "the world record's (triangle, region)": _world_feature,
    "b and c swapped": _remap([0, 1, 3, 2, 4, 5, 6]),
}
