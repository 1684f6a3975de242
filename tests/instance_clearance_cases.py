"""The set and the queries of the instanced triangle-distance tests (tests/test_gpu_instance_clearance.py), made without a
device so that what they cover can be checked on the restatement alone (tests/test_instance_clearance_reference.py).

The set is instance_near_cases.nine_instances (seven placements of lobed_528, one an exact duplicate, and the two tiny scenes).
The queries are clearance_cases.make_queries over the merged scene's positions: near, far, crossing, own, point, segment and
bad triangles, 600 of them, seed 21.  max_dist2 is (4 % of the typical world diagonal of an instance)^2.  assert_mixed states
what the set must cover at K = 64."""
from __future__ import annotations

import numpy as np

import clearance_cases as CC
import instance_near_cases as NC
import instance_point_ref as IP
import intersect_ref as IR

F = np.float32
FLOOR = 0.04
QUERIES, QUERY_SEED = 600, 21
PAIR_INTERSECTING = 15

nine_instances = NC.nine_instances


def mid_value(scene_positions, scene_of_instance, maps):
    """(4 % of the typical world diagonal)^2, as a float32"""
    return F((0.04 * NC.typical_diagonal(scene_positions, scene_of_instance, maps)) ** 2)


def world_queries(scene_positions, scene_of_instance, maps, n=QUERIES, seed=QUERY_SEED):
    """float32 [n, 3, 3] world query triangles of every kind over the merged scene"""
    merged, _ = IP.merged_positions(scene_positions, scene_of_instance, maps)
    return CC.make_queries(merged, n, seed)


def shares(queries, max_dist2, records, instances, counts) -> dict:
    """what assert_mixed measures, on the restatement's K = 64 answer"""
    with np.errstate(invalid="ignore"):
        walked = np.isfinite(IR.corners_of(queries)).all((1, 2)) & bool(F(max_dist2) >= 0)
    held = instances >= 0
    spans = np.array([len(set(row[h].tolist())) for row, h in zip(instances, held)])
    d = records["dist2"]
    tie = (held[:, 1:] & held[:, :-1] & (d[:, 1:] == d[:, :-1]) & (instances[:, 1:] != instances[:, :-1])).any(1)
    return {"count 0, walked": float((walked & (counts == 0)).mean()),
            "count 1 to 8": float(((counts >= 1) & (counts <= 8)).mean()),
            "count 9 to 64": float(((counts >= 9) & (counts <= 64)).mean()),
            "count above 64": float((counts > 64).mean()),
            "two or more instances held": float((spans >= 2).mean()),
            "adjacent records tie across instances": float(tie.mean()),
            "an intersecting record held": float((held & (records["feature"] == PAIR_INTERSECTING)).any(1).mean())}


def assert_mixed(queries, max_dist2, records, instances, counts, what):
    """over 4 % of the queries in each count band, with records of two or more instances, with two adjacent held records of
    equal dist2 on different instances, and with a feature-15 record (a floor that keeps a class from going uncovered, not a
    measurement)"""
    assert records.shape[1] == 64
    s = shares(queries, max_dist2, records, instances, counts)
    low = {k: v for k, v in s.items() if v <= FLOOR}
    assert not low, f"{what}: at or under {FLOOR:.0%} of {len(queries)} queries: {low} (all: {s})"
    return s
