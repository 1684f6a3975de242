"""The sets and query triangles of the instanced triangle-intersection tests (tests/test_gpu_instance_intersect.py), made
without a device so that what they cover can be checked on the restatement alone (tests/test_instance_intersect_reference.py).

The set is instance_near_cases.nine_instances: seven placed copies of lobed_528 (instance 4 an exact duplicate of instance 1)
and the two tiny scenes.  The queries are intersect_cases.make_queries on the merged scene (the mapped corners in instance
order): the merged scene's own triangles, moved copies of them, slicers small and large, and queries that are not walked.
assert_mixed states what they must cover.

General-position data leaves the in-plane axes 12 to 17 nothing to separate first, so intersect_cases.flat_lattice is also
placed three times by exact maps (the identity; a quarter turn about z with a translation; scale 2 with x mirrored and a
translation), with integer queries of which query j is mapped by map j mod 3: every world corner is an integer, and
intersect_cases.exact_intersects is the truth."""
from __future__ import annotations

import numpy as np

import instance_near_cases as NC
import instance_point_ref as IP
import intersect_cases as IC
import intersect_ref as IR

F = np.float32
NINE_QUERIES, NINE_QUERY_SEED = 768, 31
FLOOR = 0.04
LATTICE_QUERIES = 600

nine_instances = NC.nine_instances


def world_queries(scene_positions, scene_of_instance, maps, n=NINE_QUERIES, seed=NINE_QUERY_SEED):
    """float32 [n, 3, 3] world query triangles of every kind of intersect_cases, over the merged scene"""
    merged, _ = IP.merged_positions(scene_positions, scene_of_instance, maps)
    return IC.make_queries({"vertex_positions": merged}, n, seed)


def shares(queries, instances64, counts) -> dict:
    """what assert_mixed measures, on the restatement's K = 64 answer"""
    spans = lambda held: np.array([len(set(row[row >= 0].tolist())) for row in held])
    return {"n 0": float((counts == 0).mean()),
            "n 1 to 8": float(((counts >= 1) & (counts <= 8)).mean()),
            "n 9 to 64": float(((counts >= 9) & (counts <= 64)).mean()),
            "n above 64": float((counts > 64).mean()),
            "first 8 of two or more instances": float((spans(instances64[:, :8]) >= 2).mean()),
            "first 64 of two or more instances": float((spans(instances64) >= 2).mean())}


def assert_mixed(queries, instances64, counts, code, what):
    """over 4 % of the queries in each band of n and with held pairs of two or more instances among the first 8 and the first
    64; and nq, nt and each of the nine edge axes is the first to separate some pairs (`code`: intersect_ref.first_axis on the
    merged scene).  Returns the shares and the pairs each of the seventeen axes separates first."""
    assert instances64.shape[1] == 64
    s = shares(queries, instances64, counts)
    low = {k: v for k, v in s.items() if v <= FLOOR}
    assert not low, f"{what}: at or under {FLOOR:.0%} of {len(queries)} queries: {low} (all: {s})"
    per_axis = np.bincount(code[(code >= IR.AXIS0) & (code < IR.UNWALKED)].astype(np.int64) - IR.AXIS0, minlength=IR.AXES)
    assert min(per_axis[:11]) >= 1, (what, per_axis.tolist())
    s["first to separate, per axis"] = per_axis.tolist()
    return s


# ---- the placed lattice -----------------------------------------------------------------------------------------------------
def lattice_maps():
    """three exact maps [3, 3, 4]: the identity; a quarter turn about z with translation (20, 0, 0); scale 2 with x mirrored and
    translation (0, 30, 0).  Integer corners stay integers, exactly."""
    maps = np.zeros((3, 3, 4), F)
    maps[0, :, :3] = np.eye(3)
    maps[1, :, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    maps[1, :, 3] = (20, 0, 0)
    maps[2, :, :3] = np.diag([-2, 2, 2])
    maps[2, :, 3] = (0, 30, 0)
    return maps


def lattice_queries(seed, n=LATTICE_QUERIES):
    """float32 [n, 3, 3]: intersect_cases.flat_queries(n, seed), query j mapped by lattice map j mod 3"""
    q = IC.flat_queries(n, seed)
    maps = lattice_maps()
    out = np.empty_like(q)
    for m in range(3):
        out[m::3] = IP.map_corners(maps[m], q[m::3]).reshape(-1, 3, 3)
    assert np.array_equal(out, np.rint(out))
    return out


def placed_lattice():
    """(positions of the one scene, scene of every instance, maps)"""
    return [IC.flat_lattice().reshape(-1)], [0, 0, 0], lattice_maps()
