"""The sets and points of the instanced within-radius tests (tests/test_gpu_instance_near.py), made without a device so that
what they cover can be checked on the restatement alone (tests/test_instance_near_reference.py).

The sets are instance_point_cases.make_set's.  The points are instance_point_cases.world_points', and every even-indexed point
of radius class 1 (a finite radius) gets a wider one, max_dist2 = ((0.02 + 0.3 r^2) typical)^2 with r uniform and `typical`
the median world diagonal of the instances, so that many points have more pairs within their radius than any K kept and many
hold records of more than one instance.  assert_mixed states what the nine-instance set must cover at K = 64."""
from __future__ import annotations

import numpy as np

import instance_point_cases as IC
import instance_point_ref as IP

F = np.float32
NINE = ["lobed_528"] * 7 + ["one triangle", "11-triangle leaf"]
NINE_SEED, NINE_SPREAD, NINE_POINTS, NINE_POINT_SEED = 11, 1.5, 1536, 12
FLOOR = 0.04


def typical_diagonal(scene_positions, scene_of_instance, maps) -> float:
    sizes = []
    for i, s in enumerate(scene_of_instance):
        w = IP.map_corners(maps[i], scene_positions[s]).astype(np.float64)
        sizes.append(np.linalg.norm(w.max(0) - w.min(0)))
    return float(np.median(sizes))


def world_points(scene_positions, scene_of_instance, maps, n, seed):
    """(POINT_DTYPE points, kind per point, radius class per point): module doc"""
    pts, kind, radius = IC.world_points(scene_positions, scene_of_instance, maps, n, seed)
    r = np.random.default_rng(seed + 1).random(n)
    typical = typical_diagonal(scene_positions, scene_of_instance, maps)
    wide = (radius == 1) & (np.arange(n) % 2 == 0)
    pts["max_dist2"][wide] = (((0.02 + 0.3 * r[wide] ** 2) * typical) ** 2).astype(F)
    return pts, kind, radius


def nine_instances(positions_of):
    """(distinct scenes' positions, scene of every instance, maps, kinds, names) of the nine-instance set; positions_of(name) is
    a member's vertex_positions"""
    distinct = ["lobed_528", "one triangle", "11-triangle leaf"]
    positions = [np.asarray(positions_of(name), F).reshape(-1) for name in distinct]
    of, maps, kinds = IC.make_set(positions, [distinct.index(x) for x in NINE], seed=NINE_SEED, spread=NINE_SPREAD)
    return positions, of, maps, kinds, [distinct[s] for s in of]


def shares(points, radius, records, instances, counts) -> dict:
    """what assert_mixed measures, on the restatement's K = 64 answer"""
    walked = np.isfinite(points["p"]).all(1) & (points["max_dist2"] >= 0)
    held = instances >= 0
    spans = np.array([len(set(row[h].tolist())) for row, h in zip(instances, held)])
    d = records["dist2"]
    with np.errstate(invalid="ignore"):
        tie = (held[:, 1:] & held[:, :-1] & (d[:, 1:] == d[:, :-1]) & (instances[:, 1:] != instances[:, :-1])).any(1)
    return {"count 0, walked": float((walked & (counts == 0)).mean()),
            "count 1 to 8": float(((counts >= 1) & (counts <= 8)).mean()),
            "count 9 to 64": float(((counts >= 9) & (counts <= 64)).mean()),
            "count above 64": float((counts > 64).mean()),
            "finite radius, two or more instances held": float(((radius == 1) & (spans >= 2)).mean()),
            "adjacent records tie across instances": float(tie.mean())}


def assert_mixed(points, radius, records, instances, counts, what):
    """over 4 % of the points in each count band, with records of two or more instances under a finite radius, and with two
    adjacent held records of equal dist2 on different instances"""
    assert records.shape[1] == 64
    s = shares(points, radius, records, instances, counts)
    low = {k: v for k, v in s.items() if v <= FLOOR}
    assert not low, f"{what}: at or under {FLOOR:.0%} of {len(points)} points: {low} (all: {s})"
    return s
