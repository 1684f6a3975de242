"""CPU restatement of the instanced all-hits ray query (include/shader_ray_instance_multihit.h), for the tests.

The contract over the two restatements it composes.  For a set of N instances and one world ray with tmax > 0 (else: no
walk, zero crossings):
  - the object ray of instance i is instance_ref.object_rays with the set's W[i]; tmax is not transformed;
  - S_i is multi_hit_ref.crossings of that object ray on instance i's scene;
  - S is the union over i of {(t, u, v, triangle, i)} for the members of S_i;
  - the key is (t as a float comparison, instance index, triangle index).
Output per ray: n = |S|; K records and K instance indices holding the min(n, K) members with the smallest keys in ascending
key order, the remaining slots {tmax, 0, 0, HIT_MISS} with instance -1.
"""
from __future__ import annotations

import numpy as np

import instance_ref as I
import multi_hit_ref as M
import ray_query_ref as R

F = np.float32


def crossings(scenes, W, origins, directions, tmax, max_leaf_tests: int = 10):
    """The union S of every ray, unsorted: (ray, t, u, v, triangle, instance) arrays over all members, the walks' counters
    summed over every (ray, instance) pair (no top-level cull), nan_candidate [n] (some instance's walk met one) and
    per_instance [N, n]: the crossing count of each instance.  scenes[i] is instance i's scene (arrays or SceneArrays; an
    object may repeat), W [N, 3, 4] the set's world-to-object maps."""
    P = np.asarray(origins, F).reshape(-1, 3)
    D = np.asarray(directions, F).reshape(-1, 3)
    n = len(P)
    tmax = np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
    W = np.asarray(W, F).reshape(-1, 3, 4)
    assert len(W) == len(scenes)
    arrays = {}
    walked = {}
    parts = [[] for _ in range(6)]
    counters = {k: 0 for k in R.COUNTER_NAMES}
    nan_candidate = np.zeros(n, bool)
    per_instance = np.zeros((len(scenes), n), np.int64)
    for i, (scene, w) in enumerate(zip(scenes, W)):
        if id(scene) not in arrays:
            arrays[id(scene)] = scene if isinstance(scene, R.SceneArrays) else R.SceneArrays(scene)
        key = (id(scene), w.tobytes())           # an exact duplicate walks the same rays: the same crossings
        if key not in walked:
            o, d = I.object_rays(w, P, D)
            walked[key] = M.crossings(arrays[id(scene)], o, d, tmax, max_leaf_tests)
        ray, t, u, v, tri, c, nan, _ = walked[key]
        for lst, a in zip(parts, (ray, t, u, v, tri, np.full(len(ray), i, np.int64))):
            lst.append(a)
        for k in counters:
            counters[k] += c[k]
        nan_candidate |= nan
        per_instance[i] = np.bincount(ray, minlength=n)
    ray, t, u, v, tri, inst = (np.concatenate(p) for p in parts)
    return ray, t, u, v, tri, inst, counters, nan_candidate, per_instance, tmax


def first_k(ray, t, u, v, tri, inst, tmax, max_hits: int):
    """The first max_hits members of every ray's union by the key, from the members as flat arrays in any order:
    (hits: HIT_DTYPE [n, max_hits], instances: int32 [n, max_hits]); the other slots {tmax, 0, 0, HIT_MISS} with instance -1."""
    n = len(tmax)
    held = np.bincount(ray, minlength=n)
    hits = np.zeros((n, max_hits), R.HIT_DTYPE)
    hits["t"] = np.asarray(tmax, F)[:, None]
    hits["triangle"] = R.HIT_MISS
    instances = np.full((n, max_hits), -1, np.int32)
    order = np.lexsort((tri, inst, t, ray))      # by ray, then t (a float comparison: -0 == +0), the instance, the triangle
    ray, t, u, v, tri, inst = (a[order] for a in (ray, t, u, v, tri, inst))
    first = np.concatenate([[0], np.cumsum(held)[:-1]])
    rank = np.arange(len(ray)) - first[ray]
    keep = rank < max_hits
    for field, a in (("t", t), ("u", u), ("v", v), ("triangle", tri)):
        hits[field][ray[keep], rank[keep]] = a[keep]
    instances[ray[keep], rank[keep]] = inst[keep]
    return hits, instances


def all_hits(scenes, W, origins, directions, tmax, max_hits: int = 8, max_leaf_tests: int = 10, details: bool = False):
    """(hits: HIT_DTYPE [n, max_hits], instances: int32 [n, max_hits], counts: int32 [n], counters: dict); with
    details=True also nan_candidate [n] and per_instance [N, n]."""
    ray, t, u, v, tri, inst, counters, nan_candidate, per_instance, tmax = crossings(scenes, W, origins, directions, tmax, max_leaf_tests)
    counts = np.bincount(ray, minlength=len(tmax)).astype(np.int32)
    hits, instances = first_k(ray, t, u, v, tri, inst, tmax, max_hits)
    return (hits, instances, counts, counters, nan_candidate, per_instance) if details else (hits, instances, counts, counters)


def held_members(hits, instance: int):
    """the held records of one instance's own answer (HIT_DTYPE [n, K']) as first_k's flat arrays"""
    r, s = np.nonzero(hits["triangle"] >= 0)
    return (r.astype(np.int64), hits["t"][r, s], hits["u"][r, s], hits["v"][r, s], hits["triangle"][r, s].astype(np.int64),
            np.full(len(r), instance, np.int64))


def merge(per_instance_hits, per_instance_counts, tmax, max_hits: int):
    """The same merge over per-instance answers that are already cut at some K' (Scene.trace_all_hits on the object rays):
    per_instance_hits[i] HIT_DTYPE [n, K'], per_instance_counts[i] int32 [n].  Exact for the first max_hits <= K' wherever
    no instance crosses more than K' (the caller checks that).  Returns (hits, instances, counts)."""
    n = len(per_instance_counts[0])
    tmax = np.broadcast_to(np.asarray(tmax, F), (n,))
    parts = [held_members(h, i) for i, h in enumerate(per_instance_hits)]
    ray, t, u, v, tri, inst = (np.concatenate(p) for p in zip(*parts))
    hits, instances = first_k(ray, t, u, v, tri, inst, tmax, max_hits)
    return hits, instances, np.sum(per_instance_counts, axis=0).astype(np.int32)
