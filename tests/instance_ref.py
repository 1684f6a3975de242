"""CPU restatement of the instanced query (include/shader_ray_instance.h), for the tests.

Two rules over the ray query's own (tests/ray_query_ref.py):
- the object ray: row r of W applied to a vector adds the products W[r][c] * v[c] left to right in float32, skipping the
  entries where W[r][c] == 0; for the origin, W[r][3] is added last if it is nonzero;
- the composition: the hit with the smallest t over all instances, the lowest instance on equal t; a miss is
  (t = tmax, u = v = 0, SHRAY_HIT_MISS, instance -1), a capped walk ends the ray (SHRAY_HIT_CAP, instance -1).
"""
from __future__ import annotations

import numpy as np

import ray_query_ref as R

F = np.float32


def object_vectors(W, v, translate: bool) -> np.ndarray:
    """v [n, 3] float32 through one W [3, 4] (translate: add its column 3 too), the library's operation order."""
    W = np.asarray(W, F).reshape(3, 4)
    v = np.asarray(v, F).reshape(-1, 3)
    out = np.zeros_like(v)
    for r in range(3):
        acc = None
        for c in range(3):
            if W[r, c] != 0:
                prod = W[r, c] * v[:, c]
                acc = prod if acc is None else acc + prod
        if translate and W[r, 3] != 0:
            acc = np.full(len(v), W[r, 3], F) if acc is None else acc + W[r, 3]
        out[:, r] = np.zeros(len(v), F) if acc is None else acc
    return out


def object_rays(W, origins, directions):
    """(origins, directions) in the object space of an instance with world-to-object map W [3, 4]"""
    return object_vectors(W, origins, True), object_vectors(W, directions, False)


def compose(per_instance, tmax):
    """per_instance: a list of HIT_DTYPE arrays, one per instance in index order, each the ray query's closest hits of the
    object rays.  Returns (hits HIT_DTYPE, instances int32) by the composition rule."""
    n = len(np.atleast_1d(tmax))
    tmax = np.broadcast_to(np.asarray(tmax, F), (n,))
    hits = np.zeros(n, R.HIT_DTYPE)
    hits["t"] = tmax
    hits["triangle"] = R.HIT_MISS
    inst = np.full(n, -1, np.int32)
    capped = np.zeros(n, bool)
    for i, h in enumerate(per_instance):
        capped |= h["triangle"] == R.HIT_CAP
        # strictly closer, or the first (lowest) instance to reach this t
        better = (h["triangle"] >= 0) & ((inst < 0) | (h["t"] < hits["t"]))
        hits[better] = h[better]
        inst[better] = i
    hits["t"][capped] = F(-1)
    hits["u"][capped] = 0
    hits["v"][capped] = 0
    hits["triangle"][capped] = R.HIT_CAP
    inst[capped] = -1
    return hits, inst


def trace(scenes, W, origins, directions, tmax, **kw):
    """The composition over instances: scenes[i] (ray_query_ref.SceneArrays) placed by world-to-object W[i]."""
    per = []
    for sc, w in zip(scenes, W):
        o, d = object_rays(w, origins, directions)
        per.append(R.trace(sc, o, d, tmax, **kw)[0])
    return compose(per, tmax)


def world_to_object(object_to_world) -> np.ndarray:
    """W as the header defines it: the double inverse, rounded to float32 ([n, 3, 4]).  (The library's own inversion may round
    an entry the other way; GPU tests read its W back with InstanceSet.world_to_object.)"""
    m = np.asarray(object_to_world, np.float64).reshape(-1, 3, 4)
    A, b = m[:, :, :3], m[:, :, 3:]
    inv = np.linalg.inv(A)
    return np.concatenate([inv, -inv @ b], axis=2).astype(F)
