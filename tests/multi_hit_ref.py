"""CPU restatement of the all-hits ray query (include/shader_ray_multihit.h), for the tests.

The contract, verbatim from the header.  Rays are shray_ray, hits are shray_hit; arithmetic is the ray query's
(tests/ray_query_ref.py: the shader's range_intersect_box with true IEEE divisions over [0, 1e8], the shader's
triangle_intersect, fp32, no FMA contraction).

For one ray with tmax > 0 (else: no walk, zero hits), let B = tmax.  The crossing set S is defined without reference to any
visit order:
  - A node is entered iff its parent is entered (the root always is) and its own slab range satisfies
    !(r0 >= r1) && r0 < B.  These are exactly `enter` in ray_query_ref.trace with t held at tmax and never lowered.
  - A triangle at position j < max_leaf_tests of an entered leaf is in S iff the shader's test accepts it with bound B and
    that leaf's r0, r1 (the `ok` of ray_query_ref.trace) and dist < tmax (the ray query's report rule; it also drops the NaN
    candidates that the comparison chain lets through).
  - Its record is {t = dist, u, v, triangle}.
Output per ray: n = |S|; K records, the min(n, K) members of S with the smallest keys sorted ascending by (t as a float
comparison, then triangle index), the remaining slots {tmax, 0, 0, HIT_MISS}.

The walk below is ray_query_ref.trace's threaded walk (which visits exactly the children of entered nodes) with the bound
held at tmax; the counters are that walk's.
"""
from __future__ import annotations

import numpy as np

import ray_query_ref as R
from ray_query_ref import DET_EPS, HIT_DTYPE, HIT_MISS, RANGE_MAX, TERMINATOR, SceneArrays, _cross, _dot, _sel_max, _sel_min

F = np.float32
MULTIHIT_MAX = 64


def slab_range(boxmin, boxmax, P, D):
    """range_intersect_box over [0, 1e8] of boxes [m, 3] for rays [m, 3]: (r0, r1)"""
    r0 = np.zeros(len(P), F)
    r1 = np.full(len(P), RANGE_MAX)
    with np.errstate(all="ignore"):
        for a in range(3):
            o, d = P[:, a], D[:, a]
            ta = (boxmin[:, a] - o) / d
            tb = (boxmax[:, a] - o) / d
            forward = d >= 0
            r0 = _sel_max(r0, np.where(forward, ta, tb))
            r1 = _sel_min(r1, np.where(forward, tb, ta))
    return r0, r1


def crossings(scene, origins, directions, tmax, max_leaf_tests: int = 10):
    """The crossing set of every ray, unsorted: (ray, t, u, v, triangle) arrays over all members, the walk's counters, and
    nan_candidate [n]: the ray met a candidate that passed the comparison chain with a NaN dist (dropped from S)."""
    sc = scene if isinstance(scene, SceneArrays) else SceneArrays(scene)
    P = np.asarray(origins, F).reshape(-1, 3)
    D = np.asarray(directions, F).reshape(-1, 3)
    n = len(P)
    tmax = np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
    counts = {k: 0 for k in R.COUNTER_NAMES}
    traced = tmax > 0
    counts["traversals"] = int(traced.sum())
    code = ((D[:, 0] > 0).astype(np.int64) + 2 * (D[:, 1] > 0) + 4 * (D[:, 2] > 0))
    g = np.full(n, sc.root)
    active = np.nonzero(traced)[0]
    found = [[] for _ in range(5)]
    nan_candidate = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        while len(active):
            r = active
            counts["node_visits"] += len(r)
            node = g[r].astype(np.int64)
            hit_next = sc.hitmiss[code[r], node, 0]
            miss_next = sc.hitmiss[code[r], node, 1]
            leaf = hit_next == miss_next
            counts["leaf_visits"] += int(leaf.sum())
            start = np.where(leaf, sc.objects[node, 0], F(0))
            count = np.where(leaf, sc.objects[node, 1], F(0))
            r0, r1 = slab_range(sc.boxmin[node], sc.boxmax[node], P[r], D[r])
            enter = ~(r0 >= r1) & (r0 < tmax[r])
            in_leaf = np.nonzero(enter & leaf)[0]
            for j in range(max_leaf_tests):
                k = in_leaf[F(j) < count[in_leaf]]
                if not len(k):
                    break
                counts["triangle_tests"] += len(k)
                rr = r[k]
                tri = (start[k] + F(j)).astype(np.int64)
                v0, v1, v2 = (sc.positions[tri, m].T for m in range(3))
                e0 = tuple(v1[a] - v0[a] for a in range(3))
                e1 = tuple(v0[a] - v2[a] for a in range(3))
                Dk = tuple(D[rr, a] for a in range(3))
                M = _cross(e1, Dk)
                det = _dot(e0, M)
                ok = ~((det > -DET_EPS) & (det < DET_EPS))
                inv_det = F(1) / det
                T = tuple(P[rr, a] - v0[a] for a in range(3))
                Q = _cross(T, e0)
                dist = -_dot(e1, Q) * inv_det
                ok &= ~((dist > tmax[rr]) | (dist < r0[k]) | (dist > r1[k]))
                u = _dot(T, M) * inv_det
                ok &= ~((u < 0) | (u > 1))
                w = _dot(Dk, Q) * inv_det
                ok &= ~((w < 0) | (u + w > 1))
                nan_candidate[rr[ok & np.isnan(dist)]] = True
                ok &= dist < tmax[rr]
                for lst, a in zip(found, (rr, dist, u, w, tri)):
                    lst.append(a[ok])
            g[r] = np.where(enter, hit_next, miss_next)
            active = r[~(g[r] >= TERMINATOR)]
    ray, t, u, v, tri = (np.concatenate(lst) if lst else np.zeros(0, dt) for lst, dt in zip(found, (np.int64, F, F, F, np.int64)))
    return ray.astype(np.int64), t.astype(F), u.astype(F), v.astype(F), tri.astype(np.int64), counts, nan_candidate, tmax


def all_hits(scene, origins, directions, tmax, max_hits: int = 8, max_leaf_tests: int = 10, details: bool = False):
    """(hits: HIT_DTYPE [n, max_hits], counts: int32 [n], counters: dict); with details=True also nan_candidate [n]."""
    ray, t, u, v, tri, counters, nan_candidate, tmax = crossings(scene, origins, directions, tmax, max_leaf_tests)
    n = len(tmax)
    counts = np.bincount(ray, minlength=n).astype(np.int32)
    hits = np.zeros((n, max_hits), HIT_DTYPE)
    hits["t"] = tmax[:, None]
    hits["triangle"] = HIT_MISS
    order = np.lexsort((tri, t, ray))          # by ray, then t (a float comparison: -0 == +0), then the triangle index
    ray, t, u, v, tri = ray[order], t[order], u[order], v[order], tri[order]
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rank = np.arange(len(ray)) - first[ray]
    keep = rank < max_hits
    for field, a in (("t", t), ("u", u), ("v", v), ("triangle", tri)):
        hits[field][ray[keep], rank[keep]] = a[keep]
    return (hits, counts, counters, nan_candidate) if details else (hits, counts, counters)


# small meshes of the reference test, also traced on the GPU: (positions float32 [V, 3], triangles int32 [T, 3])
def square(z, half=1.0, base=0):
    pos = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], F)
    return pos, np.array([[0, 1, 2], [0, 2, 3]], np.int32) + base


def stack_of_squares():
    """five parallel squares at z = 0, 1, 2, 3, 4, two triangles each, split along the diagonal x = y"""
    parts = [square(float(z), base=4 * z) for z in range(5)]
    return np.concatenate([p for p, _ in parts]), np.concatenate([t for _, t in parts])


def closed_cube():
    import sdf_ref
    return sdf_ref.cube()


def coincident():
    """one triangle listed twice, and a third one behind them"""
    pos = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 1], [2, 0, 1], [0, 2, 1]], F)
    return pos, np.array([[0, 1, 2], [0, 1, 2], [3, 4, 5]], np.int32)


def tall_stack():
    """80 parallel squares 0.1 apart, every seventh level listed three times (coincident): an axial ray crosses 104 triangles,
    more than any K holds, with ties of three at equal t"""
    parts, base = [], 0
    for level in range(80):
        for _ in range(3 if level % 7 == 0 else 1):
            parts.append(square(F(level) * F(0.1), base=base))
            base += 4
    return np.concatenate([p for p, _ in parts]), np.concatenate([t for _, t in parts])


def axial_rays(n, seed):
    """rays for tall_stack: from below, above and inside the stack, along +-z exactly (with +-0 components) or tilted a
    little; tmax 1e7, +inf, or somewhere inside the stack: (origins, directions, tmax)"""
    rng = np.random.default_rng(seed)
    o = np.empty((n, 3), F)
    o[:, :2] = (rng.random((n, 2)) * 1.9 - 0.95).astype(F)
    where = rng.integers(0, 3, n)
    o[:, 2] = np.where(where == 0, -1.0, np.where(where == 1, 9.0, rng.random(n) * 7.9)).astype(F)
    up = np.where(where == 0, 1.0, np.where(where == 1, -1.0, np.where(rng.random(n) < 0.5, 1.0, -1.0)))
    d = np.empty((n, 3), F)
    d[:, :2] = (rng.normal(size=(n, 2)) * 0.02).astype(F)
    d[:, 2] = up
    exact = rng.random(n) < 0.3
    d[exact, :2] = np.where(rng.random((int(exact.sum()), 2)) < 0.5, F(0.0), F(-0.0))
    tmax = np.full(n, F(1e7))
    r = rng.random(n)
    tmax[r < 0.2] = np.inf
    cut = (r >= 0.2) & (r < 0.5)
    tmax[cut] = (rng.random(int(cut.sum())) * 9).astype(F)
    return o, d, tmax


MESHES = ("stack_of_squares", "closed_cube", "coincident")
DEEP_MESHES = ("tall_stack",)        # more crossings per ray than SHRAY_MULTIHIT_MAX


def write_mesh(pkg, path, name):
    pos, tri = globals()[name]()
    pkg.scenes.write_trisrc(path, pos, tri, normals=np.tile(np.array([0, 0, 1], F), (len(pos), 1)))
    return path
