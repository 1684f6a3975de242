"""The query triangles of the triangle-distance tests (tests/test_gpu_clearance.py).  No test and no GPU in here.

make_queries mixes, over a scene's triangles: `near` (a scene triangle shrunk a little and lifted off the surface by up to 3 %
of the scene's extent: the clearance use), `far` (the same moved 2 to 50 extents away: the walk prunes nearly everything, or
with a count and max_dist2 = +inf nothing), `crossing` (intersect_cases' slicers through the mesh: the intersecting stage),
`own` (the scene's own triangles: dist2 0 with themselves and their neighbours, shared corners), `point` and `segment` (a point
or a segment passed as a triangle: served by the features alone), and `bad` (a NaN, +inf or -inf coordinate: not walked).
"""
import numpy as np

import intersect_cases as IC

F = np.float32
KINDS = ("near", "far", "crossing", "own", "point", "segment", "bad")
SHARES = (0.30, 0.12, 0.18, 0.15, 0.08, 0.09, 0.08)


def kinds(n, seed):
    return np.random.default_rng(seed + 13).choice(len(KINDS), n, p=SHARES)


def make_queries(positions, n, seed):
    """float32 [n, 3, 3] query triangles of every kind (module doc); kinds(n, seed) gives each one's kind"""
    rng = np.random.default_rng(seed)
    tris = np.asarray(positions, F).reshape(-1, 3, 3)
    extent = IC.scene_extent(positions)
    kind = kinds(n, seed)
    pick = rng.integers(0, len(tris), n)
    base = tris[pick].astype(np.float64)
    centre = base.mean(1, keepdims=True)
    way = rng.normal(size=(n, 1, 3))
    way /= np.linalg.norm(way, axis=2, keepdims=True)
    lifted = centre + (base - centre) * (0.5 + rng.random((n, 1, 1))) + way * extent * 0.03 * rng.random((n, 1, 1))
    out = lifted.astype(F)                                                      # near
    far = kind == 1
    out[far] = (lifted[far] + way[far] * extent * (2 + 48 * rng.random((int(far.sum()), 1, 1)))).astype(F)
    crossing = kind == 2
    out[crossing] = IC.slicers(tris, int(crossing.sum()), seed + 2, 0.05, 0.6)
    out[kind == 3] = tris[pick[kind == 3]]                                      # own
    point = kind == 4
    out[point, 1] = out[point, 2] = out[point, 0]
    segment = kind == 5
    out[segment, 2] = out[segment, 0]
    bad = np.nonzero(kind == 6)[0]
    out[bad, rng.integers(0, 3, len(bad)), rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(bad))
    return out
