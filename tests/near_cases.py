"""The scenes and points of the within-radius tests (tests/test_near_reference.py, tests/test_gpu_near.py).

make_points re-states tests/test_gpu_point_query.py's: the same seven kinds of point (on the surface, near it, inside the mesh,
on a node box face, exactly at a vertex, far away, a duplicate of another) and the same radius mix (+inf, small finite, 0,
negative, NaN, non-finite p), with a quarter of the points given radii of 5 to 20 % of the scene's extent, so that many points
have more triangles within a finite radius than any K kept.
"""
import os

import numpy as np

import helpers
import point_query_ref as R

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def scene_path(name):
    return {"small_trisrc": helpers.small_trisrc, "bunny": helpers.bunny_trisrc,
            "lobed_528": lambda: os.path.join(GOLDEN, "lobed_528.trisrc"),
            "quads_mixed": lambda: os.path.join(GOLDEN, "quads_mixed.obj"),
            "quads_nonormals": lambda: os.path.join(GOLDEN, "quads_nonormals.obj")}[name]()


def scene_extent(positions) -> float:
    verts = np.asarray(positions, F).reshape(-1, 3)
    return float(np.linalg.norm(verts.max(0) - verts.min(0)))


def make_points(arrays, n, seed):
    """POINT_DTYPE points of every kind (module doc).  Radii: +inf (35 %), 5 to 20 % of the extent (25 %), up to 5 % of it
    (25 %), 0, negative, NaN (3, 2, 2 %); 2 % of the points get a non-finite coordinate."""
    rng = np.random.default_rng(seed)
    tris = np.asarray(arrays["vertex_positions"], F).reshape(-1, 3, 3)
    verts = tris.reshape(-1, 3)
    lo, hi = verts.min(0), verts.max(0)
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    extent = float(np.linalg.norm(hi - lo))
    kind = rng.integers(0, 7, n)
    p = np.zeros((n, 3), F)
    t = rng.integers(0, len(tris), n)
    b = rng.random((n, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    v = tris[t].astype(np.float64)
    on = (v[:, 0] + b[:, :1] * (v[:, 1] - v[:, 0]) + b[:, 1:] * (v[:, 2] - v[:, 0]))
    p[:] = on.astype(F)                                                                      # 0: on the surface
    near = kind == 1
    p[near] = (on[near] + rng.normal(size=(near.sum(), 3)) * extent / 100 / 1.7).astype(F)   # 1: near it
    inside = kind == 2
    p[inside] = (centre + (rng.random((inside.sum(), 3)) * 2 - 1) * 0.3 * half).astype(F)  # 2: inside the mesh
    face = np.nonzero(kind == 3)[0]                                                         # 3: on a node box face
    bmin = np.asarray(arrays["group_boxmin"], F).reshape(-1, 3)
    bmax = np.asarray(arrays["group_boxmax"], F).reshape(-1, 3)
    node = rng.integers(0, len(bmin), len(face))
    f = (bmin[node] + (bmax[node] - bmin[node]) * rng.random((len(face), 3))).astype(F)
    axis = rng.integers(0, 3, len(face))
    f[np.arange(len(face)), axis] = np.where(rng.random(len(face)) < 0.5, bmin[node, axis], bmax[node, axis])
    corner = rng.random(len(face)) < 0.2
    f[corner] = np.where(rng.random((corner.sum(), 3)) < 0.5, bmin[node[corner]], bmax[node[corner]])
    p[face] = f
    at = kind == 4
    p[at] = verts[rng.integers(0, len(verts), at.sum())]                                    # 4: exactly at vertices
    far = kind == 5
    p[far] = (centre + rng.normal(size=(far.sum(), 3)) * 100 * extent).astype(F)            # 5: far away
    dup = np.nonzero(kind == 6)[0]                                                          # 6: duplicates of others
    p[dup] = p[rng.integers(0, n, len(dup))]
    md = np.full(n, np.inf, F)
    r = rng.random(n)
    wide = (r >= 0.35) & (r < 0.60)
    md[wide] = ((0.05 + 0.15 * rng.random(wide.sum())) * extent) ** 2
    sel = (r >= 0.60) & (r < 0.85)
    md[sel] = (rng.random(sel.sum()) * extent / 20) ** 2
    md[(r >= 0.85) & (r < 0.88)] = 0.0
    md[(r >= 0.88) & (r < 0.90)] = -1.0
    md[(r >= 0.90) & (r < 0.92)] = np.nan
    bad = np.nonzero((r >= 0.92) & (r < 0.94))[0]
    p[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(bad))
    out = np.zeros(n, R.POINT_DTYPE)
    out["p"], out["max_dist2"] = p, md
    return out
