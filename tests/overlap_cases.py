"""The scenes and boxes of the box-overlap tests (tests/test_overlap_reference.py, tests/test_gpu_overlap.py).

make_boxes mixes, over a scene's arrays: voxel cells of a grid over the scene's box; boxes of 1 to 20 % of the extent centred
near surface points, and cubes about surface points sized to hold somewhat more than 64 triangles; boxes that contain the whole scene; far boxes; zero-extent boxes at a vertex, on an edge midpoint and
inside a face (where those coordinates are exactly representable, else at a vertex); boxes with a face exactly on a vertex
coordinate; inverted, NaN and infinite boxes.
"""
import numpy as np

import overlap_ref as OR
from near_cases import scene_extent, scene_path   # noqa: F401  (the tests take them from here)

F = np.float32
KINDS = ("voxel", "surface", "whole", "far", "flat", "on_vertex", "unwalked", "coarse", "medium")


def shares(triangles):
    """The share of each kind.  The boxes with many triangles are cells of a coarse grid (`coarse`): in a scene of at most 64
    triangles only they hold more than 8, so there they are more.  Boxes around the whole scene are the first two only (kinds): each passes
    every triangle through stage 0 and rejects none later."""
    coarse = 0.112 if triangles > 64 else 0.24
    medium = 0.075 if triangles > 64 else 0.0
    return (0.06, 0.70 - coarse - medium, 0.0, 0.05, 0.10, 0.04, 0.05, coarse, medium)


def voxel_grid(lo, hi, dims):
    """every cell of a dims grid over (lo, hi): plane i of an axis is lo + i * cell in fp32, so neighbours share their faces"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    dims = np.asarray(dims)
    cell = ((hi - lo) / dims.astype(F)).astype(F)
    planes = [lo[a] + np.arange(dims[a] + 1, dtype=F) * cell[a] for a in range(3)]
    i, j, k = np.meshgrid(*(np.arange(d) for d in dims), indexing="ij")
    blo = np.stack([planes[0][i], planes[1][j], planes[2][k]], -1).reshape(-1, 3)
    bhi = np.stack([planes[0][i + 1], planes[1][j + 1], planes[2][k + 1]], -1).reshape(-1, 3)
    return OR.make_boxes(blo, bhi)


def _exact(p64):
    """rows of float64 points that float32 holds exactly"""
    return (p64.astype(F).astype(np.float64) == p64).all(1)


def make_boxes(arrays, n, seed):
    """BOX_DTYPE boxes of every kind (module doc), shuffled; `kinds(n, seed)` gives each box's kind"""
    rng = np.random.default_rng(seed)
    tris = np.asarray(arrays["vertex_positions"], F).reshape(-1, 3, 3)
    verts = tris.reshape(-1, 3)
    lo, hi = verts.min(0), verts.max(0)
    size = (hi - lo).astype(np.float64)
    extent = float(np.linalg.norm(size))
    kind = kinds(n, seed, len(tris))
    blo, bhi = np.zeros((n, 3), F), np.zeros((n, 3), F)

    t = rng.integers(0, len(tris), n)
    b = rng.random((n, 2))
    b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
    v = tris[t].astype(np.float64)
    on = v[:, 0] + b[:, :1] * (v[:, 1] - v[:, 0]) + b[:, 1:] * (v[:, 2] - v[:, 0])

    s = np.nonzero(kind == 0)[0]                                    # voxel cells of grids of 8 to 32 cells a side
    dims = rng.integers(8, 33, (len(s), 3))
    cell = (size / dims).astype(F)
    at = (rng.random((len(s), 3)) * dims).astype(np.int64)
    blo[s] = lo + at.astype(F) * cell
    bhi[s] = lo + (at + 1).astype(F) * cell

    centroid = tris.astype(np.float64).mean(1)
    for which, low, high in ((7, 50, 54), (8, 8, 11)):              # cubes about surface points out to the 51st to 54th nearest centroid
        s = np.nonzero(kind == which)[0]                            # (somewhat more than 64 triangles touch them), and to the 9th to 11th
        reach = np.abs(centroid[None, :, :] - on[s][:, None, :]).max(2)
        reach.sort(1)
        nth = np.minimum(rng.integers(low, high, len(s)), len(tris) - 1)
        half = reach[np.arange(len(s)), nth][:, None] * (1.0 + 1e-3)
        blo[s], bhi[s] = (on[s] - half).astype(F), (on[s] + half).astype(F)

    s = np.nonzero(kind == 1)[0]                                    # 1 to 20 % of the extent on each axis, centred near the surface
    half = 0.005 * 20.0 ** (rng.random((len(s), 3)) ** 2) * extent  # (most are thin or long: triangles' boxes meet them, triangles less often)
    centre = on[s] + rng.normal(size=(len(s), 3)) * half * 0.7
    beside = rng.random(len(s)) < 0.75                              # 1 to 2 % of the extent, a fraction of the triangle's size away from
    half[beside] = (0.005 * (1.0 + rng.random((len(s), 3))) * extent)[beside]   # it: in its vertex box and its neighbours', often off them
    reach = np.linalg.norm(v[s].max(1) - v[s].min(1), axis=1, keepdims=True)
    aside = rng.normal(size=(len(s), 3))
    aside /= np.linalg.norm(aside, axis=1, keepdims=True)
    # ... of a vertex that lies in many triangles' vertex boxes (a pole of a fan more often than a vertex of a regular patch)
    tlo, thi = tris.min(1), tris.max(1)
    some = verts if len(verts) <= 8000 else verts[np.random.default_rng(seed + 5).choice(len(verts), 1000, replace=False)]
    depth = np.array([((tlo <= p_) & (p_ <= thi)).all(1).sum() for p_ in some], np.float64)
    deep = some[rng.choice(len(some), len(s), p=depth ** 2 / (depth ** 2).sum())]
    centre[beside] = (deep + aside * reach * (0.25 + 0.25 * rng.random((len(s), 1))))[beside]
    blo[s], bhi[s] = (centre - half).astype(F), (centre + half).astype(F)

    s = np.nonzero(kind == 2)[0]                                    # the whole scene: exactly its box, or wider
    grow = np.where(np.arange(len(s))[:, None] == 0, 0.0, rng.random((len(s), 3))) * extent
    blo[s], bhi[s] = (lo - grow).astype(F), (hi + grow).astype(F)

    s = np.nonzero(kind == 3)[0]                                    # far away
    centre = (lo + hi) / 2 + rng.choice([-1.0, 1.0], (len(s), 3)) * (3 + 100 * rng.random((len(s), 3))) * extent
    half = rng.random((len(s), 3)) * extent
    blo[s], bhi[s] = (centre - half).astype(F), (centre + half).astype(F)

    s = np.nonzero(kind == 4)[0]                                    # zero extent on one, two or three axes
    where = rng.integers(0, 3, len(s))
    p = v[s, 0].copy()                                              # at a vertex
    mid = (v[s, 0] + v[s, 1]) / 2                                   # on an edge midpoint
    inner = v[s, 0] / 2 + v[s, 1] / 4 + v[s, 2] / 4                 # inside the face
    use = (where == 1) & _exact(mid)
    p[use] = mid[use]
    use = (where == 2) & _exact(inner)
    p[use] = inner[use]
    half = rng.random((len(s), 3)) * extent * 0.04 * (rng.random((len(s), 3)) < 0.4)   # most axes flat
    half[rng.random(len(s)) < 0.4] = 0.0                                              # a point
    blo[s], bhi[s] = (p - half).astype(F), (p + half).astype(F)
    flat = half == 0
    blo[s] = np.where(flat, p.astype(F), blo[s])
    bhi[s] = np.where(flat, p.astype(F), bhi[s])

    s = np.nonzero(kind == 5)[0]                                    # a face exactly on a vertex coordinate, the box beside it
    corner = verts[rng.integers(0, len(verts), len(s))]
    half = (0.005 + 0.04 * rng.random((len(s), 3))) * extent
    centre = corner + rng.normal(size=(len(s), 3)) * half * 0.3
    l, h = (centre - half).astype(F), (centre + half).astype(F)
    axis = rng.integers(0, 3, len(s))
    upper = rng.random(len(s)) < 0.5
    rows = np.arange(len(s))
    h[rows[upper], axis[upper]] = corner[rows[upper], axis[upper]]
    l[rows[upper], axis[upper]] = np.minimum(l[rows[upper], axis[upper]], corner[rows[upper], axis[upper]])
    l[rows[~upper], axis[~upper]] = corner[rows[~upper], axis[~upper]]
    h[rows[~upper], axis[~upper]] = np.maximum(h[rows[~upper], axis[~upper]], corner[rows[~upper], axis[~upper]])
    blo[s], bhi[s] = l, h

    s = np.nonzero(kind == 6)[0]                                    # not walked: inverted, NaN, infinite
    half = (0.01 + 0.2 * rng.random((len(s), 3))) * extent
    l, h = (on[s] - half).astype(F), (on[s] + half).astype(F)
    how = rng.integers(0, 3, len(s))
    axis = rng.integers(0, 3, len(s))
    rows = np.arange(len(s))
    inv = how == 0
    l[rows[inv], axis[inv]], h[rows[inv], axis[inv]] = h[rows[inv], axis[inv]], l[rows[inv], axis[inv]]
    side = rng.random(len(s)) < 0.5
    bad = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(s))
    put = (how > 0) & side
    l[rows[put], axis[put]] = bad[put]
    put = (how > 0) & ~side
    h[rows[put], axis[put]] = bad[put]
    blo[s], bhi[s] = l, h
    return OR.make_boxes(blo, bhi)


def kinds(n, seed, triangles):
    """the kind (index into KINDS) of each of make_boxes(arrays, n, seed)'s boxes, for a scene of `triangles` triangles"""
    kind = np.random.default_rng(seed + 77).choice(len(KINDS), n, p=shares(triangles))
    kind[:2] = KINDS.index("whole")   # exactly the scene's box, and a wider one
    return kind


def coverage(code, what=""):
    """What the tests ask of a set of boxes, from the restatement's first-axis codes [boxes, triangles]: the shares of boxes with
    n == 0, n > 8 and n > 64, the share of the pairs that pass stage 0 which a later axis rejects, and the pairs each axis
    rejects first."""
    n = (code == OR.OVERLAP).sum(1)
    per_axis = np.bincount(code[(code >= 0) & (code < OR.AXES)].astype(np.int64), minlength=OR.AXES)
    past0 = int((code == OR.OVERLAP).sum() + per_axis[3:].sum())
    out = {"n == 0": float((n == 0).mean()), "n > 8": float((n > 8).mean()), "n > 64": float((n > 64).mean()),
           "later": float(per_axis[3:].sum() / max(past0, 1)), "per_axis": per_axis.tolist()}
    print(f"{what}: {code.shape[1]} triangles, {len(code)} boxes, {out}")
    return out


def assert_interesting(code, what):
    """The tests' own inputs must exercise the query (the issue's bounds), judged on the restatement alone."""
    c = coverage(code, what)
    assert c["n == 0"] > 0.05 and c["n > 8"] > 0.20, (what, c)
    if code.shape[1] > 64:
        assert c["n > 64"] > 0.10, (what, c)
    assert c["later"] > 0.10 and min(c["per_axis"][3:]) >= 1, (what, c)
