"""The scenes, query triangles and exact truth of the triangle-intersection tests (tests/test_intersect_reference.py,
tests/test_gpu_intersect.py).

make_queries mixes, over a scene's arrays: the scene's own triangles (each finds itself and its neighbours), moved copies of
them (rotated a little and shifted by a few percent of the diagonal: most miss, and most of what passes the vertex boxes is
rejected by a later axis), random slicing triangles through the centroid of 0.05 to 1 diagonals, large slicers of 1.5
diagonals (the ones that intersect more than 64 triangles), and queries that are not walked (a NaN or infinite coordinate, a
point, a segment).

flat_lattice is the scene general-position data cannot replace: a planar grid in z = 0 plus a second sheet at a constant x,
with integer coordinates and no more than 64 triangles, so that pairs are exactly coplanar and only the in-plane axes (12 to 17) can separate them.

exact_intersects is the truth on integer inputs, in fractions.Fraction: the query clipped by the scene triangle's plane as two
closed half-spaces, then by its three in-plane edge half-spaces; non-empty means intersecting.
"""
from fractions import Fraction

import numpy as np

import intersect_ref as IR
from near_cases import scene_extent, scene_path   # noqa: F401  (the tests take them from here)

F = np.float32
KINDS = ("own", "moved", "slicer", "large", "unwalked")
SHARES = (0.27, 0.23, 0.10, 0.35, 0.05)


def kinds(n, seed):
    return np.random.default_rng(seed + 77).choice(len(KINDS), n, p=SHARES)


def _rotation(rng, angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def moved_copy(positions, seed, angle=0.05, shift=0.03):
    """the scene's triangles [T, 3, 3] rotated by `angle` about the centroid on a random axis and shifted by `shift` diagonals"""
    rng = np.random.default_rng(seed)
    tris = np.asarray(positions, F).reshape(-1, 3, 3).astype(np.float64)
    verts = tris.reshape(-1, 3)
    centre, diagonal = verts.mean(0), np.linalg.norm(verts.max(0) - verts.min(0))
    way = rng.normal(size=3)
    way *= shift * diagonal / np.linalg.norm(way)
    return ((tris - centre) @ _rotation(rng, angle).T + centre + way).astype(F)


def slicers(positions, n, seed, low, high):
    """`n` random triangles about the scene's centroid, `low` to `high` scene diagonals in size"""
    rng = np.random.default_rng(seed)
    verts = np.asarray(positions, np.float64).reshape(-1, 3)
    centre, diagonal = verts.mean(0), np.linalg.norm(verts.max(0) - verts.min(0))
    size = (low + (high - low) * rng.random((n, 1, 1))) * diagonal
    at = centre + rng.normal(size=(n, 1, 3)) * 0.1 * diagonal * min(1.0, high)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    angles = rng.random((n, 1)) * 2 * np.pi + np.array([[0.0, 2.1, 4.2]])
    ring = np.cos(angles)[:, :, None] * u[:, None, :] + np.sin(angles)[:, :, None] * w[:, None, :]
    return (at + 0.5 * size * ring).astype(F)


def make_queries(arrays, n, seed):
    """float32 [n, 3, 3] query triangles of every kind (module doc); kinds(n, seed) gives each one's kind"""
    rng = np.random.default_rng(seed)
    tris = np.asarray(arrays["vertex_positions"], F).reshape(-1, 3, 3)
    kind = kinds(n, seed)
    out = np.zeros((n, 3, 3), F)
    pick = rng.integers(0, len(tris), n)
    out[kind == 0] = tris[pick[kind == 0]]
    out[kind == 1] = moved_copy(tris, seed + 1)[pick[kind == 1]]
    out[kind == 2] = slicers(tris, int((kind == 2).sum()), seed + 2, 0.05, 1.0)
    out[kind == 3] = slicers(tris, int((kind == 3).sum()), seed + 3, 1.5, 1.5)
    s = np.nonzero(kind == 4)[0]
    bad = tris[pick[s]].copy()
    how = rng.integers(0, 4, len(s))
    rows = np.arange(len(s))
    value = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(s))
    corner, axis = rng.integers(0, 3, len(s)), rng.integers(0, 3, len(s))
    put = how < 2
    bad[rows[put], corner[put], axis[put]] = value[put]
    bad[how == 2, 1] = bad[how == 2, 0]                    # a segment
    bad[how == 3, 1] = bad[how == 3, 2] = bad[how == 3, 0]   # a point
    out[s] = bad
    return out


def coverage(code, what=""):
    """What the tests ask of a set of queries, from the restatement's codes [queries, triangles]: the shares of queries with
    n == 0, n > 8 and n > 64, the share of the pairs that pass stage 0 which a later stage rejects, and the pairs each of the
    seventeen axes rejects first."""
    n = (code == IR.INTERSECT).sum(1)
    counts = np.bincount(code[(code >= 0) & (code < IR.UNWALKED)].astype(np.int64), minlength=IR.UNWALKED)
    past0 = int((code == IR.INTERSECT).sum() + counts[3:].sum())
    out = {"n == 0": float((n == 0).mean()), "n > 8": float((n > 8).mean()), "n > 64": float((n > 64).mean()), "n max": int(n.max()),
           "later": float(counts[3:].sum() / max(past0, 1)), "per_axis": counts[IR.AXIS0:].tolist()}
    print(f"{what}: {code.shape[1]} triangles, {len(code)} queries, {out}")
    return out


def assert_interesting(code, what):
    """The tests' own inputs must exercise the query (the issue's bounds), judged on the restatement alone.  Returns the pairs
    each axis rejected first: that every axis is the first somewhere is asked of the suite as a whole."""
    c = coverage(code, what)
    assert c["n == 0"] > 0.05 and c["n > 8"] > 0.20, (what, c)
    if code.shape[1] > 64:
        assert c["n > 64"] > 0.05, (what, c)
    assert c["later"] > 0.10, (what, c)
    return np.asarray(c["per_axis"])


def flat_lattice(nx=5, ny=4):
    """float32 [T, 3, 3], integer coordinates, 58 triangles: a grid of nx x ny cells of 2 x 2 in z = 0, two triangles a cell, and
    a second sheet in the plane x = 5 that crosses it, of 3 x 3 cells of 2 x 2 over y in [1, 7] and z in [-3, 3].  The corners
    of a triangle start at another one from cell to cell, so that each of its edges e0, e1, e2 is somewhere the diagonal: the
    other two are parallel to a coordinate axis, where stage 0 separates before an in-plane axis can."""
    tris = []
    for i in range(nx):
        for j in range(ny):
            x, y = 2 * i, 2 * j
            for tri in ([(x, y, 0), (x + 2, y, 0), (x + 2, y + 2, 0)], [(x, y, 0), (x + 2, y + 2, 0), (x, y + 2, 0)]):
                tris.append(tri[(i + j) % 3:] + tri[:(i + j) % 3])
    for j in range(3):
        for k in range(3):
            y, z = 1 + 2 * j, -3 + 2 * k
            for tri in ([(5, y, z), (5, y + 2, z), (5, y + 2, z + 2)], [(5, y, z), (5, y + 2, z + 2), (5, y, z + 2)]):
                tris.append(tri[(j + k) % 3:] + tri[:(j + k) % 3])
    return np.asarray(tris, F)


def flat_queries(n, seed):
    """integer query triangles for flat_lattice (coordinates in [-4, 14]): half of them in the plane z = 0, a sixth in the plane
    x = 5, the rest anywhere; a few segments"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 11, (n, 3))
    q = np.stack([a, a + rng.integers(-8, 9, (n, 3)), a + rng.integers(-8, 9, (n, 3))], 1)
    kind = rng.random(n)
    q[kind < 0.5, :, 2] = 0
    sheet = (kind >= 0.5) & (kind < 0.67)
    q[sheet, :, 0] = 5
    q[sheet, :, 2] -= 5
    thin = rng.random(n) < 0.03
    q[thin, 2] = q[thin, 1]
    return np.clip(q, -4, 14).astype(F)


def _clip(poly, height):
    """the part of the closed polygon where height >= 0 (Sutherland-Hodgman, every height taken once)"""
    h = [height(p) for p in poly]
    out = []
    for i, p in enumerate(poly):
        j = (i + 1) % len(poly)
        if h[i] >= 0:
            out.append(p)
        if (h[i] >= 0) != (h[j] >= 0):
            s = h[i] / (h[i] - h[j])
            out.append(tuple(a + s * (b - a) for a, b in zip(p, poly[j])))
    return out


def exact_cross(x, y):
    return (x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0])


def exact_intersects(q, t):
    """Two non-degenerate triangles with integer corners, as closed sets, in exact rationals: q clipped by t's plane as two
    closed half-spaces, then by the three half-spaces of t's edges in that plane; non-empty means they intersect."""
    q = [tuple(Fraction(int(x)) for x in p) for p in q]
    t = [tuple(Fraction(int(x)) for x in p) for p in t]
    sub = lambda x, y: tuple(a - b for a, b in zip(x, y))
    dot = lambda x, y: sum(a * b for a, b in zip(x, y))
    edges = [sub(t[(j + 1) % 3], t[j]) for j in range(3)]
    nt = exact_cross(edges[0], edges[1])
    planes = [(nt, t[0], 1), (nt, t[0], -1)] + [(exact_cross(nt, edges[j]), t[j], 1) for j in range(3)]
    poly = q
    for normal, through, sign in planes:
        poly = _clip(poly, lambda p: sign * dot(normal, sub(p, through)))
        if not poly:
            return False
    return True


def exact_degenerate(tri):
    tri = np.asarray(tri).astype(np.int64)
    return not np.cross(tri[1] - tri[0], tri[2] - tri[1]).any()
