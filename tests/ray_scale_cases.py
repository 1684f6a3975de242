"""Caller-supplied rays at the edges of exact_div.h's operand ranges: the shared case generator of
tests/test_ray_scale_reference.py (CPU) and tests/test_gpu_ray_scale.py (GPU).  No test and no GPU in here.

Scenes: lobed_528 and small_trisrc with every position multiplied by S = 2^k, k in S_EXPONENTS, loaded from the same file
with GEOMETRY_SCALE (host/trisrc-support.cpp multiplies the parsed float by it: exact for a power of two).

Rays of a (scene, S): tests/test_gpu_ray_query.py's random_rays (origins in twice the box, inside the mesh, on it; its tmax
mix) with the origins multiplied by S, and per (kind, edge) cell RAYS_PER_CELL of them:
  kind "uniform"    direction = unit vector * m, m one of EDGES
  kind "component"  direction = unit vector with ONE component (a random axis, a random sign) replaced by the edge value: the
                    gate is an AND over three components and each must be able to fail alone
and on S = 1 only
  kind "origin"     one to three origin components replaced by a member of ORIGIN_VALUES, the direction (not normalised)
                    from there to a point of the mesh, so the hit, if any, is near t = 1
random_rays' tmax values that are lengths (a fraction of the scene's extent) are multiplied by S / |direction|: a cut-off
inside the scaled scene.  The walk's range [0, 1e8] is not scaled, so t = S / |direction| * (a length of the unscaled scene)
must stay below it, and fs:311's |det| >= 1e-7 asks S^2 |direction| * (twice a triangle's area) to stay above: the cells
outside either are miss-only by construction.  TABLE states which, and each scene's exact_div_ok per S.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

import ray_query_ref as R
from test_gpu_ray_query import random_rays, scene_path

F = np.float32
SCENES = ("lobed_528", "small_trisrc")
S_EXPONENTS = (-71, -70, -30, 0, 30, 59, 60)
RAYS_PER_CELL = 192
ORIGIN_RAYS = 1024


def _down(x):
    return np.nextafter(F(x), F(0))


def _up(x):
    return np.nextafter(F(x), F(np.inf))


# (name, value, divisor_in_range(value) as exact_div.h documents it: [2^-40, 2^20))
EDGES = (("2^-41", F(2.0 ** -41), False), ("2^-40 - 1ulp", _down(2.0 ** -40), False), ("2^-40", F(2.0 ** -40), True),
         ("2^-40 + 1ulp", _up(2.0 ** -40), True), ("2^-20", F(2.0 ** -20), True), ("1", F(1), True), ("2^19", F(2.0 ** 19), True),
         ("2^20 - 1ulp", _down(2.0 ** 20), True), ("2^20", F(2.0 ** 20), False), ("2^21", F(2.0 ** 21), False),
         ("2^40", F(2.0 ** 40), False))
# (name, value, coordinate_in_range(value): 0, or [2^-70, 2^60))
ORIGIN_VALUES = (("+0", F(0.0), True), ("-0", F(-0.0), True), ("smallest denormal", np.uint32(1).view(F), False),
                 ("2^-71", F(2.0 ** -71), False), ("2^-70", F(2.0 ** -70), True), ("2^60 - 1ulp", _down(2.0 ** 60), True),
                 ("2^60", F(2.0 ** 60), False), ("2^61", F(2.0 ** 61), False))

# S exponent: (exact_div_ok of lobed_528, of small_trisrc, the cells of kind "uniform" per EDGES entry, of kind "component")
#   1  hits possible: the restatement reports at least 5 % hits and at least 5 % misses among the traced rays
#   0  miss-only by construction: S / |direction| >= 2^50 puts every crossing beyond the walk's 1e8, or S^2 |direction| <= 2^-50
#      puts every determinant under fs:311's 1e-7.  An origin ON the surface would still meet its own triangle at t = 0 where
#      the determinant allows it, so in these cells random_rays' origins on the mesh are replaced by origins inside it.
# Three cells are MOVED in m, as neither statement held for them: with S^2 m = 2^-20 the determinant, 2^-20 times twice a
# triangle's area (0.03 to 0.1 here), straddles the 1e-7 and the restatement reported 0 to 1 % hits through the largest
# triangles.  MOVED gives them an m of their own, 2^-10 of the edge's, on the same side of the divisor range: S^2 m = 2^-30
# puts every determinant under the epsilon, so they are miss-only by construction.  (The edges 2^-20 and 2^40 themselves are
# met at the other S, and alone on a component at S = 1.)
# exact_div_ok: a box is its triangles' corners -+ 1e-5 (box3d::add), so from S = 2^-30 down every box coordinate is about
# +-1e-5 and in range; the meshes' largest coordinates are 1.51 and 1.71, so at S = 2^59 every coordinate is still below 2^60
# (the largest 1.71 * 2^59) and at S = 2^60 most are not.
# hits possible at S = 2^30 with |direction| about 1 (S / |direction| = 2^30): the crossings within 1e8 / 2^30 = 0.09 of the
# origin -- rays that start on the surface or close to it; 10 to 23 % of the traced rays.
TABLE = {
    -71: (1, 1, "00000000000", "00000000000"),
    -70: (1, 1, "00000000000", "00000000000"),
    -30: (1, 1, "00000000000", "00000000000"),
    0:   (1, 1, "00000111111", "11111111111"),
    30:  (1, 1, "00000111111", "11111111111"),
    59:  (1, 1, "00000000000", "00000000000"),
    60:  (0, 0, "00000000000", "00000000000"),
}
ORIGIN_CELL_HITS_POSSIBLE = True
# (S exponent, kind, EDGES index): the cell's own m
MOVED = {(-30, "uniform", 10): F(2.0 ** 30), (-30, "component", 10): F(2.0 ** 30), (0, "uniform", 4): F(2.0 ** -30)}
KINDS = ("uniform", "component", "origin")


def expected_flag(name: str, s_exp: int) -> int:
    return TABLE[s_exp][SCENES.index(name)]


@dataclass
class Cell:
    kind: str                 # "uniform", "component" or "origin"
    edge: int | None          # index into EDGES (None: the origin class)
    value: np.float32 | None  # the cell's m or component: EDGES' value, or MOVED's
    rays: np.ndarray          # the indices of its rays
    hits_possible: bool

    def __repr__(self):
        return f"{self.kind}/{'' if self.edge is None else EDGES[self.edge][0]}" + ("" if self.edge is None or self.value == EDGES[self.edge][1] else f" moved to {self.value}")


@dataclass
class Case:
    name: str
    s_exp: int
    S: np.float32
    arrays: R.SceneArrays     # the scaled scene
    o: np.ndarray
    d: np.ndarray
    tmax: np.ndarray
    cells: list
    on_surface: np.ndarray    # bool [n]: the ray starts on the mesh (random_rays' third kind of origin, where it was kept)


_worlds = {}


def scale_string(s_exp: int) -> str:
    return "%.17g" % (2.0 ** s_exp)


def load_scaled(pkg, name: str, s_exp: int):
    """pkg.World of the scene's file under GEOMETRY_SCALE = 2^s_exp (the caller closes it)"""
    before = os.environ.get("GEOMETRY_SCALE")
    os.environ["GEOMETRY_SCALE"] = scale_string(s_exp)
    try:
        return pkg.World(scene_path(name))
    finally:
        if before is None:
            del os.environ["GEOMETRY_SCALE"]
        else:
            os.environ["GEOMETRY_SCALE"] = before


def base_arrays(pkg, name: str) -> R.SceneArrays:
    if (name, None) not in _worlds:
        world = pkg.World(scene_path(name))
        _worlds[(name, None)] = R.SceneArrays(world.arrays())
        world.close()
    return _worlds[(name, None)]


def triangle_rows(positions) -> np.ndarray:
    """the triangles [T, 9] as raw words, sorted: the BVH build's triangle order may change with the scale, the set may not"""
    rows = np.ascontiguousarray(positions, F).reshape(-1, 9).view(np.uint32)
    return rows[np.lexsort(rows.T[::-1])]


def scaled_arrays(pkg, name: str, s_exp: int) -> R.SceneArrays:
    """the scaled scene's arrays, once; its positions are asserted to be the unscaled ones times 2^s_exp bit for bit"""
    key = (name, s_exp)
    if key not in _worlds:
        world = load_scaled(pkg, name, s_exp)
        arrays = R.SceneArrays(world.arrays())
        world.close()
        want = base_arrays(pkg, name).positions * F(2.0 ** s_exp)
        assert np.isfinite(want).all() and (want != 0).sum() == (base_arrays(pkg, name).positions != 0).sum()   # no overflow, no underflow
        assert np.array_equal(triangle_rows(arrays.positions), triangle_rows(want)), (name, s_exp)
        _worlds[key] = arrays
    return _worlds[key]


def leaf_boxes(arrays: R.SceneArrays):
    """(lo, hi) [leaves, 3] of the leaves' triangles: corners -+ 1e-5 in float32, folded (box3d::add); a branch's box is the
    fold of its leaves', so these hold every box coordinate of the scene"""
    leaf = arrays.hitmiss[0][:, 0] == arrays.hitmiss[0][:, 1]
    bump = F(0.00001)
    lo, hi = [], []
    for start, count in arrays.objects[leaf].astype(np.int64):
        c = arrays.positions[start:start + count].reshape(-1, 3)
        lo.append((c - bump).min(0))
        hi.append((c + bump).max(0))
    return np.array(lo, F), np.array(hi, F)


def make_case(pkg, name: str, s_exp: int) -> Case:
    base = base_arrays(pkg, name)
    S = F(2.0 ** s_exp)
    per_kind = RAYS_PER_CELL * len(EDGES)
    n = 2 * per_kind + (ORIGIN_RAYS if s_exp == 0 else 0)
    seed = 1000 + 10 * S_EXPONENTS.index(s_exp) + SCENES.index(name)
    o, d, tmax = random_rays(base, n, seed=seed)
    rng = np.random.default_rng(seed + 500)
    kind = np.repeat(np.arange(3), [per_kind, per_kind, n - 2 * per_kind])
    edge = np.concatenate([np.tile(np.arange(len(EDGES)), 2 * RAYS_PER_CELL), np.full(n - 2 * per_kind, -1)])
    cell_value = np.array([[MOVED.get((s_exp, KINDS[kd], e), EDGES[e][1]) for e in range(len(EDGES))] for kd in range(2)], F)
    values = cell_value[np.minimum(kind, 1), edge]               # per ray (not looked at for kind "origin")
    _, _, uniform, component = TABLE[s_exp]
    on_surface = np.random.default_rng(seed).integers(0, 3, n) == 2     # random_rays' first draw: its origin kinds
    assert on_triangle(base, o[on_surface]).all() and not on_triangle(base, o[~on_surface]).any(), "random_rays' draws have moved"
    on_surface &= kind != 2
    miss_only = np.array([c == "0" for c in uniform + component])[np.where(kind < 2, kind * len(EDGES) + edge, 0)] & (kind < 2)
    k = np.nonzero(on_surface & miss_only)[0]
    pts = base.positions.reshape(-1, 3)
    centre, half = (pts.min(0) + pts.max(0)) / 2, (pts.max(0) - pts.min(0)) / 2
    o[k] = (centre + (rng.random((len(k), 3)) * 2 - 1) * 0.3 * half).astype(F)
    on_surface[k] = False
    o = o * S
    # kind "uniform"
    k = np.nonzero(kind == 0)[0]
    d[k] = d[k] * values[k][:, None]
    # kind "component"
    k = np.nonzero(kind == 1)[0]
    d[k, rng.integers(0, 3, len(k))] = values[k] * np.where(rng.random(len(k)) < 0.5, F(1), F(-1))
    # kind "origin"
    k = np.nonzero(kind == 2)[0]
    if len(k):
        special = np.array([v[1] for v in ORIGIN_VALUES], F)
        how_many = rng.integers(1, 4, len(k))
        for j, i in enumerate(k):
            axes = rng.choice(3, how_many[j], replace=False)
            o[i, axes] = special[rng.integers(0, len(special), how_many[j])] * np.where(rng.random(how_many[j]) < 0.5, F(1), F(-1))
        tri = base.positions[rng.integers(0, len(base.positions), len(k))].astype(np.float64)
        b = rng.random((len(k), 2))
        b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
        target = tri[:, 0] + b[:, :1] * (tri[:, 1] - tri[:, 0]) + b[:, 1:] * (tri[:, 2] - tri[:, 0])
        beyond = rng.random(len(k)) < 0.35                      # a third aim past the mesh instead: misses
        target[beyond] = (pts.min(0) + (pts.max(0) - pts.min(0)) * (rng.random((int(beyond.sum()), 3)) * 3 - 1))
        d[k] = (target - o[k].astype(np.float64)).astype(F)
    # random_rays' cut-offs inside the scene: lengths of the unscaled scene, so S / |direction| of them in t
    lengths = np.isfinite(tmax) & (tmax > 0) & (tmax != F(1e7))
    with np.errstate(all="ignore"):
        norm = np.linalg.norm(d.astype(np.float64), axis=1)
        tmax[lengths] = (tmax[lengths].astype(np.float64) * float(S) / norm[lengths]).astype(F)
    cells = []
    for kd, column in ((0, uniform), (1, component)):
        for e in range(len(EDGES)):
            cells.append(Cell(KINDS[kd], e, cell_value[kd, e], np.nonzero((kind == kd) & (edge == e))[0], column[e] == "1"))
    if s_exp == 0:
        cells.append(Cell("origin", None, None, np.nonzero(kind == 2)[0], ORIGIN_CELL_HITS_POSSIBLE))
    return Case(name, s_exp, S, scaled_arrays(pkg, name, s_exp), np.ascontiguousarray(o, F), np.ascontiguousarray(d, F), tmax.astype(F),
                cells, on_surface)


def on_triangle(arrays: R.SceneArrays, points) -> np.ndarray:
    """bool [n]: the point lies on a triangle of the mesh (in its plane within 1e-5 of the triangle's size, barycentrics within
    1e-5 of [0, 1]) -- how a reconstruction of random_rays' origin kinds is checked"""
    v = arrays.positions.astype(np.float64)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    nrm = np.cross(e1, e2)
    size = np.sqrt(np.linalg.norm(nrm, axis=1))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    out = np.zeros(len(points), bool)
    for first in range(0, len(points), 512):
        s = np.asarray(points[first:first + 512], np.float64)[:, None, :] - v[None, :, 0]
        h = np.abs((s * nrm[None]).sum(2)) / size[None]
        p1, p2 = (s * e1[None]).sum(2), (s * e2[None]).sum(2)
        den = d11 * d22 - d12 * d12
        a, b = (p1 * d22 - p2 * d12) / den, (p2 * d11 - p1 * d12) / den
        eps = 1e-5
        out[first:first + 512] = ((h < eps) & (a > -eps) & (b > -eps) & (a + b < 1 + eps)).any(1)
    return out


_cases = {}
_answers = {}


def case(pkg, name: str, s_exp: int) -> Case:
    if (name, s_exp) not in _cases:
        _cases[(name, s_exp)] = make_case(pkg, name, s_exp)
    return _cases[(name, s_exp)]


def closest(pkg, name: str, s_exp: int):
    """(hits, counters) of ray_query_ref.trace for the case, once"""
    key = ("closest", name, s_exp)
    if key not in _answers:
        c = case(pkg, name, s_exp)
        _answers[key] = R.trace(c.arrays, c.o, c.d, c.tmax)
    return _answers[key]


def all_hits(pkg, name: str, s_exp: int):
    """(hits [n, 8], counts, counters) of multi_hit_ref.all_hits for the case, once"""
    import multi_hit_ref as M
    key = ("all", name, s_exp)
    if key not in _answers:
        c = case(pkg, name, s_exp)
        _answers[key] = M.all_hits(c.arrays, c.o, c.d, c.tmax, max_hits=8)
    return _answers[key]


def fast_class(c: Case) -> np.ndarray:
    """bool [n]: the ray is in the "fast" class (else "divide"), by the restated predicates and the TABLE's flag"""
    return R.fast_division(expected_flag(c.name, c.s_exp), c.o, c.d)
