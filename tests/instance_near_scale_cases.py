"""Instanced within-radius queries at the cells of tests/instance_point_scale_cases.py: the shared case generator of
tests/test_instance_near_scale_reference.py (CPU) and tests/test_gpu_instance_near_scale.py (GPU).  No test and no GPU in here.

The set and the cells are instance_point_scale_cases' own (9 instances over lobed_528 and small_trisrc, TRIANGLES triangles;
every key of SC.CELLS).  Only the points differ:

  - instance_near_cases.world_points (the wider radii on every even finite-radius point) on the cell's maps; for the world,
    scene, cancel, ties and subnormal cells on the base maps, then scaled as SC.cell scales them.
  - the RIM class.  The finite-radius points (radius class 1) in index order, by their rank r among them: ranks 4m and 4m + 1
    form a pair (half of the finite-radius points, 15 % of all, chosen by index alone).  The second takes the first's p, and
    both take a radius from the restatement of THIS cell: d = the dist2 of p's j-th nearest pair over the whole set
    (near_over_instances with radius +inf and K = 65), j = RIM_J[m % 8]; the first gets max_dist2 = d, the second
    nextafter(d) towards -inf.  With d the count is j plus the pairs that tie with the j-th; one step under it, the number of
    pairs strictly nearer: the pair differs exactly by the inclusive `<=` against max_dist2.  (Where every dist2 is 0 the
    second radius is the negative subnormal and its point is not walked.)  The radii come from the cell's own restatement,
    not from the base cell's scaled, so that they sit on a pair's dist2 in the outside cells too.

SMALL is a second set for the two ALL_ZERO cells, whose nine-instance answer is (instance 0, triangles 0..K-1) alone:
one triangle, 11-triangle leaf, one triangle, 11-triangle leaf, lobed_528, so that the first 64 keys span five instances and
the first 8 span two.

Measured on the restatement at K = 64 (tests/test_instance_near_scale_reference.py asserts each figure's consequence), the
shares of instance_near_cases.shares in per cent of the 1,536 points, in its order (count 0 walked, count 1 to 8, count 9 to
64, count above 64, finite radius with two or more instances held, adjacent records tie across instances), then the share of
the rim pairs whose two counts differ:
  cell              0 walked  1..8  9..64  > 64  two held  cross ties   rim pairs split (of)
  world -70           9.9    13.0    8.0   52.1    10.2     30.9        100 (123)
  world -64          14.1    11.1    7.0   52.0    10.2     16.9        100 (123)
  world -40          14.1    11.1    7.0   52.0    10.2     16.9        100 (123)
  world -31          14.0    10.9    7.3   51.9    10.1     16.9        100 (123)
  world -20 .. 33    11.0    11.3    7.4   51.8    10.2     16.9        100 (123)    (and the four cancel cells)
  world 40           12.3    10.4    6.9   52.0    10.1     16.8        100 (123)
  world 63           13.0     9.8    6.2   52.7     9.4     13.2        100 (123)
  world 64           12.8     9.7    6.1   52.9     9.5     13.0        100 (123)
  scene -64, -40, 40, 64: the figures of world -64, -40, 40, 64
  far 12             13.5     8.7    7.1   53.1     9.0     21.6        100 (119)
  far 20              9.9     4.4   10.0   54.9     8.5     29.8        100 (111)
  far 23              9.6     0.13   2.1   66.3     1.2      5.9        100 (113)    (LOW_SHARES)
  ill 6              13.3     8.5    6.2   52.9     6.5     13.0        100 (106)
  ill 12             13.5     8.9    6.3   52.6     7.8     11.6        100 (114)
  ill 20             14.3     8.5    7.4   52.5     7.9     13.3        100 (116)
  negzero 0, 1       12.2     8.9    7.3   54.9    11.5     17.6        100 (109)
  ties -90, subnormal -70: 78.4 % of the points are walked and count all 13,152; the other shares are 0; every rim pair
                     splits (13,152 on the dist2, not walked one step under it).
Without the rim class "count 1 to 8" is 2.2 to 4.3 % across the cells.  Every rim pair splits because a radius one step under
the j-th dist2 never counts the j-th pair.
"""
from __future__ import annotations

import numpy as np

import instance_near_cases as NC
import instance_near_ref as IN
import instance_point_cases as IC
import instance_point_scale_cases as SC
import point_scale_cases as PC

F = np.float32
CELLS, ALL_ZERO, SCENES, INSTANCES, POINTS, SEED = SC.CELLS, SC.ALL_ZERO, SC.SCENES, SC.INSTANCES, SC.POINTS, SC.SEED
TRIANGLES = 13152
RIM_J = (1, 2, 4, 5, 8, 9, 64, 65)
RIM_K = 65
FLOOR = NC.FLOOR
MIN_RIM_SPLIT = 0.04
COVARIANT, OUTSIDE = SC.COVARIANT, SC.OUTSIDE

# TABLE: one character per entry of SC.S_EXPONENTS for the ("world", k) cells, "c" covariant (every record of every point at
# K = 64, every instance index and every count equals the k = 0 answer with q x 2^k and dist2 x 2^2k, bit for bit), "o" outside.
# MEASURED on the CPU with the restatement alone, POINTS points per cell: the share of points whose 64 records, 64 instance
# indices and count all equal the scaled k = 0 answer, and of equal counts alone:
#   k         -70    -64    -40    -31    -20      0     20     32     33     40     63     64
#   answers  32.62  37.24  38.93  56.90  100    100    100    99.87  98.76  42.38  33.40  33.20 %
#   counts   75.85  82.10  81.84  94.27  100    100    100    100    99.48  83.40  82.03  81.71 %
# (point_scale_cases.py's reasons, and its "near" row: the same arithmetic over EVERY pair kept, so a narrower range than the
# closest point's; at k = 32 two points' far records differ.  In the outside cells the rim radii, taken from the cell's own
# restatement, are not the scaled k = 0 radii either.)
#        -70-64-40-31-20  0 20 32 33 40 63 64
TABLE = "o  o  o  o  c  c  c  o  o  o  o  o".replace(" ", "")

# The shares of instance_near_cases.shares that are exempt from FLOOR, per cell: {cell: {share: measured value}}.  Only
# ("far", 23) may appear here, with these three: its float grid (one world size: SC's module doc) is coarser than most
# triangles, corners coincide and whole groups of pairs tie, so near sets of 1 to 64 pairs hardly exist.  Measured: 2 points,
# 33 points and 18 points of 1,536.
LOW_SHARES = {("far", 23): {"count 1 to 8": 2 / 1536, "count 9 to 64": 33 / 1536, "finite radius, two or more instances held": 18 / 1536}}


def flag(k: int) -> str:
    return COVARIANT if TABLE[SC.S_EXPONENTS.index(k)] == "c" else OUTSIDE


class Cell(SC.Cell):
    """SC.Cell with `rim`: int [pairs, 3] of (index of the point at the value, index of the point one step under, j)"""

    def __init__(self, key, scene_exp, of, maps, points, kind, radius, rim, positions=None, names=None):
        super().__init__(key, scene_exp, of, maps, points, kind, radius)
        self.rim, self._positions, self.names = rim, positions, names

    def positions(self, pkg):
        return self._positions if self._positions is not None else super().positions(pkg)

    def triangles(self, pkg):
        p = self.positions(pkg)
        return sum(len(p[s]) // 9 for s in self.of)


_memo = {}


def base_points(pkg):
    """instance_near_cases.world_points on the base set"""
    if "base" not in _memo:
        of, maps, *_ = SC.base(pkg)
        positions = [PC.scaled_positions(pkg, name, 0) for name in SCENES]
        _memo["base"] = NC.world_points(positions, of, maps, POINTS, seed=SEED + 1)
    return _memo["base"]


def rim_pairs(radius):
    """int [pairs, 3]: (first, second, j) by the rank among the finite-radius points (module doc)"""
    finite = np.nonzero(radius == 1)[0]
    m = np.arange(len(finite) // 4)
    return np.stack([finite[4 * m], finite[4 * m + 1], np.asarray(RIM_J)[m % len(RIM_J)]], axis=1)


def with_rim(positions, of, maps, pts, kind, radius):
    """the points with the rim class written in (copies), and the pairs"""
    pts, kind = pts.copy(), kind.copy()
    rim = rim_pairs(radius)
    a, b, j = rim[:, 0], rim[:, 1], rim[:, 2]
    pts["p"][b], kind[b] = pts["p"][a], kind[a]
    every = pts[a].copy()
    every["max_dist2"] = np.inf
    records, _, counts = IN.near_over_instances(positions, of, maps, every, RIM_K)
    assert (counts >= RIM_K).all()
    d = records["dist2"][np.arange(len(a)), j - 1]
    pts["max_dist2"][a] = d
    pts["max_dist2"][b] = np.nextafter(d, F(-np.inf))
    return pts, kind, rim


def cell(pkg, key) -> Cell:
    if key in _memo:
        return _memo[key]
    c = SC.cell(pkg, key)                   # the maps, the scenes' exponent (and its points, unused)
    positions = [PC.scaled_positions(pkg, name, 0) for name in SCENES]
    cls, x = key
    with np.errstate(all="ignore"):
        if cls in ("world", "ties", "scene"):
            pts, kind, radius = base_points(pkg)
            pts = PC.scaled_points(pts, x)
        elif cls == "cancel":
            pts, kind, radius = base_points(pkg)
        elif cls == "subnormal":
            pts, kind, radius = base_points(pkg)
            pts = SC.scaled_points_twice(pts, x, x)
        elif cls == "far":
            pts, kind, radius = NC.world_points(positions, c.of, c.maps, POINTS, seed=SEED + 10 + x)
        elif cls == "ill":
            pts, kind, radius = NC.world_points(positions, c.of, c.maps, POINTS, seed=SEED + 40 + x)
        elif cls == "negzero":
            pts, kind, radius = NC.world_points(positions, c.of, SC.negzero_maps(pkg, 0), POINTS, seed=SEED + 3)
        else:
            raise KeyError(key)
        pts, kind, rim = with_rim(c.positions(pkg), c.of, c.maps, pts, kind, radius)
    _memo[key] = Cell(key, c.scene_exp, c.of, c.maps, pts, kind, radius, rim)
    return _memo[key]


expected_cell = SC.expected_cell
walked = SC.walked


# ---- the second, small set of the ALL_ZERO cells ----------------------------------------------------------------------------
SMALL = ("one triangle", "11-triangle leaf", "one triangle", "11-triangle leaf", "lobed_528")
SMALL_KINDS = ("rotation_nonuniform", "shear", "translation", "mirror", "rotation_uniform")
SMALL_POINTS = 512


def small_cell(pkg, key) -> Cell:
    """the set SMALL at an ALL_ZERO cell: the members' positions at 2^scene_exp, the maps and points scaled as SC.cell does"""
    assert key in ALL_ZERO
    if ("small", key) in _memo:
        return _memo[("small", key)]
    distinct = ["one triangle", "11-triangle leaf", "lobed_528"]
    base = [np.asarray(IC.TINY[n], F).reshape(-1) for n in distinct[:2]] + [PC.scaled_positions(pkg, "lobed_528", 0)]
    of = [distinct.index(n) for n in SMALL]
    rng = np.random.default_rng(SEED + 70)
    maps = np.stack([IC.map_of(SMALL_KINDS[i], rng, base[s], 1.5) for i, s in enumerate(of)]).astype(F)
    pts, kind, radius = NC.world_points(base, of, maps, SMALL_POINTS, seed=SEED + 71)
    cls, x = key
    with np.errstate(all="ignore"):
        if cls == "ties":
            scene_exp, maps, pts = 0, maps * F(2.0 ** x), PC.scaled_points(pts, x)
        else:
            scene_exp = x
            maps = maps * F(2.0 ** x)
            maps[:, :, 3] *= F(2.0 ** x)
            pts = SC.scaled_points_twice(pts, x, x)
        positions = [(p * F(2.0 ** scene_exp)).astype(F) for p in base]
    _memo[("small", key)] = Cell(("small",) + key, scene_exp, of, maps, pts, kind, radius, np.zeros((0, 3), np.int64), positions, list(SMALL))
    return _memo[("small", key)]


def first_keys(pkg, c: Cell, k):
    """(instances [k], triangles [k]) of the first k keys in (instance, triangle) order: the answer where every dist2 is 0"""
    p = c.positions(pkg)
    inst = np.concatenate([np.full(len(p[s]) // 9, i, np.int32) for i, s in enumerate(c.of)])
    tri = np.concatenate([np.arange(len(p[s]) // 9, dtype=np.int32) for s in c.of])
    return inst[:k], tri[:k]


def restated(pkg, c: Cell, device=None):
    """(records [n, 64], instances [n, 64], counts [n]) of the restatement, once per cell"""
    if ("restated", c.key) not in _memo:
        _memo[("restated", c.key)] = IN.near_over_instances(c.positions(pkg), c.of, c.maps, c.points, 64, device=device)
    return _memo[("restated", c.key)]


def scale_answer(records, k, pts_scaled):
    return PC.scale_closest(records, k, pts_scaled)


def rim_counts(c: Cell, counts):
    """(counts at the value, counts one step under) of the cell's rim pairs"""
    return counts[c.rim[:, 0]], counts[c.rim[:, 1]]
