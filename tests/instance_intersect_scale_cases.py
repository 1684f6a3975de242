"""Instanced triangle-intersection queries at the cells of tests/instance_point_scale_cases.py and at the classes of
tests/instance_overlap_scale_cases.py (its module doc: the guard cells, the NaN-corner cell, the draws at 2^-147): the shared case
generator of tests/test_instance_intersect_scale_reference.py (CPU) and tests/test_gpu_instance_intersect_scale.py (GPU).  No test
and no GPU in here.

The set and the cells are instance_point_scale_cases' own.  A cell carries QUERIES query triangles [n, 3, 3] instead of points:

  world, scene, ties, subnormal, guard   the k = 0 queries scaled by the cell's power or powers of two
                                         (intersect_scale_cases.scaled_queries).
  cancel                                 the k = 0 queries unchanged.
  negzero                                queries made on the +0 maps, for both signs.
  far, ill                               queries made on the cell's own merged scene.
  ("world", 100)                         as the box query's: the cell of the fmin / fmax mutant without a NaN corner.
  nan                                    the k = 0 queries x 2^122, clipped to +-FLT_MAX; a query that is not walked at k = 0 is
                                         left as it was.

The queries of a set of maps are instance_intersect_cases.world_queries (seed 31) with every query whose index is 3 mod 4
replaced by the SMALL class, because world_queries, balanced for instance_near_cases.nine_instances, leaves "n 1 to 8" and
"first 8 of two or more instances" under the floor on this set:
  - index 3 mod 8: a small triangle through a surface point of the merged scene, crossing the surface there, its size
    SMALL_SIZES[m] times the square root of that triangle's area: it meets that triangle and perhaps its neighbours;
  - index 7 mod 8: the same through a surface point of instance 1, whose exact duplicate is instance 4: every pair comes twice,
    once in each, so the first 8 hold two instances.
At the far and ill cells the surface point is a mapped fp32 corner and the size GRID_STEPS[m] ulps of the corner's largest
coordinate (triangles of the collapsed grid's own scale), for both halves of the class.

MEASURED on the restatement (instance_intersect_ref.intersect_over_instances at K = 64), QUERIES queries a cell;
tests/test_instance_intersect_scale_reference.py asserts each figure (the table's from SHARE_COUNTS, in queries).
The shares of instance_intersect_cases.shares in per cent, in its order (n 0, n 1 to 8, n 9 to 64, n above 64, first 8 of two or
more instances, first 64 of two or more instances), and the queries walked (of 256):
  cell                       n 0   1..8  9..64  > 64  first 8 span  first 64 span  walked
  world -70                  28.1  12.5   29.3  30.1     16.8           27.7        217
  world -64, 100             16.4  20.3   33.2  30.1     21.5           32.8        248     (and scene -64)
  world 63, 64               16.4  20.3   33.2  30.1     21.9           32.8        248     (and scene 64)
  world -40 .. 32            26.6  27.3   23.8  22.3     19.5           38.3        248     (and scene -40, the four cancel cells;
                                                                                            world 33: first 64 span 39.8)
  world 40                   23.4  26.6   22.7  27.3     19.5           30.5        248     (and scene 40)
  far 12                     56.6  14.5   28.9   0.0     15.6           21.9        238     (LOW_SHARES)
  far 20                     66.0   0.0   21.1  12.9      1.6           18.8        192     (LOW_SHARES)
  far 23                     76.2   3.5   19.5   0.8      3.5           19.9        140     (LOW_SHARES)
  ill 6                      30.1  12.1   33.6  24.2     16.8           34.8        241
  ill 12                     25.4  16.8   27.3  30.5     14.1           31.3        235
  ill 20                     26.2  12.9   32.4  28.5     16.8           32.0        234
  negzero 0, 1               22.7  29.3   25.4  22.7     22.3           44.5        248
  ties -90, subnormal -70, guard -112 .. -106: no query is walked and n = 0 throughout (LOW_SHARES)
  nan 70                      3.1   0.0    0.0  96.9      0.0           96.9        248     (LOW_SHARES)
With the SMALL class every band of ("world", 0) and of the cells scaled from it is over 12 %, with no exemption.  A cell has
256 queries so that its brute force stays at a few seconds; the mix above is theirs.

Where every world coordinate is under some 2^-75 the normals (of degree 2) underflow to (0, 0, 0): the header walks no such query
and rejects every such triangle.  So the guard cells and ("draws", -147), whose query is the point triangle on a draw's corner,
cannot show the top level's guard in this query: n = 0 whatever the guard does.  The guard is shown in the box query
(tests/instance_overlap_scale_cases.py), which compiles the same stored_overlaps of instance/image_box.h; here those cells only
pin that an unwalked query begins no walk and writes -1 and 0.
"""
from __future__ import annotations

import numpy as np

import instance_intersect_cases as XC
import instance_intersect_ref as II
import instance_overlap_scale_cases as XS
import instance_point_ref as IP
import instance_point_scale_cases as SC
import intersect_ref as IR
import intersect_scale_cases as TS

F = np.float32
FLT_MAX = XS.FLT_MAX
SCENES, INSTANCES, SEED = SC.SCENES, SC.INSTANCES, SC.SEED
QUERIES, QUERY_SEED = 256, XC.NINE_QUERY_SEED
TRIANGLES = XS.TRIANGLES
FLOOR = XC.FLOOR
KEPT, CHANGED = XS.KEPT, XS.CHANGED
SMALL_EVERY = 4
SMALL_SIZES = (0.15, 0.3, 0.5, 0.8)
GRID_STEPS = (0.5, 1.0, 2.0, 3.0, 6.0, 12.0, 24.0, 48.0)
DUPLICATED = 1                      # instance 4 is its exact duplicate
GUARD_CELLS, NAN_CELL, DRAWS_KEY = XS.GUARD_CELLS, XS.NAN_CELL, XS.DRAWS_KEY
FMIN_WORLD = XS.FMIN_WORLD
CELLS = SC.CELLS + [("world", FMIN_WORLD)] + GUARD_CELLS + [NAN_CELL]
ALL_ZERO = SC.ALL_ZERO
FORM_INSTANCES = (1, 3, 8)          # the duplicated one, a general map, the shear over small_trisrc
FORM_CELLS = (("world", 0), ("world", 40), ("far", 20), ("ill", 12))


def flag(k: int) -> str:
    return KEPT if TABLE[SC.S_EXPONENTS.index(k)] == "k" else CHANGED


class Cell(XS.Cell):
    """XS.Cell with query triangles float32 [n, 3, 3] in place of the boxes; `small` marks the SMALL class"""

    def __init__(self, key, scene_exp, of, maps, queries, small=None, positions=None):
        SC.Cell.__init__(self, key, scene_exp, of, maps, queries, None, None)
        self.queries, self._positions = queries, positions
        self.small = np.zeros(len(queries), bool) if small is None else small


_memo = {}


def ring(rng, n):
    """unit vectors [n, 3, 3]: three directions 120 degrees apart in a random plane"""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    angles = rng.random((n, 1)) * 2 * np.pi + np.array([[0.0, 2.1, 4.2]])
    return np.cos(angles)[:, :, None] * u[:, None, :] + np.sin(angles)[:, :, None] * w[:, None, :]


def world_queries(positions, of, maps, seed, on_grid=False):
    """(queries [QUERIES, 3, 3], the SMALL class's mask) on the merged scene of the maps (module doc)"""
    out = XC.world_queries(positions, of, maps, QUERIES, seed).copy()
    merged, first = IP.merged_positions(positions, of, maps)
    tris = merged.reshape(-1, 3, 3).astype(np.float64)
    rng = np.random.default_rng(seed + 5)
    at = np.nonzero(np.arange(QUERIES) % SMALL_EVERY == SMALL_EVERY - 1)[0]
    twice = (at % (2 * SMALL_EVERY)) == 2 * SMALL_EVERY - 1
    t = np.where(twice, rng.integers(first[DUPLICATED], first[DUPLICATED + 1], len(at)), rng.integers(0, len(tris), len(at)))
    m = np.arange(len(at)) // 2
    if on_grid:
        p = tris[t, rng.integers(0, 3, len(at))]
        size = np.asarray(GRID_STEPS)[m % len(GRID_STEPS)] * np.spacing(np.abs(p).max(1).astype(F)).astype(np.float64)
    else:
        b = rng.random((len(at), 2))
        b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b) * 0.8 + 0.1 * (1 - 0.8)
        v = tris[t]
        p = v[:, 0] + b[:, :1] * (v[:, 1] - v[:, 0]) + b[:, 1:] * (v[:, 2] - v[:, 0])
        area = 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
        size = np.asarray(SMALL_SIZES)[m % len(SMALL_SIZES)] * np.sqrt(area)
    out[at] = (p[:, None, :] + size[:, None, None] * ring(rng, len(at))).astype(F)
    small = np.zeros(QUERIES, bool)
    small[at] = True
    return out, small


def base_queries(pkg):
    if "base" not in _memo:
        of, maps, *_ = SC.base(pkg)
        _memo["base"] = world_queries(XS.unscaled(pkg), of, maps, QUERY_SEED)
    return _memo["base"]


def nan_queries(pkg):
    base, small = base_queries(pkg)
    out = base.copy()
    go = IR.walked(base)
    out[go] = XS.clipped(base[go], XS.NAN_WORLD)
    return out, small


def cell(pkg, key) -> Cell:
    if key in _memo:
        return _memo[key]
    cls, x = key
    positions = XS.unscaled(pkg)
    with np.errstate(all="ignore"):
        if cls in ("world", "ties", "scene", "guard"):
            c = SC.cell(pkg, ("world", x) if cls == "guard" else key)
            q, small = base_queries(pkg)
            out = Cell(key, c.scene_exp, c.of, c.maps, TS.scaled_queries(q, x), small)
        elif cls == "cancel":
            c = SC.cell(pkg, key)
            out = Cell(key, c.scene_exp, c.of, c.maps, *base_queries(pkg))
        elif cls == "subnormal":
            c = SC.cell(pkg, key)
            q, small = base_queries(pkg)
            out = Cell(key, c.scene_exp, c.of, c.maps, TS.scaled_queries(TS.scaled_queries(q, x), x), small)
        elif cls in ("far", "ill"):
            c = SC.cell(pkg, key)
            out = Cell(key, 0, c.of, c.maps, *world_queries(positions, c.of, c.maps, SEED + (10 if cls == "far" else 40) + x, on_grid=True))
        elif cls == "negzero":
            c = SC.cell(pkg, key)
            out = Cell(key, 0, c.of, c.maps, *world_queries(positions, c.of, SC.negzero_maps(pkg, 0), SEED + 3))
        elif cls == "nan":
            of, *_ = SC.base(pkg)
            out = Cell(key, 64, of, XS.nan_maps(pkg, x), *nan_queries(pkg))
        else:
            raise KeyError(key)
    _memo[key] = out
    return out


expected_cell = SC.expected_cell
world_corners = XS.world_corners
stored_boxes = XS.stored_boxes


def restated(pkg, c: Cell, skip_shared=False):
    """(triangles [n, 64], instances [n, 64], counts [n]) of the restatement, once per cell"""
    if ("restated", c.key, skip_shared) not in _memo:
        _memo[("restated", c.key, skip_shared)] = II.intersect_over_instances(c.positions(pkg), c.of, c.maps, c.queries, 64, skip_shared)
    return _memo[("restated", c.key, skip_shared)]


def restate_both(scene_positions, of, maps, queries, k=64):
    """the restatement without and with SKIP_SHARED from one brute force: the shared-corner rule clears the pairs with a corner
    in common (three ==) and touches nothing else"""
    merged, first = IP.merged_positions(scene_positions, of, maps)
    member = IR.intersects(queries, merged, False)
    q, t = IR.corners_of(queries), merged.reshape(-1, 3, 3)
    shared = np.concatenate([II.shares_matrix(q[s:s + 32], t) for s in range(0, len(q), 32)])
    return II.from_membership(member, first, k), II.from_membership(member & ~shared, first, k)


def draws_cell(pkg=None) -> Cell:
    """instance_overlap_scale_cases.draws_cell with query i the triangle whose three corners are draw i's fp32 world corner"""
    if DRAWS_KEY not in _memo:
        c = XS.draws_cell(pkg)
        w = c.boxes["lo"]
        q = np.ascontiguousarray(np.repeat(w[:, None, :], 3, axis=1), F)
        _memo[DRAWS_KEY] = Cell(DRAWS_KEY, 0, c.of, c.maps, q, positions=c.positions(pkg))
    return _memo[DRAWS_KEY]


# TABLE: one character per entry of SC.S_EXPONENTS for the ("world", k) cells, "k" kept (every query's 64 indices, 64 instance
# indices and count are the k = 0 answer), "c" changed.  MEASURED on the CPU with the restatement alone, the share of queries that
# keep their k = 0 answer:
#   k       -70    -64    -40    -31    -20      0     20     32     33     40     63     64    (KEPT_COUNTS; 25.78 % at k = 100)
#   kept   25.00  26.17  98.83  100    100    100    100    100    92.97  60.16  22.66  22.66 %
# (intersect_scale_cases.py's reasons: the projections are of degree 3 and 4 and leave float32's normal range first.)
#        -70-64-40-31-20  0 20 32 33 40 63 64
TABLE = "c  c  c  k  k  k  k  k  c  c  c  c".replace(" ", "")

# The shares of instance_intersect_cases.shares that are exempt from FLOOR, per cell: {cell: {share: measured value}}, the value
# being the asserted lower bound.  The far cells: corners coincide on the float grid, whole patches are degenerate, and what is left
# meets either nothing or a great deal.  The cells where every world coordinate underflows (ties, subnormal, guard): no query is
# walked, by the header's degenerate rule, so n = 0 throughout; what they show on the GPU is that an unwalked query begins no
# walk.  The NaN-corner cell: every walked query meets the triangles of the four instances whose corners are all NaN.
NOTHING = {"n 1 to 8": 0.0, "n 9 to 64": 0.0, "n above 64": 0.0, "first 8 of two or more instances": 0.0,
           "first 64 of two or more instances": 0.0}
LOW_SHARES = {
    ("far", 12): {"n above 64": 0 / 256},
    ("far", 20): {"n 1 to 8": 0 / 256, "first 8 of two or more instances": 4 / 256},
    ("far", 23): {"n 1 to 8": 9 / 256, "n above 64": 2 / 256, "first 8 of two or more instances": 9 / 256},
    NAN_CELL: {"n 0": 8 / 256, "n 1 to 8": 0.0, "n 9 to 64": 0.0, "first 8 of two or more instances": 0.0},
    **{key: NOTHING for key in list(ALL_ZERO) + GUARD_CELLS},
}

# the corner formula's mutants (tests/test_instance_overlap_scale_reference.py's ROWS): the queries (of 256) whose brute-force
# answer changes, and the cells where none does
ROW_MUTANTS = {
    "c. a fused corner formula": {"cells": {("ill", 20): 33, NAN_CELL: 248}, "controls": [("negzero", 0)]},
    "d. subnormal results flushed": {"cells": {}, "controls": [("world", -70), ("world", 0)]},
    "e. the zero entries' products added": {"cells": {}, "controls": [("world", 0), NAN_CELL]},
}

# the walk's mutants: the queries among the first 192 of the named cell that change
WALK_MUTANTS = {"b": 187, "f": 57, "k": 9, "k control": 97}
SKIP_SHOWS = {(("world", 0), 9): 1, (("far", 12), 8): 0, (("far", 12), 9): 2, (("far", 20), 8): 0, (("far", 20), 9): 1, (("far", 23), 8): 1,
              (("far", 23), 9): 2}
# The six shares of instance_intersect_cases.shares per cell and the queries walked, in queries of 256: what the module doc's table
# states in per cent, asserted for equality
SHARE_COUNTS = {
    ('world', -70): (72, 32, 75, 77, 43, 71, 217),
    ('world', -64): (42, 52, 85, 77, 55, 84, 248),
    ('world', -40): (68, 70, 61, 57, 50, 98, 248),
    ('world', -31): (68, 70, 61, 57, 50, 98, 248),
    ('world', -20): (68, 70, 61, 57, 50, 98, 248),
    ('world', 0): (68, 70, 61, 57, 50, 98, 248),
    ('world', 20): (68, 70, 61, 57, 50, 98, 248),
    ('world', 32): (68, 70, 61, 57, 50, 98, 248),
    ('world', 33): (68, 70, 61, 57, 50, 102, 248),
    ('world', 40): (60, 68, 58, 70, 50, 78, 248),
    ('world', 63): (42, 52, 85, 77, 56, 84, 248),
    ('world', 64): (42, 52, 85, 77, 56, 84, 248),
    ('scene', -64): (42, 52, 85, 77, 55, 84, 248),
    ('scene', -40): (68, 70, 61, 57, 50, 98, 248),
    ('scene', 40): (60, 68, 58, 70, 50, 78, 248),
    ('scene', 64): (42, 52, 85, 77, 56, 84, 248),
    ('cancel', -64): (68, 70, 61, 57, 50, 98, 248),
    ('cancel', -40): (68, 70, 61, 57, 50, 98, 248),
    ('cancel', 40): (68, 70, 61, 57, 50, 98, 248),
    ('cancel', 64): (68, 70, 61, 57, 50, 98, 248),
    ('far', 12): (145, 37, 74, 0, 40, 56, 238),
    ('far', 20): (169, 0, 54, 33, 4, 48, 192),
    ('far', 23): (195, 9, 50, 2, 9, 51, 140),
    ('ill', 6): (77, 31, 86, 62, 43, 89, 241),
    ('ill', 12): (65, 43, 70, 78, 36, 80, 235),
    ('ill', 20): (67, 33, 83, 73, 43, 82, 234),
    ('negzero', 0): (58, 75, 65, 58, 57, 114, 248),
    ('negzero', 1): (58, 75, 65, 58, 57, 114, 248),
    ('ties', -90): (256, 0, 0, 0, 0, 0, 0),
    ('subnormal', -70): (256, 0, 0, 0, 0, 0, 0),
    ('world', 100): (42, 52, 85, 77, 55, 84, 248),
    ('guard', -112): (256, 0, 0, 0, 0, 0, 0),
    ('guard', -110): (256, 0, 0, 0, 0, 0, 0),
    ('guard', -109): (256, 0, 0, 0, 0, 0, 0),
    ('guard', -108): (256, 0, 0, 0, 0, 0, 0),
    ('guard', -106): (256, 0, 0, 0, 0, 0, 0),
    ('nan', 70): (8, 0, 0, 248, 0, 248, 248),
}
# the queries (of 256) whose whole K = 64 answer is the k = 0 answer, per world exponent (TABLE's percentages)
KEPT_COUNTS = {
    -70: 64,
    -64: 67,
    -40: 253,
    -31: 256,
    -20: 256,
    0: 256,
    20: 256,
    32: 256,
    33: 238,
    40: 154,
    63: 58,
    64: 58,
    100: 66,
}
# instance_intersect_cases.assert_mixed's other half: the cells where nq, nt and each of the nine edge axes is the first to separate
# some pair.  At the others products underflow or overflow and some axis separates nothing first (asserted either way).
ELEVEN_AXES_SEPARATE = [('world', -40), ('world', -31), ('world', -20), ('world', 0), ('world', 20), ('world', 32), ('world', 33), ('world', 40), ('scene', -40), ('scene', 40), ('cancel', -64), ('cancel', -40), ('cancel', 40), ('cancel', 64), ('far', 20), ('ill', 12), ('ill', 20), ('negzero', 0), ('negzero', 1)]
# the instance form's own queries at the far cells, per instance: (triangles with two corners on one grid point, triangles walked)
FAR_COLLAPSED = {
    12: {1: (0, 2208), 3: (0, 2208), 8: (0, 528)},
    20: {1: (940, 1259), 3: (1338, 793), 8: (124, 387)},
    23: {1: (2186, 22), 3: (2198, 10), 8: (526, 2)},
}
# fmin / fmax in the two-operand min and max: (queries whose answer changes, pairs added, pairs lost)
FMIN_CHANGES = {("world", FMIN_WORLD): (3, 0, 5), NAN_CELL: (248, 0, 32240), ("world", 64): (167, 44, 49143), ("world", 0): (0, 0, 0)}
