"""Instanced box-overlap queries at the cells of tests/instance_point_scale_cases.py and at three classes of their own: the
shared case generator of tests/test_instance_overlap_scale_reference.py (CPU) and tests/test_gpu_instance_overlap_scale.py (GPU).
No test and no GPU in here.

The set and the cells are instance_point_scale_cases' own (9 instances over lobed_528 and small_trisrc, 13,152 triangles; every
key of SC.CELLS).  A cell carries BOXES boxes instead of points:

  world, scene, ties, subnormal   the k = 0 boxes (instance_overlap_cases.world_boxes on the base set, seed 21), scaled by the
                                  cell's power or powers of two (overlap_scale_cases.scaled_boxes).
  cancel                          the k = 0 boxes unchanged.
  negzero                         world_boxes on the +0 maps, for both signs.
  far, ill                        world_boxes on the cell's own merged scene, and the GRID class: every box whose index is 5
                                  mod 6 is replaced by a box about a mapped fp32 corner of the cell (drawn over the merged
                                  corners) with half extent GRID_STEPS[m] ulps of that corner's largest coordinate, so that small
                                  answers exist where the float grid has collapsed and overlap_cases' sizes, taken from the
                                  scene's extent, hold hundreds of coincident corners.

and three classes that the point cells do not have:

  ("world", 100)    maps and boxes x 2^100: every corner finite, the edge products of the header's stage 2 past 2^128.  The
                    cell that tells fmin / fmax from the header's comparisons without a NaN corner.
  ("guard", k)      k in GUARD_EXPONENTS: ("world", k) about the top level's guard 2^-109, so that stored ends and query ends lie
                    on both sides of it.
  ("nan", NAN_E)    the scenes at 2^64, the linear parts x 2^NAN_E, the translations and the boxes x 2^122 and clipped to
                    +-FLT_MAX (a box that is not walked at k = 0 is left as it was).  Every map is finite and so is every
                    box; products overflow and inf - inf among the partial sums of the corner formula makes NaN corners.
  DRAWS             ("draws", -147): not the nine-instance set.  The draws of
                    tests/test_instance_overlap_reference.py::point_triangle_draws at 2^-147 in which the fp32 corner leaves the
                    box the top level stores for it, the first DRAWS_KEPT of them: instance i is draw i's one-corner scene
                    (a triangle whose three corners are the corner, in a root box that is the corner) under draw i's map, and
                    box i the zero-extent box on draw i's fp32 world corner.

MEASURED on the restatement (instance_overlap_ref.overlap_over_instances at K = 64), BOXES boxes a cell;
tests/test_instance_overlap_scale_reference.py asserts each figure (the table's from SHARE_COUNTS, in boxes).  The shares of instance_overlap_cases.shares in
per cent, in its order (walked and touching nothing, n 1 to 8, n 9 to 64, n above 64, first 8 of two or more instances, first 64
of two or more instances):
  cell                       0 walked  1..8  9..64  > 64  first 8 span  first 64 span
  world -70                    11.1     7.6   41.9  34.7      7.4          41.1
  world -64, 63, 64            11.5     7.9   41.6  34.4      7.7          41.0     (and scene -64, 64)
  world -40                    11.6     8.3   41.2  34.3      7.4          40.7     (and scene -40)
  world -31 .. 40              12.0     9.1   40.0  34.3      7.4          40.6     (and scene 40, the four cancel cells)
  world 100                    10.9     7.7   41.7  35.0      5.9          41.9
  guard -112 .. -106           10.7     6.5   43.2  35.0      6.3          42.4
  ties -90                     10.7     6.5   43.2  35.0      6.3          42.3
  subnormal -70                10.7     7.2   41.9  35.5      6.3          42.3
  far 12                       13.1    13.8   16.0  52.6      9.2          17.7
  far 20                       13.7     1.4   12.0  69.5      1.5          12.1     (LOW_SHARES)
  far 23                       13.6     0.0    0.5  81.2      0.0           0.7     (LOW_SHARES)
  ill 6                        12.3    15.2   13.9  54.3      8.3          18.6
  ill 12                       12.5    15.7   11.9  55.7      7.9          15.4
  ill 20                       13.4    14.8   13.4  53.8      8.5          15.8
  negzero 0, 1                 12.9     9.4   41.1  32.4     15.8          51.7
  nan 70                        0.0     0.0    0.0  95.4      0.0          95.4     (LOW_SHARES)
Where every world coordinate underflows (ties -90, subnormal -70) the answer is still rich: no later axis separates anything
(every later product is 0) and the set is stage 0's.  With the GRID class far 12 and the three ill cells are over the floor in
every band; it cannot help where one grid point holds a patch of every instance.

The NaN-corner cell, e = 70: per instance NAN_TRIANGLES triangles with a NaN corner (5,472 in four instances: the general maps) and INF_TRIANGLES with an infinite one;
495,170 member pairs have a NaN corner, and each of the 1,465 walked boxes holds one.
"""
from __future__ import annotations

import numpy as np

import instance_overlap_cases as XC
import instance_overlap_ref as IO
import instance_point_ref as IP
import instance_point_scale_cases as SC
import overlap_ref as OR
import overlap_scale_cases as OS
import point_scale_cases as PC
from test_instance_overlap_reference import point_triangle_draws

F = np.float32
FLT_MAX = np.finfo(F).max
SCENES, INSTANCES, SEED = SC.SCENES, SC.INSTANCES, SC.SEED
BOXES, BOX_SEED = XC.NINE_BOXES, XC.NINE_BOX_SEED
TRIANGLES = 13152
FLOOR = XC.FLOOR
KEPT, CHANGED = "kept", "changed"
GUARD_EXPONENTS = (-112, -110, -109, -108, -106)
NAN_E = 70
NAN_WORLD = 122
FMIN_WORLD = 100
GRID_EVERY, GRID_AT = 6, 5
GRID_STEPS = (0.0, 0.5, 1.0, 2.0, 3.0, 6.0, 12.0, 24.0)
DRAWS_KEY = ("draws", -147)
DRAWS_KEPT = 48

GUARD_CELLS = [("guard", k) for k in GUARD_EXPONENTS]
NAN_CELL = ("nan", NAN_E)
CELLS = SC.CELLS + [("world", FMIN_WORLD)] + GUARD_CELLS + [NAN_CELL]
ALL_ZERO = SC.ALL_ZERO


def flag(k: int) -> str:
    return KEPT if TABLE[SC.S_EXPONENTS.index(k)] == "k" else CHANGED


class Cell(SC.Cell):
    """SC.Cell with boxes (BOX_DTYPE) in place of the points; `grid` marks the boxes of the GRID class"""

    def __init__(self, key, scene_exp, of, maps, boxes, grid=None, positions=None):
        super().__init__(key, scene_exp, of, maps, boxes, None, None)
        self.boxes, self._positions = boxes, positions
        self.grid = np.zeros(len(boxes), bool) if grid is None else grid

    def positions(self, pkg):
        return self._positions if self._positions is not None else super().positions(pkg)


_memo = {}


def unscaled(pkg):
    return [PC.scaled_positions(pkg, name, 0) for name in SCENES]


def base_boxes(pkg):
    """instance_overlap_cases.world_boxes on the base set"""
    if "base" not in _memo:
        of, maps, *_ = SC.base(pkg)
        _memo["base"] = XC.world_boxes(unscaled(pkg), of, maps, BOXES, BOX_SEED)
    return _memo["base"]


def with_grid(positions, of, maps, boxes, seed):
    """the boxes with the GRID class written in (a copy), and its mask"""
    merged, _ = IP.merged_positions(positions, of, maps)
    corners = merged.reshape(-1, 3)
    rng = np.random.default_rng(seed)
    at = np.nonzero(np.arange(len(boxes)) % GRID_EVERY == GRID_AT)[0]
    c = corners[rng.integers(0, len(corners), len(at))]
    steps = np.asarray(GRID_STEPS, F)[np.arange(len(at)) % len(GRID_STEPS)]
    half = (steps * np.spacing(np.abs(c).max(1))).astype(F)[:, None]
    out = boxes.copy()
    out["lo"][at], out["hi"][at] = c - half, c + half
    grid = np.zeros(len(boxes), bool)
    grid[at] = True
    return out, grid


def clipped(x, k):
    with np.errstate(all="ignore"):
        return np.clip(x * F(2.0 ** k), -FLT_MAX, FLT_MAX).astype(F)


def nan_maps(pkg, e=NAN_E):
    of, maps, *_ = SC.base(pkg)
    m = maps.copy()
    m[:, :, :3] *= F(2.0 ** e)
    m[:, :, 3] = clipped(m[:, :, 3], NAN_WORLD)
    return m


def nan_boxes(pkg):
    base = base_boxes(pkg)
    out = base.copy()
    go = OR.walked(base)
    out["lo"][go], out["hi"][go] = clipped(base["lo"][go], NAN_WORLD), clipped(base["hi"][go], NAN_WORLD)
    return out


def cell(pkg, key) -> Cell:
    if key in _memo:
        return _memo[key]
    cls, x = key
    positions = unscaled(pkg)
    with np.errstate(all="ignore"):
        if cls in ("world", "ties", "scene", "guard"):
            c = SC.cell(pkg, ("world", x) if cls == "guard" else key)
            out = Cell(key, c.scene_exp, c.of, c.maps, OS.scaled_boxes(base_boxes(pkg), x))
        elif cls == "cancel":
            c = SC.cell(pkg, key)
            out = Cell(key, c.scene_exp, c.of, c.maps, base_boxes(pkg))
        elif cls == "subnormal":
            c = SC.cell(pkg, key)
            out = Cell(key, c.scene_exp, c.of, c.maps, OS.scaled_boxes(OS.scaled_boxes(base_boxes(pkg), x), x))
        elif cls in ("far", "ill"):
            c = SC.cell(pkg, key)
            seed = SEED + (10 if cls == "far" else 40) + x
            boxes = XC.world_boxes(positions, c.of, c.maps, BOXES, seed)
            boxes, grid = with_grid(positions, c.of, c.maps, boxes, seed + 1)
            out = Cell(key, 0, c.of, c.maps, boxes, grid)
        elif cls == "negzero":
            c = SC.cell(pkg, key)
            out = Cell(key, 0, c.of, c.maps, XC.world_boxes(positions, c.of, SC.negzero_maps(pkg, 0), BOXES, SEED + 3))
        elif cls == "nan":
            of, *_ = SC.base(pkg)
            out = Cell(key, 64, of, nan_maps(pkg, x), nan_boxes(pkg))
        else:
            raise KeyError(key)
    _memo[key] = out
    return out


expected_cell = SC.expected_cell


def world_corners(pkg, c: Cell):
    return SC.world_corners(pkg, c)


def restated(pkg, c: Cell):
    """(triangles [n, 64], instances [n, 64], counts [n]) of the restatement, once per cell"""
    if ("restated", c.key) not in _memo:
        _memo[("restated", c.key)] = IO.overlap_over_instances(c.positions(pkg), c.of, c.maps, c.boxes, 64)
    return _memo[("restated", c.key)]


def stored_boxes(pkg, c: Cell):
    """instance_point_ref.stored_box of every instance over its member's exact vertex box: [(lo, hi)]"""
    p = c.positions(pkg)
    out = []
    with np.errstate(all="ignore"):
        for i, s in enumerate(c.of):
            v = p[s].reshape(-1, 3)
            out.append(IP.stored_box(c.maps[i], v.min(0), v.max(0))[:2])
    return out


# ---- the draws ----------------------------------------------------------------------------------------------------------------
def draws_cell(pkg=None) -> Cell:
    """the set of DRAWS_KEPT one-corner scenes and the zero-extent boxes on their fp32 world corners (module doc)"""
    if DRAWS_KEY not in _memo:
        kept = []
        for M, v, w in point_triangle_draws(2.0 ** -147, 1500):
            lo, hi, _ = IP.stored_box(M, v, v)
            if ((w < lo) | (w > hi)).any():
                kept.append((M, v, w))
        kept = kept[:DRAWS_KEPT]
        assert len(kept) == DRAWS_KEPT
        maps = np.stack([M for M, _, _ in kept]).astype(F)
        positions = [np.tile(v, 3).astype(F) for _, v, _ in kept]
        w = np.stack([w for _, _, w in kept]).astype(F)
        _memo[DRAWS_KEY] = Cell(DRAWS_KEY, 0, list(range(len(kept))), maps, OR.make_boxes(w, w), positions=positions)
    return _memo[DRAWS_KEY]


# TABLE: one character per entry of SC.S_EXPONENTS for the ("world", k) cells, "k" kept (every box's 64 indices, 64 instance
# indices and count are the k = 0 answer), "c" changed.  MEASURED on the CPU with the restatement alone, the share of boxes that
# keep their k = 0 answer:
#   k       -70    -64    -40    -31    -20      0     20     32     33     40     63     64
#   kept   59.77  93.88  95.12  100    100    100    100    100    100    100    94.14  94.14 %
# (overlap_scale_cases.py's reasons: the plane's products are of degree 3 and leave float32's normal range first.)  At k = 100
# 40.8 % keep it, at ("ties", -90) 43.0 %, at ("subnormal", -70) 34.7 %.
#        -70-64-40-31-20  0 20 32 33 40 63 64
TABLE = "c  c  c  k  k  k  k  k  k  k  c  c".replace(" ", "")

# The shares of instance_overlap_cases.shares that are exempt from FLOOR, per cell: {cell: {share: measured value}}, the value
# being the asserted lower bound.  ("far", 20) and ("far", 23): the float grid is an eighth of a world size and a whole one, whole
# patches of an instance share one grid point, and a zero-extent box on a corner already holds every triangle collapsed there;
# the GRID class cannot help there.  The NaN-corner cell: every
# walked box holds the 5,472 triangles of the four instances whose corners are all NaN, so n is above 64 or the box is not walked.
LOW_SHARES = {
    ("far", 20): {"n 1 to 8": 21 / 1536, "first 8 of two or more instances": 23 / 1536},
    ("far", 23): {"n 1 to 8": 0 / 1536, "n 9 to 64": 8 / 1536, "first 8 of two or more instances": 0 / 1536,
                  "first 64 of two or more instances": 11 / 1536},
    NAN_CELL: {"touching nothing, walked": 0.0, "n 1 to 8": 0.0, "n 9 to 64": 0.0, "first 8 of two or more instances": 0.0},
}

# the cells where each of the ten later axes (the plane, the nine edge axes) is the first to separate some pair; at the others
# products underflow or overflow and some axis separates nothing first (at ALL_ZERO none does: the set is stage 0's)
LATER_AXES_SEPARATE = ([("world", k) for k in (-40, -31, -20, 0, 20, 32, 33, 40)] + [("scene", -40), ("scene", 40)] +
                       [("cancel", a) for a in SC.CANCEL_EXPONENTS] + [("far", t) for t in SC.FAR_EXPONENTS] +
                       [("ill", e) for e in SC.ILL_EXPONENTS] + [("negzero", 0), ("negzero", 1)])

# the NaN-corner cell, per instance: triangles with a NaN corner, triangles with an infinite corner; the member pairs with a NaN
# corner and the walked boxes, every one of which holds such a pair
NAN_TRIANGLES = [0, 0, 528, 2208, 0, 2208, 0, 0, 528]
INF_TRIANGLES = [528, 2208, 493, 2084, 2208, 2204, 528, 2208, 483]
NAN_MEMBER_PAIRS = 495170
NAN_WALKED = 1465

# ("guard", k): the (box, instance) decisions of the top level, over the 1,404 walked boxes x 9 instances, that a guard of 2^-110
# and a guard of 2^-108 take otherwise than 2^-109 (each is one instance walk fewer or more: the `traversals` counter).  With
# every end under the guard (k <= -113) nothing is culled under any of the three, with none near it (k >= -104) the guard is
# never consulted.  GUARD_SEPARATES: the neighbours (2^-110, 2^-108) that differ by 50 decisions or more, which the GPU test
# asserts to differ on the boxes as read back (a member's stored root box is a little wider than its vertices' own).
GUARD_DECISIONS = {-112: (831, 0), -110: (1892, 7044), -109: (386, 1892), -108: (82, 386), -106: (4, 22)}
GUARD_SEPARATES = {-112: (True, False), -110: (True, True), -109: (True, True), -108: (True, True), -106: (False, False)}

# The six shares of instance_overlap_cases.shares per cell, in boxes of 1,536, in its order: what the module doc's table states in
# per cent, asserted for equality
SHARE_COUNTS = {
    ('world', -70): (171, 117, 644, 533, 113, 632),
    ('world', -64): (176, 122, 639, 528, 119, 629),
    ('world', -40): (178, 127, 633, 527, 114, 625),
    ('world', -31): (184, 139, 615, 527, 113, 624),
    ('world', -20): (184, 139, 615, 527, 113, 624),
    ('world', 0): (184, 139, 615, 527, 113, 624),
    ('world', 20): (184, 139, 615, 527, 113, 624),
    ('world', 32): (184, 139, 615, 527, 113, 624),
    ('world', 33): (184, 139, 615, 527, 113, 624),
    ('world', 40): (184, 139, 615, 527, 113, 624),
    ('world', 63): (176, 122, 639, 528, 119, 629),
    ('world', 64): (176, 122, 639, 528, 119, 629),
    ('scene', -64): (176, 122, 639, 528, 119, 629),
    ('scene', -40): (178, 127, 633, 527, 114, 625),
    ('scene', 40): (184, 139, 615, 527, 113, 624),
    ('scene', 64): (176, 122, 639, 528, 119, 629),
    ('cancel', -64): (184, 139, 615, 527, 113, 624),
    ('cancel', -40): (184, 139, 615, 527, 113, 624),
    ('cancel', 40): (184, 139, 615, 527, 113, 624),
    ('cancel', 64): (184, 139, 615, 527, 113, 624),
    ('far', 12): (201, 212, 246, 808, 141, 272),
    ('far', 20): (211, 21, 184, 1067, 23, 186),
    ('far', 23): (209, 0, 8, 1247, 0, 11),
    ('ill', 6): (189, 233, 214, 834, 127, 285),
    ('ill', 12): (192, 241, 183, 855, 121, 237),
    ('ill', 20): (206, 228, 206, 826, 131, 242),
    ('negzero', 0): (198, 145, 631, 498, 243, 794),
    ('negzero', 1): (198, 145, 631, 498, 243, 794),
    ('ties', -90): (164, 100, 663, 538, 96, 649),
    ('subnormal', -70): (165, 111, 644, 545, 96, 649),
    ('world', 100): (168, 119, 640, 538, 91, 643),
    ('guard', -112): (164, 100, 663, 538, 96, 651),
    ('guard', -110): (164, 100, 663, 538, 96, 651),
    ('guard', -109): (164, 100, 663, 538, 96, 651),
    ('guard', -108): (164, 100, 663, 538, 96, 651),
    ('guard', -106): (164, 100, 663, 538, 96, 651),
    ('nan', 70): (0, 0, 0, 1465, 0, 1465),
}
# the boxes (of 1,536) whose whole K = 64 answer is the k = 0 answer (TABLE's percentages)
KEPT_COUNTS = {
    ('world', -70): 918,
    ('world', -64): 1442,
    ('world', -40): 1461,
    ('world', -31): 1536,
    ('world', -20): 1536,
    ('world', 0): 1536,
    ('world', 20): 1536,
    ('world', 32): 1536,
    ('world', 33): 1536,
    ('world', 40): 1536,
    ('world', 63): 1446,
    ('world', 64): 1446,
    ('ties', -90): 660,
    ('subnormal', -70): 533,
    ('world', 100): 626,
}
# fmin / fmax: (pairs added, pairs lost)
FMIN_PAIRS = {("world", FMIN_WORLD): (266, 24), NAN_CELL: (0, 190450), ("world", 0): (0, 0)}
# the boxes (of 1,536) whose answer fmin / fmax in min3 / max3 change
FMIN_CHANGES = {("world", FMIN_WORLD): 125, NAN_CELL: 1465, ("world", 0): 0}

# the corner formula's mutants: the boxes (of 1,536) whose brute-force answer changes, and the cells where none does
ROW_MUTANTS = {
    "c. a fused corner formula": {"cells": {("ill", 20): 87, ("world", 0): 13, NAN_CELL: 1465}, "controls": [("negzero", 0)]},
    "d. subnormal results flushed": {"cells": {("subnormal", -70): 1298, ("ties", -90): 4}, "controls": [("world", 0)]},
    "e. the zero entries' products added": {"cells": {}, "controls": [("world", 0), ("negzero", 1), ("subnormal", -70), NAN_CELL]},
}

# the walk's mutants: the boxes among the first 192 of the named cell that change
WALK_MUTANTS = {"b": 185, "f": 127, "f at negzero": 66, "k": 13, "k control": 96}
SKIP_SHOWS = {(("far", 12), 8): 1, (("far", 23), 8): 0, (("ill", 12), 8): 2, (("world", 0), 9): 4}
