"""Caller-supplied boxes on scenes scaled by S = 2^k, far beyond the coordinates of order 1 that every other box-overlap test
uses: the shared case generator of tests/test_overlap_scale_reference.py (CPU) and tests/test_gpu_overlap_scale.py (GPU).  No
test and no GPU in here.

Scenes: lobed_528 and small_trisrc with every position multiplied by S, k in S_EXPONENTS (on the GPU loaded from the same file
under GEOMETRY_SCALE, tests/ray_scale_cases.py's load_scaled; on the CPU `positions * S` in numpy, so that the triangle order
is the unscaled scene's).  The meshes' largest coordinate is 1.71; a few hundred coordinates are rounding noise about 0
(1e-17, 2^-56): 0 / 10 of them are subnormal at k = -70 and 336 / 696 at k = -90; every other coordinate stays a normal
float32, none becomes 0 and none infinite.

Boxes of a cell (scene, k): overlap_cases.make_boxes of the UNSCALED scene, BOXES of them with one seed per scene, `lo` and
`hi` multiplied by S.  That is exact while the result is a normal float32, and it is for nearly every coordinate at every k.
The largest box coordinate is a far box's, some 500 (2^9), so nothing reaches infinity at k = 64 and no walked box turns
unwalked.  The smallest non-zero ones are the mesh's own noise coordinates, which the zero-extent and on-vertex kinds copy,
and faces of voxel and surface boxes that come within 1e-11 of a coordinate plane: 93 / 42 box coordinates are subnormal at
k = -90, none at k = -70 or above, and none reaches 0.  Scaling by a power of two keeps lo <= hi, lo > hi (no coordinate
underflows to 0), NaN and the infinities, so the same 2,291 / 2,285 boxes are walked at every k.

On S = 1, a second class ("special", like the point file's): make_boxes of the unscaled scene with one to three of a box's
six coordinates replaced by a member of SPECIAL_VALUES with a random sign, a non-finite coordinate that is left replaced by 0,
then lo and hi exchanged on every axis where lo > hi: every such box is walked.  Box 0 is (-FLT_MAX, FLT_MAX)^3.  The same
replacement over the boxes of k = 64, against that scene, is "special64": only there can a special coordinate make a product
overflow (MEASURED below).

TABLE states, per scene and k, whether every box's set is the S = 1 set ("k", kept) or some box's differs ("c", changed).  It
was filled from the CPU measurement below, never from a GPU; where the set changes the header's definition still holds bit
for bit, which is what the GPU test asserts at every cell.
"""
from __future__ import annotations

import numpy as np

import overlap_cases as OC
import overlap_ref as OR
import ray_scale_cases as X

F = np.float32
FLT_MAX = np.finfo(F).max
SCENES = X.SCENES
S_EXPONENTS = (-90, -70, -64, -40, -28, -27, 0, 44, 45, 50, 64, 67)   # (67: ADDED_FOR_NAN below)
BOXES = 2400
SPECIAL_BOXES = 2400
KEPT, CHANGED = "kept", "changed"
SPECIAL_CELLS = {"special": 0, "special64": 64}   # class -> the exponent of its scene

# (name, value): a coordinate of a box in the "special" class (S = 1); the sign is drawn
SPECIAL_VALUES = (("0", F(0.0)), ("smallest denormal", np.uint32(1).view(F)), ("2^-64", F(2.0 ** -64)), ("2^63", F(2.0 ** 63)),
                  ("2^64", F(2.0 ** 64)), ("FLT_MAX", FLT_MAX))

# TABLE[scene]: one character per entry of S_EXPONENTS, "k" kept, "c" changed.
#
# MEASURED on the CPU with the restatement alone (overlap_ref.first_axis on `positions * S` against boxes(name, k)), BOXES boxes
# per cell, seeds seed_of(name).  Per k, lobed_528 / small_trisrc: boxes whose set differs from S = 1, pairs added + pairs lost,
# the share of boxes with n = 0, n > 8, n > 64, and the later axes (3 the plane, 4 .. 12 the edges) that still separate a pair.
# At every k 2,291 / 2,285 of the 2,400 boxes are walked.
#   k    differ       added + lost            n = 0          n > 8          n > 64         later axes that separate
#   -90  1521 / 1562  3860 + 0 / 5478 + 0     0.228 / 0.198  0.247 / 0.437  0.107 / 0.104  none: the set is stage 0's
#   -70   478 / 1034   735 + 8 / 2202 + 142   0.350 / 0.233  0.210 / 0.386  0.106 / 0.104  every edge axis, not the plane
#   -64   190 / 156    389 + 0 /  361 + 0     0.368 / 0.268  0.209 / 0.364  0.106 / 0.104  every edge axis, not the plane
#   -40   115 / 130    204 + 37 / 254 + 43    0.395 / 0.278  0.209 / 0.363  0.106 / 0.104  all ten (the plane 1614 / 1488 pairs, 1781 / 1699 at S = 1)
#   -28     0 / 0                             0.398 / 0.279  0.209 / 0.363  0.106 / 0.104  all ten, the S = 1 counts
#   -27, 0, 44: as -28 (at 44 the first separating axis of 5 / 0 pairs moves from the plane to an edge; the set does not)
#    45   158 / 0       76 + 129 / 0 + 0      0.406 / 0.279  0.209 / 0.363  0.106 / 0.104  all ten
#    50   187 / 153    386 + 0 /  358 + 0     0.369 / 0.268  0.209 / 0.363  0.106 / 0.104  every edge axis, not the plane
#    64   as 50, pair for pair
# Below the range the degree-3 products (the plane's d and r) lose bits to underflow, then are 0 (0 > 0 separates nothing: from
# k = -64 down the plane axis is gone); the degree-2 edge products follow, and at k = -90 every later product is 0 and the set is
# exactly the set of triangles that pass stage 0.  Above it the plane's products overflow: at k = 45 pairs are both lost and added,
# from k = 50 up the plane separates nothing (inf > inf and every comparison with a NaN are false), while the edge axes (degree 2)
# separate the same pairs at k = 50 and k = 64.  One step beyond the header's range, k = -28 keeps every set on both
# scenes and k = 45 on small_trisrc: the header's -27 <= k <= 44 was measured on the scenes normalised to a largest coordinate of
# 1.7 with other boxes (tests/test_overlap_reference.py) and is the narrower statement.
#    67  1134 / 595   1679 + 657 / 1148 + 86  0.369 / 0.266  0.219 / 0.366  0.107 / 0.104  every edge axis, not the plane
# ADDED_FOR_NAN.  Up to k = 64 a NaN arises in the plane stage alone (degree 3), which takes no min or max: the edge stage's
# projections p = e.u v.w - e.w v.u are of degree 2 and stay finite, because stage 0 is exact and so bounds |v| by the box's half
# extent plus the triangle's own.  Where a huge box does push a p to inf - inf (the special class at 2^64) the same magnitudes
# make that axis' r infinite, and no comparison with it separates whatever min3 returns.  A NaN reaches min3 / max3 beside a finite
# r only when the triangle's own edges square past 2^128, from k = 66 up on these meshes (edges of 0.1 to 0.4): there
# min(min(p0, p1), NaN) is NaN and does not separate where fmin would return a finite p0 that does.  k = 67 is the cell that
# tells `fminf` or a NaN-dropping v_min_f32 from the header's comparisons (tests/test_overlap_scale_reference.py: 461 / 83
# boxes change; 0 at every k <= 65 and in both special classes).
# The special classes, all 2,400 boxes walked: at S = 1 1,909 / 1,895 boxes have n > 0 and no stage 1 or 2 value is non-finite
# (the meshes' edges are below 1, so no product of an edge with a coordinate of at most FLT_MAX / 2 overflows); "special64", the
# same replacement over the boxes and scene of k = 64, where FLT_MAX is 2^63 times the mesh and 2^63 and 2^64 are its own
# size: 1,875 / 1,882 boxes with n > 0, 2,030 / 1,994 with a pair that meets a NaN or an infinity.
TABLE = {
    #               -90-70-64-40-28-27  0 44 45 50 64 67
    "lobed_528":    "c  c  c  c  k  k  k  k  c  c  c  c".replace(" ", ""),
    "small_trisrc": "c  c  c  c  k  k  k  k  k  c  c  c".replace(" ", ""),
}


def flag(name: str, s_exp: int) -> str:
    return KEPT if TABLE[name][S_EXPONENTS.index(s_exp)] == "k" else CHANGED


def as_dict(arrays) -> dict:
    """the array make_boxes reads"""
    return {"vertex_positions": np.asarray(arrays.positions, F).reshape(-1)}


def seed_of(name: str) -> int:
    return 11 + 10 * SCENES.index(name)


_boxes = {}


def base_boxes(pkg, name: str) -> np.ndarray:
    """the unscaled scene's boxes, once"""
    if name not in _boxes:
        _boxes[name] = OC.make_boxes(as_dict(X.base_arrays(pkg, name)), BOXES, seed=seed_of(name))
    return _boxes[name]


def scaled_boxes(boxes: np.ndarray, s_exp: int) -> np.ndarray:
    """lo * S and hi * S in float32"""
    S = F(2.0 ** s_exp)
    out = boxes.copy()
    with np.errstate(all="ignore"):
        out["lo"], out["hi"] = boxes["lo"] * S, boxes["hi"] * S
    return out


def boxes(pkg, name: str, s_exp: int) -> np.ndarray:
    return scaled_boxes(base_boxes(pkg, name), s_exp)


def special_boxes(pkg, name: str, which: str = "special") -> np.ndarray:
    """a special class (module doc): SPECIAL_CELLS[which] is its scale"""
    key = (name, which)
    if key not in _boxes:
        seed = 700 + seed_of(name) + SPECIAL_CELLS[which]
        out = OC.make_boxes(as_dict(X.base_arrays(pkg, name)), SPECIAL_BOXES, seed=seed)
        out = scaled_boxes(out, SPECIAL_CELLS[which])
        rng = np.random.default_rng(seed + 1)
        values = np.array([v for _, v in SPECIAL_VALUES], F)
        c = np.concatenate([out["lo"], out["hi"]], 1)            # [n, 6]
        how_many = rng.integers(1, 4, len(c))
        for i in range(len(c)):
            at = rng.choice(6, how_many[i], replace=False)
            v = values[rng.integers(0, len(values), how_many[i])]
            c[i, at] = np.where(rng.random(how_many[i]) < 0.5, -v, v)
        c[~np.isfinite(c)] = 0
        c[0] = (-FLT_MAX,) * 3 + (FLT_MAX,) * 3
        lo, hi = c[:, :3], c[:, 3:]
        swap = lo > hi
        out["lo"], out["hi"] = np.where(swap, hi, lo), np.where(swap, lo, hi)
        assert OR.walked(out).all()
        _boxes[key] = out
    return _boxes[key]


def inputs(pkg, name: str, cell):
    """(positions * S float32 [T * 9] in the unscaled scene's triangle order, boxes) of a cell: an exponent or a special class"""
    if cell in SPECIAL_CELLS:
        return scaled_positions(pkg, name, SPECIAL_CELLS[cell]), special_boxes(pkg, name, cell)
    return scaled_positions(pkg, name, cell), boxes(pkg, name, cell)


def scaled_positions(pkg, name: str, s_exp: int) -> np.ndarray:
    """positions * S in numpy, float32 [T * 9]: the unscaled scene's triangle order"""
    with np.errstate(all="ignore"):
        return (X.base_arrays(pkg, name).positions * F(2.0 ** s_exp)).reshape(-1)


_codes = {}


def codes(pkg, name: str, cell) -> np.ndarray:
    """overlap_ref.first_axis of the cell (an exponent or a special class) on the CPU's `positions * S`, once"""
    key = (name, cell)
    if key not in _codes:
        _codes[key] = OR.first_axis(*inputs(pkg, name, cell))
    return _codes[key]


def row_order(positions) -> np.ndarray:
    """the permutation that sorts the triangles [T, 9] by their raw words: two loads of one scene are compared through it (the
    builder's triangle order may change with the scale, the set of triangles may not)"""
    rows = np.ascontiguousarray(positions, F).reshape(-1, 9).view(np.uint32)
    return np.lexsort(rows.T[::-1])
