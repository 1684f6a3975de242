"""Query triangles on scenes scaled by S = 2^k, far beyond the coordinates of order 1 that every other triangle-intersection
test uses: the shared case generator of tests/test_intersect_scale_reference.py (CPU) and tests/test_gpu_intersect_scale.py
(GPU).  No test and no GPU in here.

Scenes: lobed_528 and small_trisrc with every position multiplied by S, k in S_EXPONENTS (on the GPU loaded from the same file
under GEOMETRY_SCALE, tests/ray_scale_cases.py's load_scaled; on the CPU `positions * S` in numpy, so that the triangle order
is the unscaled scene's).

Queries of a cell (scene, k): intersect_cases.make_queries of the UNSCALED scene, QUERIES of them with one seed per scene, the
corners multiplied by S in float32.

Why each exponent is a cell (MEASURED below has the figures):
  -80            nothing is walked: every query's normal has underflowed to (0, 0, 0)
  -74            about half the queries are still walked and every scene triangle is degenerate (nt == 0): n = 0 everywhere
  -72            the mixed underflow cell: walked and unwalked queries, valid and degenerate scene triangles, all of them
                 through the underflow of the kernel's own cross product
  -64, -50, -40  subnormal and zero products in the projections: the cells that see flushed subnormals
  -34 / -33      the lower end of the header's range from outside and from inside
  29 / 30        its upper end from inside and from outside
  32, 40         overflow reaches first the degree-4 projections (on nq x f and nt x e): the cells where a fused
                 multiply-add and a NaN-dropping min / max first change a set
  50, 64         overflow reaches the lower-degree projections as well: the cells that see `A . q0` folded to 0

On S = 1 a second class ("special"): make_queries of the unscaled scene with one to three of a query's nine coordinates
replaced by a member of SPECIAL_VALUES with a random sign, a non-finite coordinate that is left replaced by 0.  The same
replacement over the queries of k = 64, against that scene, is "special64".

A third, small class runs on intersect_cases.flat_lattice: its integer queries with the sign of every zero coordinate flipped
(minus_zero).  The header's == makes -0 equal +0, with and without SKIP_SHARED, and no sum or product of the test tells the two
apart in a comparison, so the set must be that of the +0 queries.

TABLE states, per scene and k, whether every query's set is the S = 1 set ("k", kept) or some query's differs ("c", changed).
It was filled from the CPU measurement below, never from a GPU; where the set changes the header's definition still holds bit
for bit, which is what the GPU test asserts at every cell.
"""
from __future__ import annotations

import numpy as np

import intersect_cases as IC
import intersect_ref as IR
import ray_scale_cases as X

F = np.float32
FLT_MAX = np.finfo(F).max
SCENES = X.SCENES
S_EXPONENTS = (-80, -74, -72, -64, -50, -40, -34, -33, 0, 29, 30, 32, 40, 50, 64)
QUERIES = 1200
KEPT, CHANGED = "kept", "changed"
SPECIAL_CELLS = {"special": 0, "special64": 64}   # class -> the exponent of its scene

# (name, value): a coordinate of a query in a special class; the sign is drawn
SPECIAL_VALUES = (("0", F(0.0)), ("smallest denormal", np.uint32(1).view(F)), ("2^-64", F(2.0 ** -64)), ("2^63", F(2.0 ** 63)),
                  ("2^64", F(2.0 ** 64)), ("FLT_MAX", FLT_MAX))

# TABLE[scene]: one character per entry of S_EXPONENTS, "k" kept, "c" changed.
#
# MEASURED on the CPU with the restatement alone (intersect_ref.first_axis of queries(name, k) on `positions * S`), QUERIES
# queries per cell, seeds seed_of(name).  Per k, lobed_528 / small_trisrc: queries walked (WALKED below), queries whose set
# differs from S = 1, pairs added + pairs lost, the shares of queries with n = 0, n > 8 and n > 64, and which of the 17 axes
# (1 nq, 2 nt, 3-11 f x e, 12-14 nq x f, 15-17 nt x e) are still the first to separate some pair.
#   k    walked       differ       added + lost                    n = 0          n > 8          n > 64         axes that still separate first
#   -80     0 / 0      895 / 837        0 + 30131 /      0 + 55747  1.000 / 1.000  0.000 / 0.000  0.000 / 0.000  none / none
#   -74   529 / 493    895 / 837        0 + 30131 /      0 + 55747  1.000 / 1.000  0.000 / 0.000  0.000 / 0.000  none / none
#   -72  1071 / 602    982 / 859   172184 + 2283  / 148560 + 44709  0.118 / 0.523  0.703 / 0.440  0.417 / 0.378  none / none
#   -64  1125 / 1128   953 / 941   187681 + 0     / 808313 + 0      0.074 / 0.099  0.750 / 0.720  0.417 / 0.401  none / none
#   -50  1125 / 1128   952 / 940    23712 + 2383  /  76487 + 4951   0.074 / 0.100  0.749 / 0.719  0.364 / 0.398  1,3-11 / 1,3-11
#   -40  1125 / 1128     0 / 0          0 + 0     /      0 + 0      0.254 / 0.302  0.675 / 0.667  0.072 / 0.345  1-11 / 1-11
#   -34  1125 / 1128     1 / 60         0 + 1     /      0 + 112    0.254 / 0.302  0.675 / 0.667  0.072 / 0.345  1-11,16 / 1-11,15-17
#   -33  1125 / 1128     0 / 0          0 + 0     /      0 + 0      0.254 / 0.302  0.675 / 0.667  0.072 / 0.345  1-11 / 1-11
#     0  1125 / 1128     0 / 0          0 + 0     /      0 + 0      0.254 / 0.302  0.675 / 0.667  0.072 / 0.345  1-11 / 1-11
#    29  1125 / 1128     0 / 0          0 + 0     /      0 + 0      0.254 / 0.302  0.675 / 0.667  0.072 / 0.345  1-11 / 1-11
#    30  1125 / 1128    71 / 92         0 + 2063  /      0 + 5077   0.257 / 0.306  0.672 / 0.663  0.060 / 0.302  1-12 / 1-12
#    32  1125 / 1128    10 / 8          0 + 19    /      0 + 28     0.254 / 0.302  0.673 / 0.666  0.072 / 0.345  1-12 / 1-12
#    40  1125 / 1128   203 / 186        0 + 383   /      0 + 365    0.256 / 0.302  0.675 / 0.667  0.072 / 0.345  1-13,15-17 / 1-13,15-17
#    50  1125 / 1128  1031 / 995   187661 + 219   / 808299 + 171    0.074 / 0.099  0.750 / 0.720  0.417 / 0.401  2-8,16-17 / 2-8,13,16-17
#    64  1125 / 1128  1029 / 1000  187661 + 211   / 808302 + 178    0.074 / 0.099  0.750 / 0.720  0.417 / 0.401  2-8,17 / 2-8,13,17
# Below the range.  nq and nt are of degree 2, the projections on them and on f x e of degree 3, those on nq x f and nt x e of
# degree 4.  At k = -34 the degree-4 projections have lost enough bits to underflow to change 1 / 60 queries; k = -40 keeps every
# set again, by accident (DESIGN section 19 names that stretch), and is a cell for what it shows of flushed subnormals.  At
# k = -50 the degree-4 axes and nt's own separate nothing any more, at k = -64 and -72 no axis does: every projection is 0, 0 > 0
# separates nothing, and the set is stage 0's less the degenerate triangles.  From k = -72 down nq and nt themselves underflow
# to (0, 0, 0), piece by piece: at k = -72 43 of 528 / 1,783 of 2,208 scene triangles are degenerate for some walked query
# and 129 / 598 queries are no longer walked, at k = -74 every scene triangle is degenerate and 529 / 493 queries are still
# walked (n = 0 for all of them, by the degenerate rule and not by the walk), at k = -80 no query is walked.
# Above the range.  At k = 30 the first degree-4 projections overflow: an infinite or NaN projection does not separate, and
# min3 / max3 pass a NaN on or drop it by its position, as the header's comparisons say; pairs are only lost up to k = 40.  From
# k = 50 up the projections of degree 3 overflow as well and most pairs that pass stage 0 are members.
# With SKIP_SHARED 25,611 of 30,131 / 51,113 of 55,747 members remain at k = 0 and 213,270 of 217,581 / 859,415 of 863,871 at
# k = 64.
# The special classes: 1,183 / 1,195 ("special") and 1,184 / 1,189 ("special64") of the 1,200 queries stay walked; n = 0 for
# 0.189 / 0.199 and 0.027 / 0.036 of them, n > 8 for 0.552 / 0.610 and 0.901 / 0.892; in "special" each of the 17 axes is the
# first to separate some pair.
TABLE = {
    #               -80-74-72-64-50-40-34-33  0 29 30 32 40 50 64
    "lobed_528":    "c  c  c  c  c  k  c  k  k  k  c  c  c  c  c".replace(" ", ""),
    "small_trisrc": "c  c  c  c  c  k  c  k  k  k  c  c  c  c  c".replace(" ", ""),
}
# queries walked per entry of S_EXPONENTS (the special classes: SPECIAL_WALKED)
WALKED = {
    "lobed_528":    (0, 529, 1071, 1125, 1125, 1125, 1125, 1125, 1125, 1125, 1125, 1125, 1125, 1125, 1125),
    "small_trisrc": (0, 493, 602, 1128, 1128, 1128, 1128, 1128, 1128, 1128, 1128, 1128, 1128, 1128, 1128),
}
SPECIAL_WALKED = {"lobed_528": {"special": 1183, "special64": 1184}, "small_trisrc": {"special": 1195, "special64": 1189}}


def flag(name: str, s_exp: int) -> str:
    return KEPT if TABLE[name][S_EXPONENTS.index(s_exp)] == "k" else CHANGED


def walked_count(name: str, cell) -> int:
    return SPECIAL_WALKED[name][cell] if cell in SPECIAL_CELLS else WALKED[name][S_EXPONENTS.index(cell)]


def as_dict(arrays) -> dict:
    """the array make_queries reads"""
    return {"vertex_positions": np.asarray(arrays.positions, F).reshape(-1)}


def seed_of(name: str) -> int:
    return 11 + 10 * SCENES.index(name)


_queries = {}


def base_queries(pkg, name: str) -> np.ndarray:
    """the unscaled scene's queries [QUERIES, 3, 3], once"""
    if name not in _queries:
        _queries[name] = IC.make_queries(as_dict(X.base_arrays(pkg, name)), QUERIES, seed=seed_of(name))
    return _queries[name]


def scaled_queries(queries: np.ndarray, s_exp: int) -> np.ndarray:
    """the corners times S in float32"""
    with np.errstate(all="ignore"):
        return np.asarray(queries, F) * F(2.0 ** s_exp)


def queries(pkg, name: str, s_exp: int) -> np.ndarray:
    return scaled_queries(base_queries(pkg, name), s_exp)


def special_queries(pkg, name: str, which: str = "special") -> np.ndarray:
    """a special class (module doc): SPECIAL_CELLS[which] is its scale"""
    key = (name, which)
    if key not in _queries:
        seed = 700 + seed_of(name) + SPECIAL_CELLS[which]
        out = IC.make_queries(as_dict(X.base_arrays(pkg, name)), QUERIES, seed=seed)
        c = scaled_queries(out, SPECIAL_CELLS[which]).reshape(-1, 9)
        rng = np.random.default_rng(seed + 1)
        values = np.array([v for _, v in SPECIAL_VALUES], F)
        how_many = rng.integers(1, 4, len(c))
        for i in range(len(c)):
            at = rng.choice(9, how_many[i], replace=False)
            v = values[rng.integers(0, len(values), how_many[i])]
            c[i, at] = np.where(rng.random(how_many[i]) < 0.5, -v, v)
        c[~np.isfinite(c)] = 0
        _queries[key] = np.ascontiguousarray(c.reshape(-1, 3, 3))
    return _queries[key]


def scaled_positions(pkg, name: str, s_exp: int) -> np.ndarray:
    """positions * S in numpy, float32 [T * 9]: the unscaled scene's triangle order"""
    with np.errstate(all="ignore"):
        return (X.base_arrays(pkg, name).positions * F(2.0 ** s_exp)).reshape(-1)


def inputs(pkg, name: str, cell):
    """(positions * S float32 [T * 9] in the unscaled scene's triangle order, queries [n, 3, 3]) of a cell: an exponent or a
    special class"""
    if cell in SPECIAL_CELLS:
        return scaled_positions(pkg, name, SPECIAL_CELLS[cell]), special_queries(pkg, name, cell)
    return scaled_positions(pkg, name, cell), queries(pkg, name, cell)


_codes = {}


def codes(pkg, name: str, cell, skip_shared: bool = False) -> np.ndarray:
    """intersect_ref.first_axis of the cell (an exponent or a special class) on the CPU's `positions * S`, once"""
    key = (name, cell, skip_shared)
    if key not in _codes:
        pos, q = inputs(pkg, name, cell)
        _codes[key] = IR.first_axis(q, pos, skip_shared)
    return _codes[key]


def minus_zero(queries) -> np.ndarray:
    """the queries with the sign of every zero coordinate flipped: +0 becomes -0 and -0 becomes +0"""
    q = np.array(queries, F)
    q[q == 0] = -q[q == 0]
    return q
