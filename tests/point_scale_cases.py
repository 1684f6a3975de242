"""Caller-supplied points on scenes scaled by S = 2^k, far beyond the coordinates of order 1 that every other point-query test
uses: the shared case generator of tests/test_point_scale_reference.py (CPU) and tests/test_gpu_point_query_scale.py (GPU),
for closest_points, triangles_within / near_counts, signed_distance and winding_number / winding_signed_distance.  No test and
no GPU in here.

Scenes: lobed_528 and small_trisrc with every position multiplied by S, k in S_EXPONENTS (on the GPU loaded from the same file
under GEOMETRY_SCALE, tests/ray_scale_cases.py's load_scaled; on the CPU `positions * S` in numpy, so that the triangle order
and the tree are the unscaled scene's).  The meshes' largest coordinate is 1.71; a few hundred coordinates are
rounding noise about 0 (1e-17, 2^-56) and go subnormal near k = -70, every other one stays normal; none becomes 0 or infinite.

Points of a cell (scene, k): make_points of the UNSCALED scene (tests/test_gpu_point_query.py's, or tests/near_cases.py's with
its wider radii for the within-radius query), POINTS of them, with p multiplied by S and max_dist2 by S twice.  Both are exact
while the result is a normal float32, so every kind of point survives: on the surface, near it, inside, on a node box face, at
a vertex, far away, duplicates; radius +inf, finite, 0, negative, NaN; a non-finite coordinate.  (Beyond: a finite max_dist2 * S * S
rounds to a subnormal from about k = -60 down, to 0 from about k = -73 down, and to +inf where it is 2^(128 - 2k) or more (1 at k = 64); 0
stays 0 and -1 stays negative.)

On S = 1 only, a second class ("special", like the ray file's "origin" kind): one to three coordinates of p replaced by a member
of SPECIAL_VALUES with a random sign, against the unscaled mesh.

TABLE states, per client and k, whether the restatement at S is the exact image of the restatement at S = 1 ("covariant": each
record equals the S = 1 record scaled by the power of S that field carries, bit for bit, for every point) or not ("outside":
at least one record differs; there the definition itself still holds bit for bit and so do its invariants, which is what
the CPU file asserts).  It was filled from the CPU measurement below, never from a GPU.
"""
from __future__ import annotations

import numpy as np

import near_cases
import point_query_ref as R
import ray_scale_cases as X
import test_gpu_point_query as Q

F = np.float32
SCENES = X.SCENES
S_EXPONENTS = (-70, -64, -40, -31, -20, 0, 20, 32, 33, 40, 63, 64)
POINTS = 2400
SPECIAL_POINTS = 2400
CLIENTS = ("closest", "near", "sdf", "winding")
COVARIANT, OUTSIDE = "covariant", "outside"

# (name, value): a coordinate of p in the "special" class (S = 1)
SPECIAL_VALUES = (("+0", F(0.0)), ("-0", F(-0.0)), ("smallest denormal", np.uint32(1).view(F)), ("2^-64", F(2.0 ** -64)),
                  ("2^63", F(2.0 ** 63)), ("2^64", F(2.0 ** 64)))

# TABLE[client][scene]: one character per entry of S_EXPONENTS, "c" covariant, "o" outside.
#
# Measured on the CPU with the restatements alone (point_query_ref.closest, near_ref.near at K = 64, sdf_ref.derive / signed,
# winding_ref.Restated in the exact mode, each on `positions * S`), POINTS points per cell, walking k one step at a time
# between the entries (k = -36 .. -18 and 28 .. 45).  "Equal" is the share of points whose whole record equals the scaled
# S = 1 record.  lobed_528 / small_trisrc:
#   closest   100 % for -25 <= k <= 32 / -25 <= k <= 33.
#             Below: k = -26 99.96 / 99.88 %, -27 99.88 / 98.3 %, -28 98.8 / 73.9 %, -29 75 / 55 %, -30 54 / 54 %, -31 54 / 54 %,
#             -40 48 / 47 %, -64 44 / 43 %, -70 42 / 40 %, -90 4 / 4 % (every dist2 is 0 and triangle 0 wins every walked point).
#             Above: k = 33 99.75 % (6 points) / 100 %, 34 67 / 99.4 %, 35 49 / 69 %, 36 48 / 51 %, 40 47.5 / 48.5 %,
#             63 and 64 36 / 37 %.
#             The terms va, vb, vc are of degree 4: (edge)^2 (distance)^2 S^4.  They leave float32's normal range (2^-126) for
#             the points nearest the surface below S = 2^-25, and pass 2^128 for the farthest ones (make_points' far class, a
#             hundred extents away) above S = 2^32.
#   near      the same arithmetic over EVERY pair, with a wide radius that keeps far pairs, so a narrower range: 100 % for
#             -25 <= k <= 30 / -24 <= k <= 28 (k = 31, 32: 2 points / k = 29 .. 32: 1 or 2 points; k = 33 97.6 / 99.9 %,
#             34 47 / 92 %, 40 37 / 35 %, 64 31 / 28 %; k = -26 1 / 2 points, -30 53 / 52 %, -40 35 / 33 %, -70 32 / 30 %).
#   sdf       the closest record, sqrtf(dist2) and the sign data (nhat and the angle-weighted sums, all of degree 0).  The
#             sign data alone is bit-identical for -27 <= k <= 33 / -26 <= k <= 34: dot(n, n) is of degree 4 and underflows or
#             overflows under sqrtf; from k = -36 down and k = 35 / 37 up every triangle counts as degenerate (nhat = 0), between
#             -35 / -34 and 34 / 36 some do.  Values and sign data together: -26 <= k <= 32 / -26 <= k <= 33.
#   winding   exact mode (beta = inf): det and den are of degree 3, atan_yx takes their ratio.  Bit-identical for
#             -33 <= k <= 31 / -34 <= k <= 31 (k = 32 98.4 / 98.3 %, 33 89 %, 40 83 / 84 %; k = -35 99.9 %, -40 50 / 34 %).
#             w = +0 for every finite point from k = -57 down (every det underflows to 0: the zero rule).  w is NaN for a
#             finite point where det meets inf - inf: none up to k = 36, 4 % at k = 37, 17 % at k = 40, 75 % at k = 43, every
#             point from k = 44 up.
#             Finite beta is not covariant anywhere: box3d::add pads the boxes by an absolute 1e-5, which moves r and the
#             box-centre fallback of P.  Measured max |w(beta = 2) - w(exact)| over the points at least 1e-3 extents from the
#             surface: k = -31 .. -26: 0 (the pad is thousands of extents, every node is near: the walk IS the exact sum);
#             k = -25 9e-9 / 3e-8; k = -20 2.8e-8 / 4.8e-8; k = 0 and 20 3.8e-2 / 4.2e-2 (far points; w > 0.5 agrees with the
#             exact mode on every one of them at each of these k).
#             The NaN rule of finite beta at the overflow end: T_far's dot(d, m), m = M d, is of degree 5 (M of degree 3), so
#             it meets inf - inf long before the exact mode's degree 3 does.  No finite point is NaN up to k = 20; the far
#             class is from k = 21 (5 % of the points), 90 % at k = 27, every finite point for 28 <= k <= 34 / 36.  From
#             k = 35 / 37 up A_t = 0.5 * sqrtf(dot(n, n)) is +inf, P = S / A is NaN or 0 and d2 > br * br is false at every
#             node: the walk is the exact sum again, bit for bit, NaN where that is.
TABLE = {
    #                          -70-64-40-31-20  0 20 32 33 40 63 64
    "closest": {"lobed_528":    "o  o  o  o  c  c  c  c  o  o  o  o".replace(" ", ""),
                "small_trisrc": "o  o  o  o  c  c  c  c  c  o  o  o".replace(" ", "")},
    "near":    {"lobed_528":    "o  o  o  o  c  c  c  o  o  o  o  o".replace(" ", ""),
                "small_trisrc": "o  o  o  o  c  c  c  o  o  o  o  o".replace(" ", "")},
    "sdf":     {"lobed_528":    "o  o  o  o  c  c  c  c  o  o  o  o".replace(" ", ""),
                "small_trisrc": "o  o  o  o  c  c  c  c  c  o  o  o".replace(" ", "")},
    "winding": {"lobed_528":    "o  o  o  c  c  c  c  o  o  o  o  o".replace(" ", ""),
                "small_trisrc": "o  o  o  c  c  c  c  o  o  o  o  o".replace(" ", "")},
}
# the exact mode's w over finite points (the measurement above): never NaN up to this k, always from that k; +0 down from the last
EXACT_WINDING_NAN_FREE_MAX_EXPONENT = 36
EXACT_WINDING_ALL_NAN_MIN_EXPONENT = 44
EXACT_WINDING_ALL_ZERO_MAX_EXPONENT = -57
# finite beta: no finite point's w is NaN up to this k
FINITE_BETA_MAX_EXPONENT = 20
# Not a cell of the TABLE: the scale at which EVERY dist2 of every point underflows to 0 (the far class included: (2^14)^2 *
# 2^-180 rounds to 0), so that every walked point sees nothing but ties.  At k = -70 dist2 is still a non-zero subnormal
# beyond 0.03 extents.  Its misses are the unwalked points alone (4 %), below the cells' 5 % guard.
ALL_TIES_UNDERFLOW = -90


def flag(client: str, name: str, s_exp: int) -> str:
    return COVARIANT if TABLE[client][name][S_EXPONENTS.index(s_exp)] == "c" else OUTSIDE


def as_dict(arrays: X.R.SceneArrays) -> dict:
    """the three arrays make_points reads"""
    return {"vertex_positions": arrays.positions.reshape(-1), "group_boxmin": arrays.boxmin.reshape(-1),
            "group_boxmax": arrays.boxmax.reshape(-1)}


def seed_of(name: str, client: str) -> int:
    return 5 + 10 * SCENES.index(name) + (1 if client == "near" else 0)


def base_points(pkg, name: str, client: str = "closest") -> np.ndarray:
    """the unscaled scene's points: near_cases.make_points for the within-radius query, test_gpu_point_query's otherwise"""
    make = near_cases.make_points if client == "near" else Q.make_points
    return make(as_dict(X.base_arrays(pkg, name)), POINTS, seed=seed_of(name, client))


def scaled_points(points: np.ndarray, s_exp: int) -> np.ndarray:
    """p * S and max_dist2 * S * S in float32 (S^2 itself is no float32 at |k| >= 64)"""
    S = F(2.0 ** s_exp)
    out = points.copy()
    with np.errstate(all="ignore"):
        out["p"] = points["p"] * S
        out["max_dist2"] = (points["max_dist2"] * S) * S
    return out


def points(pkg, name: str, s_exp: int, client: str = "closest") -> np.ndarray:
    return scaled_points(base_points(pkg, name, client), s_exp)


def special_points(pkg, name: str, client: str = "closest") -> np.ndarray:
    """the S = 1 class: make_points of the unscaled scene with one to three coordinates of p replaced by SPECIAL_VALUES"""
    make = near_cases.make_points if client == "near" else Q.make_points
    seed = 700 + seed_of(name, client)
    pts = make(as_dict(X.base_arrays(pkg, name)), SPECIAL_POINTS, seed=seed)
    rng = np.random.default_rng(seed + 1)
    values = np.array([v for _, v in SPECIAL_VALUES], F)
    p = pts["p"].copy()
    how_many = rng.integers(1, 4, len(p))
    for i in range(len(p)):
        axes = rng.choice(3, how_many[i], replace=False)
        v = values[rng.integers(0, len(values), how_many[i])]
        p[i, axes] = np.where((v != 0) & (rng.random(how_many[i]) < 0.5), -v, v)
    pts["p"] = p
    return pts


def scaled_positions(pkg, name: str, s_exp: int) -> np.ndarray:
    """positions * S in numpy, float32 [T * 9]: the unscaled scene's triangle order"""
    return (X.base_arrays(pkg, name).positions * F(2.0 ** s_exp)).reshape(-1)


def scale_closest(records: np.ndarray, s_exp: int, pts_scaled: np.ndarray) -> np.ndarray:
    """the covariant prediction: S = 1 records (any shape) with q * S and dist2 * S * S; a miss carries the scaled point's p and
    max_dist2 as given (pts_scaled broadcasts against records' leading axis)"""
    S = F(2.0 ** s_exp)
    out = records.copy()
    with np.errstate(all="ignore"):
        out["q"] = records["q"] * S
        out["dist2"] = (records["dist2"] * S) * S
    miss = records["triangle"] < 0
    p = np.broadcast_to(pts_scaled["p"].reshape((-1,) + (1,) * (records.ndim - 1) + (3,)), records["q"].shape)
    md = np.broadcast_to(pts_scaled["max_dist2"].reshape((-1,) + (1,) * (records.ndim - 1)), records["dist2"].shape)
    out["q"][miss] = p[miss]
    out["dist2"][miss] = md[miss]
    return out


def same_floats(a, b) -> np.ndarray:
    """elementwise: equal bits, or both NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def same_records(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """bool per record (the records' own shape): all 32 bytes equal"""
    return (R.as_bits(a) == R.as_bits(b)).all(1).reshape(a.shape)
