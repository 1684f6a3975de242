"""CPU restatement of the ray query (include/shader_ray_query.h), for the tests.

The shader's group_intersect (raytracer.es.fs:386-443) as the literal threaded walk over the eight (hit, miss) link tables,
vectorised over rays, in float32 throughout and in the shader's operation order: true divisions in the slab test
(fs:200-217), GLSL's max / min (the second operand wins only on a strict compare), dot products added left to right,
the triangle test of fs:297-346 with e0 = v1 - v0 and e1 = v0 - v2.  The running closest hit starts at the ray's tmax.

Input: the flattened arrays of World.arrays() / DeviceWorld.flat_arrays() (shader-ray_amd/host.py: desc_arrays).
"""
from __future__ import annotations

import numpy as np

F = np.float32
RANGE_MAX = F(1e8)        # the traversal's range, fs:491
TERMINATOR = F(16777215)  # fs:384
DET_EPS = F(0.0000001)    # fs:311
HIT_MISS, HIT_CAP = -1, -2
HIT_DTYPE = np.dtype([("t", np.float32), ("u", np.float32), ("v", np.float32), ("triangle", np.int32)])
COUNTER_NAMES = ("node_visits", "leaf_visits", "triangle_tests", "traversals", "bad_hits")


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sel_max(x, y):
    return np.where(x < y, y, x)


def _sel_min(x, y):
    return np.where(y < x, y, x)


class SceneArrays:
    """The arrays the walk reads, as float32 numpy arrays."""

    def __init__(self, arrays: dict):
        self.positions = np.asarray(arrays["vertex_positions"], F).reshape(-1, 3, 3)   # [triangle, vertex, xyz]
        self.boxmin = np.asarray(arrays["group_boxmin"], F).reshape(-1, 3)
        self.boxmax = np.asarray(arrays["group_boxmax"], F).reshape(-1, 3)
        self.objects = np.asarray(arrays["group_objects"], F).reshape(-1, 2)
        self.hitmiss = np.stack([np.asarray(arrays[f"group_hitmiss_{c}"], F).reshape(-1, 2) for c in range(8)])
        self.root = F(arrays["tree_root"])


def trace(scene, origins, directions, tmax, max_bvh_iterations: int = 400, max_leaf_tests: int = 10):
    """Closest-hit queries of rays (origins [n, 3], directions [n, 3], tmax [n] or scalar).  Returns (hits: HIT_DTYPE [n],
    counters: dict of COUNTER_NAMES summed over the rays).  max_bvh_iterations = 0: no cap."""
    sc = scene if isinstance(scene, SceneArrays) else SceneArrays(scene)
    P = np.asarray(origins, F).reshape(-1, 3)
    D = np.asarray(directions, F).reshape(-1, 3)
    n = len(P)
    tmax = np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
    t = tmax.copy()
    which = np.full(n, F(-1))
    hu = np.zeros(n, F)
    hv = np.zeros(n, F)
    counts = {k: 0 for k in COUNTER_NAMES}
    traced = tmax > 0                                    # tmax <= 0 or NaN: a miss, no traversal
    counts["traversals"] = int(traced.sum())
    code = ((D[:, 0] > 0).astype(np.int64) + 2 * (D[:, 1] > 0) + 4 * (D[:, 2] > 0))
    g = np.full(n, sc.root)
    active = np.nonzero(traced)[0]
    capped = np.zeros(n, bool)
    i = 0
    with np.errstate(all="ignore"):
        while len(active):
            r = active
            counts["node_visits"] += len(r)
            node = g[r].astype(np.int64)
            hit_next = sc.hitmiss[code[r], node, 0]
            miss_next = sc.hitmiss[code[r], node, 1]
            leaf = hit_next == miss_next
            counts["leaf_visits"] += int(leaf.sum())
            start = np.where(leaf, sc.objects[node, 0], F(0))
            count = np.where(leaf, sc.objects[node, 1], F(0))
            r0 = np.zeros(len(r), F)
            r1 = np.full(len(r), RANGE_MAX)
            for a in range(3):
                o, d = P[r, a], D[r, a]
                ta = (sc.boxmin[node, a] - o) / d
                tb = (sc.boxmax[node, a] - o) / d
                forward = d >= 0
                r0 = _sel_max(r0, np.where(forward, ta, tb))
                r1 = _sel_min(r1, np.where(forward, tb, ta))
            enter = ~(r0 >= r1) & (r0 < t[r])
            # the leaf's triangles, in order (fs:405-418)
            in_leaf = np.nonzero(enter & leaf)[0]
            for j in range(max_leaf_tests):
                k = in_leaf[F(j) < count[in_leaf]]
                if not len(k):
                    break
                counts["triangle_tests"] += len(k)
                rr = r[k]
                tri = (start[k] + F(j)).astype(np.int64)
                v0, v1, v2 = (sc.positions[tri, m].T for m in range(3))
                e0 = tuple(v1[a] - v0[a] for a in range(3))
                e1 = tuple(v0[a] - v2[a] for a in range(3))
                Dk = tuple(D[rr, a] for a in range(3))
                M = _cross(e1, Dk)
                det = _dot(e0, M)
                ok = ~((det > -DET_EPS) & (det < DET_EPS))
                inv_det = F(1) / det
                T = tuple(P[rr, a] - v0[a] for a in range(3))
                Q = _cross(T, e0)
                dist = -_dot(e1, Q) * inv_det
                ok &= ~((dist > t[rr]) | (dist < r0[k]) | (dist > r1[k]))
                u = _dot(T, M) * inv_det
                ok &= ~((u < 0) | (u > 1))
                w = _dot(Dk, Q) * inv_det
                ok &= ~((w < 0) | (u + w > 1))
                acc = rr[ok]
                t[acc] = dist[ok]
                which[acc] = (start[k] + F(j))[ok]
                hu[acc] = u[ok]
                hv[acc] = w[ok]
            g[r] = np.where(enter, hit_next, miss_next)
            done = g[r] >= TERMINATOR
            last = (max_bvh_iterations > 0) and (i == max_bvh_iterations - 1)
            if last:
                cap = r[~done]
                t[cap] = F(-1)                           # set_bad_hit, fs:436-438
                capped[cap] = True
                active = active[:0]
            else:
                active = r[~done]
            i += 1
    counts["bad_hits"] = int(capped.sum())
    hits = np.zeros(n, HIT_DTYPE)
    hit = traced & ~capped & (which >= 0) & (t < tmax)
    hits["triangle"] = np.where(capped, HIT_CAP, np.where(hit, which.astype(np.int64), HIT_MISS))
    hits["t"] = np.where(traced & (which >= 0), t, np.where(capped, t, tmax))
    hits["u"] = hu
    hits["v"] = hv
    return hits, counts


# exact_div.h's range predicates, restated on the raw exponent field (NaN and inf fail every one of them; a denormal's field
# is 0, below every range).  The walk above divides; these only say which form of the slab test the library may choose.
def magnitude_in(v, lo_exp: int, hi_exp: int):
    """2^lo_exp <= |v| < 2^(hi_exp + 1)"""
    e = ((np.ascontiguousarray(v, F).view(np.uint32) >> 23) & 0xff).astype(np.int64) - 127
    return (e >= lo_exp) & (e <= hi_exp)


def divisor_in_range(b):
    return magnitude_in(b, -40, 19)


def coordinate_in_range(c):
    return (np.asarray(c, F) == 0) | magnitude_in(c, -70, 59)


def scene_exact_div_ok(boxmin, boxmax) -> int:
    """the scene's flag: every box coordinate is 0 or has magnitude in [2^-70, 2^60)"""
    return int(coordinate_in_range(boxmin).all() and coordinate_in_range(boxmax).all())


def fast_division(flag: int, origins, directions):
    """bool [n]: the ray may take div_by_constant4 (wave_traversal.h: lane_begin, multihit.hip: make_slab); else it divides"""
    o, d = np.asarray(origins, F).reshape(-1, 3), np.asarray(directions, F).reshape(-1, 3)
    return bool(flag) & divisor_in_range(d).all(1) & coordinate_in_range(o).all(1)


def xform(m, v, w):
    """trace_common.h: xform -- column-major mat4 times (v, w), float32, in the shader's order ([n, 3] v)."""
    m = np.asarray(m, F).reshape(16)
    v = np.asarray(v, F).reshape(-1, 3)
    w = F(w)
    return np.stack([((m[r] * v[:, 0] + m[4 + r] * v[:, 1]) + m[8 + r] * v[:, 2]) + m[12 + r] * w for r in range(3)], axis=1)


def camera_rays(oracle, params, width: int, height: int):
    """The object-space 1-spp pixel-centre rays of a frame ([h * w, 3] origins and directions, row 0 = bottom): the oracle's
    primary ray at ((px + .5) / w, (py + .5) / h), then the object transform of trace_ray."""
    fw, fh = F(width), F(height)
    origins = np.empty((height * width, 3), F)
    dirs = np.empty((height * width, 3), F)
    for py in range(height):
        v = (F(py) + F(0.5)) / fh
        for px in range(width):
            u = (F(px) + F(0.5)) / fw
            o, d = oracle.primary_ray(params, float(u), float(v))
            origins[py * width + px] = o
            dirs[py * width + px] = d
    return xform(params.object_matrix, origins, 1.0), xform(params.object_normal_matrix, dirs, 0.0)
