"""Restatement of the signed distance query (include/shader_ray_sdf.h), for the tests.

numpy float32, one rounding per operation, in the header's order: the weld of corners by position, the face normals, the
corner angles through the renderer's atan_yx, the vertex and edge pseudonormals summed step by step (the k-th corner of
every vertex at once, the k-th slot of every edge at once: no np.add.at or sum, whose order is not the contract's), the
topology counts and the sign of a closest-point record.  Vertex and edge numbers here are np.unique's; the header exposes
none, and nothing below depends on them.

Also the ground truth the sign is checked against: the generalized winding number in float64 (the solid angles of Van
Oosterom and Strackee, IEEE Trans. Biomed. Eng. 30(2), 1983), which is 1 inside a closed outward-wound mesh and 0 outside.
"""
from __future__ import annotations

import numpy as np

F = np.float32
SIGN_DATA_FLOATS = 21
# the two corners of edge slots AB, AC, BC in the triangle's traversal a -> b -> c -> a: (from, to)
SLOT_ENDS = ((0, 1), (2, 0), (1, 2))


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], axis=-1)


def atan_yx(y, x):
    """csrc/trace_common.h atan_yx, elementwise in float32"""
    y, x = np.asarray(y, F), np.asarray(x, F)
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        hi = np.where(ax < ay, ay, ax)
        lo = np.where(ax < ay, ax, ay)
        q = lo / hi
        fold = q > F(0.414213562)
        z = np.where(fold, (q - F(1)) / (q + F(1)), q)
        zz = z * z
        poly = F(0.0803788006) * zz
        poly = (poly + F(-0.138722613)) * zz
        poly = (poly + F(0.199771404)) * zz
        poly = poly + F(-0.33332932)
        angle = z + (z * zz) * poly
        angle = np.where(fold, F(0.785398163) + angle, angle)
        angle = np.where(ay > ax, F(1.57079633) - angle, angle)
        angle = np.where(x < F(0), F(3.14159265) - angle, angle)
        angle = np.where(y < F(0), -angle, angle)
        return np.where(hi == F(0), F(0), angle).astype(F)


def weld(positions):
    """vertex number per corner: equal float coordinates (-0 == +0) weld, a corner with a non-finite coordinate stands alone"""
    p = np.asarray(positions, F).reshape(-1, 3)
    finite = np.isfinite(p).all(1)
    keys = np.where(p == F(0), F(0), p).view(np.uint32)
    vertex = np.zeros(len(p), np.int64)
    if finite.any():
        _, inverse = np.unique(keys[finite], axis=0, return_inverse=True)
        vertex[finite] = inverse.reshape(-1)
    base = int(vertex[finite].max()) + 1 if finite.any() else 0
    vertex[~finite] = base + np.arange(int((~finite).sum()))
    return vertex


def face_normals(tris):
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    with np.errstate(all="ignore"):
        n = _cross(b - a, c - a)
        length = np.sqrt(_dot(n, n))
        bad = (length == F(0)) | ~np.isfinite(length)
        nh = np.where(bad[:, None], F(0), n / length[:, None])
    return nh.astype(F), bad


def corner_angles(tris):
    """alpha per corner, [T, 3]"""
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    out = []
    with np.errstate(all="ignore"):
        for u, w in ((b - a, c - a), (c - b, a - b), (a - c, b - c)):
            x = _cross(u, w)
            alpha = atan_yx(np.sqrt(_dot(x, x)), _dot(u, w))
            out.append(np.where((_dot(u, u) == F(0)) | (_dot(w, w) == F(0)), F(0), alpha))
    return np.stack(out, axis=1).astype(F)


def _stepwise_sums(group, order_key, terms, groups):
    """per group, the float32 sum of its terms in ascending order_key, from +0, one rounding per step"""
    order = np.lexsort((order_key, group))
    g = group[order]
    starts = np.r_[0, np.nonzero(g[1:] != g[:-1])[0] + 1]
    rank = np.arange(len(g)) - np.repeat(starts, np.diff(np.r_[starts, len(g)]))
    sums = np.zeros((groups, 3), F)
    t = terms[order]
    for k in range(int(rank.max()) + 1 if len(rank) else 0):
        sel = rank == k
        with np.errstate(all="ignore"):
            sums[g[sel]] = sums[g[sel]] + t[sel]
    return sums


def derive(positions):
    """{"sign_data": float32 [T, 7, 3] (nhat, vertex a, b, c, edge AB, AC, BC), "info": the surface_info dict}"""
    tris = np.asarray(positions, F).reshape(-1, 3, 3)
    T = len(tris)
    nh, degenerate = face_normals(tris)
    alpha = corner_angles(tris).reshape(-1)
    vertex = weld(positions)
    V = int(vertex.max()) + 1 if T else 0
    corner = np.arange(3 * T)
    with np.errstate(all="ignore"):
        terms = alpha[:, None] * np.repeat(nh, 3, axis=0)
    vsum = _stepwise_sums(vertex, corner, terms.astype(F), V)

    v3 = vertex.reshape(-1, 3)
    frm = np.stack([v3[:, f] for f, _ in SLOT_ENDS], axis=1).reshape(-1)
    to = np.stack([v3[:, t] for _, t in SLOT_ENDS], axis=1).reshape(-1)
    pairs = np.stack([np.minimum(frm, to), np.maximum(frm, to)], axis=1)
    if T:
        _, edge = np.unique(pairs, axis=0, return_inverse=True)
        edge = edge.reshape(-1)
    else:
        edge = np.zeros(0, np.int64)
    E = int(edge.max()) + 1 if T else 0
    esum = _stepwise_sums(edge, corner, np.repeat(nh, 3, axis=0), E)

    sign = np.zeros((T, 7, 3), F)
    sign[:, 0] = nh
    sign[:, 1:4] = vsum[vertex].reshape(T, 3, 3)
    sign[:, 4:7] = esum[edge].reshape(T, 3, 3)

    uses = np.bincount(edge, minlength=E)
    mis = 0
    two = np.nonzero(uses == 2)[0]
    if len(two):
        order = np.lexsort((corner, edge))
        first = np.r_[0, np.cumsum(uses)[:-1]]
        s0, s1 = order[first[two]], order[first[two] + 1]
        mis = int((frm[s0] == frm[s1]).sum())
    info = {"vertices": V, "edges": E, "boundary_edges": int((uses == 1).sum()), "nonmanifold_edges": int((uses >= 3).sum()),
            "misoriented_edges": mis, "degenerate_triangles": int(degenerate.sum())}
    info["closed"] = int(info["boundary_edges"] == 0 and info["nonmanifold_edges"] == 0 and info["misoriented_edges"] == 0)
    return {"sign_data": sign, "info": info}


def signed(points, records, sign_data):
    """the header's signed distance of each closest-point record (point_query_ref.CLOSEST_DTYPE), NaN on a miss"""
    p = np.asarray(points["p"], F)
    q = np.asarray(records["q"], F)
    d2 = np.asarray(records["dist2"], F)
    tri = records["triangle"]
    region = records["region"]
    hit = tri >= 0
    slot = np.where(region == 6, 0, region + 1)
    nrm = sign_data[np.where(hit, tri, 0), np.clip(slot, 0, 6)]
    with np.errstate(all="ignore"):
        s = _dot(p - q, nrm)
        d = np.sqrt(d2)
    out = np.where((s < F(0)) & (d2 > F(0)), -d, d).astype(F)
    return np.where(hit, out, F(np.nan)).astype(F)


def unweighted_sign_data(positions):
    """the variant the tests show to be wrong: vertex pseudonormals as the plain sum of the incident face normals"""
    tris = np.asarray(positions, F).reshape(-1, 3, 3)
    out = derive(positions)["sign_data"].copy()
    nh, _ = face_normals(tris)
    vertex = weld(positions)
    vsum = _stepwise_sums(vertex, np.arange(len(vertex)), np.repeat(nh, 3, axis=0), int(vertex.max()) + 1)
    out[:, 1:4] = vsum[vertex].reshape(-1, 3, 3)
    return out


def winding_number(positions, points, chunk=1 << 20):
    """float64 generalized winding number of each point (1 inside a closed outward-wound mesh, 0 outside)"""
    tris = np.asarray(positions, np.float64).reshape(-1, 3, 3)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.zeros(len(p))
    step = max(1, chunk // max(1, len(tris)))
    for s in range(0, len(p), step):
        r = tris[None, :, :, :] - p[s:s + step, None, None, :]
        a, b, c = r[..., 0, :], r[..., 1, :], r[..., 2, :]
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        det = np.einsum("...i,...i", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("...i,...i", a, b) * lc + np.einsum("...i,...i", a, c) * lb + np.einsum("...i,...i", b, c) * la
        out[s:s + step] = (2.0 * np.arctan2(det, den)).sum(1) / (4.0 * np.pi)
    return out


# small closed meshes, outward winding: (positions float32 [V, 3], triangles int32 [T, 3])
def cube():
    """the unit cube [0, 1]^3, two triangles per face"""
    pos = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    tri = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return pos, np.array(tri, np.int32)


def tetrahedron():
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    return pos, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)


def fan_spike(n=24, height=6.0):
    """a steep square pyramid (apex at height, base [-1, 1]^2 at z = 0) whose +x side is split at the apex into a fan of n
    thin triangles: the apex's incident face normals are far from orthogonal, and n of them share one face's angle"""
    base = np.array([[1, -1, 0], [1, 1, 0], [-1, 1, 0], [-1, -1, 0]], F)
    apex = np.array([[0, 0, height]], F)
    s = np.linspace(-1, 1, n + 1).astype(F)
    edge = np.stack([np.ones(n + 1, F), s, np.zeros(n + 1, F)], axis=1)[1:-1]   # inner points of the +x base edge
    pos = np.concatenate([base, apex, edge]).astype(F)
    ring = [0] + list(range(5, 5 + n - 1)) + [1]                                # the +x base edge, -y to +y
    tri = [(ring[k], ring[k + 1], 4) for k in range(n)]                          # the fan at the apex
    tri += [(1, 2, 4), (2, 3, 4), (3, 0, 4)]                                     # the other three sides
    tri += [(0, 3, 2)] + [(ring[k + 1], ring[k], 2) for k in range(n)]            # the base, a fan at (-1, 1)
    return pos, np.array(tri, np.int32)


def corners_of(pos, tri):
    """the scene's corner positions (9 floats per triangle)"""
    return np.asarray(pos, F)[np.asarray(tri)].reshape(-1)
