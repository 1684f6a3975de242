"""CPU restatement of the refit (include/shader_ray_refit.h) in numpy: the box3d::add fold of every node's triangles with the
reference's float32 arithmetic (vectormath.h:121-129, :189-195), the SAH cost of a tree over its boxes, the operand-range
flag of exact_div.h, and the in-order node numbering of get_shader_data (world.cpp:145-177).

A tree is the pre-order arrays of shray_tree_desc (World.export_tree, shray_device_tree_download): `TreeArrays.of(desc)`."""
from __future__ import annotations

import ctypes as C

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
BUMPOUT = F(0.00001)
SAH_CTRAV, SAH_CISEC = 1.0, 4.0     # bvh.cpp:28-58


class TreeArrays:
    """numpy copies of a shray_tree_desc's pre-order arrays (root = node 0; a node, its negative subtree, its positive subtree)."""

    def __init__(self, parent, negative, positive, box, direction, start, triangles, triangle_vertices):
        self.parent, self.negative, self.positive = parent, negative, positive
        self.box = box                      # float32 [n, 6]: boxmin.xyz, boxmax.xyz
        self.direction = direction          # float32 [n, 3]: the split direction
        self.start, self.triangles = start, triangles
        self.triangle_vertices = triangle_vertices   # int32 [T, 3], post-build order

    @classmethod
    def of(cls, desc) -> "TreeArrays":
        n, t = desc.node_count, desc.triangle_count

        def take(ptr, count, dtype):
            return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True) if count else np.zeros(0, dtype)

        return cls(take(desc.node_parent, n, np.int32), take(desc.node_negative, n, np.int32), take(desc.node_positive, n, np.int32),
                   take(desc.node_box, 6 * n, F).reshape(n, 6), take(desc.node_direction, 3 * n, F).reshape(n, 3),
                   take(desc.node_start, n, np.int32), take(desc.node_triangles, n, np.int32),
                   take(desc.triangle_vertices, 3 * t, np.int32).reshape(t, 3))

    @property
    def node_count(self) -> int:
        return len(self.negative)


def triangle_boxes(corners) -> tuple[np.ndarray, np.ndarray]:
    """box3d().add(v0, v1, v2) of every triangle: corners float32 [T, 3, 3] -> (lo, hi) float32 [T, 3].  Finite inputs: no NaN and
    no -0.0 arises (v -+ 1e-5 is zero only as +0.0), so the order-free np.minimum equals std::min's fold."""
    c = np.asarray(corners, F).reshape(-1, 3, 3)
    lo = np.minimum(np.full((len(c), 3), FLT_MAX, F), (c - BUMPOUT).min(axis=1))
    hi = np.maximum(np.full((len(c), 3), -FLT_MAX, F), (c + BUMPOUT).max(axis=1))
    return lo.astype(F), hi.astype(F)


def node_boxes(tree: TreeArrays, corners) -> np.ndarray:
    """Every node's box, float32 [n, 6] in pre-order: a leaf folds its range's triangle boxes (box3d's initial +-FLT_MAX for an
    empty range), a branch its children's -- the fold of its own range, which is the union of theirs."""
    lo, hi = triangle_boxes(corners)
    n = tree.node_count
    out = np.empty((n, 6), F)
    for k in range(n - 1, -1, -1):            # pre-order: children come after their parent
        if tree.negative[k] < 0:
            s, c = int(tree.start[k]), int(tree.triangles[k])
            if c:
                out[k, :3] = lo[s:s + c].min(axis=0)
                out[k, 3:] = hi[s:s + c].max(axis=0)
            else:
                out[k, :3], out[k, 3:] = FLT_MAX, -FLT_MAX
        else:
            a, b = out[tree.negative[k]], out[tree.positive[k]]
            out[k, :3] = np.minimum(a[:3], b[:3])
            out[k, 3:] = np.maximum(a[3:], b[3:])
    return out


def box_area(boxes) -> np.ndarray:
    """2 (dx dy + dx dz + dy dz) in double, dx = max(0, max.x - min.x) (box3d::dim's clamp)"""
    b = np.asarray(boxes, F).reshape(-1, 6).astype(np.float64)
    d = np.maximum(0.0, b[:, 3:] - b[:, :3])
    return 2.0 * (d[:, 0] * d[:, 1] + d[:, 0] * d[:, 2] + d[:, 1] * d[:, 2])


def sah_cost(tree: TreeArrays, boxes) -> float:
    """sum over nodes of area(n) / area(root) * (SAH_CTRAV for a branch, SAH_CISEC * count for a leaf); 0 for a root of area 0"""
    area = box_area(boxes)
    if not area[0] > 0.0:
        return 0.0
    weight = np.where(tree.negative < 0, SAH_CISEC * tree.triangles.astype(np.float64), SAH_CTRAV)
    return float(np.sum(area / area[0] * weight))


def exact_div_ok(boxes) -> bool:
    """every box coordinate is 0 or has magnitude in [2^-70, 2^60) (exact_div.h's operand range, shray_scene_create)"""
    m = np.abs(np.asarray(boxes, F))
    return bool(np.all((m == 0) | ((m >= F(2.0 ** -70)) & (m < F(2.0 ** 60)))))


def in_order_index(tree: TreeArrays) -> np.ndarray:
    """pre-order node -> its number in get_shader_data's arrays (generate_group_indices, world.cpp:145-177)"""
    n = tree.node_count
    size = np.ones(n, np.int64)
    for k in range(n - 1, -1, -1):
        if tree.negative[k] >= 0:
            size[k] = 1 + size[tree.negative[k]] + size[tree.positive[k]]
    first = np.zeros(n, np.int64)       # the first number of a node's subtree
    index = np.zeros(n, np.int64)
    for k in range(n):
        if tree.negative[k] >= 0:
            index[k] = first[k] + size[tree.negative[k]]
            first[tree.negative[k]] = first[k]
            first[tree.positive[k]] = index[k] + 1
        else:
            index[k] = first[k]
    return index


def flat_boxes(tree: TreeArrays, boxes) -> tuple[np.ndarray, np.ndarray]:
    """(group_boxmin, group_boxmax) float32 [n * 3] in get_shader_data's numbering"""
    index = in_order_index(tree)
    bmin, bmax = np.empty((tree.node_count, 3), F), np.empty((tree.node_count, 3), F)
    bmin[index], bmax[index] = boxes[:, :3], boxes[:, 3:]
    return bmin.reshape(-1), bmax.reshape(-1)


def tree_desc(tree: TreeArrays, boxes, vertex_data) -> "object":
    """A shray_tree_desc (the package's TreeDesc) of `tree` with new node boxes and vertex_data float32 [V, 9] -- the input of
    shray_flatten_device for the scene a refit must equal.  The arrays are kept alive on the returned object."""
    from __graft_entry__ import load_package
    N = load_package()._native
    keep = {"parent": np.ascontiguousarray(tree.parent, np.int32), "negative": np.ascontiguousarray(tree.negative, np.int32),
            "positive": np.ascontiguousarray(tree.positive, np.int32), "box": np.ascontiguousarray(boxes, F).reshape(-1),
            "direction": np.ascontiguousarray(tree.direction, F).reshape(-1),
            "start": np.ascontiguousarray(tree.start, np.int32), "triangles": np.ascontiguousarray(tree.triangles, np.int32),
            "tv": np.ascontiguousarray(tree.triangle_vertices, np.int32).reshape(-1),
            "vd": np.ascontiguousarray(vertex_data, F).reshape(-1, 9)}
    d = N.TreeDesc()
    d.struct_size = C.sizeof(N.TreeDesc)
    d.node_count = tree.node_count
    i32 = C.POINTER(C.c_int32)
    f32 = C.POINTER(C.c_float)
    d.node_parent, d.node_negative, d.node_positive = (keep[k].ctypes.data_as(i32) for k in ("parent", "negative", "positive"))
    d.node_box, d.node_direction = keep["box"].ctypes.data_as(f32), keep["direction"].ctypes.data_as(f32)
    d.node_start, d.node_triangles = keep["start"].ctypes.data_as(i32), keep["triangles"].ctypes.data_as(i32)
    d.triangle_count = len(tree.triangle_vertices)
    d.triangle_vertices = keep["tv"].ctypes.data_as(i32)
    d.vertex_count = len(keep["vd"])
    d.vertex_data = keep["vd"].ctypes.data_as(f32)
    d._keep = keep
    return d
