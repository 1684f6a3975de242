"""CPU restatement of what scene creation derives from a tree (shray_scene_create, shray_scene_create_from_device; read back by
shray_scene_derived_download): the eight octant copies of the packed tree, the packed triangles, the fp16 normals, the pair records
and the deepest ray stack, in the record formats of csrc/packed_layout.h.

The tree is the pre-order arrays of shray_tree_desc (refit_ref.TreeArrays); the packed order is that pre-order.  The boxes come from
the flattener's arrays, numbered in-order (refit_ref.in_order_index)."""
from __future__ import annotations

import numpy as np

from refit_ref import TreeArrays, in_order_index

F, U32 = np.float32, np.uint32
LEAF_FLAG = 0x80000000
AXIS_HOT_SHIFT = 29            # device form: a' = 1 << (29 + axis) | name
NAME_SHIFT = 2                 # a node's name = its byte offset / 8 = index * 32 / 8
PAIR_INDEX_MASK, PAIR_COUNT_SHIFT, PAIR_COUNT_MASK, PAIR_AXIS_SHIFT = 0x003fffff, 22, 0x7f, 29


def half_bits(values) -> np.ndarray:
    """binary32 -> binary16 bits, round to nearest even, as csrc/half_bits.h: float_to_half_bits computes them (np.float16 keeps a
    NaN's payload; this gives every NaN the quiet 0x7e00)"""
    u = np.ascontiguousarray(values, F).reshape(-1).view(U32).astype(np.int64)
    sign = (u >> 16) & 0x8000
    mag = u & 0x7fffffff
    # subnormal halves: mag in [0x33000001, 0x38800000)
    shift = np.clip(126 - (mag >> 23), 14, 24)
    mant = (mag & 0x7fffff) | 0x800000
    q = mant >> shift
    rem = mant & ((1 << shift) - 1)
    halfway = 1 << (shift - 1)
    subnormal = q + ((rem > halfway) | ((rem == halfway) & ((q & 1) == 1)))
    normal = (mag + 0xfff + ((mag >> 13) & 1) - 0x38000000) >> 13
    out = np.where(mag > 0x7f800000, 0x7e00,
          np.where(mag >= 0x477ff000, 0x7c00,
          np.where(mag < 0x33000001, 0,
          np.where(mag < 0x38800000, subnormal, normal))))
    return (sign | out).astype(np.uint16)


def split_axis(tree: TreeArrays) -> np.ndarray:
    """a branch's split axis: the first nonzero component of its direction (sd_pack_nodes); 0 for a leaf"""
    d = np.asarray(tree.direction, F).reshape(-1, 3)
    axis = np.where(d[:, 0] != 0, 0, np.where(d[:, 1] != 0, 1, 2))
    return np.where(tree.negative >= 0, axis, 0).astype(np.int64)


def node_boxes(tree: TreeArrays, group_boxmin, group_boxmax) -> tuple[np.ndarray, np.ndarray]:
    """(lo, hi) float32 [n, 3] in pre-order, from the flattener's in-order arrays"""
    index = in_order_index(tree)
    return (np.asarray(group_boxmin, F).reshape(-1, 3)[index], np.asarray(group_boxmax, F).reshape(-1, 3)[index])


def octant_copies(tree: TreeArrays, group_boxmin, group_boxmax) -> np.ndarray:
    """uint32 [8, n, 8]: copy o holds every node as DeviceNode's words { entry.x, entry.y, exit.x, exit.y, entry.z, exit.z, a', b' }.
    Bit k of o set: the ray's D[k] >= 0, so it enters by the min plane of axis k; a branch's a' names the child it visits first
    (the negative one when the split axis' bit is set), b' the other; a leaf keeps { start, 0x80000000 | count }."""
    lo, hi = node_boxes(tree, group_boxmin, group_boxmax)
    leaf = tree.negative < 0
    axis = split_axis(tree)
    neg_name = np.where(leaf, 0, tree.negative).astype(np.int64) << NAME_SHIFT
    pos_name = np.where(leaf, 0, tree.positive).astype(np.int64) << NAME_SHIFT
    out = np.zeros((8, tree.node_count, 8), U32)
    for o in range(8):
        enters_low = np.array([(o >> k) & 1 for k in range(3)], bool)
        entry, leave = np.where(enters_low, lo, hi).view(U32), np.where(enters_low, hi, lo).view(U32)
        out[o, :, 0:2], out[o, :, 2:4], out[o, :, 4], out[o, :, 5] = entry[:, :2], leave[:, :2], entry[:, 2], leave[:, 2]
        negative_first = ((o >> axis) & 1) == 1
        out[o, :, 6] = np.where(leaf, tree.start, (1 << (AXIS_HOT_SHIFT + axis)) | np.where(negative_first, neg_name, pos_name))
        out[o, :, 7] = np.where(leaf, LEAF_FLAG | tree.triangles.astype(np.int64), np.where(negative_first, pos_name, neg_name))
    return out


def packed_triangles(vertex_positions) -> np.ndarray:
    """uint32 [T + 1, 9]: { v0, e0 = v1 - v0, e1 = v0 - v2 } per triangle (raytracer.es.fs:304-305), then a spare record of zeros"""
    v = np.asarray(vertex_positions, F).reshape(-1, 3, 3)
    tris = np.concatenate([v[:, 0], v[:, 1] - v[:, 0], v[:, 0] - v[:, 2]], axis=1).astype(F)
    return np.concatenate([tris, np.zeros((1, 9), F)]).view(U32)


def pair_records(tree: TreeArrays, group_boxmin, group_boxmax) -> np.ndarray:
    """uint32 [n, 16], PackedPair: a branch's record holds { neg.boxmin, neg.link, neg.boxmax, neg.info, pos.boxmin, pos.link,
    pos.boxmax, pos.info }; a leaf's is zeros.  link = child | min(count, 127) << 22 | 0x80000000 (a leaf), child | axis << 29 (a
    branch); info = the leaf's first triangle.  No records ([0, 16]) for a tree of more than 2^22 nodes."""
    n = tree.node_count
    if n > PAIR_INDEX_MASK + 1:
        return np.zeros((0, 16), U32)
    lo, hi = node_boxes(tree, group_boxmin, group_boxmax)
    leaf = tree.negative < 0
    axis = split_axis(tree)
    out = np.zeros((n, 16), U32)
    b = np.nonzero(~leaf)[0]
    for first, child in ((0, tree.negative[b]), (8, tree.positive[b])):
        count = np.minimum(tree.triangles[child].astype(np.int64), PAIR_COUNT_MASK)
        out[b, first:first + 3] = lo[child].view(U32)
        out[b, first + 3] = np.where(leaf[child], child | (count << PAIR_COUNT_SHIFT) | LEAF_FLAG, child | (axis[child] << PAIR_AXIS_SHIFT))
        out[b, first + 4:first + 7] = hi[child].view(U32)
        out[b, first + 7] = np.where(leaf[child], tree.start[child], 0)
    return out


def deepest_stack(tree: TreeArrays) -> int:
    """The most far children a ray can have pending: at a branch, its own one plus one for every ancestor whose NEAR child the
    path goes through, maximised over branches and the eight direction codes (bit k of a code set: the negative child is near
    at a split along k).  0 for a tree that is one leaf."""
    near = np.zeros((tree.node_count, 8), np.int64)
    axis = split_axis(tree)
    codes = np.arange(8)
    deepest, level = 0, np.array([0])
    while len(level):
        b = level[tree.negative[level] >= 0]
        if not len(b):
            break
        deepest = max(deepest, 1 + int(near[b].max()))
        negative_near = (codes[None, :] >> axis[b][:, None]) & 1
        near[tree.negative[b]] = near[b] + negative_near
        near[tree.positive[b]] = near[b] + (1 - negative_near)
        level = np.concatenate([tree.negative[b], tree.positive[b]])
    return deepest


def derived_arrays(tree: TreeArrays, flat: dict) -> dict:
    """Scene.derived_arrays() restated from the tree and the flattener's arrays (World.arrays(): group_boxmin, group_boxmax,
    vertex_positions, vertex_normals).  packed_tris keeps the spare record, which derived_arrays() does not read back."""
    corners = len(np.asarray(flat["vertex_positions"]).reshape(-1)) // 3
    return {"packed_nodes": octant_copies(tree, flat["group_boxmin"], flat["group_boxmax"]),
            "packed_tris": packed_triangles(flat["vertex_positions"]),
            "normals16": half_bits(np.asarray(flat["vertex_normals"], F).reshape(-1)[:3 * corners]),
            "pair_nodes": pair_records(tree, flat["group_boxmin"], flat["group_boxmax"]),
            "stack_levels": max(3, deepest_stack(tree))}
