"""Restatement of the instance-pair collision matrix (include/shader_ray_instance_pairs.h), for the tests.

The header's definition, over tests/instance_intersect_ref.py: cell (a, b) is the instance form's membership of instance a
(own_membership with skip_own) restricted to the columns of instance b -- its sum is the count (consequence 1), its smallest
(row, column) in row-major order the key (consequence 2).  memberships() computes those blocks once; brute() reads the matrix
off them.

restated_pairs is the kernel's scheme in plain python: one workgroup per 64 triangles of a row's instance, the workgroups in
an order the caller gives, every workgroup walking the instances b and reading and writing the shared cells as the kernel does
(the ANY skip, the first-only skip, one sum and one minimum per wave and instance), every decision replaceable so that
tests/test_instance_pairs_reference.py can show which input catches which mistake.  What a lane finds in an instance is read
off the membership: the walk inside an instance is instance_intersect_ref.restated_walk's and is restated there.

walk_counters_sum is the counting form: the sum over the ordered pairs (a, b), b != a, of instance_intersect_ref.walk_counters
with b's tree and image boxes, a's world rows as the queries and the box the top level stores for b.

For sets too large for a dense membership table on the host: member_pairs is the per-pair test on torch tensors
(point_query_ref.TorchOps, the same bits) with the members as index pairs, brute_of_pairs a cell from them, and
pair_walk_counters one ordered pair's counting walk without the table.
"""
from __future__ import annotations

import numpy as np

import instance_intersect_ref as II
import instance_point_ref as IP
import intersect_ref as IR

F = np.float32
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
ANY, FIRST_ONLY, COUNTS = "any", "first only", "counts"
MODES = (ANY, FIRST_ONLY, COUNTS)
LANES = 64
COUNTERS = ("node_visits", "leaf_visits", "triangle_tests", "traversals")


def key_ta_first(ta, tb):
    return (int(ta) << 32) | int(tb)


def key_tb_first(ta, tb):
    """a mutant: the scene triangle leads the key"""
    return (int(tb) << 32) | int(ta)


def memberships(scene_positions, scene_of_instance, maps, skip_shared=False, device=None):
    """(blocks, walked): blocks[a][b] is bool [triangles of a, triangles of b], the header's M(a, ., b, .) with b == a cleared;
    walked[a] is bool [triangles of a], the queries of instance a that are walked.  What instance_intersect_ref.own_membership
    gives with skip_own (tests/test_instance_pairs_reference.py compares the two), from one merged scene.  With `device` the
    pairs are tested there (member_pairs: the same bits)."""
    n = len(maps)
    merged, first = IP.merged_positions(scene_positions, scene_of_instance, maps)
    world = merged.reshape(-1, 3, 3)
    blocks, walked = [], []
    for a in range(n):
        rows = world[first[a]:first[a + 1]]
        member = IR.intersects(rows, merged, skip_shared) if device is None else intersects_torch(rows, world, skip_shared, device)
        member[:, first[a]:first[a + 1]] = False
        blocks.append([member[:, first[b]:first[b + 1]] for b in range(n)])
        walked.append(IR.walked(rows))
    return blocks, walked


def member_pairs(q, tris, skip_shared=False, device="cpu", pairs=1 << 25):
    """(qi, ti) int64 arrays in row-major order: the pairs (query q[qi], triangle tris[ti]) that are members, what
    np.nonzero(intersect_ref.intersects(q, tris, skip_shared)) gives, computed on `device` through point_query_ref.TorchOps
    (each fp32 operation computed in float64 and rounded to float32: the same bits as numpy's); stage 0, which is comparisons
    only, in chunks of about `pairs` pairs.  For sets too large for a dense table on the host."""
    import torch

    import point_query_ref as PQ
    o = PQ.TorchOps(device)
    lo3 = lambda x, y, z: torch.where(torch.where(x < y, x, y) < z, torch.where(x < y, x, y), z)
    hi3 = lambda x, y, z: torch.where(torch.where(x > y, x, y) > z, torch.where(x > y, x, y), z)
    q, tris = np.ascontiguousarray(q, F).reshape(-1, 3, 3), np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    Q, T = o.f(q), o.f(tris)
    walk = torch.as_tensor(IR.walked(q), device=device)
    lo, hi = lo3(Q[:, 0], Q[:, 1], Q[:, 2]), hi3(Q[:, 0], Q[:, 1], Q[:, 2])
    least, most = lo3(T[:, 0], T[:, 1], T[:, 2]), hi3(T[:, 0], T[:, 1], T[:, 2])
    step = max(1, pairs // max(1, len(tris)))
    found = []
    for s0 in range(0, len(q), step):
        apart = ((least[None] > hi[s0:s0 + step, None]) | (most[None] < lo[s0:s0 + step, None])).any(2)
        at = torch.nonzero(~apart & walk[s0:s0 + step, None])
        found.append((at[:, 0] + s0, at[:, 1]))
    qi, ti = torch.cat([f[0] for f in found]), torch.cat([f[1] for f in found])
    if len(qi) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    Q, T = Q[qi], T[ti]
    col = lambda x, i: tuple(x[:, i, k] for k in range(3))
    sub = lambda x, y: tuple(o.sub(x[k], y[k]) for k in range(3))
    cross = lambda x, y: (o.sub(o.mul(x[1], y[2]), o.mul(x[2], y[1])), o.sub(o.mul(x[2], y[0]), o.mul(x[0], y[2])),
                          o.sub(o.mul(x[0], y[1]), o.mul(x[1], y[0])))
    dot = lambda x, y: o.add(o.add(o.mul(x[0], y[0]), o.mul(x[1], y[1])), o.mul(x[2], y[2]))
    origin = col(Q, 0)
    qs = [sub(col(Q, i), origin) for i in range(3)]
    vs = [sub(col(T, i), origin) for i in range(3)]
    f = (sub(qs[1], qs[0]), sub(qs[2], qs[1]), sub(qs[0], qs[2]))
    e = (sub(vs[1], vs[0]), sub(vs[2], vs[1]), sub(vs[0], vs[2]))
    nq, nt = cross(f[0], f[1]), cross(e[0], e[1])
    axes = [nq, nt] + [cross(f[i], e[j]) for i in range(3) for j in range(3)] + [cross(nq, f[i]) for i in range(3)] + \
        [cross(nt, e[j]) for j in range(3)]
    member = ~((nt[0] == 0) & (nt[1] == 0) & (nt[2] == 0))
    for A in axes:
        s = [dot(A, v) for v in vs]
        p = [dot(A, x) for x in qs]
        member &= ~((lo3(*s) > hi3(*p)) | (hi3(*s) < lo3(*p)))
    if skip_shared:
        member &= ~(Q[:, :, None, :] == T[:, None, :, :]).all(3).any(2).any(1)
    return qi[member].cpu().numpy(), ti[member].cpu().numpy()


def intersects_torch(q, tris, skip_shared, device):
    """intersect_ref.intersects(q, tris, skip_shared) as a dense table, from member_pairs"""
    out = np.zeros((len(q), len(tris)), bool)
    qi, ti = member_pairs(q, tris, skip_shared, device)
    out[qi, ti] = True
    return out


def brute_of_pairs(qi, ti):
    """(key, count) of one cell from member_pairs' (qi, ti), which come in row-major order"""
    return (NONE, 0) if len(qi) == 0 else (np.uint64(key_ta_first(qi[0], ti[0])), len(qi))


def brute(blocks, rows=None, upper=False):
    """(first: uint64 [r, n], counts: int64 [r, n]) of memberships()'s blocks: consequences 1 and 2 (and 5 for `upper`)"""
    n = len(blocks)
    rows = range(n) if rows is None else rows
    first = np.full((len(rows), n), NONE, np.uint64)
    counts = np.zeros((len(rows), n), np.int64)
    for r, a in enumerate(rows):
        for b in range(n):
            block = blocks[a][b]
            if (upper and b <= a) or not block.any():
                continue
            counts[r, b] = int(block.sum())
            ta, tb = divmod(int(np.argmax(block.reshape(-1))), block.shape[1])   # the first set entry in row-major order
            first[r, b] = np.uint64(key_ta_first(ta, tb))
    return first, counts


def split_keys(first):
    """(triangle_a, triangle_b) int32 of uint64 keys, -1 where none"""
    first = np.asarray(first, np.uint64)
    return (first >> np.uint64(32)).astype(np.uint32).view(np.int32), (first & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def workgroups(blocks, rows):
    """the launch's workgroups in grid order: (row index, instance, first triangle), ceil(triangles / 64) per row"""
    out = []
    for r, a in enumerate(rows):
        triangles = blocks[a][a].shape[0]
        out += [(r, a, g * LANES) for g in range((triangles + LANES - 1) // LANES)]
    return out


def restated_pairs(blocks, walked, mode, order=None, rows=None, upper=False, *, scene_of=None, top_culled=None,
                   own_is=lambda b, a, scene_of: b == a, upper_skips=lambda b, a: b <= a,
                   any_cell=lambda counts, r, a, b, first_row: counts[r, b], key=key_ta_first, key_lead=lambda k: k >> 32,
                   add_always=True):
    """The kernel's scheme.  `blocks`, `walked`: memberships()'s.  `mode`: ANY, FIRST_ONLY or COUNTS.  `order`: a permutation
    of range(len(workgroups(blocks, rows))), the order in which the workgroups run (None: grid order); a workgroup runs to its
    end before the next begins, which is one of the interleavings the device may take -- the argument in DESIGN section 31 is
    that the cells' final values do not depend on it.  `top_culled`: None, or top_culled[a][b] bool [triangles of a]: the lanes
    the top level keeps out of b.  The keyword arguments replace one decision each: which instance is the query's own, which
    instances SHRAY_PAIRS_UPPER leaves out, which cell the ANY skip reads, the key and the part of it the first-only skip
    compares with the lane's triangle, and whether a wave's count is added even when its key does not lower the cell's.
    Returns (first uint64 [r, n] or None, counts int64 [r, n] or None)."""
    n = len(blocks)
    rows = list(range(n) if rows is None else rows)
    first_row = rows[0] if rows else 0
    first = np.full((len(rows), n), NONE, np.uint64)
    counts = np.zeros((len(rows), n), np.int64)
    groups = workgroups(blocks, rows)
    for g in (range(len(groups)) if order is None else order):
        r, a, t0 = groups[g]
        triangles = blocks[a][a].shape[0]
        lanes = range(t0, min(t0 + LANES, triangles))
        for b in range(n):
            if own_is(b, a, scene_of) or (upper and upper_skips(b, a)):
                continue
            if mode == ANY and any_cell(counts, r, a, b, first_row) != 0:
                continue
            cell = int(first[r, b])
            total, least = 0, int(NONE)
            for ta in lanes:
                if not walked[a][ta] or (top_culled is not None and top_culled[a][b][ta]):
                    continue
                if mode == FIRST_ONLY and key_lead(cell) < ta:
                    continue
                hit = np.flatnonzero(blocks[a][b][ta])
                if len(hit) == 0:
                    continue
                total += 1 if mode == ANY else len(hit)
                least = min(least, key(ta, int(hit[0])))
            if total == 0:
                continue
            if mode == ANY:
                counts[r, b] = 1
                continue
            if mode == COUNTS and (add_always or least < cell):
                counts[r, b] += total
            first[r, b] = np.uint64(min(cell, least))
    if mode == ANY:
        return None, counts
    return first, (counts if mode == COUNTS else None)


def stored_boxes_of(scene_positions, scene_of_instance, maps):
    """the boxes a top level stores for the instances, from instance_point_ref.stored_box on each scene's vertex box"""
    out = []
    for i, M in enumerate(maps):
        v = np.asarray(scene_positions[scene_of_instance[i]], F).reshape(-1, 3)
        out.append(IP.stored_box(M, v.min(0), v.max(0))[:2])
    return out


def top_culls(scene_positions, scene_of_instance, maps, stored):
    """top_culled for restated_pairs: [a][b] bool [triangles of a], instance_intersect_ref.guarded_misses of b's stored box
    against the query's vertex box (a set of one instance culls nothing)"""
    n = len(maps)
    out = []
    for a in range(n):
        lo, hi = II.vertex_box(II.own_queries(scene_positions, scene_of_instance, maps, a))
        out.append([np.asarray(II.guarded_misses(np.asarray(stored[b][0], F)[None], np.asarray(stored[b][1], F)[None], lo, hi)) if n > 1
                    else np.zeros(len(lo), bool) for b in range(n)])
    return out


def walk_counters_sum(trees, scene_positions, scene_of_instance, maps, stored, rows=None, upper=False, skip_shared=False, any_only=False):
    """The counting form's four counters, and `members` int64 [r, n] (the count matrix as the walks find it).  trees[s] is
    (refit_ref.TreeArrays, node boxes float32 [nodes, 6], object corners [T, 3, 3] in the tree's order) of distinct scene s;
    `stored`: the box (lo, hi) the set's top level stores for every instance."""
    n = len(maps)
    rows = list(range(n) if rows is None else rows)
    total = dict.fromkeys(COUNTERS, 0)
    members = np.zeros((len(rows), n), np.int64)
    for r, a in enumerate(rows):
        queries = II.own_queries(scene_positions, scene_of_instance, maps, a)
        for b in range(n):
            if b == a or (upper and b <= a):
                continue
            tree, node_boxes, corners = trees[scene_of_instance[b]]
            w = II.walk_counters(tree, node_boxes, corners, maps[b], queries, top_box=stored[b] if n > 1 else None, skip_shared=skip_shared,
                                 any_only=any_only)
            assert (w["members"][w["traversals"] == 0] == 0).all(), "no pair is behind a culled instance"
            for c in COUNTERS:
                total[c] += int(w[c].sum())
            members[r, b] = int((w["members"] * IR.walked(queries)).sum())
    return total, members


def pair_walk_counters(tree, node_boxes, world_b, M, queries, top_box):
    """instance_intersect_ref.walk_counters without its dense membership table, for members too large for one (the walk that
    does not stop at a member never reads it): the four counters of the queries' walks of ONE instance, summed.
    `world_b`: the instance's world corners [T, 3, 3] in the tree's order."""
    nb = np.asarray(node_boxes, F).reshape(-1, 6)
    q = IR.corners_of(queries)
    lo, hi = II.vertex_box(q)
    go = IR.walked(q)
    if top_box is not None:
        go = go & ~II.guarded_misses(np.asarray(top_box[0], F)[None], np.asarray(top_box[1], F)[None], lo, hi)
    ilo, ihi = IP.image_box(np.asarray(M, F).reshape(3, 4), nb[:, :3], nb[:, 3:])
    w = IR.walk_counters(tree, np.concatenate([ilo, ihi], axis=1), world_b, np.ascontiguousarray(q[go]))
    out = {c: int(w[c].sum()) for c in IR.COUNTERS}
    out["traversals"] = int(go.sum())
    return out, go
