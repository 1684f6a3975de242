"""The instance-pair collision matrix on the GPU (include/shader_ray_instance_pairs.h) against the brute force of
tests/instance_pairs_ref.py: every cell of `first` and of `counts`, in the three modes (SHRAY_PAIRS_ANY, keys only, keys and
counts), on the host path and the device path.  The nine-instance set of tests/instance_intersect_cases.py with
SHRAY_PAIRS_UPPER, SHRAY_PAIRS_SKIP_SHARED, row ranges and an empty range; the order-dependent forms launched twice; sets of
one and of two instances; members of 1, 11, 63, 64, 65 and 528 triangles in one set (the workgroup table's edges); two scenes
of different heights; 301 tiny instances (the search over many one-workgroup rows); the counters against
instance_pairs_ref.walk_counters_sum with the stored boxes as read back; InstanceSet.instances_colliding; a refit, a device
update and the matrix on one side stream, then a host update; the refusals that read the set; sixteen overlapping copies of
lobed_528, where many waves add to every cell."""
import ctypes as C

import numpy as np
import pytest

import instance_intersect_cases as XC
import instance_pairs_ref as PR
import instance_point_cases as IC
import refit_ref
import test_gpu_instance_point as G
from test_gpu_instance_overlap import stored_boxes
from test_gpu_instance_point import build, member
from test_gpu_ray_query import loaded

pytestmark = pytest.mark.gpu

F = np.float32
EYE = IC.EYE
PATHS = ("host", "device")
POISON = -7
_answers = {}
_made = []


@pytest.fixture(scope="module", autouse=True)
def close_what_the_module_made():
    yield
    _answers.clear()
    for s in G._sets:
        s.close()
    G._sets.clear()
    for x in reversed(_made):
        x.close()
    _made.clear()
    for _, sc in G._members.values():
        sc.close()
    G._members.clear()


def run(s, mode, path, rows=None, upper=False, skip_shared=False):
    """(first uint64 [r, n] or None, counts int64 [r, n] or None) of one query.  host: the blocking forms through
    collision_matrix / collision_pairs; device: collision_pairs_into into poisoned tensors on the current torch stream."""
    import torch
    n = s.count
    first_row, row_count = (0, n) if rows is None else (rows.start, len(rows))
    if path == "host":
        if mode == PR.ANY:
            got = s.collision_matrix(rows, upper, skip_shared)
            assert got.dtype == np.bool_ and got.shape == (row_count, n)
            return None, got.astype(np.int64)
        ta, tb, cnt = s.collision_pairs(rows, counts=mode == PR.COUNTS, upper=upper, skip_shared=skip_shared)
        assert ta.dtype == np.int32 and tb.dtype == np.int32 and ta.shape == tb.shape == (row_count, n)
        assert (cnt is None) == (mode != PR.COUNTS) and (cnt is None or (cnt.dtype == np.int64 and cnt.shape == (row_count, n)))
        assert np.array_equal(ta < 0, tb < 0)
        return ((ta.astype(np.int64).astype(np.uint64) << np.uint64(32)) | tb.view(np.uint32).astype(np.uint64)), cnt
    assert path == "device"
    cells = max(row_count * n, 1)
    first = torch.full((cells + 3,), POISON, dtype=torch.int64, device="cuda") if mode != PR.ANY else None
    counts = torch.full((cells + 3,), POISON, dtype=torch.int64, device="cuda") if mode != PR.FIRST_ONLY else None
    s.collision_pairs_into(first.data_ptr() if first is not None else 0, counts.data_ptr() if counts is not None else 0, first_row, row_count,
                           mode == PR.ANY, upper, skip_shared, torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    out = []
    for t in (first, counts):
        if t is None:
            out.append(None)
            continue
        assert bool((t[row_count * n:] == POISON).all()), "nothing is written past the rows"
        out.append(t[:row_count * n].cpu().numpy().reshape(row_count, n))
    return (None if out[0] is None else out[0].view(np.uint64)), out[1]


def wanted(brute, mode):
    first, counts = brute
    return {PR.ANY: (None, (counts > 0).astype(np.int64)), PR.FIRST_ONLY: (first, None), PR.COUNTS: (first, counts)}[mode]


def assert_cells(got, want, what):
    for name, g, w in zip(("first", "counts"), got, want):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
            bad = np.argwhere(g != w)
            assert len(bad) == 0, f"{what}: {len(bad)} cells of {name} differ, first {bad[:5].tolist()}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


def check_every_form(s, brute, what, paths=PATHS, **flags):
    for mode in PR.MODES:
        for path in paths:
            assert_cells(run(s, mode, path, **flags), wanted(brute, mode), f"{what}, {mode}, {path}")


def nine(pkg):
    """(positions, scene of every instance, maps, the set, blocks, walked, the brute force)"""
    if "nine" not in _answers:
        positions, of, maps, kinds, names = XC.nine_instances(lambda name: member(pkg, name)[0])
        assert kinds[4] == "duplicate of 1"
        s = build(pkg, names, maps, "nine instances")
        blocks, walked = PR.memberships(positions, of, maps)
        _answers["nine"] = (positions, of, maps, s, blocks, walked, PR.brute(blocks))
    return _answers["nine"]


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_the_nine_instance_set_in_the_three_modes(pkg, gpu):
    positions, of, maps, s, blocks, walked, brute = nine(pkg)
    first, counts = brute
    assert (counts > 0).sum() == 14 and counts[1, 4] == counts[4, 1] == 7488 and (counts[0, 6], counts[6, 0]) == (488, 487)
    check_every_form(s, brute, "nine instances")
    ta, tb, cnt = s.collision_pairs(device=True)
    import torch
    torch.cuda.current_stream().synchronize()
    assert ta.is_cuda and ta.dtype == torch.int32 and cnt.dtype == torch.int64
    want_ta, want_tb = PR.split_keys(first)
    assert np.array_equal(ta.cpu().numpy(), want_ta) and np.array_equal(tb.cpu().numpy(), want_tb) and np.array_equal(cnt.cpu().numpy(), counts)
    assert s.collision_pairs(counts=False, device=True)[2] is None
    assert s.colliding_pairs(upper=False).tolist() == np.argwhere(counts > 0).tolist()
    pairs = s.colliding_pairs()
    assert pairs.dtype == np.int32 and pairs.tolist() == [[0, 6], [0, 8], [1, 4], [2, 8], [3, 8], [6, 8], [7, 8]]


@pytest.mark.parametrize("mode", [PR.ANY, PR.FIRST_ONLY])
def test_the_forms_that_skip_by_what_a_cell_holds_give_equal_bytes_twice(pkg, gpu, mode):
    positions, of, maps, s, blocks, walked, brute = nine(pkg)
    once, again = run(s, mode, "device"), run(s, mode, "device")
    for a, b in zip(once, again):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()
    assert_cells(again, wanted(brute, mode), f"{mode}, the second launch")


def test_upper_and_skip_shared(pkg, gpu):
    positions, of, maps, s, blocks, walked, brute = nine(pkg)
    upper = PR.brute(blocks, upper=True)
    keep = np.triu(np.ones((9, 9), bool), 1)
    assert np.array_equal(upper[1], np.where(keep, brute[1], 0)) and (upper[1] > 0).sum() == 7
    check_every_form(s, upper, "UPPER", upper=True)
    shared = PR.brute(PR.memberships(positions, of, maps, skip_shared=True)[0])
    assert shared[1][1, 4] == 0 and shared[1][0, 6] == 488, "the twins' pairs all share a corner, the others none"
    check_every_form(s, shared, "SKIP_SHARED", skip_shared=True)
    both = (np.where(keep, shared[0], PR.NONE), np.where(keep, shared[1], 0))
    check_every_form(s, both, "UPPER | SKIP_SHARED", upper=True, skip_shared=True)


@pytest.mark.parametrize("rows", [range(0, 1), range(4, 9), range(8, 9), range(5, 5), range(9, 9)])
def test_row_ranges(pkg, gpu, rows):
    """Consequence 6, and row_count = 0 writes nothing (run() poisons the device buffers and looks past the rows)."""
    positions, of, maps, s, blocks, walked, brute = nine(pkg)
    part = (brute[0][rows.start:rows.stop], brute[1][rows.start:rows.stop])
    assert part[0].shape == (len(rows), 9)
    check_every_form(s, part, f"rows {rows}", rows=rows)
    check_every_form(s, PR.brute(blocks, rows, upper=True), f"rows {rows}, UPPER", rows=rows, upper=True)


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_sets_of_one_and_of_two_instances(pkg, gpu):
    lobed = member(pkg, "lobed_528")[0]
    s = build(pkg, ["lobed_528"], EYE[None], "one instance")
    none = (np.full((1, 1), PR.NONE, np.uint64), np.zeros((1, 1), np.int64))
    check_every_form(s, none, "one instance")
    assert s.colliding_pairs().shape == (0, 2) and not s.collision_matrix().any()
    # two: a copy shifted by a fifth of the part's size
    shift = EYE.copy()
    shift[:, 3] = F(0.2) * (lobed.reshape(-1, 3).max(0) - lobed.reshape(-1, 3).min(0))
    maps = np.stack([EYE, shift])
    s = build(pkg, ["lobed_528", "lobed_528"], maps, "two instances")
    brute = PR.brute(PR.memberships([lobed], [0, 0], maps)[0])
    assert brute[1][0, 1] > 100 and brute[1][1, 0] > 100 and brute[1][0, 0] == brute[1][1, 1] == 0, brute[1]
    check_every_form(s, brute, "two instances")
    check_every_form(s, PR.brute(PR.memberships([lobed], [0, 0], maps)[0], upper=True), "two instances, UPPER", upper=True)
    assert s.colliding_pairs().tolist() == [[0, 1]]


# 3 ---------------------------------------------------------------------------------------------------------------------------
CUTS = (63, 64, 65)


def cut_scene(pkg, tmp, triangles):
    """(vertex_positions, resident scene) of the first `triangles` triangles of lobed_528's list, a scene of their own"""
    lobed = member(pkg, "lobed_528")[0].reshape(-1, 3, 3)[:triangles]
    path = str(tmp / f"cut_{triangles}.obj")
    pkg.scenes.write_obj(path, lobed.reshape(-1, 3).astype(np.float64), np.arange(3 * triangles).reshape(-1, 3))
    world = pkg.World(path)
    _made.append(world)
    positions = np.asarray(world.arrays()["vertex_positions"], F).copy()
    assert len(positions) == 9 * triangles
    scene = pkg.Scene(world.flatten())
    _made.append(scene)
    return positions, scene


def edge_set(positions_of):
    """(scene of every instance, maps) of the set whose members have 1, 11, 63, 64, 65 and 528 triangles, each of the three
    cuts placed a second time by the same map: a twin meets every one of its triangles, the last lane of a full workgroup and
    the one lane of a second workgroup among them.  positions_of: the six distinct scenes' positions."""
    of = [0, 1, 2, 3, 4, 5, 2, 3, 4]
    _, maps, _ = IC.make_set(positions_of, of, seed=63, spread=0.4, kinds=["rotation_nonuniform", "shear", "mirror", "translation",
                                                                           "rotation_uniform", "identity", "shear", "mirror", "translation"])
    maps = np.array(maps)
    maps[6], maps[7], maps[8] = maps[2], maps[3], maps[4]
    return of, maps


def test_members_of_1_11_63_64_65_and_528_triangles(pkg, gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("instance_pairs")
    cuts = [cut_scene(pkg, tmp, t) for t in CUTS]
    distinct = [member(pkg, "one triangle"), member(pkg, "11-triangle leaf")] + cuts + [member(pkg, "lobed_528")]
    positions = [d[0] for d in distinct]
    assert [len(p) // 9 for p in positions] == [1, 11, 63, 64, 65, 528]
    of, maps = edge_set(positions)
    s = pkg.tracer.InstanceSet([distinct[k][1] for k in of], maps)
    _made.append(s)
    blocks, walked = PR.memberships(positions, of, maps)
    brute = PR.brute(blocks)
    for a, b, triangles in ((2, 6, 63), (3, 7, 64), (4, 8, 65)):
        assert blocks[a][b].diagonal().all() and blocks[b][a].diagonal().all(), "a twin meets each of its triangles, the last one too"
        assert brute[1][a, b] == brute[1][b, a] >= triangles
    assert (brute[1] > 0).sum() >= 12 and (brute[1][5] > 0).sum() >= 3, brute[1]
    check_every_form(s, brute, "1, 11, 63, 64, 65 and 528 triangles")
    check_every_form(s, (brute[0][2:6], brute[1][2:6]), "1, 11, 63, 64, 65 and 528 triangles, rows 2 to 5", rows=range(2, 6))


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["two scenes of different heights", "301 tiny instances"])
def test_sets_equal_the_brute_force(pkg, gpu, which):
    names, maps, kinds = G.the_set(pkg, which)
    s = build(pkg, names, maps, which)
    distinct = sorted(set(names))
    positions, of = [member(pkg, d)[0] for d in distinct], [distinct.index(x) for x in names]
    blocks, walked = PR.memberships(positions, of, maps)
    brute = PR.brute(blocks)
    set_cells = int((brute[1] > 0).sum())
    print(which, "set cells", set_cells, "largest count", int(brute[1].max()))
    assert set_cells >= (2 if len(names) == 2 else 300), (which, set_cells)
    check_every_form(s, brute, which)
    if len(names) > 2:
        rows = range(100, 203)
        check_every_form(s, (brute[0][100:203], brute[1][100:203]), f"{which}, rows {rows}", paths=("device",), rows=rows)
        check_every_form(s, PR.brute(blocks, upper=True), f"{which}, UPPER", paths=("device",), upper=True)


# 5 ---------------------------------------------------------------------------------------------------------------------------
def nine_trees(pkg, positions):
    """per distinct scene of the nine-instance set: (refit_ref.TreeArrays, node boxes, object corners in the tree's order)"""
    world = loaded(pkg, "lobed_528")[0]
    desc = world.export_tree()
    lobed_tree = refit_ref.TreeArrays.of(desc)
    vd = np.ctypeslib.as_array(desc.vertex_data, shape=(desc.vertex_count * 9,)).reshape(-1, 9)
    lobed_corners = np.ascontiguousarray(vd[lobed_tree.triangle_vertices][:, :, :3])
    assert np.array_equal(lobed_corners.reshape(-1).view(np.uint32), positions[0].view(np.uint32)), "the scene's triangles are in the tree's order"
    i32 = lambda *v: np.array(v, np.int32)
    trees = [(lobed_tree, lobed_tree.box, positions[0].reshape(-1, 3, 3))]
    for p in positions[1:]:
        corners = p.reshape(-1, 3, 3)
        v = corners.reshape(-1, 3)
        box = np.concatenate([v.min(0) - 1e-5, v.max(0) + 1e-5]).astype(F)[None]        # helpers.single_leaf_scene's
        trees.append((refit_ref.TreeArrays(i32(-1), i32(-1), i32(-1), None, None, i32(0), i32(len(corners)), None), box, corners))
    return trees


def test_the_counters_of_the_nine_instance_set(pkg, gpu):
    """node_visits, leaf_visits, triangle_tests and traversals of the counting form, equal to the sum over the ordered pairs
    (a, b), b != a, of instance_intersect_ref.walk_counters on b's own tree with a's world triangles as the queries and the box
    the set's top level stores for b; samples = the query triangles of the rows."""
    positions, of, maps, s, blocks, walked, brute = nine(pkg)
    stored = stored_boxes(pkg, s, 9)
    trees = nine_trees(pkg, positions)
    triangles = [len(positions[k]) // 9 for k in of]
    for rows, upper, skip_shared in ((None, False, False), (range(4, 9), True, False), (range(0, 2), False, True)):
        total, members = PR.walk_counters_sum(trees, positions, of, maps, stored, rows, upper, skip_shared)
        want = PR.brute(PR.memberships(positions, of, maps, True)[0] if skip_shared else blocks, rows, upper)
        assert np.array_equal(members, want[1]), "the counting walk finds every member"
        ta, tb, cnt, tally = s.collision_pairs(rows, upper=upper, skip_shared=skip_shared, counters=True)
        assert np.array_equal(cnt, want[1]) and np.array_equal(ta, PR.split_keys(want[0])[0]) and np.array_equal(tb, PR.split_keys(want[0])[1])
        for c in PR.COUNTERS:
            assert tally[c] == total[c], (rows, upper, c, tally, total)
        asked = range(9) if rows is None else rows
        assert tally["samples"] == sum(triangles[a] for a in asked)
        assert tally["shaded_hits"] == tally["env_lookups"] == tally["bad_hits"] == 0
        if rows is None and not upper:
            walked_rows = sum(int(walked[a].sum()) for a in asked)
            assert walked_rows < total["traversals"] < 8 * walked_rows, "the top level culls some instances and not all"
    # keys only, counted: the same walk (nothing is skipped by what a cell holds), and the keys
    total, _ = PR.walk_counters_sum(trees, positions, of, maps, stored)
    ta, tb, cnt, tally = s.collision_pairs(counts=False, counters=True)
    assert cnt is None and np.array_equal(ta, PR.split_keys(brute[0])[0]) and all(tally[c] == total[c] for c in PR.COUNTERS), (tally, total)


def test_a_row_collides_iff_instances_colliding_says_so(pkg, gpu):
    """Consequence 7."""
    positions, of, maps, s, blocks, walked, brute = nine(pkg)
    colliding = s.instances_colliding()
    assert colliding.tolist() == [a != 5 for a in range(9)]
    assert np.array_equal(s.collision_pairs()[2].any(axis=1), colliding) and np.array_equal(s.collision_matrix().any(axis=1), colliding)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_refit_update_and_matrix_on_one_stream_and_after_a_host_update(pkg, gpu):
    """A device refit of a member, a device update with moved maps and the matrix, enqueued on one side stream with nothing
    between them; then a host update with other maps.  Each against the brute force of the state the query must see."""
    import torch
    world, _, _ = loaded(pkg, "lobed_528")
    own = pkg.Scene(world.flatten())            # a scene of its own: it is refit below
    small_positions, small = member(pkg, "small_trisrc")
    before = np.asarray(own.geometry()["vertex_positions"], F).reshape(-1)
    names = ["lobed_528", "small_trisrc", "lobed_528", "lobed_528", "small_trisrc"]
    members = [own if x == "lobed_528" else small for x in names]
    of = [0 if x == "lobed_528" else 1 for x in names]
    kinds = ["rotation_nonuniform", "shear", "mirror", "translation", "rotation_uniform"]
    maps = [IC.make_set([before, small_positions], of, seed=70 + k, spread=0.8, kinds=kinds[k:] + kinds[:k])[1] for k in range(3)]
    s = pkg.tracer.InstanceSet(members, maps[0])
    try:
        moved = (before.reshape(-1, 3) * F(1.3) + F(0.2)).astype(F)
        now = [moved.reshape(-1), small_positions]
        at_first = run(s, PR.COUNTS, "host")
        assert_cells(at_first, PR.brute(PR.memberships([before, small_positions], of, maps[0])[0]), "before anything moved")
        d_moved, d_maps = torch.from_numpy(moved).cuda(), torch.from_numpy(maps[1]).cuda()
        first = torch.full((25,), POISON, dtype=torch.int64, device="cuda")
        counts = torch.full((25,), POISON, dtype=torch.int64, device="cuda")
        flags = torch.full((25,), POISON, dtype=torch.int64, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            own.refit(d_moved, stream_ptr=side.cuda_stream)
            s.update_into(d_maps.data_ptr(), side.cuda_stream)
            s.collision_pairs_into(first.data_ptr(), counts.data_ptr(), stream_ptr=side.cuda_stream)
            s.collision_pairs_into(0, flags.data_ptr(), any_only=True, stream_ptr=side.cuda_stream)
        side.synchronize()
        assert s.update_status() == -1
        want = PR.brute(PR.memberships(now, of, maps[1])[0])
        assert (want[1] != at_first[1]).sum() >= 4 and (want[1] > 0).sum() >= 4, "the refit and the update moved something"
        assert_cells((first.cpu().numpy().view(np.uint64).reshape(5, 5), counts.cpu().numpy().reshape(5, 5)), want, "one stream")
        assert np.array_equal(flags.cpu().numpy().reshape(5, 5), (want[1] > 0).astype(np.int64)), "one stream, ANY"
        # a host update: the device copy of the maps is behind it until the next query stages them on its stream
        s.update(maps[2])
        want2 = PR.brute(PR.memberships(now, of, maps[2])[0])
        assert (want2[1] != want[1]).sum() >= 4, "the host update moved something"
        check_every_form(s, want2, "after a host update")
    finally:
        s.close()
        own.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_the_refusals_that_read_the_set_and_their_order(pkg, gpu):
    import torch
    s = build(pkg, ["lobed_528", "one triangle"], np.stack([EYE, EYE]), "refusals")
    N = pkg._native
    lib = N.load_instance_pairs()
    dev, host, cnt = lib.shray_instance_pairs_intersect_device, lib.shray_instance_pairs_intersect, lib.shray_instance_pairs_intersect_counters
    error = lambda: N.load_hip().shray_last_error().decode()
    op = lambda first_row=0, row_count=2, flags=0: C.byref(pkg.tracer._pairs_params(first_row, row_count, bool(flags & 1), bool(flags & 4),
                                                                                     bool(flags & 2)))
    d = torch.full((64,), POISON, dtype=torch.int64, device="cuda")
    base, V = d.data_ptr(), C.c_void_p
    # rows beyond the set come before "nothing is asked for", and that before the alignment
    for first_row, row_count in ((0, 3), (2, 1), (3, 0), (1, 2), (0, 1 << 30), (2147483647, 2147483647)):
        assert dev(s._handle, op(first_row, row_count), None, None, None) == -1 and "are not all among the set's 2 instances" in error()
    assert dev(s._handle, op(), None, None, None) == -1 and "nothing is asked for" in error()
    assert dev(s._handle, op(2, 0), None, None, None) == -1 and "nothing is asked for" in error()
    assert dev(s._handle, op(), V(base + 4), None, None) == -1 and "8-byte aligned" in error()
    assert dev(s._handle, op(), V(base), V(base + 260), None) == -1 and "8-byte aligned" in error()
    assert dev(s._handle, op(flags=1), None, V(base + 2), None) == -1 and "8-byte aligned" in error()
    torch.cuda.synchronize()
    assert bool((d == POISON).all()), "a refused call writes nothing"
    h = np.full(16, POISON, np.int64)
    assert host(s._handle, op(0, 3), V(h.ctypes.data), None) == -1 and "are not all among" in error()
    assert host(s._handle, op(), V(h.ctypes.data + 4), None) == -1 and "8-byte aligned" in error()
    tally = N.Counters()
    assert cnt(s._handle, op(1, 2), V(h.ctypes.data), None, C.byref(tally)) == -1 and "are not all among" in error()
    assert (h == POISON).all()
    # an empty range at either end is a no-op, and its counters are zero
    assert dev(s._handle, op(0, 0), V(base), V(base + 256), None) == 0 and dev(s._handle, op(2, 0), V(base), None, None) == 0
    tally.samples = tally.node_visits = 9
    assert cnt(s._handle, op(1, 0), V(h.ctypes.data), None, C.byref(tally)) == 0 and tally.as_dict() == dict.fromkeys(tally.as_dict(), 0)
    torch.cuda.synchronize()
    assert bool((d == POISON).all()) and (h == POISON).all()
    # the wrappers: a range outside the set reaches the library, which refuses it
    for rows in (range(1, 3), (2, 1), (-1, 1)):
        with pytest.raises(N.ShrayError) as err:
            s.collision_pairs(rows)
        assert err.value.code == -1
        with pytest.raises(N.ShrayError):
            s.collision_matrix(rows)
    with pytest.raises(ValueError):
        s.collision_pairs(range(0, 2, 2))
    with pytest.raises(ValueError):
        s.collision_pairs(counters=True, device=True)
    assert s.collision_pairs((1, 0))[0].shape == (0, 2) and s.collision_matrix((2, 0)).shape == (0, 2)
    # the two members do collide: the valid call answers
    got = s.collision_matrix()
    assert got.shape == (2, 2) and not got[0, 0] and not got[1, 1]


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_sixteen_overlapping_copies_many_waves_per_cell(pkg, gpu):
    """Contention: 16 copies of lobed_528 that all overlap, nine workgroups per row adding to each of the row's fifteen
    cells.  The pairs that pass stage 0 are tested once, on the GPU through point_query_ref.TorchOps
    (instance_pairs_ref.intersects_torch, held against numpy in tests/test_instance_pairs_reference.py)."""
    lobed = member(pkg, "lobed_528")[0]
    of = [0] * 16
    _, maps, _ = IC.make_set([lobed], of, seed=16, spread=0.3)
    s = build(pkg, ["lobed_528"] * 16, maps, "sixteen copies")
    blocks, walked = PR.memberships([lobed], of, maps, device="cuda")
    brute = PR.brute(blocks)
    off = ~np.eye(16, dtype=bool)
    print("sixteen copies: set cells", int((brute[1] > 0).sum()), "of 240, counts from", int(brute[1][off].min()), "to", int(brute[1].max()))
    assert (brute[1][off] > 0).mean() > 0.75 and brute[1][1, 4] == brute[1][4, 1] >= 528, "the copies overlap; 4 is 1's twin"
    busy = [(np.add.reduceat(blocks[a][b].any(1), np.arange(0, 528, PR.LANES)) > 0).sum() for a in range(16) for b in range(16) if a != b]
    assert np.mean(busy) > 4, "several workgroups of a row hold members of a cell"
    for again in range(2):
        check_every_form(s, brute, f"sixteen copies, launch {again}", paths=("device",))
    check_every_form(s, brute, "sixteen copies", paths=("host",))
